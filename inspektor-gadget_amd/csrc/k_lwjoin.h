// k_lwjoin.h -- the two-register last-writer machine of igx_lw_join as an associative summary.
// Device code and plain host C++17 (a CPU driver can run the same functions).
//
// Rows are taken in the order "sorted by key, ties by row"; pos is a row's position in that
// order.  Per register the summary holds the last writer in the range it covers, as
// ((pos + 1) << 1) | is_set (0: no writer in the range):
//   a   SET_A sets; TAKE_A clears, whether it emits or not (a TAKE on an empty A leaves it empty)
//   b   SET_B sets; CLEAR_B clears
//   h   the last run head (first position of a key), as pos + 1 (0: none in the range)
// A register is present iff its last writer is a set at or after the last head.  Nothing a row
// does depends on the state it finds -- a TAKE_A only reads it -- so lw_combine(A, B), the summary
// of range A followed by range B, takes each field from B where B has one and from A otherwise:
// the "last non-zero" monoid, three times.  lw_step is the same machine one row at a time.
#pragma once

#include <cstdint>

#include "k_pred.h"

struct LwSum {
    uint64_t a, b;
    uint32_t h, pad;
};

// a row's code: bits 0-2 the kind (4: the row does not exist for the join), bit 3 run head
constexpr uint32_t LW_SET_A = 0, LW_SET_B = 1, LW_CLEAR_B = 2, LW_TAKE_A = 3, LW_NONE = 4, LW_HEAD = 8;

IGX_HD inline __attribute__((always_inline)) LwSum lw_elem(uint32_t pos, uint32_t code) {
    LwSum e{};
    const uint32_t k = code & 7u;
    const uint64_t p1 = (uint64_t)pos + 1;
    e.h = (code & LW_HEAD) ? (uint32_t)p1 : 0u;
    if (k == LW_SET_A) e.a = (p1 << 1) | 1u;
    if (k == LW_TAKE_A) e.a = p1 << 1;
    if (k == LW_SET_B) e.b = (p1 << 1) | 1u;
    if (k == LW_CLEAR_B) e.b = p1 << 1;
    return e;
}

IGX_HD inline __attribute__((always_inline)) LwSum lw_combine(const LwSum &x, const LwSum &y) {
    LwSum r;
    r.a = y.a ? y.a : x.a;
    r.b = y.b ? y.b : x.b;
    r.h = y.h ? y.h : x.h;
    r.pad = 0;
    return r;
}

// The rows held in the registers of the run that `st` ends in: positions + 1, 0 for empty.
IGX_HD inline __attribute__((always_inline)) void lw_live(const LwSum &st, uint32_t *a, uint32_t *b) {
    const uint32_t ap = (uint32_t)(st.a >> 1), bp = (uint32_t)(st.b >> 1);
    *a = ((st.a & 1u) && ap >= st.h) ? ap : 0u;
    *b = ((st.b & 1u) && bp >= st.h) ? bp : 0u;
}

// What a row does on the state before it.  Returns 1 for an emitting TAKE_A; *a and *b are then
// the positions + 1 of its A row and its B row (b 0: none).
IGX_HD inline __attribute__((always_inline)) int lw_step(LwSum &st, uint32_t pos, uint32_t code, uint32_t *a,
                                                        uint32_t *b) {
    const uint32_t k = code & 7u;
    const uint64_t p1 = (uint64_t)pos + 1;
    int take = 0;
    if (code & LW_HEAD) st.h = (uint32_t)p1;
    if (k == LW_SET_A) st.a = (p1 << 1) | 1u;
    if (k == LW_SET_B) st.b = (p1 << 1) | 1u;
    if (k == LW_CLEAR_B) st.b = p1 << 1;
    if (k == LW_TAKE_A) {
        uint32_t la, lb;
        lw_live(st, &la, &lb);
        if (la) {
            take = 1;
            *a = la;
            *b = lb;
        }
        st.a = p1 << 1;
    }
    return take;
}
