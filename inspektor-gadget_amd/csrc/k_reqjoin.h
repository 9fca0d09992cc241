// k_reqjoin.h -- the start/issue/done state machine of igx_req_join as an associative summary.
// Device code and plain host C++17 (a CPU driver can run the same functions).
//
// Rows are taken in the order "sorted by req, ties by row"; pos is a row's position in that
// order.  Every field is a position + 1 (0: none in the range the summary covers):
//   id   last ISSUE-or-DONE, as ((pos + 1) << 1) | is_issue
//   s    last START
//   h    last run head (first position of a req)
//   ok   last DONE known to succeed
//   ld   the leading DONE: a DONE with no ISSUE-or-DONE before it inside the range, whose
//        success depends on what comes before the range (at most one per range)
//   lh   the last run head at or before ld inside the range
// A DONE succeeds iff the last ISSUE-or-DONE before it is an ISSUE with no run head after it
// (biotop.bpf.c:97-99: a DONE without a start entry returns at once).  rj_combine(A, B) is the
// summary of range A followed by range B; rj_step is the same machine one row at a time on a
// summary that starts at position 0 (so it holds no unresolved leading DONE).
#pragma once

#include <cstdint>

#include "k_pred.h"

struct RjSum {
    uint64_t id;
    uint32_t s, h, ok, ld, lh, pad;
};

// a row's code: bits 0-1 the kind (3: the row does not exist for the join), bit 2 run head
constexpr uint32_t RJ_NONE = 3, RJ_HEAD = 4;

IGX_HD inline __attribute__((always_inline)) RjSum rj_elem(uint32_t pos, uint32_t code) {
    RjSum e{};
    const uint32_t k = code & 3u, p1 = pos + 1;
    e.h = (code & RJ_HEAD) ? p1 : 0u;
    if (k == IGX_REQ_START) e.s = p1;
    if (k == IGX_REQ_ISSUE) e.id = ((uint64_t)p1 << 1) | 1u;
    if (k == IGX_REQ_DONE) {
        e.id = (uint64_t)p1 << 1;
        e.ld = p1;
        e.lh = e.h;
    }
    return e;
}

IGX_HD inline __attribute__((always_inline)) RjSum rj_combine(const RjSum &a, const RjSum &b) {
    RjSum r;
    r.id = b.id ? b.id : a.id;
    r.s = b.s ? b.s : a.s;
    r.h = b.h ? b.h : a.h;
    r.pad = 0;
    uint32_t ok = a.ok > b.ok ? a.ok : b.ok;
    if (b.ld && a.id) {
        // b's leading DONE meets a's last ISSUE-or-DONE: same run iff no head lies between them
        const bool res = (a.id & 1u) && b.lh == 0 && (uint32_t)(a.id >> 1) >= a.h;
        if (res && b.ld > ok) ok = b.ld;
        r.ld = a.ld;
        r.lh = a.lh;
    } else if (b.ld) {   // a holds no ISSUE-or-DONE (so no leading DONE either): still open
        r.ld = b.ld;
        r.lh = b.lh ? b.lh : a.h;
    } else {
        r.ld = a.ld;
        r.lh = a.lh;
    }
    r.ok = ok;
    return r;
}

// What a row does on the state before it.  Returns 1 for a successful DONE; *issue and *who
// are then the positions + 1 of its ISSUE and START (who 0: none).
IGX_HD inline __attribute__((always_inline)) int rj_step(RjSum &st, uint32_t pos, uint32_t code, uint32_t *issue,
                                                        uint32_t *who) {
    const uint32_t k = code & 3u, p1 = pos + 1;
    int done = 0;
    if (code & RJ_HEAD) st.h = p1;
    if (k == IGX_REQ_START) st.s = p1;
    if (k == IGX_REQ_ISSUE) st.id = ((uint64_t)p1 << 1) | 1u;
    if (k == IGX_REQ_DONE) {
        const uint32_t ip = (uint32_t)(st.id >> 1);
        if ((st.id & 1u) && ip >= st.h) {
            done = 1;
            *issue = ip;
            *who = (st.s >= st.h && st.s > st.ok) ? st.s : 0u;
            st.ok = p1;
        }
        st.id = (uint64_t)p1 << 1;
    }
    return done;
}

// The rows of the run that ends after `st` which are still live: the ISSUE (position + 1, 0:
// none) and the START.
IGX_HD inline __attribute__((always_inline)) void rj_live(const RjSum &st, uint32_t *issue, uint32_t *start) {
    const uint32_t ip = (uint32_t)(st.id >> 1);
    *issue = ((st.id & 1u) && ip >= st.h) ? ip : 0u;
    *start = (st.s >= st.h && st.s > st.ok) ? st.s : 0u;
}
