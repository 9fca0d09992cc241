// k_traceloop.h -- traceloop's enter / exit / cont join (igx_traceloop_join) as an associative
// summary.  Device code and plain host C++17 (a CPU driver can run the same functions).
//
// All rows of both streams share one row id space: syscall row i is id i, cont row j is id
// ns + j.  tl_key packs what the order inside a group needs into one u64, so that a stable sort
// by (mntns, mono_ts, key) puts a group's rows together as
//     subgroup (pid, id): its exits, its enters, its dead rows; next subgroup; ...
// with the conts of parameter i in a subgroup "pid 0, id i".
// A *group* is a run of equal (mntns, mono_ts), a *subgroup* a run of equal key >> 2 inside it.
// An enter's match (tracer.go:438-441: the first exit with its id and pid) is the smallest exit
// row of its subgroup.  The summary takes minima over row ids, so it does not rely on the order
// of the rows inside a subgroup; the key's low bits only spare the code pass a gather.
//
// Per position the code byte holds the row's kind, a cont's parameter index and the two head
// bits.  TlSum is the summary of a range of positions; every row field is a row id, TL_NO = none:
//   ng          group heads in the range
//   flags       TL_GH / TL_SH: the range holds a group / subgroup head; TL_SKIP: an enter of
//               exit, exit_group or rt_sigreturn in the tail group
//   the tail group (after the last group head, or the whole range):
//     e0        its first enter (smallest row)
//     m, mx     the smallest non-skip enter whose subgroup has an exit, and that subgroup's
//               first exit -- over the subgroups that are closed inside the range
//     c[i]      the first cont of parameter i
//   te, tx      the open subgroup at the end of the range (after the last subgroup head): its
//               smallest non-skip enter and its smallest exit
//   le, lx      the same for the rows before the first subgroup head, whose subgroup may have
//               begun before the range (only kept while the range holds no group head)
// tl_combine(A, B) is the summary of A followed by B.  A group that ends inside a range is dropped
// from its summary: the pass that needs a group's result reads it at the group's last position
// from the summary of everything before it, which starts at a group head (tl_final).
#pragma once

#include <cstdint>

#include "k_pred.h"

constexpr uint32_t TL_NO = 0xFFFFFFFFu;

// row kinds (code bits 0-2)
constexpr uint32_t TL_NONE = 0, TL_ENTER = 1, TL_ENTER_SKIP = 2, TL_EXIT = 3, TL_CONT = 4;
// code bits 3-5: a cont's parameter index; bit 6 group head, bit 7 subgroup head
constexpr uint32_t TL_CODE_GH = 0x40, TL_CODE_SH = 0x80;
// summary flags
constexpr uint32_t TL_GH = 1, TL_SH = 2, TL_SKIP = 4;
constexpr int TL_PARAMS = 6;

// sort key of a syscall row: exits (0) before enters (1); 3: the row does not exist
IGX_HD inline uint64_t tl_key_sys(uint32_t pid, uint16_t id, uint8_t typ, bool valid) {
    const uint64_t k = !valid || typ > 1 ? 3u : (typ == 0 ? 1u : 0u);
    return ((uint64_t)pid << 18) | ((uint64_t)id << 2) | k;
}
// sort key of a cont row: kind 2 with the parameter index where a syscall row has its id and no
// pid, so that no byte varies that the syscall keys leave alone (the sort skips those).  Conts may
// thus share a subgroup with the syscall rows of pid 0 and id = index, which changes nothing: a
// cont only sets c[index].  3: does not exist.
IGX_HD inline uint64_t tl_key_cont(uint8_t index, bool valid) {
    return valid && index < TL_PARAMS ? ((uint64_t)index << 2) | 2u : 3u;
}
IGX_HD inline bool tl_skip(uint16_t id, uint16_t nr_exit, uint16_t nr_exit_group, uint16_t nr_rt_sigreturn) {
    return id == nr_exit || id == nr_exit_group || id == nr_rt_sigreturn;
}
// the code's kind bits from a key
IGX_HD inline uint32_t tl_kind(uint64_t key, uint16_t nr_exit, uint16_t nr_exit_group, uint16_t nr_rt_sigreturn) {
    const uint32_t k = (uint32_t)key & 3u;
    if (k == 0) return TL_EXIT;
    if (k == 2) return TL_CONT | (((uint32_t)(key >> 2) & 7u) << 3);
    if (k == 3) return TL_NONE;
    return tl_skip((uint16_t)(key >> 2), nr_exit, nr_exit_group, nr_rt_sigreturn) ? TL_ENTER_SKIP : TL_ENTER;
}

struct TlSum {
    uint32_t ng, flags;
    uint32_t e0, m, mx;
    uint32_t te, tx, le, lx;
    uint32_t c[TL_PARAMS];
    uint32_t pad;
};

IGX_HD inline __attribute__((always_inline)) uint32_t tl_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

IGX_HD inline __attribute__((always_inline)) TlSum tl_identity() {
    TlSum s;
    s.ng = 0;
    s.flags = 0;
    s.e0 = s.m = s.mx = s.te = s.tx = s.le = s.lx = TL_NO;
    for (int i = 0; i < TL_PARAMS; ++i) s.c[i] = TL_NO;
    s.pad = 0;
    return s;
}

IGX_HD inline __attribute__((always_inline)) TlSum tl_elem(uint32_t row, uint32_t code) {
    TlSum s = tl_identity();
    const uint32_t k = code & 7u;
    if (code & TL_CODE_GH) {
        s.ng = 1;
        s.flags |= TL_GH;
    }
    if (code & TL_CODE_SH) s.flags |= TL_SH;
    if (k == TL_ENTER || k == TL_ENTER_SKIP) s.e0 = row;
    if (k == TL_ENTER) s.te = row;
    if (k == TL_ENTER_SKIP) s.flags |= TL_SKIP;
    if (k == TL_EXIT) s.tx = row;
    if (k == TL_CONT) {
        const uint32_t idx = (code >> 3) & 7u;
        for (int i = 0; i < TL_PARAMS; ++i)
            if ((uint32_t)i == idx) s.c[i] = row;
    }
    return s;
}

// (m, mx) with the candidate (e, x) taken in if both exist and e is smaller
IGX_HD inline __attribute__((always_inline)) void tl_take(uint32_t &m, uint32_t &mx, uint32_t e, uint32_t x) {
    if (e != TL_NO && x != TL_NO && e < m) {
        m = e;
        mx = x;
    }
}

IGX_HD inline __attribute__((always_inline)) TlSum tl_combine(const TlSum &a, const TlSum &b) {
    if (b.flags & TL_GH) {   // a's tail group ends inside the range
        TlSum r = b;
        r.ng = a.ng + b.ng;
        return r;
    }
    TlSum r;
    r.ng = a.ng;
    r.flags = a.flags | b.flags;
    r.pad = 0;
    r.e0 = tl_min(a.e0, b.e0);
    for (int i = 0; i < TL_PARAMS; ++i) r.c[i] = tl_min(a.c[i], b.c[i]);
    r.m = a.m;
    r.mx = a.mx;
    tl_take(r.m, r.mx, b.m, b.mx);
    if (b.flags & TL_SH) {
        // a's open subgroup ends with b's rows before b's first subgroup head
        const uint32_t se = tl_min(a.te, b.le), sx = tl_min(a.tx, b.lx);
        if (a.flags & TL_SH) {   // it began inside a: closed
            tl_take(r.m, r.mx, se, sx);
            r.le = a.le;
            r.lx = a.lx;
        } else {                 // it may have begun before a
            r.le = se;
            r.lx = sx;
        }
        r.te = b.te;
        r.tx = b.tx;
    } else {
        r.te = tl_min(a.te, b.te);
        r.tx = tl_min(a.tx, b.tx);
        r.le = a.le;
        r.lx = a.lx;
    }
    return r;
}

// What a group comes to, from the summary of positions [0, its last position]: e0, m, mx, the
// first conts, and whether a skip enter completed.
struct TlGroup {
    uint32_t e0, m, mx, flags;   // flags: TL_SKIP, TL_HASCONT
};
constexpr uint32_t TL_HASCONT = 8;

IGX_HD inline __attribute__((always_inline)) TlGroup tl_final(const TlSum &s) {
    TlGroup g;
    g.e0 = s.e0;
    g.m = s.m;
    g.mx = s.mx;
    tl_take(g.m, g.mx, s.te, s.tx);   // the last subgroup is closed by the group's end
    g.flags = s.flags & TL_SKIP;
    for (int i = 0; i < TL_PARAMS; ++i)
        if (s.c[i] != TL_NO) g.flags |= TL_HASCONT;
    return g;
}

// The event class of syscall row `row` with kind k in a group that came to g: 0 complete,
// 1 incomplete enter, 2 incomplete exit, TL_DROP none (tracer.go:362-530, igx.h).
constexpr uint32_t TL_DROP = 0xFF;
IGX_HD inline __attribute__((always_inline)) uint32_t tl_class(const TlGroup &g, uint32_t row, uint32_t k) {
    if (k == TL_ENTER_SKIP) return 0;
    if (k == TL_ENTER) {
        if (g.m == row) return 0;
        return g.m == TL_NO && !(g.flags & TL_SKIP) ? 1u : TL_DROP;
    }
    if (k == TL_EXIT) return g.m == TL_NO ? 2u : TL_DROP;
    return TL_DROP;
}
