// k_tcptrace.h -- what the probes of trace tcp decide per row, before and beside their maps
// (pkg/gadgets/trace/tcp/tracer/bpf/tcptracer.bpf.c).  Device code and plain host C++17: the
// device kernel (k_tcptrace.hip) and a CPU driver run the same function.
//
// A row is one probe firing with the fields the probe reads.  tcp_classify_row says which kind of
// igx_chain_join the row is (or IGX_TCP_NO_KIND), which event it emits on its own (accept, close)
// and the 40-byte tuple key: saddr 16, daddr 16, sport 2, dport 2, netns 4 (tuple_key_t, :31-43),
// here as ten 32-bit words.
//
//   fill_tuple (:79-122)   netns is read first and is not tested; then saddr, daddr, dport, sport,
//                          and the first zero among those stops it with every later field still
//                          zero.  AF_INET reads 4 bytes of each address (the other 12 key bytes
//                          stay zero whatever the row holds), AF_INET6 tests all 16; any other
//                          family fails after netns.
//   filter_event (:147-166) family, mount namespace, pid, uid -- at connect-enter, close and
//                          accept only.
//
// The set-state probe's delete with an incomplete tuple (:308-309 -> :327) is "nothing": the key
// it would delete has a zero among saddr / daddr / dport / sport, and a key is stored only by a
// connect-return whose fill_tuple succeeded (:212-222), so no stored key has a zero there.
//
// A modelling decision: the reference's return probe reads the socket through the pointer the
// kprobe stored (:210); the row model carries the socket's fields on the connect-return row,
// because the socket whose connect returns on a thread is the one the thread entered with.  The
// two differ only when a thread's kprobe was missed while an older entry of the same thread is
// still in the map; that is not reproduced, as max_entries is not.
//
// The tuple words are written for PASS / TAKE / DROP rows and for rows with an event, and are
// zero for every other row.
#pragma once

#include <cstdint>

#include "k_pred.h"

constexpr uint32_t TCP_P_CONNECT_ENTER = 0, TCP_P_CONNECT_RETURN = 1, TCP_P_CLOSE = 2, TCP_P_SET_STATE = 3,
                   TCP_P_ACCEPT_RETURN = 4;
constexpr uint32_t TCP_K_ENTER = 0, TCP_K_PASS = 1, TCP_K_ABORT = 2, TCP_K_TAKE = 3, TCP_K_DROP = 4, TCP_K_NONE = 255;
constexpr uint32_t TCP_EV_NONE = 0, TCP_EV_ACCEPT = 1, TCP_EV_CLOSE = 2;
constexpr uint32_t TCP_AF_INET = 2, TCP_AF_INET6 = 10;
constexpr uint32_t TCP_ST_ESTABLISHED = 1, TCP_ST_SYN_SENT = 2, TCP_ST_SYN_RECV = 3, TCP_ST_CLOSE = 7,
                   TCP_ST_NEW_SYN_RECV = 12;
constexpr uint32_t TCP_TUPLE_WORDS = 10;

struct TcpRow {
    uint32_t probe, pid, uid, state, family, netns;
    uint64_t mntns;
    int32_t ret;
    uint32_t saddr[4], daddr[4];
    uint32_t dport, sport, num;   // 16-bit values, as the socket holds them
};

struct TcpFilter {
    uint32_t pid;             // 0: none
    uint32_t uid;             // 0xFFFFFFFF: none
    const uint64_t *mntns;    // sorted ascending; null: no mount-namespace filter
    uint32_t n_mntns;
};

struct TcpOut {
    uint32_t tuple[TCP_TUPLE_WORDS];
    uint32_t kind, event;
};

IGX_HD inline __attribute__((always_inline)) bool tcp_fill_tuple(const TcpRow &r, uint32_t family, uint32_t *t) {
    for (uint32_t i = 0; i < TCP_TUPLE_WORDS; ++i) t[i] = 0;
    t[9] = r.netns;                                                        // :84
    if (family == TCP_AF_INET) {
        t[0] = r.saddr[0];                                                 // :88-90
        if (t[0] == 0) return false;
        t[4] = r.daddr[0];                                                 // :92-94
        if (t[4] == 0) return false;
    } else if (family == TCP_AF_INET6) {
        for (int i = 0; i < 4; ++i) t[i] = r.saddr[i];                     // :98-101
        if ((t[0] | t[1] | t[2] | t[3]) == 0) return false;
        for (int i = 0; i < 4; ++i) t[4 + i] = r.daddr[i];                 // :102-105
        if ((t[4] | t[5] | t[6] | t[7]) == 0) return false;
    } else {
        return false;                                                      // :109-110
    }
    const uint32_t dport = r.dport & 0xFFFFu, sport = r.sport & 0xFFFFu;
    t[8] = dport << 16;                                                    // :113-115
    if (dport == 0) return false;
    t[8] |= sport;                                                         // :117-119
    return sport != 0;
}

// true: the probe returns before it does anything (:147-166)
IGX_HD inline __attribute__((always_inline)) bool tcp_filter_event(const TcpRow &r, const TcpFilter &f) {
    if (r.family != TCP_AF_INET && r.family != TCP_AF_INET6) return true;
    if (f.mntns) {
        uint32_t lo = 0, hi = f.n_mntns;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (f.mntns[mid] < r.mntns) lo = mid + 1;
            else hi = mid;
        }
        if (lo >= f.n_mntns || f.mntns[lo] != r.mntns) return true;
    }
    if (f.pid && r.pid != f.pid) return true;
    if (f.uid != 0xFFFFFFFFu && r.uid != f.uid) return true;
    return false;
}

IGX_HD inline __attribute__((always_inline)) void tcp_classify_row(const TcpRow &r, const TcpFilter &f, TcpOut *o) {
    uint32_t t[TCP_TUPLE_WORDS];
    for (uint32_t i = 0; i < TCP_TUPLE_WORDS; ++i) t[i] = 0;
    uint32_t kind = TCP_K_NONE, event = TCP_EV_NONE;
    bool keep = false;   // whether the tuple is part of the result
    if (r.probe == TCP_P_CONNECT_ENTER) {
        if (!tcp_filter_event(r, f)) kind = TCP_K_ENTER;                   // :182-185
    } else if (r.probe == TCP_P_CONNECT_RETURN) {
        keep = r.ret == 0 && tcp_fill_tuple(r, r.family, t);               // :207-213
        kind = keep ? TCP_K_PASS : TCP_K_ABORT;
    } else if (r.probe == TCP_P_SET_STATE) {
        if (r.state == TCP_ST_ESTABLISHED || r.state == TCP_ST_CLOSE) {    // :303-304
            keep = tcp_fill_tuple(r, r.family, t);                         // :308-309
            if (keep) kind = r.state == TCP_ST_CLOSE ? TCP_K_DROP : TCP_K_TAKE;
        }
    } else if (r.probe == TCP_P_CLOSE) {
        if (!tcp_filter_event(r, f) && r.state != TCP_ST_SYN_SENT && r.state != TCP_ST_SYN_RECV &&
            r.state != TCP_ST_NEW_SYN_RECV) {                              // :269-280
            keep = tcp_fill_tuple(r, r.family, t);                         // :283-284
            if (keep) event = TCP_EV_CLOSE;
        }
    } else if (r.probe == TCP_P_ACCEPT_RETURN) {
        if (!tcp_filter_event(r, f)) {                                     // :351-352
            (void)tcp_fill_tuple(r, r.family, t);                          // :357: result ignored
            const uint32_t num = r.num & 0xFFFFu;
            const uint32_t sport = ((num & 0xFFu) << 8) | (num >> 8);      // :358
            t[8] = (t[8] & 0xFFFF0000u) | sport;
            keep = (t[0] | t[1] | t[2] | t[3]) != 0 && (t[4] | t[5] | t[6] | t[7]) != 0 && (t[8] >> 16) != 0 &&
                   sport != 0;                                             // :360-361
            if (keep) event = TCP_EV_ACCEPT;
        }
    }
    for (uint32_t i = 0; i < TCP_TUPLE_WORDS; ++i) o->tuple[i] = keep ? t[i] : 0u;
    o->kind = kind;
    o->event = event;
}
