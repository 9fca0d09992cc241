// k_seccomp.h -- what advise seccomp-profile's device side (k_seccomp.hip) and a CPU driver must
// agree on: the row classifier of ig_seccomp_e (advise/seccomp/tracer/bpf/seccomp.bpf.c:67-139),
// the hash that places a mount namespace in the slot table, and the u32 code that launch 1
// leaves per row for launch 2.  Device code and plain host C++17.
//
// The BPF program is a sequential machine per mount namespace M: runc's rows record nothing until
// M's first runc prctl(PR_GET_PDEATHSIG), which arms the entry (the value's footer byte).  In
// closed form, with g(M) the smallest stream index of an arming-type row of M that survived the
// drop checks: a runc row i of M records iff i > g(M) and it is not one of the two excluded
// calls; footer = 1 iff g(M) exists.  The classes below are what a row can be to that rule.
#pragma once

#include <cstdint>

#include "k_stack.h"   // st_mix

constexpr uint32_t SC_SYSCALLS = 500;                  // SYSCALLS_COUNT
constexpr uint32_t SC_VALUE_BYTES = SC_SYSCALLS + 1;   // presence bytes, then the footer ("armed")
constexpr uint32_t SC_WORDS = 16;                      // u32 words of a slot's bitmap (bit id), 64 bytes
constexpr uint64_t SC_PR_GET_PDEATHSIG = 2, SC_PR_SET_NO_NEW_PRIVS = 38;
constexpr uint64_t SC_NO_GATE = ~0ull;

enum : uint32_t {
    SC_DROP = 0,    // compat, id >= 500 or mntns == 0: no entry is made
    SC_PLAIN = 1,   // not runc: records
    SC_ARM = 2,     // runc prctl(PR_GET_PDEATHSIG): a gate candidate; records when past the gate
    SC_GATED = 3,   // any other runc row: records when past the gate
    SC_TOUCH = 4,   // runc prctl(PR_SET_NO_NEW_PRIVS) or seccomp(): the entry exists, nothing recorded
};

// comm4: the first four bytes of comm, little-endian.  All 64 bits of arg0 are compared.
// An excluded call is TOUCH whether or not the entry is armed: it never records either way.
IGX_HD inline __attribute__((always_inline)) uint32_t sc_classify(uint64_t mntns, uint32_t id, uint64_t arg0,
                                                                  uint32_t comm4, uint32_t compat, uint32_t nr_prctl,
                                                                  uint32_t nr_seccomp) {
    if (compat != 0 || id >= SC_SYSCALLS || mntns == 0) return SC_DROP;
    if (comm4 != 0x636E7572u) return SC_PLAIN;   // 'r' 'u' 'n' 'c'
    if (id == nr_prctl && arg0 == SC_PR_GET_PDEATHSIG) return SC_ARM;
    if ((id == nr_prctl && arg0 == SC_PR_SET_NO_NEW_PRIVS) || id == nr_seccomp) return SC_TOUCH;
    return SC_GATED;
}

// Whether a row of class cls at stream index idx records, given its namespace's gate.
IGX_HD inline __attribute__((always_inline)) bool sc_records(uint32_t cls, uint64_t idx, uint64_t gate) {
    return cls == SC_PLAIN || ((cls == SC_ARM || cls == SC_GATED) && gate != SC_NO_GATE && idx > gate);
}

// A namespace's home slot in a table of nslots (a power of two); probing is linear from there.
IGX_HD inline __attribute__((always_inline)) uint64_t sc_hash(uint64_t mntns) {
    return st_mix(mntns + 0x9E3779B97F4A7C15ull);
}
IGX_HD inline __attribute__((always_inline)) uint64_t sc_home(uint64_t mntns, uint64_t nslots) {
    return sc_hash(mntns) & (nslots - 1);
}

// The per-row code: class in bits 0-2, id in bits 3-11, slot in bits 12-31 (so nslots <= 2^20).
// A DROP row's code is 0.
constexpr uint32_t SC_SLOT_BITS = 20;
constexpr uint64_t SC_MAX_SLOTS = 1ull << SC_SLOT_BITS;
IGX_HD inline __attribute__((always_inline)) uint32_t sc_pack(uint32_t slot, uint32_t id, uint32_t cls) {
    return (slot << 12) | (id << 3) | cls;
}
IGX_HD inline __attribute__((always_inline)) uint32_t sc_code_slot(uint32_t code) { return code >> 12; }
IGX_HD inline __attribute__((always_inline)) uint32_t sc_code_id(uint32_t code) { return (code >> 3) & 0x1FFu; }
IGX_HD inline __attribute__((always_inline)) uint32_t sc_code_class(uint32_t code) { return code & 7u; }
