// k_stack.h -- what profile cpu's device side and its host entry points must agree on: the row
// hash of the interner (igx_intern_*) and the kernel symbol search (igx_ksym_lookup).
// Device code and plain host C++17 (a CPU driver can run the same functions).
//
// Row hash.  A row is row_bytes / 8 little-endian u64 words.  Word k contributes
// st_word(w, k), a 64-bit mix of the word with its position, the contributions are added
// (mod 2^64) and st_finish mixes the sum with the row length.  Addition commutes, so the
// device may sum the contributions in any order (a lane takes two words, a wave reduction adds
// the lanes) and still get, bit for bit, what st_hash_row computes word by word; the position
// inside every contribution is what makes the hash depend on the order of the words.
//
// A row's home slot in a table of S slots (S a power of two) is hash & (S - 1); the tag a slot
// keeps beside its reference is hash >> 32.
#pragma once

#include <cstdint>
#include <cstring>

#include "k_pred.h"

// murmur3's 64-bit finaliser
IGX_HD inline __attribute__((always_inline)) uint64_t st_mix(uint64_t x) {
    x ^= x >> 33;
    x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33;
    x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33;
    return x;
}

// the contribution of word w at position k
IGX_HD inline __attribute__((always_inline)) uint64_t st_word(uint64_t w, uint32_t k) {
    return st_mix(w + 0x9E3779B97F4A7C15ull * ((uint64_t)k + 1));
}

IGX_HD inline __attribute__((always_inline)) uint64_t st_finish(uint64_t sum, uint32_t row_bytes) {
    return st_mix(sum ^ ((uint64_t)row_bytes << 32));
}

// The hash of the row_bytes (a multiple of 8) bytes at p; reads exactly those bytes.
IGX_HD inline uint64_t st_hash_row(const uint8_t *p, uint32_t row_bytes) {
    uint64_t sum = 0;
    for (uint32_t k = 0; k < row_bytes / 8; ++k) {
        uint64_t w;
        memcpy(&w, p + 8 * (size_t)k, 8);
        sum += st_word(w, k);
    }
    return st_finish(sum, row_bytes);
}

// findKernelSymbol (pkg/gadgets/profile/cpu/tracer/tracer.go:184-208) as written, over the
// table in the order given: the index of the symbol, or IGX_NO_COL for "[unknown]".  The last
// comparison is against `addr`, the last address probed, not against ip: in a sorted table of
// two or more symbols an ip below every symbol resolves to symbol 0, and a table of one symbol
// resolves only when that symbol's address is 0.
IGX_HD inline uint32_t st_ksym_find(const uint64_t *sym, uint64_t nsyms, uint64_t ip) {
    int64_t start = 0, end = (int64_t)nsyms - 1;
    uint64_t addr = 0;
    while (start < end) {
        const int64_t mid = start + (end - start + 1) / 2;
        addr = sym[mid];
        if (addr <= ip)
            start = mid;
        else
            end = mid - 1;
    }
    if (start == end && sym[start] <= addr) return (uint32_t)start;
    return IGX_NO_COL;
}
