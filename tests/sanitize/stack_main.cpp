// Host driver for csrc/k_stack.h (plain C++17, built with ASan + UBSan by
// tests/test_stack_core_host.py).
//  - st_ksym_find against a second, straightforward implementation of findKernelSymbol
//    (tracer.go:184-208) on seeded random sorted and unsorted tables of 0 to 1000 symbols, with
//    addresses on, between, below and above the symbols.  Tables live in heap blocks of exactly
//    nsyms words, so an index outside [0, nsyms) is an ASan report.
//  - st_hash_row over every row_bytes from 8 to 1024 on heap buffers that end exactly at the
//    row: a read past the row is an ASan report.  It must equal the sum of st_word over the
//    words taken in another order (what the device's lanes and wave reduction do), and change
//    when two different words swap places.
// Prints ST_OK, or the first mismatch and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "k_stack.h"

// the Go function transcribed with ints and a vector, as directly as it reads
static uint32_t plain_find(const std::vector<uint64_t> &syms, uint64_t ip) {
    long long end = (long long)syms.size() - 1;
    uint64_t addr = 0;
    long long start = 0;
    for (; start < end;) {
        long long mid = start + (end - start + 1) / 2;
        addr = syms.at((size_t)mid);
        if (addr <= ip) {
            start = mid;
        } else {
            end = mid - 1;
        }
    }
    if (start == end && syms.at((size_t)start) <= addr) return (uint32_t)start;
    return IGX_NO_COL;
}

int main() {
    std::mt19937_64 g(20240607);
    for (int iter = 0; iter < 3000; ++iter) {
        const size_t n = iter < 8 ? (size_t)iter : g() % 1001;
        std::vector<uint64_t> v(n);
        const int mode = (int)(g() % 4);
        for (auto &x : v) x = mode == 3 ? g() % 64 : (g() >> (g() % 40));
        if (mode != 1) std::sort(v.begin(), v.end());
        if (mode == 2 && n > 4) std::shuffle(v.begin() + (long)(n / 2), v.end(), g);   // a shuffled tail
        uint64_t *heap = n ? (uint64_t *)std::malloc(n * 8) : nullptr;
        if (n) std::memcpy(heap, v.data(), n * 8);
        for (int q = 0; q < 64; ++q) {
            uint64_t ip;
            switch (g() % 5) {
            case 0: ip = n ? v[g() % n] : 0; break;
            case 1: ip = n ? v[g() % n] + 1 + g() % 16 : 1; break;
            case 2: ip = 0; break;
            case 3: ip = ~0ull; break;
            default: ip = g() >> (g() % 40);
            }
            const uint32_t a = st_ksym_find(heap, n, ip), b = plain_find(v, ip);
            if (a != b) {
                std::printf("ksym mismatch: table %d (%zu symbols) ip %llx: %u vs %u\n", iter, n,
                            (unsigned long long)ip, a, b);
                return 1;
            }
        }
        std::free(heap);
    }
    for (uint32_t rb = 8; rb <= 1024; rb += 8) {
        uint8_t *row = (uint8_t *)std::malloc(rb);
        for (uint32_t i = 0; i < rb; ++i) row[i] = (uint8_t)g();
        const uint64_t h = st_hash_row(row, rb);
        uint64_t sum = 0;
        for (uint32_t k = rb / 8; k-- > 0;) {   // the words backwards
            uint64_t w;
            std::memcpy(&w, row + 8 * k, 8);
            sum += st_word(w, k);
        }
        if (st_finish(sum, rb) != h) {
            std::printf("hash is not the sum of its words: row_bytes %u\n", rb);
            return 1;
        }
        if (rb >= 16) {
            const uint32_t i = (uint32_t)(g() % (rb / 8)), j = (i + 1 + (uint32_t)(g() % (rb / 8 - 1))) % (rb / 8);
            uint64_t wi, wj;
            std::memcpy(&wi, row + 8 * i, 8);
            std::memcpy(&wj, row + 8 * j, 8);
            if (wi != wj) {
                std::memcpy(row + 8 * i, &wj, 8);
                std::memcpy(row + 8 * j, &wi, 8);
                if (st_hash_row(row, rb) == h) {
                    std::printf("hash ignores word order: row_bytes %u words %u %u\n", rb, i, j);
                    return 1;
                }
            }
        }
        // a shorter row with the same leading bytes hashes differently (the length is mixed in)
        if (rb > 8 && st_hash_row(row, rb - 8) == st_hash_row(row, rb)) {
            std::printf("hash ignores the row length: row_bytes %u\n", rb);
            return 1;
        }
        std::free(row);
    }
    std::printf("ST_OK\n");
    return 0;
}
