// Host driver for csrc/k_reqjoin.h (plain C++17, built with ASan + UBSan by
// tests/test_reqjoin_core_host.py): the join's summary operator against its own row-by-row
// machine.  Over seeded random code streams (kinds, "does not exist" rows, run heads; START-heavy,
// DONE-heavy and no-START mixes) it checks, for every position, that the summary of the rows
// before it -- combined under a random parenthesisation, as tiles, waves and lanes combine them
// on the device -- gives the state the sequential machine has there, that stepping from it emits
// the same (done, issue, who), and that two random parenthesisations of a whole stream agree
// field by field (associativity).  Prints RJ_OK, or the first mismatch and exits 1.
#include <cstdio>
#include <random>
#include <vector>

#include "k_reqjoin.h"

static bool same(const RjSum &a, const RjSum &b) {
    return a.id == b.id && a.s == b.s && a.h == b.h && a.ok == b.ok && a.ld == b.ld && a.lh == b.lh;
}

static RjSum tree(const std::vector<RjSum> &v, size_t lo, size_t hi, std::mt19937 &g) {
    if (hi - lo == 1) return v[lo];
    const size_t mid = lo + 1 + g() % (hi - lo - 1);
    const RjSum a = tree(v, lo, mid, g), b = tree(v, mid, hi, g);
    return rj_combine(a, b);
}

int main() {
    std::mt19937 g(12345);
    for (int iter = 0; iter < 20000; ++iter) {
        const uint32_t n = 1 + g() % 60;
        const int mode = g() % 4;
        std::vector<uint32_t> code(n);
        for (uint32_t p = 0; p < n; ++p) {
            uint32_t k;
            if (mode == 0) k = g() % 4;
            else if (mode == 1) k = (g() % 10 < 7) ? 0 : g() % 4;
            else if (mode == 2) k = (g() % 3) ? 2 : g() % 4;
            else k = 1 + g() % 2;
            const bool head = p == 0 || g() % (mode == 3 ? 20 : 5) == 0;
            code[p] = k | (head ? RJ_HEAD : 0u);
        }
        std::vector<RjSum> el(n);
        for (uint32_t p = 0; p < n; ++p) el[p] = rj_elem(p, code[p]);
        RjSum seq{};
        for (uint32_t p = 0; p < n; ++p) {
            RjSum pre{};
            if (p) pre = tree(el, 0, p, g);
            if (pre.id != seq.id || pre.s != seq.s || pre.h != seq.h || pre.ok != seq.ok) {
                std::printf("state mismatch: stream %d position %u\n", iter, p);
                return 1;
            }
            uint32_t i1 = 0, w1 = 0, i2 = 0, w2 = 0;
            const int d1 = rj_step(pre, p, code[p], &i1, &w1), d2 = rj_step(seq, p, code[p], &i2, &w2);
            if (d1 != d2 || i1 != i2 || w1 != w2) {
                std::printf("emit mismatch: stream %d position %u\n", iter, p);
                return 1;
            }
        }
        if (n >= 3 && !same(tree(el, 0, n, g), tree(el, 0, n, g))) {
            std::printf("associativity mismatch: stream %d\n", iter);
            return 1;
        }
    }
    std::printf("RJ_OK\n");
    return 0;
}
