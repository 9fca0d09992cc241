// Host driver for csrc/k_lwjoin.h (plain C++17, built with ASan + UBSan by
// tests/test_lwjoin_core_host.py): the join's summary operator against its own row-by-row
// machine.  Over seeded random code streams (the four kinds, "does not exist" rows, run heads;
// uniform, SET_A-heavy, TAKE-heavy and B-only-between-A-and-T mixes) it checks, for every position,
// that the summary of the rows before it -- combined under a random parenthesisation, as tiles,
// waves and lanes combine them on the device -- gives the state the sequential machine has there,
// run head included, that stepping from it emits the same (take, a, b) and leaves the same live
// rows, and that two random parenthesisations of a whole stream agree field by field
// (associativity).  A third machine, written with plain registers and no summary, checks the
// emissions themselves.  Prints LW_OK, or the first mismatch and exits 1.
#include <cstdio>
#include <random>
#include <vector>

#include "k_lwjoin.h"

static bool same(const LwSum &x, const LwSum &y) { return x.a == y.a && x.b == y.b && x.h == y.h; }

static LwSum tree(const std::vector<LwSum> &v, size_t lo, size_t hi, std::mt19937 &g) {
    if (hi - lo == 1) return v[lo];
    const size_t mid = lo + 1 + g() % (hi - lo - 1);
    const LwSum a = tree(v, lo, mid, g), b = tree(v, mid, hi, g);
    return lw_combine(a, b);
}

int main() {
    std::mt19937 g(24680);
    for (int iter = 0; iter < 20000; ++iter) {
        const uint32_t n = 1 + g() % 60;
        const int mode = g() % 4;
        std::vector<uint32_t> code(n);
        for (uint32_t p = 0; p < n; ++p) {
            uint32_t k;
            if (mode == 0) k = g() % 5;
            else if (mode == 1) k = (g() % 10 < 7) ? LW_SET_A : g() % 5;
            else if (mode == 2) k = (g() % 3) ? LW_TAKE_A : g() % 5;
            else k = p == 0 ? LW_SET_A : (p == n - 1 ? LW_TAKE_A : 1 + g() % 2);
            const bool head = p == 0 || (mode != 3 && g() % 5 == 0);
            code[p] = k | (head ? LW_HEAD : 0u);
        }
        std::vector<LwSum> el(n);
        for (uint32_t p = 0; p < n; ++p) el[p] = lw_elem(p, code[p]);
        LwSum seq{};
        uint32_t regA = 0, regB = 0;   // the plain machine: position + 1 held, 0 empty
        for (uint32_t p = 0; p < n; ++p) {
            LwSum pre{};
            if (p) pre = tree(el, 0, p, g);
            if (!same(pre, seq)) {
                std::printf("state mismatch: stream %d position %u\n", iter, p);
                return 1;
            }
            uint32_t a1 = 0, b1 = 0, a2 = 0, b2 = 0;
            const int t1 = lw_step(pre, p, code[p], &a1, &b1), t2 = lw_step(seq, p, code[p], &a2, &b2);
            if (t1 != t2 || a1 != a2 || b1 != b2 || !same(pre, seq)) {
                std::printf("emit mismatch: stream %d position %u\n", iter, p);
                return 1;
            }
            const uint32_t k = code[p] & 7u;
            if (code[p] & LW_HEAD) regA = regB = 0;
            int t3 = 0;
            uint32_t a3 = 0, b3 = 0;
            if (k == LW_SET_A) regA = p + 1;
            if (k == LW_SET_B) regB = p + 1;
            if (k == LW_CLEAR_B) regB = 0;
            if (k == LW_TAKE_A && regA) {
                t3 = 1;
                a3 = regA;
                b3 = regB;
                regA = 0;
            }
            uint32_t la, lb;
            lw_live(seq, &la, &lb);
            if (t3 != t2 || a3 != a2 || b3 != b2 || la != regA || lb != regB) {
                std::printf("machine mismatch: stream %d position %u\n", iter, p);
                return 1;
            }
        }
        if (n >= 3 && !same(tree(el, 0, n, g), tree(el, 0, n, g))) {
            std::printf("associativity mismatch: stream %d\n", iter);
            return 1;
        }
        if (!same(tree(el, 0, n, g), seq)) {
            std::printf("total mismatch: stream %d\n", iter);
            return 1;
        }
    }
    // positions at the top of the range: (pos + 1) << 1 needs 33 bits
    {
        LwSum st{};
        uint32_t a = 0, b = 0;
        const uint32_t top = 0xFFFFFFFDu;   // the last position of a batch of 2^32 - 2 rows
        (void)lw_step(st, top - 1, LW_SET_A | LW_HEAD, &a, &b);
        if (!lw_step(st, top, LW_TAKE_A, &a, &b) || a != top || b != 0 ||
            !same(lw_combine(lw_elem(top - 1, LW_SET_A | LW_HEAD), lw_elem(top, LW_TAKE_A)), st)) {
            std::printf("top-of-range mismatch\n");
            return 1;
        }
    }
    std::printf("LW_OK\n");
    return 0;
}
