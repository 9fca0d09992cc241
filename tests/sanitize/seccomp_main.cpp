// Host driver for csrc/k_seccomp.h (plain C++17, built with ASan + UBSan by
// tests/test_seccomp_core_host.py).
//  - sc_pack / sc_code_* round trip: every slot x every id with the class rotating, and every id
//    x every class on slots spread over the whole range (the full triple product is 2.6e9 codes).
//  - The closed form the device uses equals the row-by-row machine of ig_seccomp_e
//    (seccomp.bpf.c:67-139), transcribed below with a 501-byte value per namespace.  The closed
//    form is run as the device runs it: per batch, pass 1 classifies with sc_classify, makes the
//    entry, lowers the namespace's gate to the smallest global index of an ARM row and writes the
//    packed code; pass 2 reads only the codes and marks with sc_records.  Seeded random streams
//    are cut into random batches, with deletes between batches; after every batch the found flag
//    and all 501 bytes of every namespace in play must agree.  Slot state lives in heap blocks of
//    exactly the table's size, so a slot or word out of range is an ASan report.
// Prints SC_OK, or the first mismatch and exits 1.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "k_seccomp.h"

struct Row {
    uint64_t mntns;
    uint32_t id;
    uint64_t arg0;
    char comm[16];
    uint8_t compat;
};

using Value = std::array<uint8_t, SC_VALUE_BYTES>;

// the BPF program as it reads
struct Machine {
    uint32_t nr_prctl, nr_seccomp;
    std::map<uint64_t, Value> map;
    void row(const Row &r) {
        if (r.compat) return;
        if (r.id >= 500) return;
        const int is_runc = r.comm[0] == 'r' && r.comm[1] == 'u' && r.comm[2] == 'n' && r.comm[3] == 'c';
        if (r.mntns == 0) return;
        auto it = map.find(r.mntns);
        if (it == map.end()) it = map.emplace(r.mntns, Value{}).first;
        Value &v = it->second;
        if (is_runc) {
            if (v[500] == 0) {
                if (r.id == nr_prctl && r.arg0 == 2) v[500] = 1;
                return;
            }
            if ((r.id == nr_prctl && r.arg0 == 38) || r.id == nr_seccomp) return;
        }
        v[r.id] = 1;
    }
};

// the two passes over a dense table: slot = order of first appearance
struct TwoPass {
    uint32_t nr_prctl, nr_seccomp;
    size_t nslots;
    std::map<uint64_t, uint32_t> slot_of;
    uint64_t *gate;
    uint32_t *bits;
    uint8_t *live;
    uint64_t fed = 0;
    TwoPass(uint32_t p, uint32_t s, size_t n) : nr_prctl(p), nr_seccomp(s), nslots(n) {
        gate = (uint64_t *)std::malloc(n * 8);
        bits = (uint32_t *)std::calloc(n * SC_WORDS, 4);
        live = (uint8_t *)std::calloc(n, 1);
        for (size_t i = 0; i < n; ++i) gate[i] = SC_NO_GATE;
    }
    ~TwoPass() {
        std::free(gate);
        std::free(bits);
        std::free(live);
    }
    bool batch(const Row *rows, size_t n) {
        uint32_t *code = (uint32_t *)std::malloc(n ? n * 4 : 4);
        for (size_t i = 0; i < n; ++i) {
            const Row &r = rows[i];
            uint32_t comm4;
            std::memcpy(&comm4, r.comm, 4);
            const uint32_t cls = sc_classify(r.mntns, r.id, r.arg0, comm4, r.compat, nr_prctl, nr_seccomp);
            code[i] = 0;
            if (cls == SC_DROP) continue;
            auto it = slot_of.find(r.mntns);
            if (it == slot_of.end()) {
                if (slot_of.size() == nslots) return false;
                it = slot_of.emplace(r.mntns, (uint32_t)slot_of.size()).first;
            }
            const uint32_t s = it->second;
            live[s] = 1;
            if (cls == SC_ARM && gate[s] > fed + i) gate[s] = fed + i;
            code[i] = sc_pack(s, r.id, cls);
        }
        for (size_t i = 0; i < n; ++i) {
            const uint32_t c = code[i], cls = sc_code_class(c);
            if (cls == SC_DROP || cls == SC_TOUCH) continue;
            const uint32_t s = sc_code_slot(c), id = sc_code_id(c);
            if (sc_records(cls, fed + i, gate[s])) bits[(size_t)s * SC_WORDS + (id >> 5)] |= 1u << (id & 31);
        }
        std::free(code);
        fed += n;
        return true;
    }
    void del(uint64_t m) {
        auto it = slot_of.find(m);
        if (it == slot_of.end()) return;
        const uint32_t s = it->second;
        std::memset(bits + (size_t)s * SC_WORDS, 0, SC_WORDS * 4);
        gate[s] = SC_NO_GATE;
        live[s] = 0;
    }
    bool peek(uint64_t m, Value &v) const {
        v.fill(0);
        auto it = slot_of.find(m);
        if (it == slot_of.end() || !live[it->second]) return false;
        const uint32_t s = it->second;
        for (uint32_t i = 0; i < SC_SYSCALLS; ++i) v[i] = (bits[(size_t)s * SC_WORDS + (i >> 5)] >> (i & 31)) & 1;
        v[SC_SYSCALLS] = gate[s] != SC_NO_GATE;
        return true;
    }
};

static int fail(const char *what, unsigned long long a, unsigned long long b, unsigned long long c) {
    std::printf("MISMATCH %s: %llu %llu %llu\n", what, a, b, c);
    return 1;
}

int main() {
    // pack / unpack (z: a zero the compiler cannot see, so the loops run)
    volatile uint32_t zero = 0;
    const uint32_t z = zero;
    for (uint32_t slot = 0; slot < SC_MAX_SLOTS; ++slot)
        for (uint32_t id = 0; id < SC_SYSCALLS; ++id) {
            const uint32_t cls = (slot + id) % 5, c = sc_pack(slot + z, id + z, cls + z);
            if (sc_code_slot(c) != slot || sc_code_id(c) != id || sc_code_class(c) != cls)
                return fail("pack", slot, id, cls);
        }
    for (uint32_t k = 0; k <= 4096; ++k) {
        const uint32_t slot = k == 4096 ? (uint32_t)SC_MAX_SLOTS - 1 : k * (uint32_t)(SC_MAX_SLOTS / 4096);
        for (uint32_t id = 0; id < SC_SYSCALLS; ++id)
            for (uint32_t cls = 0; cls < 5; ++cls) {
                const uint32_t c = sc_pack(slot, id, cls);
                if (sc_code_slot(c) != slot || sc_code_id(c) != id || sc_code_class(c) != cls)
                    return fail("pack", slot, id, cls);
                if ((cls == SC_DROP) != (sc_code_class(c) == SC_DROP)) return fail("drop code", slot, id, cls);
            }
    }
    if (sc_pack(0, 0, SC_DROP) != 0) return fail("drop is 0", 0, 0, 0);
    // home slots stay below the table size
    for (uint64_t ns = 1; ns <= SC_MAX_SLOTS; ns <<= 1)
        for (uint64_t m = 0; m < 1000; ++m)
            if (sc_home(m * 0x9E3779B97F4A7C15ull + m, ns) >= ns) return fail("home", m, ns, 0);

    // closed form == machine
    std::mt19937_64 g(20241020);
    static const char *const comms[] = {"runc", "runc:[2:INIT]", "run", "runx", "Runc", "runcrunc01234567", "sh", ""};
    for (int iter = 0; iter < 400; ++iter) {
        const bool arm64 = iter & 1;
        const uint32_t nr_prctl = arm64 ? 167 : 157, nr_seccomp = arm64 ? 277 : 317;
        const size_t pool = 1 + g() % 12, nrows = g() % 3000;
        const int runc_pct = 10 + (int)(g() % 80);
        std::vector<uint64_t> ns(pool);
        for (auto &m : ns) m = g() % 7 == 0 ? 0 : (g() | 1) >> (g() % 50);
        std::vector<Row> rows(nrows);
        for (auto &r : rows) {
            r.mntns = ns[g() % pool];
            const unsigned k = (unsigned)(g() % 16);
            r.id = k < 3 ? nr_prctl : k == 3 ? nr_seccomp : k == 4 ? 500 : k == 5 ? 0xFFFFFFFFu : k == 6 ? 499
                                                                                                        : (uint32_t)(g() % 520);
            const unsigned a = (unsigned)(g() % 8);
            r.arg0 = a < 2 ? 2 : a < 4 ? 38 : a == 4 ? 2 + (1ull << 32) : a == 5 ? 38 + (1ull << 40) : g() % 64;
            const char *c = (int)(g() % 100) < runc_pct ? comms[g() % 2] : comms[2 + g() % 6];
            std::memset(r.comm, 0, 16);
            std::memcpy(r.comm, c, std::min<size_t>(16, std::strlen(c)));
            r.compat = g() % 23 == 0;
        }
        Machine mach{nr_prctl, nr_seccomp, {}};
        TwoPass two(nr_prctl, nr_seccomp, pool);
        size_t at = 0;
        while (true) {
            const size_t n = std::min<size_t>(nrows - at, g() % 4 == 0 ? 0 : g() % 700);
            // heap copy of exactly the batch: a read past it is an ASan report
            Row *b = (Row *)std::malloc(n ? n * sizeof(Row) : 1);
            if (n) std::memcpy(b, rows.data() + at, n * sizeof(Row));
            for (size_t i = 0; i < n; ++i) mach.row(b[i]);
            const bool ok = two.batch(b, n);
            std::free(b);
            if (!ok) return fail("table full", iter, at, pool);
            at += n;
            for (uint64_t m : ns) {
                Value v;
                const bool f = two.peek(m, v);
                auto it = mach.map.find(m);
                if (f != (it != mach.map.end())) return fail("found", iter, at, m);
                if (f && v != it->second) return fail("value", iter, at, m);
            }
            if (at == nrows) break;
            for (int d = (int)(g() % 3); d > 0; --d) {
                const uint64_t m = g() % 5 == 0 ? g() : ns[g() % pool];
                mach.map.erase(m);
                two.del(m);
            }
        }
    }
    std::puts("SC_OK");
    return 0;
}
