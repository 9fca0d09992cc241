// tcptrace_main.cpp -- csrc/k_tcptrace.h's per-row function on the CPU (built with ASan + UBSan by
// tests/test_tcptrace_core_host.py) against a second restatement of tcptracer.bpf.c that is written
// the way the BPF programs are: a zeroed tuple_key_t filled field by field with early returns.
//
// The table is the one of tests/tcptracer_ref.py's field_table(), in the same loop order: every
// probe with its ret / state cases, three families, saddr and daddr in four patterns each (zero,
// first word only, bytes 12..15 only, all), dport / sport / num zero or not; each row is checked
// without a filter and under a pid, a uid and a mount-namespace filter (sets of 1, 2 and 1024 ids).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "k_tcptrace.h"

namespace {

struct Key {            // tuple_key_t (:31-43), packed to its 40 bytes
    uint8_t saddr[16], daddr[16];
    uint16_t sport, dport;
    uint32_t netns;
};
static_assert(sizeof(Key) == 40, "tuple_key_t");

bool zero(const uint8_t *p, int n) {
    for (int i = 0; i < n; ++i)
        if (p[i]) return false;
    return true;
}

bool plain_fill(Key *t, const TcpRow &r, uint32_t family) {
    t->netns = r.netns;
    const int len = family == 2 ? 4 : family == 10 ? 16 : 0;
    if (!len) return false;
    std::memcpy(t->saddr, r.saddr, len);
    if (zero(t->saddr, len)) return false;
    std::memcpy(t->daddr, r.daddr, len);
    if (zero(t->daddr, len)) return false;
    t->dport = (uint16_t)r.dport;
    if (t->dport == 0) return false;
    t->sport = (uint16_t)r.sport;
    if (t->sport == 0) return false;
    return true;
}

bool plain_skip(const TcpRow &r, const TcpFilter &f) {
    if (r.family != 2 && r.family != 10) return true;
    if (f.mntns) {
        bool found = false;
        for (uint32_t i = 0; i < f.n_mntns; ++i) found = found || f.mntns[i] == r.mntns;
        if (!found) return true;
    }
    if (f.pid && r.pid != f.pid) return true;
    if (f.uid != (uint32_t)-1 && r.uid != f.uid) return true;
    return false;
}

// kind, event and key of one row; key stays zero unless the row is PASS / TAKE / DROP or an event
void plain(const TcpRow &r, const TcpFilter &f, uint32_t *kind, uint32_t *event, Key *out) {
    Key t;
    std::memset(&t, 0, sizeof t);
    std::memset(out, 0, sizeof *out);
    *kind = 255;
    *event = 0;
    switch (r.probe) {
    case 0:
        if (!plain_skip(r, f)) *kind = 0;
        return;
    case 1:
        if (r.ret != 0 || !plain_fill(&t, r, r.family)) {
            *kind = 2;
            return;
        }
        *kind = 1;
        break;
    case 2:
        if (plain_skip(r, f)) return;
        if (r.state == 2 || r.state == 3 || r.state == 12) return;
        if (!plain_fill(&t, r, r.family)) return;
        *event = 2;
        break;
    case 3:
        if (r.state != 1 && r.state != 7) return;
        if (!plain_fill(&t, r, r.family)) return;
        *kind = r.state == 7 ? 4 : 3;
        break;
    case 4:
        if (plain_skip(r, f)) return;
        (void)plain_fill(&t, r, r.family);
        t.sport = (uint16_t)(((r.num & 0xFF) << 8) | ((r.num >> 8) & 0xFF));
        if (zero(t.saddr, 16) || zero(t.daddr, 16) || t.dport == 0 || t.sport == 0) return;
        *event = 1;
        break;
    default:
        return;
    }
    *out = t;
}

const uint8_t PATTERNS[4][16] = {
    {0},
    {0x0a, 0, 0, 1},
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xde, 0xad, 0xbe, 0xef},
    {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16},
};

}  // namespace

int main() {
    const int aux[12][3] = {{0, 0, 0}, {1, 0, 0}, {1, -111, 0}, {2, 0, 1}, {2, 0, 2}, {2, 0, 3},
                            {2, 0, 12}, {2, 0, 7}, {3, 0, 1}, {3, 0, 7}, {3, 0, 2}, {4, 0, 0}};
    const uint32_t fams[3] = {2, 10, 1};
    std::vector<uint64_t> big(1024);
    for (int i = 0; i < 1024; ++i) big[i] = 4026532000ull + 2 * i;   // the even ids
    const uint64_t one[1] = {4026532003ull}, two[2] = {4026532001ull, 4026532010ull};
    const TcpFilter filters[6] = {{0, 0xFFFFFFFFu, nullptr, 0}, {12, 0xFFFFFFFFu, nullptr, 0}, {0, 0, nullptr, 0},
                                  {0, 0xFFFFFFFFu, one, 1},     {0, 2, two, 2},               {11, 1, big.data(), 1024}};
    unsigned long rows = 0, checks = 0, kinds[256] = {0}, events[3] = {0};
    for (const auto &a : aux)
        for (uint32_t fam : fams)
            for (int sa = 0; sa < 4; ++sa)
                for (int da = 0; da < 4; ++da)
                    for (int bits = 0; bits < 8; ++bits) {
                        const unsigned long j = rows++;
                        TcpRow r;
                        std::memset(&r, 0, sizeof r);
                        r.probe = a[0], r.ret = a[1], r.state = a[2], r.family = fam;
                        std::memcpy(r.saddr, PATTERNS[sa], 16);
                        std::memcpy(r.daddr, PATTERNS[da], 16);
                        r.dport = bits & 1 ? 0x5000 : 0;
                        r.sport = bits & 2 ? 0x1F90 : 0;
                        r.num = bits & 4 ? 0x0050 : 0;
                        r.netns = 4026531840u + j % 3;
                        r.pid = 10 + j % 5, r.uid = j % 3, r.mntns = 4026532000ull + j % 11;
                        for (const TcpFilter &f : filters) {
                            TcpOut o;
                            tcp_classify_row(r, f, &o);
                            uint32_t kind, event;
                            Key k;
                            plain(r, f, &kind, &event, &k);
                            if (o.kind != kind || o.event != event || std::memcmp(o.tuple, &k, 40) != 0) {
                                std::printf("MISMATCH row %lu probe %u fam %u: kind %u/%u event %u/%u\n", j, r.probe,
                                            fam, o.kind, kind, o.event, event);
                                return 1;
                            }
                            ++checks;
                            if (f.mntns == nullptr && f.pid == 0 && f.uid == 0xFFFFFFFFu) {
                                ++kinds[kind];
                                ++events[event];
                            }
                        }
                    }
    // every outcome occurs in the unfiltered table, so the comparison is not vacuous
    if (rows != 4608 || !kinds[0] || !kinds[1] || !kinds[2] || !kinds[3] || !kinds[4] || !kinds[255] || !events[1] ||
        !events[2]) {
        std::printf("table does not cover every outcome\n");
        return 1;
    }
    std::printf("TCP_OK rows=%lu checks=%lu pass=%lu take=%lu accept=%lu close=%lu\n", rows, checks, kinds[1],
                kinds[3], events[1], events[2]);
    return 0;
}
