// Host driver for csrc/k_traceloop.h (plain C++17, built with ASan + UBSan by
// tests/test_traceloop_core_host.py): the join's keys, codes, summary operator and class rule, run
// on the CPU the way the device runs them, against Tracer.Read's three maps and loops restated row
// by row (tracer.go:313-317, :338-345, :362-530).
//
// For every stream: the rows of both streams are keyed (tl_key_sys / tl_key_cont), stably sorted
// by (mntns, mono_ts, key) and coded (tl_kind, group and subgroup heads); the positions are cut
// into tiles of random sizes, 1 included; each tile is summarised under a random parenthesisation
// (as lanes, waves and threads combine on the device), the tile summaries are scanned into
// carries, and every position's state is carry + the tile's rows before it.  tl_final at each
// group's last position and tl_class per syscall row give the events, which are ordered by
// (sort_ts, row) and compared with the map program's, field by field.  Streams: the hand-worked
// groups of tests/test_traceloop_ref.py, random streams with few timestamps (collisions), two
// containers, dead rows, and single groups of thousands of rows.  Prints TL_OK, or the first
// mismatch and exits 1.
#include <algorithm>
#include <cstdio>
#include <map>
#include <random>
#include <tuple>
#include <vector>

#include "k_traceloop.h"

struct Sys {
    uint64_t mntns, mono, sort;
    uint8_t typ;
    uint16_t id;
    uint32_t pid;
    uint8_t valid;
};
struct Cont {
    uint64_t mntns, mono;
    uint8_t index, valid;
};
struct Event {
    uint64_t sort;
    uint32_t row, exit, cls;
    uint32_t cont[TL_PARAMS];
    bool operator==(const Event &o) const {
        return sort == o.sort && row == o.row && exit == o.exit && cls == o.cls &&
               std::equal(cont, cont + TL_PARAMS, o.cont);
    }
};
static const uint16_t NR[3] = {60, 231, 15};

static void order(std::vector<Event> &ev) {
    std::sort(ev.begin(), ev.end(), [](const Event &a, const Event &b) { return std::tie(a.sort, a.row) < std::tie(b.sort, b.row); });
}

// ---- Tracer.Read, one container at a time ------------------------------------------------------
static std::vector<Event> by_maps(const std::vector<Sys> &s, const std::vector<Cont> &c) {
    std::vector<Event> out;
    std::map<uint64_t, int> containers;
    for (const Sys &r : s) containers[r.mntns] = 1;
    for (const Cont &r : c) containers[r.mntns] = 1;
    for (const auto &kv : containers) {
        std::map<uint64_t, std::vector<uint32_t>> cont_map, enter_map, exit_map;
        for (uint32_t i = 0; i < s.size(); ++i) {
            if (s[i].mntns != kv.first || !s[i].valid) continue;
            if (s[i].typ == 0) enter_map[s[i].mono].push_back(i);
            else if (s[i].typ == 1) exit_map[s[i].mono].push_back(i);
        }
        for (uint32_t j = 0; j < c.size(); ++j)
            if (c[j].mntns == kv.first && c[j].valid) cont_map[c[j].mono].push_back(j);
        std::vector<uint64_t> stamps;
        for (const auto &e : enter_map) stamps.push_back(e.first);
        for (uint64_t ts : stamps) {
            const std::vector<uint32_t> enters = enter_map[ts];   // the slice the range statement took
            for (uint32_t e : enters) {
                Event ev{s[e].sort, e, TL_NO, 0, {}};
                for (int i = 0; i < TL_PARAMS; ++i) {
                    ev.cont[i] = TL_NO;
                    auto it = cont_map.find(ts);
                    if (it == cont_map.end()) continue;
                    for (uint32_t j : it->second)
                        if (c[j].index == i) {
                            ev.cont[i] = j;
                            break;
                        }
                }
                cont_map.erase(ts);
                if (s[e].id == NR[0] || s[e].id == NR[1] || s[e].id == NR[2]) {
                    enter_map.erase(ts);
                    out.push_back(ev);
                    continue;
                }
                auto xi = exit_map.find(ts);
                if (xi == exit_map.end()) continue;
                for (uint32_t x : xi->second) {
                    if (s[e].id != s[x].id || s[e].pid != s[x].pid) continue;
                    ev.exit = x;
                    enter_map.erase(ts);
                    exit_map.erase(ts);
                    out.push_back(ev);
                    break;
                }
            }
        }
        for (const auto &e : enter_map)
            for (uint32_t r : e.second) out.push_back(Event{s[r].sort, r, TL_NO, 1, {TL_NO, TL_NO, TL_NO, TL_NO, TL_NO, TL_NO}});
        for (const auto &e : exit_map)
            for (uint32_t r : e.second) out.push_back(Event{s[r].sort, r, TL_NO, 2, {TL_NO, TL_NO, TL_NO, TL_NO, TL_NO, TL_NO}});
    }
    order(out);
    return out;
}

// ---- the device's way ----------------------------------------------------------------------------
static TlSum tree(const std::vector<TlSum> &v, size_t lo, size_t hi, std::mt19937 &g) {
    if (hi == lo) return tl_identity();
    if (hi - lo == 1) return v[lo];
    const size_t mid = lo + 1 + g() % (hi - lo - 1);
    const TlSum a = tree(v, lo, mid, g), b = tree(v, mid, hi, g);
    return tl_combine(a, b);
}

static std::vector<Event> by_summary(const std::vector<Sys> &s, const std::vector<Cont> &c, std::mt19937 &g) {
    const uint32_t ns = (uint32_t)s.size(), n = ns + (uint32_t)c.size();
    std::vector<uint64_t> mn(n), ts(n), key(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (i < ns) {
            mn[i] = s[i].mntns, ts[i] = s[i].mono;
            key[i] = tl_key_sys(s[i].pid, s[i].id, s[i].typ, s[i].valid != 0);
        } else {
            mn[i] = c[i - ns].mntns, ts[i] = c[i - ns].mono;
            key[i] = tl_key_cont(c[i - ns].index, c[i - ns].valid != 0);
        }
    }
    std::vector<uint32_t> perm(n);
    for (uint32_t i = 0; i < n; ++i) perm[i] = i;
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
        return std::tie(mn[a], ts[a], key[a]) < std::tie(mn[b], ts[b], key[b]);
    });
    std::vector<uint32_t> code(n);
    std::vector<TlSum> el(n);
    for (uint32_t p = 0; p < n; ++p) {
        const uint32_t r = perm[p];
        bool gh = p == 0, sh = false;
        if (!gh) {
            const uint32_t q = perm[p - 1];
            gh = ts[r] != ts[q] || mn[r] != mn[q];
            sh = (key[r] >> 2) != (key[q] >> 2);
        }
        code[p] = tl_kind(key[r], NR[0], NR[1], NR[2]) | (gh ? TL_CODE_GH : 0u) | (gh || sh ? TL_CODE_SH : 0u);
        el[p] = tl_elem(r, code[p]);
    }
    // tiles of random sizes: summaries, carries
    std::vector<uint32_t> cut{0};
    const uint32_t maxtile = 1 + g() % (n > 1000 ? 300 : 9);
    while (cut.back() < n) cut.push_back(std::min(n, cut.back() + 1 + (uint32_t)(g() % maxtile)));
    std::vector<TlSum> carry(cut.size());
    TlSum run = tl_identity();
    for (size_t t = 0; t + 1 < cut.size(); ++t) {
        carry[t] = run;
        run = tl_combine(run, tree(el, cut[t], cut[t + 1], g));
    }
    // groups: the result at each group's last position, by group number; each row's group number
    std::vector<TlGroup> grp;
    std::vector<std::vector<uint32_t>> gcont;
    std::vector<uint32_t> gid(n);
    for (size_t t = 0; t + 1 < cut.size(); ++t) {
        for (uint32_t p = cut[t]; p < cut[t + 1]; ++p) {
            const TlSum st = tl_combine(carry[t], tree(el, cut[t], p + 1, g));
            gid[p] = st.ng - 1;
            if (p + 1 == n || (code[p + 1] & TL_CODE_GH)) {
                if (st.ng - 1 != grp.size()) {
                    std::printf("group number %u at position %u, expected %zu\n", st.ng - 1, p, grp.size());
                    std::exit(1);
                }
                grp.push_back(tl_final(st));
                gcont.push_back(std::vector<uint32_t>(st.c, st.c + TL_PARAMS));
            }
        }
    }
    std::vector<Event> out;
    for (uint32_t p = 0; p < n; ++p) {
        const uint32_t r = perm[p], k = code[p] & 7u;
        if (r >= ns) continue;
        const TlGroup &gr = grp[gid[p]];
        const uint32_t cl = tl_class(gr, r, k);
        if (cl == TL_DROP) continue;
        Event ev{s[r].sort, r, cl == 0 && gr.m == r ? gr.mx : TL_NO, cl, {}};
        for (int i = 0; i < TL_PARAMS; ++i) {
            const uint32_t v = cl == 0 && gr.e0 == r ? gcont[gid[p]][i] : TL_NO;
            ev.cont[i] = v == TL_NO ? TL_NO : v - ns;
        }
        out.push_back(ev);
    }
    order(out);
    return out;
}

static int check(const std::vector<Sys> &s, const std::vector<Cont> &c, std::mt19937 &g, const char *what, int iter) {
    const std::vector<Event> a = by_maps(s, c), b = by_summary(s, c, g);
    if (a.size() != b.size()) {
        std::printf("%s %d: %zu events by the maps, %zu by the summary\n", what, iter, a.size(), b.size());
        return 1;
    }
    for (size_t j = 0; j < a.size(); ++j)
        if (!(a[j] == b[j])) {
            std::printf("%s %d: event %zu: maps (row %u exit %u class %u), summary (row %u exit %u class %u)\n", what,
                        iter, j, a[j].row, a[j].exit, a[j].cls, b[j].row, b[j].exit, b[j].cls);
            return 1;
        }
    return 0;
}

static Sys S(uint64_t mono, uint8_t typ, uint16_t id, uint32_t pid, uint64_t sort = 0, uint64_t mntns = 1) {
    return Sys{mntns, mono, sort ? sort : mono, typ, id, pid, 1};
}

int main() {
    std::mt19937 g(20240);
    // the hand-worked groups (tests/test_traceloop_ref.py), alone and concatenated
    std::vector<std::pair<std::vector<Sys>, std::vector<Cont>>> table = {
        {{S(10, 0, 1, 7), S(10, 1, 1, 7)}, {{1, 10, 1, 1}, {1, 10, 0, 1}}},
        {{S(11, 0, 1, 7), S(11, 1, 1, 7)}, {{1, 11, 0, 1}, {1, 11, 0, 1}}},
        {{S(12, 0, 1, 7)}, {}},
        {{S(13, 1, 1, 7)}, {}},
        {{}, {{1, 14, 0, 1}, {1, 14, 1, 1}}},
        {{S(15, 0, 231, 7)}, {}},
        {{S(16, 0, 1, 7), S(16, 0, 2, 8), S(16, 1, 1, 7), S(16, 1, 2, 8)}, {}},
        {{S(17, 0, 1, 7), S(17, 0, 2, 8), S(17, 1, 2, 8)}, {{1, 17, 0, 1}}},
        {{S(18, 0, 231, 7), S(18, 0, 2, 8), S(18, 1, 2, 8)}, {{1, 18, 0, 1}}},
        {{S(19, 0, 231, 7), S(19, 1, 3, 9)}, {}},
        {{S(20, 0, 1, 7), S(20, 1, 1, 8)}, {}},
        {{S(21, 0, 1, 7), S(21, 1, 1, 7)}, {{1, 21, 6, 1}}},
        {{S(22, 0, 1, 7, 0, 1), S(22, 1, 1, 7, 0, 2)}, {}},
        {{S(23, 2, 1, 7), S(23, 1, 1, 7)}, {}},
        {{S(24, 0, 1, 7, 5), S(25, 0, 1, 7, 5)}, {}},
    };
    std::vector<Sys> all_s;
    std::vector<Cont> all_c;
    for (size_t t = 0; t < table.size(); ++t) {
        if (check(table[t].first, table[t].second, g, "table", (int)t + 1)) return 1;
        all_s.insert(all_s.end(), table[t].first.begin(), table[t].first.end());
        all_c.insert(all_c.end(), table[t].second.begin(), table[t].second.end());
    }
    if (check(all_s, all_c, g, "table", 0)) return 1;
    // random streams: few timestamps, few pids and ids, skip syscalls, dead rows, two containers
    for (int iter = 0; iter < 20000; ++iter) {
        const uint32_t ns = g() % 15, nc = g() % 7, nts = 1 + g() % 3, nmn = 1 + g() % 2;
        std::vector<Sys> s(ns);
        std::vector<Cont> c(nc);
        for (Sys &r : s) {
            r.mntns = 1 + g() % nmn;
            r.mono = 100 + g() % nts;
            r.sort = 1000 + g() % 4;
            r.typ = g() % 10 == 0 ? 2 : g() % 2;
            r.id = g() % 4 == 0 ? NR[g() % 3] : g() % 3;   // pid 0 with id 0..2: the conts' subgroups
            r.pid = g() % 3;
            r.valid = g() % 12 != 0;
        }
        for (Cont &r : c) {
            r.mntns = 1 + g() % nmn;
            r.mono = 100 + g() % nts;
            r.index = g() % 8;
            r.valid = g() % 12 != 0;
        }
        if (check(s, c, g, "random", iter)) return 1;
    }
    // single groups of thousands of rows
    for (int iter = 0; iter < 6; ++iter) {
        const uint32_t ns = 3000 + g() % 2000, nc = g() % 500;
        std::vector<Sys> s(ns);
        std::vector<Cont> c(nc);
        for (Sys &r : s) {
            r.mntns = 1;
            r.mono = 7;
            r.sort = 1000 + g() % 50;
            r.typ = iter == 1 ? 0 : g() % 2;
            r.id = iter < 3 && g() % 50 == 0 ? NR[g() % 3] : 1 + g() % 40;
            r.pid = 1 + g() % 40;
            r.valid = 1;
        }
        if (iter == 4)   // every exit belongs to another pid: nothing completes
            for (Sys &r : s) r.pid = r.typ ? 100 : 1;
        for (Cont &r : c) r = Cont{1, 7, (uint8_t)(g() % 7), 1};
        if (check(s, c, g, "large", iter)) return 1;
    }
    std::printf("TL_OK\n");
    return 0;
}
