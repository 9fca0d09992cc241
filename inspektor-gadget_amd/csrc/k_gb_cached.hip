// k_gb_cached.hip -- the group-by's cached form (kernel (2) for skewed streams) over the HBM
// table of k_gb_table.h: the LDS key cache, its two rings and both probers, k_groupby, AUTO's
// estimate of the cache's miss share (k_gb_estimate), the cache's seeds (k_gb_seeds), and their
// launchers (gb_launch_cached, gb_launch_estimate, gb_seeds_compute).
//
// Each workgroup (1024 threads, one per CU) keeps an LDS key cache: 8-way set associative
// on the key hash, entries hold the full key, its slot and the workgroup's partial aggregates;
// first come, never evicted, so the Zipf-hot keys settle in LDS and their events cost only
// their own input bytes plus LDS atomics.  A miss is resolved at once, while its row is in
// registers: HBM probe, adoption of a free LDS entry when its set has one, and otherwise
// its HBM updates go to the server wave through an LDS ring (see "HBM atomics through an
// LDS ring").  Eight waves stream rows, seven resolve misses, the sixteenth issues the atomics.  The
// cache is committed with HBM atomics at the end.
#include "k_gb_table.h"

namespace {

constexpr uint32_t ST_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t ST_BUSY = 0xFFFFFFFEu;
constexpr uint32_t GHOST = 1024;                 // admission filter entries (LDS)

template <int KW>
struct LdsCache {
    static constexpr int KP = (KW + 3) & ~3;   // key words padded to 16 B
    uint32_t *tag;     // E: 0 = empty, else the low hash word | 1 (set once, by the claimer)
    uint32_t *st;      // E: ST_EMPTY until published, then the HBM slot
    uint32_t *key;     // E x KP
    uint64_t *agg;     // naggs x E
    uint64_t *first;   // E
    uint32_t *ghost;   // GHOST recent miss tags (admission filter)
    uint32_t E;        // 8 x nsets
    uint32_t nsets;
};

// full key compare: every quad is loaded before any is compared (a short-circuit compare
// becomes one LDS round trip per quad)
template <int KW>
__device__ __forceinline__ bool lds_key_eq(const LdsCache<KW> &c, uint32_t e, const uint32_t (&k)[KW]) {
    constexpr int NQ = LdsCache<KW>::KP / 4;
    const uint4 *p = reinterpret_cast<const uint4 *>(c.key) + (uint64_t)e * (LdsCache<KW>::KP / 4);
    uint4 q[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) q[i] = p[i];
    // the padding words are compared too (lds_adopt zeroes them): the loads stay whole
    // 16-byte reads instead of being narrowed to the key's words and split
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        diff |= q[i].x ^ (4 * i + 0 < KW ? k[4 * i + 0] : 0u);
        diff |= q[i].y ^ (4 * i + 1 < KW ? k[4 * i + 1] : 0u);
        diff |= q[i].z ^ (4 * i + 2 < KW ? k[4 * i + 2] : 0u);
        diff |= q[i].w ^ (4 * i + 3 < KW ? k[4 * i + 3] : 0u);
    }
    asm volatile("" : "+v"(diff));   // keep the OR of XORs: LLVM splits `== 0` into per-word compares
    return diff == 0;
}

// The cached kernel's stream loads: non-temporal, so the event stream does not push the
// table's key records out of the caches -- except for the top-file key, whose kernel is faster
// with plain loads (C5 5.94-5.98 -> 5.84 ms with a plain-load build, C2 3.7 -> 4.0).
template <class L>
constexpr bool cached_stream_nt() { return !std::is_same<L, StaticLayout<8, 4, 4, 4>>::value; }

// The LDS cache is 8-way set associative: the key hash's high word picks a set of 8
// consecutive entries, its low word (| 1) is the entry's tag.  A lookup reads the set's 8
// tags with two 16-byte LDS loads and compares full keys only on a tag match, so a miss
// costs two LDS reads, not a walk.  Entries are first come, never evicted: the claimer
// CASes the tag from 0, writes the key, then publishes the HBM slot in `st` (release); a
// reader that matches a tag but still sees ST_EMPTY treats it as a miss (its event takes
// the HBM path, which is only slower).
__device__ __forceinline__ uint32_t lds_tag(uint64_t h) { return (uint32_t)h | 1u; }

template <int KW>
__device__ __forceinline__ uint32_t lds_set(const LdsCache<KW> &c, uint64_t h) {
    return (uint32_t)(((h >> 32) * (uint64_t)c.nsets) >> 32) * 8u;
}

template <int KW>
__device__ __forceinline__ void lds_tags(const LdsCache<KW> &c, uint32_t base, uint32_t (&tg)[8]) {
    const uint4 t0 = *reinterpret_cast<const uint4 *>(c.tag + base);
    const uint4 t1 = *reinterpret_cast<const uint4 *>(c.tag + base + 4);
    tg[0] = t0.x; tg[1] = t0.y; tg[2] = t0.z; tg[3] = t0.w;
    tg[4] = t1.x; tg[5] = t1.y; tg[6] = t1.z; tg[7] = t1.w;
}

// `closed`: the set can never hold this key in this launch -- all 8 tags are set (a tag is set once
// and entries are never evicted) and none is the key's.  A matching tag whose entry is not yet
// published is an adoption in flight, possibly of this key: not closed.
template <int KW>
__device__ __forceinline__ int lds_lookup(const LdsCache<KW> &c, const uint32_t (&k)[KW], uint64_t h, uint32_t &gs,
                                          bool &closed) {
    const uint32_t base = lds_set(c, h), t = lds_tag(h);
    uint32_t tg[8];
    lds_tags(c, base, tg);
    uint32_t m = 0, open = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        m |= (tg[j] == t ? 1u : 0u) << j;
        open |= (tg[j] == 0 ? 1u : 0u);
    }
    closed = !m && !open;
    while (m) {   // usually zero or one candidate
        const uint32_t e = base + (uint32_t)(__builtin_ffs((int)m) - 1);
        m &= m - 1;
        const uint32_t s = __hip_atomic_load(&c.st[e], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (s < ST_BUSY && lds_key_eq<KW>(c, e, k)) {
            gs = s;
            return (int)e;
        }
    }
    return -1;
}

template <int KW>
__device__ __forceinline__ int lds_lookup(const LdsCache<KW> &c, const uint32_t (&k)[KW], uint64_t h, uint32_t &gs) {
    bool closed;
    return lds_lookup<KW>(c, k, h, gs, closed);
}

// adopt a free entry of the key's set for a key just resolved in HBM
// Admission filter of the LDS cache.  Entries are never evicted, so admitting every missing
// key fills the cache with whichever keys come first, and the Zipf tail -- rare keys, but
// most of the misses together -- takes most entries.  A key is admitted on its second miss
// seen through a direct-mapped table of recent miss tags (GHOST entries): a tail key is
// overwritten before it misses again, a mid-frequency key is not.  (Simulated on the C2
// stream: 60 % -> 67 % LDS hits per CU at 1 088 entries; ideal LFU per set is 69 %.)
template <int KW>
__device__ __forceinline__ bool ghost_admit(const GbArgs &a, const LdsCache<KW> &c, uint64_t h) {
    if (!a.admit_mask) return true;
    // entry = tag (low 2 bits cleared) | misses seen before this one (0..3)
    const uint32_t g = (uint32_t)(h >> 20) & (GHOST - 1), t = lds_tag(h) & ~3u;
    const uint32_t cur = c.ghost[g];
    if ((cur & ~3u) == t) {
        const uint32_t seen = (cur & 3u) + 1u;
        if (seen >= a.admit_mask) return true;
        c.ghost[g] = t | seen;
        return false;
    }
    c.ghost[g] = t;   // racing writers: either tag wins, both outcomes are valid
    return false;
}

template <int KW>
__device__ __forceinline__ int lds_adopt(const LdsCache<KW> &c, const uint32_t (&k)[KW], uint64_t h, uint32_t gs) {
    const uint32_t base = lds_set(c, h);
    uint32_t tg[8];
    lds_tags(c, base, tg);
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) m |= (tg[j] == 0 ? 1u : 0u) << j;
    if (!m) return -1;   // set full
    const uint32_t e = base + (uint32_t)(__builtin_ffs((int)m) - 1);
    if (atomicCAS(&c.tag[e], 0u, lds_tag(h)) != 0u) return -1;   // lost the race: HBM path
    uint4 *kp = reinterpret_cast<uint4 *>(c.key) + (uint64_t)e * (LdsCache<KW>::KP / 4);
#pragma unroll
    for (int i = 0; i < LdsCache<KW>::KP / 4; ++i)
        kp[i] = make_uint4(4 * i + 0 < KW ? k[4 * i + 0] : 0u, 4 * i + 1 < KW ? k[4 * i + 1] : 0u,
                           4 * i + 2 < KW ? k[4 * i + 2] : 0u, 4 * i + 3 < KW ? k[4 * i + 3] : 0u);
    __hip_atomic_store(&c.st[e], gs, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    return (int)e;
}

template <int KW, int NA>
__device__ __forceinline__ void lds_accumulate(const GbArgs &a, const LdsCache<KW> &c, int slot,
                                               const uint64_t (&v)[NA], uint64_t gidx) {
#pragma unroll
    for (int x = 0; x < NA; ++x)
        if (x < (int)a.naggs && v[x])
            atomicAdd(reinterpret_cast<unsigned long long *>(&c.agg[x * c.E + slot]), (unsigned long long)v[x]);
    // rows arrive nearly in index order: a plain read skips most of the minima
    if (gidx < c.first[slot]) atomicMin(reinterpret_cast<unsigned long long *>(&c.first[slot]), (unsigned long long)gidx);
}

// ---- HBM atomics through an LDS ring ---------------------------------------------------
// A wave's vmcnt counts its stores and atomics with its loads, in issue order, so a miss's
// memory-side atomics delayed that wave's next load wait by their whole acknowledgement
// latency (longer than a load's).  Producer waves therefore push each HBM update as a
// 16-byte ring entry {slot, lap|what, value} into LDS, and one server wave per workgroup
// issues them; it loads nothing, so nothing ever waits on their acknowledgement.
constexpr uint32_t ARING = 512;             // HBM-update ring entries (16 B each)
constexpr uint32_t WHAT_MIN = 15;           // entry kind: atomicMin on `first`
// (Round 6 tried padding each lane's run of entries so that no miss's updates straddle an 8-lane
// group of the server's instruction: the memory-side atomic requests fell by 1M of the 7M that
// grouping predicted, and the kernels did not get faster -- DESIGN.md §4, "Round 6: the
// memory-side atomics".  Not kept.)

struct Ring {
    uint2 *lo;            // {slot, (lap << 4) | what}
    uint64_t *hi;         // value
    uint32_t *ctl;        // [0] tail (reserved), [1] head (consumed), [2] producer waves done
};

__device__ __forceinline__ uint32_t ring_lap(uint32_t p) { return (p / ARING + 1u) << 4; }

// Push this lane's HBM updates (the aggregates it adds, and a first-index minimum when
// gidx < first_ins) for slot gs.  Called by the active (missing) lanes of a producer wave.
template <int NA>
__device__ __forceinline__ void ring_push(const GbArgs &a, const Ring &r, uint32_t gs, const uint64_t (&v)[NA],
                                          uint64_t gidx, uint64_t first_ins) {
    if (a.direct) {   // the prober issues its own atomics (no server wave)
#pragma unroll
        for (int x = 0; x < NA; ++x)
            if (x < (int)a.naggs && v[x]) gadd(rec_agg(a, gs, x), (unsigned long long)v[x]);
        if (gidx < first_ins) gmin(rec_first(a, gs), (unsigned long long)gidx);
        return;
    }
    // A lane's entries are consecutive in the ring, so the server issues one slot's updates
    // from adjacent lanes of one instruction: they fall in the slot's value record, one 64-B
    // line, and leave the CU as one memory-side atomic request instead of one per update
    // (top file: count and bytes of the same op, two updates per miss).
    bool has[NA + 1];
    uint32_t c = 0;
#pragma unroll
    for (int x = 0; x <= NA; ++x) {
        has[x] = x < NA ? (x < (int)a.naggs && v[x] != 0) : gidx < first_ins;
#ifdef IGX_DIAG_NO_SUM_PUSH   // diagnostic build only (wrong sums): the bound of the logged sums' whole path
        if (x < NA && a.log && (v[x < NA ? x : 0] >> 32) == 0 && gs < LOG_SLOT_LIMIT) has[x] = false;
#endif
#ifdef IGX_DIAG_HALF_ATOMICS   // diagnostic build only (wrong sums): the bound of one atomic per miss
        if (NA == 4 && (x == 1 || x == 3)) has[x] = false;
#endif
        c += has[x] ? 1u : 0u;
    }
    const uint64_t lt = lanemask_lt();
    uint32_t pre = 0, total = 0;   // wave prefix / total of c (c <= NA + 1 <= 5: three bits)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const uint64_t m = __ballot((c >> b) & 1u);
        pre += (uint32_t)__popcll(m & lt) << b;
        total += (uint32_t)__popcll(m) << b;
    }
    if (!total) return;
    const uint64_t active = __ballot(true);
    const uint32_t leader = (uint32_t)__ffsll((long long)active) - 1;
    uint32_t base = 0;
    if ((threadIdx.x & 63) == leader) base = atomicAdd(&r.ctl[0], total);
    base = __shfl(base, (int)leader);
    // wait for room: the server frees entries as it issues them
    uint32_t spins = 0;
    for (; base + total - __hip_atomic_load(&r.ctl[1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) > ARING;) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > SPIN_LIMIT) { atomicOr(a.err, 16u); return; }   // never expected: fail, do not hang
    }
    if ((a.dbg & 65536u) && spins && (threadIdx.x & 63) == leader)
        atomicAdd(a.dbg_cnt + 6, 1ull * spins);   // prober: update ring full
    uint32_t p = base + pre;
#pragma unroll
    for (int x = 0; x <= NA; ++x) {
        if (has[x]) {
            r.hi[p % ARING] = x < NA ? v[x] : gidx;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            r.lo[p % ARING] = make_uint2(gs, ring_lap(p) | (x < NA ? (uint32_t)x : WHAT_MIN));
            ++p;
        }
    }
}

// Diagnostics (IGX_GB_DEBUG bit 18, the debug kernels only): what one wave-wide atomic
// instruction becomes at the memory side, counted into dbg_cnt[base ..]: +0 lanes, +1 of them
// minima, +2 distinct (value record, opcode) pairs -- the L2 sends a record's same-opcode lanes
// of one instruction as one request --, +3 distinct (128-B line, opcode) pairs,
// +4 instructions whose first record continues the previous instruction's last (a miss's
// updates split over two instructions).  Kept per wave in registers, added at the end.
__device__ __forceinline__ void atomics_account(const GbArgs &a, bool live, uint32_t slot, bool is_min, uint32_t lane,
                                                uint32_t base) {
    uint64_t todo = __ballot(live);
    if (!todo) return;
    const uint64_t nmin = (uint64_t)__popcll(__ballot(live && is_min));
    uint64_t recs = 0, lines = 0;
    const uint32_t per_line = max(1u, 128u / (a.vrec_words * 8));
    while (todo) {
        const uint32_t l = (uint32_t)__ffsll((long long)todo) - 1;
        const uint32_t s0 = __shfl(slot, (int)l), k0 = __shfl((uint32_t)is_min, (int)l);
        todo &= ~__ballot(live && slot == s0 && (uint32_t)is_min == k0);
        ++recs;
    }
    todo = __ballot(live);
    while (todo) {
        const uint32_t l = (uint32_t)__ffsll((long long)todo) - 1;
        const uint32_t s0 = __shfl(slot, (int)l) / per_line, k0 = __shfl((uint32_t)is_min, (int)l);
        todo &= ~__ballot(live && slot / per_line == s0 && (uint32_t)is_min == k0);
        ++lines;
    }
    const uint64_t nlive = (uint64_t)__popcll(__ballot(live));
    if (lane == 0) {
        atomicAdd(a.dbg_cnt + base, (unsigned long long)nlive);
        atomicAdd(a.dbg_cnt + base + 1, (unsigned long long)nmin);
        atomicAdd(a.dbg_cnt + base + 2, (unsigned long long)recs);
        atomicAdd(a.dbg_cnt + base + 3, (unsigned long long)lines);
    }
}

// the server wave: issue ring entries in order until every producer is done and the ring
// is empty
template <bool DBG>
__device__ __forceinline__ void ring_serve(const GbArgs &a, const Ring &r, uint32_t lane) {
    uint32_t head = 0;
    [[maybe_unused]] uint32_t prev_last = 0xFFFFFFFFu;   // diagnostics: the last record of the previous instruction
    // The update log (k_gb_log.hip): a batch's sums leave as one contiguous wave store of 8-byte
    // records into this workgroup's region instead of as atomics.  This wave is the region's only
    // writer, so lpos is its cursor.  A minimum, a value of 2^32 or more, a slot the record cannot
    // hold and every entry of a batch the region has no room for go out as atomics as before; in a
    // logged batch such an entry's position holds a null record, so positions stay dense.
    const bool logging = !DBG && a.log != nullptr;
    uint64_t *lg = a.log + (uint64_t)blockIdx.x * a.log_cap;
    uint32_t lpos = 0, n_logged = 0, n_value = 0, n_full = 0;
    for (;;) {
        const uint32_t t = __hip_atomic_load(&r.ctl[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (t == head) {
            if (__hip_atomic_load(&r.ctl[2], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == NWAVES - 1 - a.nl &&
                __hip_atomic_load(&r.ctl[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == head)
                break;
            __builtin_amdgcn_s_sleep(2);   // idle until the probers push or finish (no limit:
            if (DBG && (a.dbg & 65536u) && lane == 0) atomicAdd(a.dbg_cnt + 7, 1ull);   // server idle
            continue;                      // they bound their own waits)
        }
        const uint32_t n = min(t - head, 64u);
        const bool room = logging && lpos + n <= a.log_cap;
        uint32_t slot = 0xFFFFFFFFu, what = 0;
        if (lane < n) {
            const uint32_t p = head + lane;
            uint64_t w;
            uint32_t spins = 0;
            while (((uint32_t)((w = __hip_atomic_load(reinterpret_cast<uint64_t *>(&r.lo[p % ARING]),
                                                      __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) >> 32) &
                    ~15u) != ring_lap(p)) {
                __builtin_amdgcn_s_sleep(1);
                if (++spins > SPIN_LIMIT) { atomicOr(a.err, 16u); break; }
            }
            const uint64_t val = r.hi[p % ARING];
            slot = (uint32_t)w;
            what = (uint32_t)(w >> 32) & 15u;
            bool logged = false;
            if (logging && what != WHAT_MIN) {
                const bool small = (val >> 32) == 0;
                const bool fits = small && slot < LOG_SLOT_LIMIT;
                if (!small) ++n_value;
                if (fits && !room) ++n_full;
                logged = fits && room;
                n_logged += logged ? 1u : 0u;
            }
            if (room)
                __builtin_nontemporal_store(logged ? log_record(slot, what, (uint32_t)val) : ~0ull, lg + lpos + lane);
            if (logged) {   // the reduce pass adds it
            } else if (DBG && (a.dbg & 131072u)) {   // diagnostics: plain stores instead of the atomics
                if (what == WHAT_MIN) *rec_first(a, slot) = val;
                else *rec_agg(a, slot, (int)what) = val;
            } else if (!(DBG && (a.dbg & 4u))) {
                if (what == WHAT_MIN) gmin(rec_first(a, slot), val);
#ifndef IGX_DIAG_NO_SERVER_ADDS   // diagnostic build only (wrong sums): what the server's adds cost
                else gadd(rec_agg(a, slot, (int)what), val);
#else
                else asm volatile("" ::"v"(val));   // the ring read stays
#endif
            }
        }
        if (DBG && (a.dbg & 262144u)) {
            const bool live = lane < n;
            atomics_account(a, live, slot, what == WHAT_MIN, lane, 8);
            // the same pairs split at 32-, 16- and 8-lane boundaries: which grouping of the
            // instruction's lanes the memory-side request count follows
            for (uint32_t g = 0; g < 3; ++g) {
                const uint32_t sh = 5 - g;
                uint64_t todo = __ballot(live);
                uint64_t cnt = 0;
                while (todo) {
                    const uint32_t l = (uint32_t)__ffsll((long long)todo) - 1;
                    const uint32_t s0 = __shfl(slot, (int)l), k0 = __shfl(what == WHAT_MIN ? 1u : 0u, (int)l);
                    todo &= ~__ballot(live && slot == s0 && (what == WHAT_MIN ? 1u : 0u) == k0 && (lane >> sh) == (l >> sh));
                    ++cnt;
                }
                if (lane == 0) atomicAdd(a.dbg_cnt + 13 + g, (unsigned long long)cnt);
            }
            const uint32_t first_slot = __shfl(slot, 0), last_slot = __shfl(slot, (int)(n - 1));
            if (lane == 0 && first_slot == prev_last) atomicAdd(a.dbg_cnt + 12, 1ull);
            prev_last = last_slot;
        }
        head += n;
        if (room) lpos += n;
        if (lane == 0) __hip_atomic_store(&r.ctl[1], head, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (logging) {
        for (int o = 32; o > 0; o >>= 1) {
            n_logged += __shfl_xor(n_logged, o);
            n_value += __shfl_xor(n_value, o);
            n_full += __shfl_xor(n_full, o);
        }
        if (lane == 0) {
            a.log_cnt[blockIdx.x] = lpos;
            unsigned long long *st = reinterpret_cast<unsigned long long *>(a.err) + LOG_STAT_WORD;
            if (n_logged) atomicAdd(st, (unsigned long long)n_logged);
            if (n_value) atomicAdd(st + 1, (unsigned long long)n_value);
            if (n_full) atomicAdd(st + 2, (unsigned long long)n_full);
        }
    }
}

// ---- loader -> prober hand-off: the miss ring -----------------------------------------
// A loader that misses the LDS cache does not probe HBM itself (its next row would wait
// for the probe's round trip): it writes the row's key, hash, index and aggregate values
// into a ring cell and moves on.  Prober waves take 64 cells at a time and resolve them.
// Cells follow the bounded MPMC sequence protocol: cell i starts with seq = i; the
// producer of position p waits for seq == p, fills the cell and sets seq = p + 1; the
// consumer of p waits for seq == p + 1, reads the cell and sets seq = p + MRING.
constexpr uint32_t MRING = 256;
constexpr uint32_t CELL_CLOSED = 1u << 31;   // in a cell's high index word: the key's LDS set is closed

template <int KW, int NA>
struct MissRing {
    static constexpr int KQ = LdsCache<KW>::KP / 4;          // key quads
    static constexpr int EQ = KQ + 1 + (NA + 1) / 2;         // + {hash, index} + values
    uint4 *cell;      // MRING x EQ
    uint32_t *seq;    // MRING
    uint32_t *ctl;    // [0] tail (reservations), [1] head (claims), [2] loader waves done
    uint32_t *err;
    unsigned long long *waits;   // diagnostics (IGX_GB_DEBUG bit 16): sleep counts, else null
};

template <int KW, int NA>
__device__ __forceinline__ void miss_push(const MissRing<KW, NA> &m, const uint32_t (&k)[KW], uint64_t h,
                                          uint64_t gidx, const uint64_t (&v)[NA], bool closed) {
    const uint64_t active = __ballot(true);
    const uint32_t leader = (uint32_t)__ffsll((long long)active) - 1;
    uint32_t base = 0;
    if ((threadIdx.x & 63) == leader) base = atomicAdd(&m.ctl[0], (uint32_t)__popcll(active));
    base = __shfl(base, (int)leader);
    const uint32_t p = base + (uint32_t)__popcll(active & lanemask_lt());
    uint32_t *sq = &m.seq[p % MRING];
    uint32_t spins = 0;
    for (; __hip_atomic_load(sq, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != p;) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > SPIN_LIMIT) { atomicOr(m.err, 16u); return; }
    }
    if (m.waits && spins) atomicAdd(m.waits + 4, (unsigned long long)spins);   // loader: ring full
    uint4 *cl = m.cell + (uint64_t)(p % MRING) * MissRing<KW, NA>::EQ;
#pragma unroll
    for (int q = 0; q < MissRing<KW, NA>::KQ; ++q)
        cl[q] = make_uint4(4 * q + 0 < KW ? k[4 * q + 0] : 0u, 4 * q + 1 < KW ? k[4 * q + 1] : 0u,
                           4 * q + 2 < KW ? k[4 * q + 2] : 0u, 4 * q + 3 < KW ? k[4 * q + 3] : 0u);
    // the loader's `closed` rides in the index word's top bit (indices stay below IDX_LIMIT = 2^48)
    cl[MissRing<KW, NA>::KQ] = make_uint4((uint32_t)h, (uint32_t)(h >> 32), (uint32_t)gidx,
                                          (uint32_t)(gidx >> 32) | (closed ? CELL_CLOSED : 0u));
#pragma unroll
    for (int x = 0; x < NA; x += 2) {
        const uint64_t v1 = x + 1 < NA ? v[x + 1] : 0ull;
        cl[MissRing<KW, NA>::KQ + 1 + x / 2] = make_uint4((uint32_t)v[x], (uint32_t)(v[x] >> 32), (uint32_t)v1,
                                                          (uint32_t)(v1 >> 32));
    }
    __hip_atomic_store(sq, p + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// A miss whose cell says `closed` skips the second lookup, the admission filter and the adoption
// attempt (none can succeed: the set is full of other keys for the rest of the launch) and goes
// straight to the probe and the update ring; either way its sums are added and its index is a
// candidate minimum, so the result does not depend on the bit.
// Probers resolve PB misses per lane at a time (PB = 1: two per lane measured slower -- C5
// 6.41 -> 6.72-6.80 ms, C2 unchanged, and for the 72-B key they spill): the LDS cache again (a prober may have adopted the key since), then
// the HBM table, then adoption of a free LDS entry or the HBM-update ring.

template <int KW, int NA>
struct MissRow {
    uint32_t k[KW];
    uint64_t h, gidx;
    uint64_t v[NA];
    uint32_t closed;   // non-zero: the loader saw the key's LDS set full of other keys (no lookup, no adoption)
};

template <int KW, int NA>
__device__ __forceinline__ void read_cell(const MissRing<KW, NA> &m, uint32_t p, MissRow<KW, NA> &x) {
    const uint4 *cl = m.cell + (uint64_t)(p % MRING) * MissRing<KW, NA>::EQ;
#pragma unroll
    for (int q = 0; q < MissRing<KW, NA>::KQ; ++q) {
        const uint4 t = cl[q];
        if (4 * q + 0 < KW) x.k[4 * q + 0] = t.x;
        if (4 * q + 1 < KW) x.k[4 * q + 1] = t.y;
        if (4 * q + 2 < KW) x.k[4 * q + 2] = t.z;
        if (4 * q + 3 < KW) x.k[4 * q + 3] = t.w;
    }
    const uint4 hq = cl[MissRing<KW, NA>::KQ];
    x.h = (uint64_t)hq.x | ((uint64_t)hq.y << 32);
    x.gidx = (uint64_t)hq.z | ((uint64_t)(hq.w & ~CELL_CLOSED) << 32);
    x.closed = hq.w & CELL_CLOSED;
#ifdef IGX_DIAG_CLOSED_SKIP_ALL   // diagnostic build only: every miss skips the LDS work (nothing is adopted)
    x.closed = CELL_CLOSED;
#endif
#pragma unroll
    for (int i = 0; i < NA; i += 2) {
        const uint4 t = cl[MissRing<KW, NA>::KQ + 1 + i / 2];
        x.v[i] = (uint64_t)t.x | ((uint64_t)t.y << 32);
        if (i + 1 < NA) x.v[i + 1] = (uint64_t)t.z | ((uint64_t)t.w << 32);
    }
}

// The state-machine prober: every lane owns one miss and advances it by one step per round
// trip, so a lane that has to claim a record (CAS, then key / value stores, then `ready`)
// does not hold the other 63 lanes for the extra round trips.  Per iteration: free lanes
// take cells from the miss ring; lanes in PROBE load their slot's record, lanes in CASQ
// issue their claim; one wait covers all of it (and the previous iteration's stores); then
// PUB lanes publish, CAS lanes act on the result, PROBE lanes read their record.
// States: FREE -> PROBE -> (found: FREE) | (empty: CASQ -> CAS -> (won: PUB -> FREE) |
// (lost: PROBE)).
template <int KW, int NA, bool DBG>
__device__ __forceinline__ void finish_miss(const GbArgs &a, const LdsCache<KW> &c, const Ring &r,
                                            const MissRow<KW, NA> &x, uint32_t gs, uint64_t first_ins,
                                            bool claimed = false) {
    const int ad = !x.closed && ghost_admit<KW>(a, c, x.h) ? lds_adopt<KW>(c, x.k, x.h, gs) : -1;
    if (claimed) return;   // the claim wrote this event's values into the new record
    if (ad >= 0) lds_accumulate<KW, NA>(a, c, ad, x.v, x.gidx);
    else ring_push<NA>(a, r, gs, x.v, x.gidx, first_ins);
}

// A kept key's first miss of the interval (its `ready` carries an earlier epoch of the
// generation): `ready` takes the interval's epoch and first_ins = gidx + 1 -- an upper bound the
// value record will meet, because this event's own minimum is pushed (gidx < first_ins) -- and
// the slot is marked occupied.  Racing re-stamps of one key each push their own minimum, so
// whichever `ready` lands, every later reader's first_ins is met.  Returns the first_ins to use.
template <int KW>
__device__ __forceinline__ uint64_t restamp(const GbArgs &a, uint64_t s, uint64_t gidx) {
    if (gidx >= IDX_LIMIT) {   // an index column value that `ready` cannot carry
        atomicOr(a.err, 8u);
        return READY_IDX;          // still correct: every event pushes its minimum
    }
    st_agent(reinterpret_cast<uint64_t *>(a.krec + s * a.krec_len + koff_of(KW) + 8), (a.ep << 48) | (gidx + 2));
    __builtin_nontemporal_store((uint8_t)1, a.occb + s);
    return gidx + 1;
}

template <int KW, int NA, bool DBG>
__device__ __forceinline__ void prober_sm(const GbArgs &a, const LdsCache<KW> &c, const Ring &r,
                                          const MissRing<KW, NA> &m, uint32_t lane, uint32_t gep,
                                          uint32_t *nclaim) {
    constexpr uint32_t KOFF = koff_of(KW);
    constexpr int NQ = probe_quads<KW>();
    constexpr uint32_t FREE = 0, PROBE = 1, CASQ = 2, PUB = 3;
    const __amdgpu_buffer_rsrc_t rs = rec_rsrc(a);
    MissRow<KW, NA> x;
    uint32_t st = FREE, s = 0, probes = 0, tries = 0, reread = 0;
    uint64_t expect = 0;
    for (uint32_t idle = 0;;) {
        // 1. refill the free lanes with cells the loaders have reserved
        const uint64_t fm = __ballot(st == FREE);
        bool drained = false;
        if (fm) {
            const uint32_t tail = __hip_atomic_load(&m.ctl[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
            const bool done = __hip_atomic_load(&m.ctl[2], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == a.nl;
            const uint32_t head = __hip_atomic_load(&m.ctl[1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
            const uint32_t avail = (int32_t)(tail - head) > 0 ? tail - head : 0u;
            const uint32_t want = min((uint32_t)__popcll(fm), avail);
            drained = done && avail == 0;
            if (want) {
                const uint32_t leader = (uint32_t)__ffsll((long long)fm) - 1;
                uint32_t base = 0;
                if (lane == leader) base = atomicAdd(&m.ctl[1], want);
                base = __shfl(base, (int)leader);
                const uint32_t rank = (uint32_t)__popcll(fm & lanemask_lt());
                if (st == FREE && rank < want) {
                    const uint32_t p = base + rank;
                    uint32_t *sq = &m.seq[p % MRING];
                    bool have = true;
                    for (uint32_t spins = 0;
                         __hip_atomic_load(sq, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != p + 1;) {
                        if (__hip_atomic_load(&m.ctl[2], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == a.nl &&
                            p >= __hip_atomic_load(&m.ctl[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                            have = false;   // over-claimed past the end of a finished stream
                            break;
                        }
                        __builtin_amdgcn_s_sleep(1);
                        if (++spins > SPIN_LIMIT) { atomicOr(a.err, 16u); have = false; break; }
                    }
                    if (have) {
                        read_cell<KW, NA>(m, p, x);
                        __hip_atomic_store(sq, p + MRING, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                        uint32_t gs = SLOT_OVF;
                        const int slot = x.closed ? -1 : lds_lookup<KW>(c, x.k, x.h, gs);   // adopted meanwhile?
                        if (slot >= 0) {
                            lds_accumulate<KW, NA>(a, c, slot, x.v, x.gidx);
                        } else {
                            st = PROBE;
                            s = (uint32_t)home_slot(a, x.h);
                            probes = 0;
                            tries = 0;
                            reread = 0;
                        }
                    }
                }
            }
        }
        const uint64_t busy = __ballot(st != FREE);
        if (!busy) {
            if (drained) break;
            __builtin_amdgcn_s_sleep(1);   // waiting for misses: as long as the stream lasts
            if (++idle > SPIN_LIMIT) { atomicOr(a.err, 16u); break; }
            continue;
        }
        idle = 0;
        // 2. issue this round trip's loads and claims
        const uint64_t tag = (x.h & ~EP_MAX) | gep;
        uint8_t *rec = a.krec + (uint64_t)s * a.krec_len;
        uint32_t d[NQ * 4];
        uint64_t cas_old = 0;
        const bool probed = st == PROBE;   // only these lanes have a record in d this round
        if (probed) load_rec<NQ>(rs, s * a.krec_len, d);
        if (st == CASQ)
            cas_old = atomicCAS(reinterpret_cast<unsigned long long *>(rec + KOFF), (unsigned long long)expect,
                                (unsigned long long)tag);
        // 3. one wait: probe data, claims, and the previous iteration's stores
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // 4. publish the records claimed last iteration (their stores are now complete)
        if (st == PUB) {
            st_agent(reinterpret_cast<uint64_t *>(rec + KOFF + 8), (a.ep << 48) | (x.gidx + 1));
            __builtin_nontemporal_store((uint8_t)1, a.occb + s);
            finish_miss<KW, NA, DBG>(a, c, r, x, s, x.gidx, true);
            st = FREE;
        }
        // 5. claims: won -> write key and value record now, publish next iteration
        if (st == CASQ) {
            if (cas_old == expect) {
#pragma unroll
                for (int w = 0; w < KW; w += 2) {
                    if (w + 1 < KW)
                        st_agent(reinterpret_cast<uint64_t *>(rec + 4 * w), (uint64_t)x.k[w] | ((uint64_t)x.k[w + 1] << 32));
                    else
                        st_agent(reinterpret_cast<uint32_t *>(rec + 4 * w), x.k[w]);
                }
                vrec_init<NA>(a, s, x.gidx, x.v);   // with this event's own values (finish_miss skips them)
                st = PUB;
            } else if (cas_old == tag) {
                st = PROBE;   // lost to a claim of the same hash: read its key once `ready` is set
                if (++tries > (1u << 18)) { atomicOr(a.err, 2u); st = FREE; }
            } else {
                st = PROBE;   // lost to another key (the CAS saw the current tag): next slot
                reread = 0;
                s = (uint32_t)next_slot(a, s);
                if (++probes >= a.max_probe) { atomicOr(a.err, 4u); st = FREE; }
            }
        }
        {   // this round's claims (every earlier PUB lane published in step 4)
            const uint64_t pub = __ballot(st == PUB);
            if (pub && lane == 0) atomicAdd(nclaim, (uint32_t)__popcll(pub));
        }
        // 6. probe results (lanes that lost a claim in step 5 read their record next round)
        if (probed && st == PROBE) {
            const uint64_t t = (uint64_t)d[KOFF / 4] | ((uint64_t)d[KOFF / 4 + 1] << 32);
            const uint64_t ready = (uint64_t)d[KOFF / 4 + 2] | ((uint64_t)d[KOFF / 4 + 3] << 32);
            if ((t & EP_MAX) != gep) {
                expect = t;          // empty in this generation: claim it next round trip
                st = CASQ;
                if (++tries > (1u << 18)) { atomicOr(a.err, 2u); st = FREE; }
            } else if (t == tag) {
                if (!ready_pub(ready, gep, a.ep)) {
                    if (++tries > (1u << 18)) { atomicOr(a.err, 2u); st = FREE; }   // the claimer is still writing
                } else {
                    bool eq = true;
#pragma unroll
                    for (int w = 0; w < KW; ++w) eq = eq && (d[w] == x.k[w]);
                    if (eq) {
                        const uint64_t fi = (ready >> 48) == a.ep ? (ready & READY_IDX) - 1 : restamp<KW>(a, s, x.gidx);
                        finish_miss<KW, NA, DBG>(a, c, r, x, s, fi);
                        st = FREE;
                    } else if (!reread) {
                        reread = 1;  // the key quads may predate `ready`: read once more
                        ++tries;
                    } else {
                        reread = 0;
                        s = (uint32_t)next_slot(a, s);
                        if (++probes >= a.max_probe) { atomicOr(a.err, 4u); st = FREE; }
                    }
                }
            } else {
                reread = 0;
                s = (uint32_t)next_slot(a, s);
                if (++probes >= a.max_probe) { atomicOr(a.err, 4u); st = FREE; }
            }
        }
    }
}

// Cooperative claim stores (the whole wave calls it; `claim` marks the lanes that won a
// slot's tag this round).  A claimer's key record (key words, padding, tag) and value record
// (first = its event index, its own values) are spread over the wave -- lane l writes quad
// l % CQ of the (l / CQ)-th claim of the round -- so each record leaves as one store
// instruction's adjacent 16-B pieces: one write-through request per 64 B, instead of a request
// per 16-B store of a lane writing its record alone (C5: 5 of a claim's 8 requests, C2: 7 of 10).
// Ends with s_waitcnt vmcnt(0): the records are visible before the claimers publish `ready`.
template <int KW, int NA, bool WAIT = true>
__device__ __forceinline__ void claim_store_coop(const GbArgs &a, bool claim, uint32_t s, const uint32_t (&k)[KW],
                                                 uint64_t tag, uint64_t gidx, const uint64_t (&v)[NA]) {
    constexpr uint32_t KOFF = koff_of(KW);
    constexpr int KQ = (int)((KOFF + 8) / 16);   // key quads, through the tag word when it ends one
    constexpr int VQ = (NA + 2) / 2;             // first + NA aggregates
    constexpr int CQ = KQ + VQ;
    constexpr uint32_t RPI = 64 / CQ;            // claims per store instruction
    const uint32_t lane = threadIdx.x & 63;
    uint32_t w[CQ * 4];
#pragma unroll
    for (int i = 0; i < KQ * 4; ++i) {
        const uint32_t b = 4u * (uint32_t)i;
        w[i] = b < 4u * KW ? k[i] : (b < KOFF ? 0u : (b == KOFF ? (uint32_t)tag : (uint32_t)(tag >> 32)));
    }
#pragma unroll
    for (int i = 0; i < VQ * 2; ++i) {
        const uint64_t x = i == 0 ? gidx : (i - 1 < NA && (uint32_t)(i - 1) < a.naggs ? v[i - 1 < NA ? i - 1 : 0] : 0ull);
        w[KQ * 4 + 2 * i] = (uint32_t)x;
        w[KQ * 4 + 2 * i + 1] = (uint32_t)(x >> 32);
    }
    const uint32_t r = lane / CQ, q = lane % CQ;
    const __amdgpu_buffer_rsrc_t rk = rec_rsrc(a);
    for (uint64_t todo = __ballot(claim); todo;) {
        uint64_t m = todo;
        for (uint32_t i = 0; i < r && m; ++i) m &= m - 1;   // the r-th claimer of the round
        const bool mine = r < RPI && m != 0;
        const uint32_t src = mine ? (uint32_t)__ffsll((long long)m) - 1 : lane;
        const uint32_t slot = __shfl(s, (int)src);
        uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int qq = 0; qq < CQ; ++qq) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t y = __shfl(w[4 * qq + j], (int)src);
                if (q == (uint32_t)qq) o[j] = y;
            }
        }
        if (mine) {
            const u4v val = {o[0], o[1], o[2], o[3]};
            if (q < (uint32_t)KQ) {
                __builtin_amdgcn_raw_buffer_store_b128(val, rk, slot * a.krec_len + 16 * q, 0, 16 /* sc1 */);
            } else {
                const uint32_t off = 16 * (q - KQ), vlen = a.vrec_words * 8;
                uint64_t *vr = a.vrec + (uint64_t)slot * a.vrec_words;
                if (off + 16 <= vlen) {
                    if (a.vrec_total) {
                        const __amdgpu_buffer_rsrc_t rv =
                            __builtin_amdgcn_make_buffer_rsrc(a.vrec, (short)0, (int)a.vrec_total, 0x00020000);
                        __builtin_amdgcn_raw_buffer_store_b128(val, rv, slot * a.vrec_words * 8 + off, 0, 16 /* sc1 */);
                    } else {
                        st_agent(vr + off / 8, (uint64_t)o[0] | ((uint64_t)o[1] << 32));
                        st_agent(vr + off / 8 + 1, (uint64_t)o[2] | ((uint64_t)o[3] << 32));
                    }
                } else if (off < vlen) {
                    st_agent(vr + off / 8, (uint64_t)o[0] | ((uint64_t)o[1] << 32));
                }
            }
        }
        for (uint32_t i = 0; i < RPI && todo; ++i) todo &= todo - 1;
    }
    if constexpr (WAIT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// The batch prober: a wave takes 64 cells of the miss ring and resolves them together, one
// round trip per round: every unresolved lane reads its current slot's record; a lane that
// finds it empty claims it (CAS), and the round's claims are written cooperatively
// (claim_store_coop) and published (`ready`, then the occupancy byte) at the top of the next
// round -- which waits for its probe loads anyway -- or, when the batch is resolved, before the
// wave takes its next cells, so the stores overlap the LDS adoption and ring pushes instead of
// a wait of their own.  A lane that meets its own tag
// not yet published -- possibly claimed by a lane of this very wave -- reads it again next
// round instead of spinning.  Resolved misses then adopt a free LDS entry or go to the
// HBM-update ring.
template <int KW, int NA, bool DBG, int PB>
__device__ __forceinline__ void prober(const GbArgs &a, const LdsCache<KW> &c, const Ring &r,
                                       const MissRing<KW, NA> &m, uint32_t lane, uint32_t gep,
                                       uint32_t *nclaim) {
    constexpr uint32_t KOFF = koff_of(KW);
    constexpr int NQ = probe_quads<KW>();
    const __amdgpu_buffer_rsrc_t rs = rec_rsrc(a);
    // a claim written but not yet published: its slot (SLOT_OVF: none) and event index
    uint32_t pend_s[PB];
    uint64_t pend_g[PB];
#pragma unroll
    for (int j = 0; j < PB; ++j) pend_s[j] = SLOT_OVF;
    auto publish = [&]() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the claims' key / value stores
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            if (pend_s[j] != SLOT_OVF) {
                st_agent(reinterpret_cast<uint64_t *>(a.krec + (uint64_t)pend_s[j] * a.krec_len + KOFF + 8),
                         (a.ep << 48) | (pend_g[j] + 1));
                __builtin_nontemporal_store((uint8_t)1, a.occb + pend_s[j]);
                pend_s[j] = SLOT_OVF;
            }
        }
    };
    for (;;) {
        publish();   // the previous batch's last claims (their stores overlapped its LDS work)
        uint32_t claim = 0;
        if (lane == 0) claim = atomicAdd(&m.ctl[1], 64u * PB);
        claim = __shfl(claim, 0);
        MissRow<KW, NA> x[PB];
        bool have[PB], act[PB];
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            const uint32_t p = claim + lane + 64u * j;
            uint32_t *sq = &m.seq[p % MRING];
            uint32_t spins = 0;
            have[j] = true;
            while (__hip_atomic_load(sq, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != p + 1) {
                if (__hip_atomic_load(&m.ctl[2], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == a.nl) {
                    if (p >= __hip_atomic_load(&m.ctl[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                        have[j] = false;   // past the last miss of a finished stream
                        break;
                    }
                    // the loaders are done, so the cell is being written right now: bounded
                    if (++spins > SPIN_LIMIT) { atomicOr(a.err, 16u); have[j] = false; break; }
                }
                __builtin_amdgcn_s_sleep(1);   // waiting for misses: as long as the stream lasts
                if (DBG && m.waits) atomicAdd(m.waits + 5, 1ull);              // prober: ring empty
            }
            if (have[j]) {
                read_cell<KW, NA>(m, p, x[j]);
                __hip_atomic_store(sq, p + MRING, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);   // free
            }
        }
        bool any = false;
#pragma unroll
        for (int j = 0; j < PB; ++j) any = any || have[j];
        if (__ballot(any) == 0) break;
        uint32_t gs[PB];
        uint64_t first_ins[PB], s[PB];
        bool claimed[PB], reread[PB];
        uint32_t probes[PB], tries[PB];
        uint32_t d[PB][NQ * 4];
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            act[j] = false;
            gs[j] = SLOT_OVF;
            first_ins[j] = 0;
            claimed[j] = reread[j] = false;
            probes[j] = tries[j] = 0;
            if (have[j]) {
                uint32_t g = SLOT_OVF;
                const int slot = x[j].closed ? -1 : lds_lookup<KW>(c, x[j].k, x[j].h, g);
                if (slot >= 0) lds_accumulate<KW, NA>(a, c, slot, x[j].v, x[j].gidx);
                else act[j] = true;
            }
            if (DBG && (a.dbg & 256u) && act[j]) {   // diagnostics: no probe (the home slot, unverified)
                gs[j] = (uint32_t)home_slot(a, x[j].h);
                act[j] = false;
            }
            s[j] = home_slot(a, x[j].h);
            if (act[j]) load_rec<NQ>(rs, (uint32_t)(s[j] * a.krec_len), d[j]);
        }
        for (;;) {
            bool more = false;
#pragma unroll
            for (int j = 0; j < PB; ++j) more = more || act[j];
            if (!__ballot(more)) break;
            publish();   // waits for this round's probe loads, which it needs anyway
#pragma unroll
            for (int j = 0; j < PB; ++j) {
                const uint64_t tag = (x[j].h & ~EP_MAX) | gep;
                bool won = false;
                if (act[j]) {
                    uint8_t *rec = a.krec + s[j] * a.krec_len;
                    uint64_t t = (uint64_t)d[j][KOFF / 4] | ((uint64_t)d[j][KOFF / 4 + 1] << 32);
                    uint64_t ready = (uint64_t)d[j][KOFF / 4 + 2] | ((uint64_t)d[j][KOFF / 4 + 3] << 32);
                    bool next = false;
                    if ((t & EP_MAX) != gep) {   // empty in this generation: claim it
                        if (x[j].gidx >= IDX_LIMIT) {   // an index column value that `ready` cannot carry
                            atomicOr(a.err, 8u);
                            act[j] = false;
                        } else {
                            const uint64_t old = atomicCAS(reinterpret_cast<unsigned long long *>(rec + KOFF),
                                                           (unsigned long long)t, (unsigned long long)tag);
                            if (old == t) {
                                won = true;
                                act[j] = false;
                                gs[j] = (uint32_t)s[j];
                            } else {
                                t = old;     // a claim raced ours: its key may still be in flight
                                ready = 0;
                            }
                        }
                    }
                    if (act[j]) {
                        if (t == tag) {
                            if (!ready_pub(ready, gep, a.ep)) {
                                if (++tries[j] > (1u << 22)) { atomicOr(a.err, 2u); act[j] = false; }   // read again
                            } else {
                                bool eq = true;
#pragma unroll
                                for (int w = 0; w < KW; ++w) eq = eq && (d[j][w] == x[j].k[w]);
                                if (eq) {
                                    gs[j] = (uint32_t)s[j];
                                    first_ins[j] = (ready >> 48) == a.ep ? (ready & READY_IDX) - 1
                                                                         : restamp<KW>(a, s[j], x[j].gidx);
                                    act[j] = false;
                                } else if (!reread[j]) {
                                    // the quads of one snapshot are separate loads: `ready` may have
                                    // been sampled after the key quads, so read the record once more
                                    reread[j] = true;
                                } else {
                                    next = true;
                                }
                            }
                        } else {
                            next = true;
                        }
                    }
                    if (next) {
                        reread[j] = false;
                        s[j] = next_slot(a, s[j]);
                        if (++probes[j] >= a.max_probe) { atomicOr(a.err, 4u); act[j] = false; }
                    }
                }
                if (const uint64_t wm = __ballot(won)) {
                    if (lane == 0) atomicAdd(nclaim, (uint32_t)__popcll(wm));
                    claim_store_coop<KW, NA, false>(a, won, (uint32_t)s[j], x[j].k, tag, x[j].gidx, x[j].v);
                    if (won) {   // published by the next publish() (next round or next batch)
                        pend_s[j] = (uint32_t)s[j];
                        pend_g[j] = x[j].gidx;
                        first_ins[j] = x[j].gidx;
                        claimed[j] = true;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < PB; ++j)
                if (act[j]) load_rec<NQ>(rs, (uint32_t)(s[j] * a.krec_len), d[j]);
        }
#pragma unroll
        for (int j = 0; j < PB; ++j) {
            if (gs[j] == SLOT_OVF) continue;
            const int ad = !x[j].closed && ghost_admit<KW>(a, c, x[j].h) ? lds_adopt<KW>(c, x[j].k, x[j].h, gs[j]) : -1;
            if (claimed[j]) continue;   // a claim's values are in its new record already
            if (ad >= 0) lds_accumulate<KW, NA>(a, c, ad, x[j].v, x[j].gidx);
            else ring_push<NA>(a, r, gs[j], x[j].v, x[j].gidx, first_ins[j]);
        }
    }
}

// SAMPLE: the same kernel counting the seed sample (seeds_compute), a template instance of its
// own so that traces and profiles keep its launches apart from the interval's
// P: the update's row plan (k_gb_table.h), RowPlanRT for the run-time shape.  The host launches a
// plan's instance only for an update that matches it field by field (plan_for_update), so what
// the plan fixes is written over the arguments here and the compiler folds it everywhere.
template <class L, bool DBG, int NA, bool SAMPLE = false, class P = RowPlanRT>
__global__ __launch_bounds__(GTB) void k_groupby(GbArgs a) {
    constexpr int KW = L::KW;
    if constexpr (!P::RT) {
        static_assert(!DBG && !SAMPLE, "row plans are for the production kernel");
        a.naggs = P::D.naggs;
        a.fidx = nullptr;
        a.dbg = 0;
    }
    extern __shared__ uint64_t lds[];
    __shared__ uint32_t ring_ctl[8];
    LdsCache<KW> c;
    c.E = a.lds_entries;
    c.nsets = a.lds_entries / 8;
    const uint32_t E = c.E;
    c.first = lds;
    c.agg = lds + E;
    c.key = reinterpret_cast<uint32_t *>(lds + (1 + a.naggs) * E);
    c.st = c.key + (uint64_t)E * LdsCache<KW>::KP;
    c.tag = c.st + E;
    Ring r;
    r.hi = reinterpret_cast<uint64_t *>(c.tag + E);   // E is a multiple of 8: 8-B aligned
    r.lo = reinterpret_cast<uint2 *>(r.hi + ARING);
    r.ctl = ring_ctl;
    MissRing<KW, NA> m;
    m.cell = reinterpret_cast<uint4 *>(r.lo + ARING);   // 16-B aligned (see launch)
    m.seq = reinterpret_cast<uint32_t *>(m.cell + MRING * MissRing<KW, NA>::EQ);
    m.ctl = ring_ctl + 4;
    m.err = a.err;
    m.waits = (DBG && (a.dbg & 65536u)) ? a.dbg_cnt : nullptr;
    c.ghost = m.seq + MRING;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t e = threadIdx.x; e < E; e += GTB) {
        c.st[e] = ST_EMPTY;
        c.tag[e] = 0;
        c.first[e] = ~0ull;
        for (uint32_t x = 0; x < a.naggs; ++x) c.agg[x * E + e] = 0;
    }
    for (uint32_t e = threadIdx.x; e < ARING; e += GTB) r.lo[e] = make_uint2(0, 0);
    for (uint32_t e = threadIdx.x; e < MRING; e += GTB) m.seq[e] = e;
    for (uint32_t e = threadIdx.x; e < GHOST; e += GTB) c.ghost[e] = 0;
    if (threadIdx.x < 8) ring_ctl[threadIdx.x] = 0;
    __syncthreads();
    if (a.nseeds && *a.seed_gep == *a.gen) {
        // the keys a row sample counted most often, adopted by every workgroup up front (their
        // slots are the generation's: the seeds were looked up in it)
        constexpr uint32_t SW = LdsCache<KW>::KP + 4;
        for (uint32_t i = threadIdx.x; i < a.nseeds; i += GTB) {
            const uint32_t *sr = a.seeds + (uint64_t)i * SW;
            const uint32_t slot = sr[LdsCache<KW>::KP];
            if (slot == SLOT_OVF) continue;
            uint32_t k[KW];
#pragma unroll
            for (int w = 0; w < KW; ++w) k[w] = sr[w];
            const uint64_t h = (uint64_t)sr[LdsCache<KW>::KP + 2] | ((uint64_t)sr[LdsCache<KW>::KP + 3] << 32);
            (void)lds_adopt<KW>(c, k, h, slot);
        }
        __syncthreads();
    }

    if (wave == NWAVES - 1 && !a.direct) {
        ring_serve<DBG>(a, r, lane);
    } else if (wave >= a.nl) {
        // the generation this interval belongs to (the reset kernel decided it on the device)
        const uint32_t gep = (uint32_t)__builtin_amdgcn_readfirstlane(
            (int)(uint32_t)__hip_atomic_load(a.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (a.sm) prober_sm<KW, NA, DBG>(a, c, r, m, lane, gep, &ring_ctl[3]);
        else prober<KW, NA, DBG, 1>(a, c, r, m, lane, gep, &ring_ctl[3]);
        if (lane == 0) atomicAdd(&r.ctl[2], 1u);
    } else {
        const uint32_t PTB = a.nl * 64;   // rows per workgroup step
        const uint64_t stride = (uint64_t)gridDim.x * PTB;
        uint64_t base = (uint64_t)blockIdx.x * PTB + wave * 64;
        RowRaw<L, NA> R;
        uint32_t nmiss = 0;
        if (base < a.n) issue_row<L, NA, cached_stream_nt<L>(), P>(a, min(base + lane, a.n - 1), R);
        for (; base < a.n; base += stride) {
            const uint64_t row = base + lane;
            uint32_t k[KW];
            uint64_t v[NA];
            bool ok = decode_row<L, NA, P>(a, row, R, k, v) && row < a.n;
            if (base + stride < a.n) issue_row<L, NA, cached_stream_nt<L>(), P>(a, min(base + stride + lane, a.n - 1), R);
            const uint64_t h = hash_key<KW>(k);
            if (DBG && (a.dbg & 1u)) {   // diagnostics: load + hash only
                if (ok && h == 0x1234567ull && v[0] == 7) atomicAdd(a.dbg_cnt + 3, 1ull);   // keep live
                ok = false;
            }
            // an index column value `ready` cannot carry fails the interval here, before the cache:
            // an LDS hit never reaches a claim's or a re-stamp's check (a seeded key may see only
            // hits), and the state-machine probers claim without one
            if (ok && a.fidx && row_gidx(a, row) >= IDX_LIMIT) {
                atomicOr(a.err, 8u);
                ok = false;
            }
            if (ok) {
                uint32_t gs = SLOT_OVF;
                bool closed;
                const int slot = lds_lookup<KW>(c, k, h, gs, closed);
                if (DBG && (a.dbg & 8u)) {
                    atomicAdd(a.dbg_cnt + (slot >= 0 ? 0 : 1), 1ull);
                    if (slot < 0 && closed) atomicAdd(a.dbg_cnt + 2, 1ull);   // of the misses: closed sets
                }
                if (slot >= 0) {
                    if (!(DBG && (a.dbg & 512u)))   // diagnostics: bit9 no LDS accumulate
                        lds_accumulate<KW, NA>(a, c, slot, v, row_gidx(a, row));
                } else if (!(DBG && (a.dbg & 2u))) {
                    miss_push<KW, NA>(m, k, h, row_gidx(a, row), v, closed);
                    ++nmiss;
                }
            }
        }
        // LDS misses of this interval (err block + 8): the host picks the prober for the next one
        for (int o = 32; o > 0; o >>= 1) nmiss += __shfl_xor(nmiss, o);
        if (lane == 0 && nmiss) atomicAdd(reinterpret_cast<unsigned long long *>(a.err + 2), (unsigned long long)nmiss);
        if (lane == 0) atomicAdd(&m.ctl[2], 1u);
    }

    __syncthreads();
    // the cache's sums: one lane per (entry, aggregate), so an entry's adds leave from adjacent
    // lanes of one instruction into its value record -- one memory-side request per record (the
    // update ring's shape) instead of one per aggregate from a lane that owns the entry
    const uint32_t na = a.naggs;
    for (uint32_t q0 = threadIdx.x & ~63u; q0 < E * na; q0 += GTB) {   // whole waves (the diagnostics' ballots)
        const uint32_t q = q0 + lane;
        const uint32_t e = q / na, x = q - e * na;
        const uint32_t gs = q < E * na ? c.st[e] : ST_EMPTY;
        const uint64_t s = gs < ST_BUSY ? c.agg[x * E + e] : 0ull;
        if (s) gadd(rec_agg(a, gs, (int)x), (unsigned long long)s);
        if (DBG && (a.dbg & 262144u)) atomics_account(a, s != 0, gs, false, lane, 16);
    }
    for (uint32_t e = threadIdx.x; e < E; e += GTB) {
        const uint32_t gs = c.st[e];
        if (gs >= ST_BUSY) continue;
        const uint64_t f = c.first[e];
        const uint64_t rd = ld_agent(reinterpret_cast<const uint64_t *>(a.krec + (uint64_t)gs * a.krec_len +
                                                                        koff_of(KW) + 8));
        // a `ready` not (yet visibly) of this interval bounds nothing: push the minimum
        const uint64_t fi = (rd >> 48) == a.ep ? (rd & READY_IDX) - 1 : ~0ull;
        if (f < fi) gmin(rec_first(a, gs), (unsigned long long)f);
        // a seeded key may have had only LDS hits (never probed, so nothing marked it): every
        // entry with events marks its group occupied (the adopted ones again, harmlessly)
        if (a.nseeds && f != ~0ull) __builtin_nontemporal_store((uint8_t)1, a.occb + gs);
        if (DBG && (a.dbg & 262144u) && f < fi) atomicAdd(a.dbg_cnt + 20, 1ull);   // flush minima
    }
    if (threadIdx.x == 0 && ring_ctl[3])   // the workgroup's claims: the generation's key count
        atomicAdd(reinterpret_cast<unsigned long long *>(a.gen + 2), (unsigned long long)ring_ctl[3]);
}

// ---- AUTO's re-probe: the cached form's LDS miss share, estimated ---------------------------
// After a run of partitioned intervals AUTO asks whether the stream has turned skewed enough for
// the cached form.  Running a whole interval cached to find out cost C4 7.6 ms against 3.0; the
// probe interval now runs partitioned, and this kernel replays the cache's admission on a sample
// of the rows: the cached kernel's per-workgroup row interleaving, its E-entry 8-way sets and
// its second-miss ghost filter, on the key hash alone (a tag match counts as a hit; no HBM slot,
// no sums).  Its misses go to the error block's miss word, which the cached kernel would have
// written; fin_apply scales them to the interval.
template <class L, int NA>
__global__ __launch_bounds__(GTB) void k_gb_estimate(GbArgs a, uint64_t nsample) {
    constexpr int KW = L::KW;
    extern __shared__ uint64_t lds[];
    LdsCache<KW> c{};
    c.E = a.lds_entries;
    c.nsets = a.lds_entries / 8;
    c.tag = reinterpret_cast<uint32_t *>(lds);
    c.ghost = c.tag + c.E;
    for (uint32_t e = threadIdx.x; e < c.E; e += GTB) c.tag[e] = 0;
    for (uint32_t e = threadIdx.x; e < GHOST; e += GTB) c.ghost[e] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t n = min(a.n, nsample);
    const uint64_t stride = (uint64_t)gridDim.x * GTB;
    uint32_t nmiss = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * GTB + wave * 64; base < n; base += stride) {
        const uint64_t row = base + lane;
        RowRaw<L, NA> R;
        issue_row<L, NA>(a, min(row, n - 1), R);
        uint32_t k[KW];
        uint64_t v[NA];
        if (!(decode_row<L, NA>(a, row, R, k, v) && row < n)) continue;
        const uint64_t h = hash_key<KW>(k);
        const uint32_t sb = lds_set(c, h), t = lds_tag(h);
        uint32_t tg[8];
        lds_tags(c, sb, tg);
        bool hit = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) hit = hit || tg[j] == t;
        if (hit) continue;
        ++nmiss;
        if (!ghost_admit<KW>(a, c, h)) continue;
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) m |= (tg[j] == 0 ? 1u : 0u) << j;
        if (m) (void)atomicCAS(&c.tag[sb + (uint32_t)(__builtin_ffs((int)m) - 1)], 0u, t);
    }
    for (int o = 32; o > 0; o >>= 1) nmiss += __shfl_xor(nmiss, o);
    if (lane == 0 && nmiss) atomicAdd(reinterpret_cast<unsigned long long *>(a.err + 2), (unsigned long long)nmiss);
}

// ---- the LDS cache's seeds -----------------------------------------------------------------
// Seed i is the key of sample-table slot sslots[i] (igx_groupby_sort's top-E by count over a row
// sample), looked up in the table's current generation (a key not there is no seed: seeds are
// only ever found keys, never claimed).  Also records the generation they belong to.
template <class L>
__global__ __launch_bounds__(256) void k_gb_seeds(GbArgs a, const uint8_t *__restrict__ skrec, uint32_t skrec_len,
                                                  const uint32_t *__restrict__ sslots, uint32_t nseeds,
                                                  uint32_t *__restrict__ seeds, uint64_t *__restrict__ seed_gep) {
    constexpr int KW = L::KW;
    constexpr uint32_t KP = LdsCache<KW>::KP, KOFF = koff_of(KW);
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t gep = (uint32_t)*a.gen;
    if (i == 0) *seed_gep = gep;
    if (i >= nseeds) return;
    uint32_t *out = seeds + (uint64_t)i * (KP + 4);
    const uint32_t ss = sslots[i];
    if (ss == 0xFFFFFFFFu) {   // fewer sampled keys than seeds
        out[KP] = SLOT_OVF;
        return;
    }
    uint32_t k[KW];
#pragma unroll
    for (int w = 0; w < KW; ++w) k[w] = reinterpret_cast<const uint32_t *>(skrec + (uint64_t)ss * skrec_len)[w];
    const uint64_t h = hash_key<KW>(k);
    const uint64_t tag = (h & ~EP_MAX) | gep;
    uint32_t found = SLOT_OVF;
    uint64_t s = home_slot(a, h);
    for (uint32_t probe = 0; probe < a.max_probe; ++probe) {
        const uint8_t *r = a.krec + s * a.krec_len;
        const uint64_t t = *reinterpret_cast<const uint64_t *>(r + KOFF);
        if ((t & EP_MAX) != gep) break;   // an empty slot of the generation: the key is not there
        if (t == tag && ready_pub(*reinterpret_cast<const uint64_t *>(r + KOFF + 8), gep, a.ep)) {
            bool eq = true;
#pragma unroll
            for (int w = 0; w < KW; ++w) eq = eq && reinterpret_cast<const uint32_t *>(r)[w] == k[w];
            if (eq) {
                found = (uint32_t)s;
                break;
            }
        }
        s = next_slot(a, s);
    }
#pragma unroll
    for (uint32_t w = 0; w < KP; ++w) out[w] = (int)w < KW ? k[w] : 0u;
    out[KP] = found;
    out[KP + 1] = 0;
    out[KP + 2] = (uint32_t)h;
    out[KP + 3] = (uint32_t)(h >> 32);
}

// ---- launchers ---------------------------------------------------------------------------
constexpr size_t GB_LDS_TOTAL = 156 * 1024;    // cache + the two rings (dynamic LDS)

// The cached kernel's dynamic LDS for naggs aggregates in its NA-slot variant, in the order
// k_groupby carves it: E cache entries (whole 8-way sets, as many as the budget holds) of
// `entry` bytes each (first, sums, key, st, tag), then the two rings and the ghost filter
// (`rings` bytes).  The launchers, the estimate and the seeds all size by this one function.
struct GbLds {
    size_t entry, rings;
    uint32_t E;
    size_t bytes() const { return E * entry + rings; }
};
template <class L, int NA>
GbLds gb_lds(uint32_t naggs) {
    GbLds g{};
    g.entry = 4 + 4 + 8 + 8 * naggs + 4 * LdsCache<L::KW>::KP;
    g.rings = ARING * 16 + MRING * (16 * MissRing<L::KW, NA>::EQ + 4) + GHOST * 4;
    g.E = 8 * (uint32_t)std::max<size_t>(1, std::min<size_t>(1024, (GB_LDS_TOTAL - g.rings) / (8 * g.entry)));
    return g;
}
// the cached kernel's LDS cache entries (E) for a table of naggs aggregates
template <class L>
uint32_t gb_entries_for(uint32_t naggs) {
    return naggs <= 2 ? gb_lds<L, 2>(naggs).E : gb_lds<L, AMAX>(naggs).E;
}

template <class L, bool DBG, int NA, bool SAMPLE = false, class P = RowPlanRT>
void launch_gb_as(igx_ctx *ctx, GbArgs &a, uint32_t blocks) {
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_groupby<L, DBG, NA, SAMPLE, P>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, GB_LDS_TOTAL);
        attr = true;
    }
    const GbLds g = gb_lds<L, NA>(a.naggs);
    a.lds_entries = g.E;
    hipLaunchKernelGGL((k_groupby<L, DBG, NA, SAMPLE, P>), dim3(blocks), dim3(GTB), g.bytes(), ctx->stream, a);
}

// k_gb_estimate with the cached kernel's geometry (its E and its GHOST filter)
template <class L, int NA>
void launch_estimate_as(igx_ctx *ctx, GbArgs a, uint32_t blocks, uint64_t nsample) {
    a.lds_entries = gb_lds<L, NA>(a.naggs).E;
    a.admit_mask = std::max<uint32_t>(a.admit_mask, 1u);
    const size_t lds = ((size_t)a.lds_entries + GHOST) * 4;
    hipLaunchKernelGGL((k_gb_estimate<L, NA>), dim3(blocks), dim3(GTB), lds, ctx->stream, a, nsample);
}

// The diagnostic variants (IGX_GB_DEBUG) are compiled for the top-tcp key only, so the
// production kernels carry none of their code.  Tables with at most two aggregates run a
// kernel that carries two aggregate slots (fewer registers, fewer loads).
// An update whose shape is a registered row plan's runs that plan's instance (plan: its id from
// plan_for_update, 0: none or switched off).
template <class L>
void launch_gb(igx_ctx *ctx, GbArgs &a, uint32_t blocks, int plan) {
    if constexpr (std::is_same<L, StaticLayout<16, 16, 8, 4, 16, 2, 2, 2>>::value) {
        if (a.dbg) {
            launch_gb_as<L, true, 2>(ctx, a, blocks);
            return;
        }
        if (plan == TopTcpPlan::D.id) {
            launch_gb_as<L, false, 2, false, TopTcpPlan>(ctx, a, blocks);
            return;
        }
    }
    if constexpr (std::is_same<L, StaticLayout<8, 4, 4, 4>>::value) {
        if (plan == TopFilePlan::D.id && !a.dbg) {
            launch_gb_as<L, false, AMAX, false, TopFilePlan>(ctx, a, blocks);
            return;
        }
    }
#ifdef IGX_GB_DEBUG_FILE
    if constexpr (std::is_same<L, StaticLayout<8, 4, 4, 4>>::value) {
        if (a.dbg) {
            launch_gb_as<L, true, AMAX>(ctx, a, blocks);
            return;
        }
    }
#endif
    if (a.naggs <= 2) launch_gb_as<L, false, 2>(ctx, a, blocks);
    else launch_gb_as<L, false, AMAX>(ctx, a, blocks);
}

// The sample-seeded LDS cache (tools/cache_sim.py: C2 33.7 -> 31.2 % misses, C5 45.4
// -> 42.6 %, against 30.7 / 42.2 % for an ideal top-E cache).  The first SEED_SAMPLE rows of the
// interval's first update are counted by key in a scratch table (the cached kernel with one COUNT
// aggregate, as its SAMPLE instance: profiles keep its launches apart; the direct form took
// 2.7-3.1 ms for these 1.5M rows -- a sample's hot keys queue on one record's atomics), its top-E
// groups by count are selected on the device (igx_groupby_sort),
// and k_gb_seeds looks each of them up in the table's current generation.  Every workgroup of the
// interval's cached updates adopts the found ones before its stream starts.  Hot keys of a
// stream are stable, so the seeds are recomputed every SEED_EVERY seeded intervals (and after a
// generation ended); seeds of another generation are never adopted (the kernel compares).
constexpr uint64_t SEED_SAMPLE = 1u << 20;      // sampled rows: max(1M, rows / SEED_DIV)
constexpr uint64_t SEED_DIV = 128;

template <class L>
int seeds_compute_static(igx_table *t, igx_ctx *ctx, const GbArgs &a) {
    const uint32_t E = gb_entries_for<L>(t->naggs);
    uint64_t div = SEED_DIV;
    if (const char *d = std::getenv("IGX_GB_SEED_DIV")) div = std::max<uint64_t>(1, std::strtoull(d, nullptr, 0));   // A/B knob
    const uint64_t S = std::min<uint64_t>(a.n, std::max<uint64_t>(SEED_SAMPLE, a.n / div));
    if (t->seed_tab && t->seed_tab->cap < S) {
        igx_groupby_destroy(t->seed_tab);
        t->seed_tab = nullptr;
    }
    if (!t->seed_tab) {
        igx_agg cnt{};
        cnt.kind = IGX_AGG_COUNT;
        cnt.col = IGX_NO_COL;
        cnt.cond_col = IGX_NO_COL;
        cnt.out_width = 8;
        igx_table *st = nullptr;
        int rc = igx_groupby_create(ctx, t->key_widths, t->nkeys, &cnt, 1, std::max<uint64_t>(S, 4ull * E), &st);
        if (rc) return rc;
        if (st->wide) {   // the sample runs the cached form, which a wide table does not have
            igx_groupby_destroy(st);
            return IGX_ENOTSUP;
        }
        st->persist = false;
        st->seed_on = false;
        st->mode = IGX_GB_CACHED;
        t->seed_tab = st;
    }
    if (t->seeds_cap < E) {
        (void)hipFree(t->seeds);
        (void)hipFree(t->seed_slots);
        t->seeds = nullptr;
        t->seed_slots = nullptr;
        t->seeds_cap = 0;
        IGX_HIP(ctx, hipMalloc(&t->seeds, (size_t)E * (LdsCache<L::KW>::KP + 4) * 4));
        IGX_HIP(ctx, hipMalloc(&t->seed_slots, (size_t)E * 4));
        if (!t->seed_gep) IGX_HIP(ctx, hipMalloc(&t->seed_gep, 8));
        t->seeds_cap = E;
    }
    igx_table *st = t->seed_tab;
    (void)fin_collect(st, nullptr);   // the last sample's read-back (landed long ago)
    st->fin_status = IGX_OK;
    (void)igx_groupby_reset(st);
    // the same columns and fused predicates, the sample's rows, one COUNT into the sample table
    // (aggregate 0's columns are still loaded: predicates and guards may read their raw values)
    GbArgs b = a;
    b.n = S;
    b.naggs = 1;
    b.vcount[0] = 1;
    b.hascond[0] = 0;
    b.valid = a.valid;
    bind_records(st, b);
    b.dbg = 0;
    b.sm = 0;
    b.direct = 0;
    b.nl = NL_DEFAULT;
    b.seeds = nullptr;
    b.seed_gep = nullptr;
    b.nseeds = 0;
    b.log = nullptr;
    st->rows_fed = S;
    st->fin_since_update = false;
    st->interval_direct = st->interval_part = false;
    st->occb_dirty = true;
    launch_gb_as<L, false, 2, true>(ctx, b, (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((S + GTB - 1) / GTB,
                                                                                           (uint64_t)ctx->num_cus)));
    IGX_HIP(ctx, hipGetLastError());
    int rc = igx_groupby_finalize_async(st, nullptr);
    if (rc) return rc;
    igx_tsortkey key{};
    key.src = IGX_TSRC_AGG;
    key.index = 0;
    key.desc = 1;
    rc = igx_groupby_sort(st, &key, 1, E, t->seed_slots);
    if (rc) return rc;
    hipLaunchKernelGGL(k_gb_seeds<L>, dim3((E + 255) / 256), dim3(256), 0, ctx->stream, a, st->krec, st->krec_len,
                       t->seed_slots, E, t->seeds, t->seed_gep);
    IGX_HIP(ctx, hipGetLastError());
    t->nseeds = E;
    return IGX_OK;
}

}  // namespace

void gb_cached_load() {
    hipFuncAttributes fa;
    (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_groupby<TcpKey, false, 2, false>));
}

int gb_launch_cached(igx_table *t, GbArgs &a, uint32_t blocks) {
    return gb_with_layout(t, [&](auto tag) {
        using L = typename decltype(tag)::type;
        t->rowplan_last = t->rowplan_on && !a.dbg ? plan_for_update<L>(a) : 0;
        launch_gb<L>(t->ctx, a, blocks, t->rowplan_last);
        return (int)IGX_OK;
    });
}

int gb_launch_estimate(igx_table *t, const GbArgs &a, uint32_t blocks, uint64_t nsample) {
    return gb_with_layout(t, [&](auto tag) {
        using L = typename decltype(tag)::type;
        if (a.naggs <= 2) launch_estimate_as<L, 2>(t->ctx, a, blocks, nsample);
        else launch_estimate_as<L, AMAX>(t->ctx, a, blocks, nsample);
        return (int)IGX_OK;
    });
}

int gb_seeds_compute(igx_table *t, const GbArgs &a) {
    return gb_with_layout(t, [&](auto tag) -> int {
        using L = typename decltype(tag)::type;
        // static key layouts only (the reference's BPF key structs)
        if constexpr (L::is_static) return seeds_compute_static<L>(t, t->ctx, a);
        else return IGX_ENOTSUP;
    });
}
