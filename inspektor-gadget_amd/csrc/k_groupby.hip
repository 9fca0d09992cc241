// k_groupby.hip -- keyed per-interval aggregation (kernel (2)).
//
// Reference semantics: the top gadgets' BPF hash maps, e.g. probe_ip
// (pkg/gadgets/top/tcp/tracer/bpf/tcptop.bpf.c:33-110): build a fixed key struct,
// lookup-or-insert, `+=` into the value; nextStats (tracer.go:147-226) drains one Stats
// row per key.  Keys are compared in full (exact, like the BPF map's memcmp), values
// wrap at their declared width, and each group remembers the global index of its first
// event -- the canonical pre-sort order that replaces BPF map order.
//
// The HBM table, its protocol and the list of key layouts are k_gb_table.h.  An update runs in
// one of three forms, each a translation unit of its own: cached (k_gb_cached.hip), direct
// (k_gb_direct.hip) and partitioned (k_gb_part.hip, k_gb_part_c.hip).  This file is the table's
// host side -- create / reset / destroy, the plan of an update and the choice of its form
// (launch_form), finalize, gather, select, lookup and sort -- and the kernels that read or
// clear the table without a key layout.
#include "k_gb_table.h"

namespace {

// Full clear of tags and `ready` (keys and value records are left as is).  Needed only
// when the epoch counter wraps: every other interval starts by bumping the epoch.
__global__ void k_table_clear(uint8_t *krec, uint32_t krec_len, uint32_t koff, uint64_t ns) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += stride)
        *reinterpret_cast<uint4 *>(krec + i * krec_len + koff) = make_uint4(0, 0, 0, 0);
}

// ---- finalize: list the occupied slots in ascending order, from the occupancy bitmap ----
constexpr int CT = 256 * 32;   // slots per compaction tile (256 threads x one 32-slot word)

// occupancy bitmap of an interval whose claims did not set it (the direct form): slot s is
// occupied iff its tag carries the interval's epoch.  One lane per 32-slot word; the tags
// are 8-byte loads at the record stride.
__global__ __launch_bounds__(256) void k_occ_from_tags(const uint8_t *__restrict__ krec, uint32_t krec_len,
                                                       uint32_t koff, uint64_t ns, uint64_t ep,
                                                       uint32_t *__restrict__ occ) {
    const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (w * 32 >= ns) return;
    uint32_t m = 0;
#pragma unroll 8
    for (uint32_t b = 0; b < 32; ++b) {
        const uint64_t s = w * 32 + b;
        const uint64_t t = s < ns ? *reinterpret_cast<const uint64_t *>(krec + s * krec_len + koff) : 0;
        m |= ((t & EP_MAX) == ep ? 1u : 0u) << b;
    }
    occ[w] |= m;   // OR: earlier cached updates of the interval may have set bits already
}

// 4 bytes of the byte map (each 0 or 1) -> 4 bits, byte j -> bit j
__device__ __forceinline__ uint32_t byte_bits(uint32_t w) { return (w | (w >> 7) | (w >> 14) | (w >> 21)) & 0xFu; }

// per-tile counts of occupied slots; with occb, first folds the byte map's 32 bytes of each
// bitmap word into it and clears them (the byte map is left zero for the next interval)
__global__ __launch_bounds__(256) void k_slots_count(uint32_t *__restrict__ occ, uint64_t nwords,
                                                     uint32_t *__restrict__ cnt, uint8_t *__restrict__ occb) {
    __shared__ uint32_t wc[4];
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t m = i < nwords ? occ[i] : 0u;
    if (occb && i < nwords) {
        uint4 *b = reinterpret_cast<uint4 *>(occb) + 2 * i;
        const uint4 b0 = b[0], b1 = b[1];
        const uint32_t w[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
        uint32_t f = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) f |= byte_bits(w[j]) << (4 * j);
        if (f) {
            m |= f;
            occ[i] = m;
            b[0] = make_uint4(0, 0, 0, 0);
            b[1] = make_uint4(0, 0, 0, 0);
        }
    }
    uint32_t c = (uint32_t)__popc(m);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// finalize's read-back, written by the kernel that knows the group count straight into the
// table's coherent pinned buffer (no copy after it): err block {bits, pad, LDS misses}, count
// (then, released after them, the finalize's sequence number: the host polls it instead of
// recording an event, whose release would flush L2 between finalize and the top-K)
// It also closes the interval's books in the generation block: an interval that started its
// generation holds every group as a claim (the key count is its group count), one that
// continued adds its claims; a failed interval ends the generation.
__device__ __forceinline__ void fin_export(const uint32_t *err, uint64_t total, uint64_t *host, uint64_t seq, uint64_t ep) {
    const uint64_t e0 = *reinterpret_cast<const volatile uint64_t *>(err);
    const uint64_t e1 = *reinterpret_cast<const volatile uint64_t *>(err + 2);
    volatile uint64_t *gen = reinterpret_cast<volatile uint64_t *>(const_cast<uint32_t *>(err)) + GEN_WORD;
    const bool fresh = gen[0] == ep;
    const uint64_t claims = fresh ? total : gen[2];
    const uint64_t keys = (uint32_t)e0 ? ~0ull : (fresh ? total : gen[1] + claims);
    gen[1] = keys;
    gen[2] = 0;
    __hip_atomic_store(host, e0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(host + 1, e1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(host + 2, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(host + 4, claims, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(host + 5, keys, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    for (int x = 0; x < 4; ++x)   // the update log's counters ride the same read-back
        __hip_atomic_store(host + LOG_STAT_WORD + x,
                           *(reinterpret_cast<const volatile uint64_t *>(err) + LOG_STAT_WORD + x), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    __hip_atomic_store(host + 3, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(1024) void k_slots_scan(uint32_t *__restrict__ v, uint64_t m, uint64_t *__restrict__ total,
                                                     const uint32_t *__restrict__ err, uint64_t *__restrict__ host,
                                                     uint64_t seq, uint64_t ep) {
    __shared__ uint32_t part[1024];
    const uint64_t per = (m + 1023) / 1024;
    const uint64_t b = threadIdx.x * per, e = min(m, b + per);
    uint32_t s = 0;
    for (uint64_t i = b; i < e; ++i) s += v[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        uint32_t x = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += x;
        __syncthreads();
    }
    uint32_t run = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (uint64_t i = b; i < e; ++i) {
        uint32_t c = v[i];
        v[i] = run;
        run += c;
    }
    if (threadIdx.x == 1023) {
        *total = part[1023];
        fin_export(err, part[1023], host, seq, ep);
    }
}

// The tile's slot list, staged in LDS and written out as one contiguous run.  With off null
// the tile's base is the sum of the counts of the tiles before it (read here: no scan kernel,
// for tables of at most SLOTS_INLINE_TILES tiles), and the last tile writes the total.
constexpr uint32_t SLOTS_INLINE_TILES = 4096;
__global__ __launch_bounds__(256) void k_slots_write(const uint32_t *__restrict__ occ, uint64_t nwords,
                                                     const uint32_t *__restrict__ off, const uint32_t *__restrict__ cnt,
                                                     uint32_t *__restrict__ out, uint64_t *__restrict__ total,
                                                     const uint32_t *__restrict__ err, uint64_t *__restrict__ host,
                                                     uint64_t seq, uint64_t ep) {
    __shared__ uint32_t wsum[4], pre[4];
    __shared__ uint32_t buf[256 * 32];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t m = i < nwords ? occ[i] : 0u;
    const uint32_t c = (uint32_t)__popc(m);
    uint32_t inc = c;   // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t x = __shfl_up(inc, d);
        if ((int)lane >= d) inc += x;
    }
    if (lane == 63) wsum[wave] = inc;
    uint32_t base = 0;
    if (off) {
        base = off[blockIdx.x];
    } else {
        for (uint32_t j = threadIdx.x; j < blockIdx.x; j += 256) base += cnt[j];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) base += __shfl_xor(base, d);
        if (lane == 0) pre[wave] = base;
    }
    __syncthreads();
    if (!off) base = pre[0] + pre[1] + pre[2] + pre[3];
    uint32_t loc = inc - c;
    for (uint32_t w = 0; w < wave; ++w) loc += wsum[w];
    const uint32_t tile_n = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    const uint32_t s0 = (uint32_t)(i * 32);
    while (m) {
        const uint32_t bit = (uint32_t)__ffs(m) - 1;
        buf[loc++] = s0 + bit;
        m &= m - 1;
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < tile_n; j += 256) out[base + j] = buf[j];
    if (!off && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        *total = (uint64_t)base + tile_n;
        fin_export(err, (uint64_t)base + tile_n, host, seq, ep);
    }
}

// an interval's reset: the occupancy bitmap and the error block in one launch, and the byte
// map when claims since the last finalize left bytes in it (nb16 of its 16-B quads, else 0).
// It also decides the interval's generation: with `may` (the host's part: the last interval
// was finalized and this one is planned in the cached form) and the generation's keys within
// `limit`, the generation goes on and the last interval's groups (groups[0 .. *ng), finalize's
// slot list) get their value records back to first = UINT64_MAX, sums 0 (vq 16-B quads each);
// otherwise this interval starts a generation at its own epoch.  Every thread reads the same
// words (nothing in this launch writes gen[1] or the slot list), so all agree.
struct ResetGen {
    uint64_t *gen;            // the generation block (err words GEN_WORD..)
    uint64_t ep, limit;
    const uint32_t *groups;
    const uint64_t *ng;
    uint64_t *vrec;
    uint32_t vw, may;         // value-record words (1 or an even number), the host's part
};
__global__ __launch_bounds__(256) void k_reset_clear(uint32_t *__restrict__ occ, uint64_t nwords,
                                                     uint32_t *__restrict__ err, uint4 *__restrict__ occb,
                                                     uint64_t nb16, ResetGen rg) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    const uint64_t n4 = nwords / 4;
    for (uint64_t q = i; q < n4; q += stride) reinterpret_cast<uint4 *>(occ)[q] = make_uint4(0, 0, 0, 0);
    for (uint64_t q = i; q < nb16; q += stride) occb[q] = make_uint4(0, 0, 0, 0);
    if (i < (nwords & 3)) occ[n4 * 4 + i] = 0;
    if (i < 4) err[i] = 0;
    if (i >= 2 * LOG_STAT_WORD && i < 2 * LOG_STAT_WORD + 8) err[i] = 0;   // the update log's counters
    const bool cont = rg.may && rg.gen[1] <= rg.limit;
    if (cont) {
        // one lane per 16-B quad of a record, a record's quads in adjacent lanes: each record
        // leaves as one store instruction's contiguous pieces (one write request per record, the
        // claim stores' shape), not one request per quad of a lane writing its record alone.
        // RU slot-list loads are issued before their stores: one at a time, each store waited
        // for its own load's round trip and the pass was latency-bound.
        constexpr int RU = 8;
        const uint64_t ng = *rg.ng;
        const uint32_t qs = rg.vw == 1 ? 0u : (uint32_t)__builtin_ctz(rg.vw / 2);   // log2 quads per record
        const uint64_t total = ng << qs;
        const uint32_t *__restrict__ groups = rg.groups;
        uint64_t *__restrict__ vrec = rg.vrec;
        for (uint64_t j0 = i; j0 < total; j0 += RU * stride) {
            uint32_t slot[RU];
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const uint64_t j = j0 + u * stride;
                slot[u] = j < total ? groups[j >> qs] : 0u;
            }
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const uint64_t j = j0 + u * stride;
                if (j >= total) break;
                const uint32_t q = (uint32_t)(j & ((1ull << qs) - 1));
                uint64_t *v = vrec + (uint64_t)slot[u] * rg.vw;
                if (rg.vw == 1) *v = ~0ull;
                else reinterpret_cast<uint4 *>(v)[q] = q ? make_uint4(0, 0, 0, 0) : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0);
            }
        }
    }
    if (i == 0) {
        if (!cont) rg.gen[0] = rg.ep;
        rg.gen[2] = 0;
    }
}

// the interval's planned generation did not hold (its first update runs the direct or the
// partitioned form, which start their own): it starts a generation at its epoch
__global__ void k_gen_restart(uint64_t *gen, uint64_t ep) {
    gen[0] = ep;
    gen[2] = 0;
}

// materialise selected groups as packed rows key | aggs | first (the Stats rows of
// nextStats, tracer.go:186-219); aggregates wrap to their out_width (the BPF value width)
struct AggMasks {
    uint32_t m[2 * AMAX];   // (lo, hi) word masks per aggregate
};

__global__ void k_gather_rows(const uint8_t *__restrict__ krec, uint32_t krec_len, const uint64_t *__restrict__ vrec,
                              uint32_t vw, uint32_t key_words, uint32_t naggs, AggMasks am,
                              const uint32_t *__restrict__ idx, uint64_t ns, uint64_t k, uint8_t *__restrict__ out) {
    const uint64_t r = blockIdx.x;
    if (r >= k) return;
    const uint32_t row_words = key_words + 2 * naggs + 2;
    uint32_t *o = reinterpret_cast<uint32_t *>(out) + r * row_words;
    const uint32_t g = idx[r];
    const bool ok = g < ns;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(krec + (uint64_t)g * krec_len);
    const uint32_t *val = reinterpret_cast<const uint32_t *>(vrec + (uint64_t)g * vw);
    for (uint32_t w = threadIdx.x; w < row_words; w += blockDim.x) {
        uint32_t v = 0;
        if (ok) {
            if (w < key_words) v = src[w];
            else if (w < key_words + 2 * naggs) v = val[2 + (w - key_words)] & am.m[w - key_words];
            else v = val[w - key_words - 2 * naggs];
        }
        o[w] = v;
    }
}

// ---- threshold selection and key lookup over a finalized table -----------------------------
// The two device steps of the cross-rank threshold top-K: "which of my groups
// hold aggregate x >= T" and "what do I hold for these keys in this interval".  Both only read
// the table.

// the interval's groups (finalize's slot list, its count read here) whose aggregate `agg`,
// masked to its out_width as k_gather_rows masks it, is >= thr.  *count receives how many
// qualify (zeroed before the launch); the first cap of them, in the order the waves' atomics
// land, go to out.  One atomic per wave and sweep step.
__global__ __launch_bounds__(256) void k_select_ge(const uint32_t *__restrict__ groups, const uint64_t *__restrict__ ng,
                                                   uint64_t ns, const uint64_t *__restrict__ vrec, uint32_t vw,
                                                   uint32_t agg, uint64_t mask, uint64_t thr,
                                                   uint32_t *__restrict__ out, uint64_t cap,
                                                   unsigned long long *__restrict__ count) {
    const uint64_t n = min(*ng, ns);
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    const uint32_t lane = threadIdx.x & 63;
    // whole waves step together (the ballot below needs every lane of the wave in the loop)
    for (uint64_t r0 = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); r0 < n; r0 += stride) {
        const uint64_t r = r0 + lane;
        uint32_t slot = 0;
        bool q = false;
        if (r < n) {
            slot = groups[r];
            q = slot < ns && (vrec[(uint64_t)slot * vw + 1 + agg] & mask) >= thr;
        }
        const uint64_t b = __ballot(q);
        if (!b) continue;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(count, (unsigned long long)__popcll(b));
        base = __shfl(base, 0);
        const uint64_t pos = base + (uint64_t)__popcll(b & ((1ull << lane) - 1));
        if (q && pos < cap) out[pos] = slot;
    }
}

// Query i's key (KW words, those past key_words zero, as the update kernels lay a key out) is
// probed in the table's current generation like k_gb_seeds probes a seed: read-only, the chain
// ends at the generation's first empty slot or after max_probe slots.  A key record that is
// found is a group of this interval only if finalize listed its slot (the occupancy bitmap:
// a key kept from an earlier interval of the generation has its record but no bit).  Found:
// out row = k_gather_rows' row of the slot, found[i] = 1; else a zero row and 0.
template <int KW>
__global__ __launch_bounds__(256) void k_gb_lookup(GbArgs a, const uint8_t *__restrict__ qkeys, uint32_t qstride,
                                                   uint64_t nq, uint32_t key_words, AggMasks am,
                                                   uint8_t *__restrict__ out, uint8_t *__restrict__ found) {
    constexpr uint32_t KOFF = koff_of(KW);
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    const uint32_t gep = (uint32_t)*a.gen;
    const uint32_t *qk = reinterpret_cast<const uint32_t *>(qkeys + i * qstride);
    uint32_t k[KW];
#pragma unroll
    for (int w = 0; w < KW; ++w) k[w] = (uint32_t)w < key_words ? qk[w] : 0u;
    const uint64_t h = hash_key<KW>(k);
    const uint64_t tag = (h & ~EP_MAX) | gep;
    uint32_t hit = SLOT_OVF;
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
                hit = (uint32_t)s;
                break;
            }
        }
        s = next_slot(a, s);
    }
    const bool ok = hit != SLOT_OVF && ((a.occ[hit >> 5] >> (hit & 31)) & 1u);
    const uint32_t row_words = key_words + 2 * a.naggs + 2;
    uint32_t *o = reinterpret_cast<uint32_t *>(out) + i * row_words;
    const uint32_t *val = reinterpret_cast<const uint32_t *>(a.vrec + (uint64_t)(ok ? hit : 0u) * a.vrec_words);
    for (uint32_t w = 0; w < row_words; ++w) {
        uint32_t v = 0;
        if (ok) {
            if (w < key_words) v = qk[w];
            else if (w < key_words + 2 * a.naggs) v = val[2 + (w - key_words)] & am.m[w - key_words];
            else v = val[w - key_words - 2 * a.naggs];
        }
        o[w] = v;
    }
    found[i] = ok ? 1 : 0;
}

// rows kept by `in` (nullable: all) and every predicate of dp -> out (u8; in may be out)
__global__ __launch_bounds__(256) void k_pred_mask(DevPreds dp, const uint8_t *in, uint64_t n, uint8_t *out) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        out[i] = (uint8_t)((!in || in[i]) && preds_match_all(dp, i));
}

}  // namespace

extern "C" int igx_groupby_create(igx_ctx *ctx, const uint32_t *key_widths, uint32_t nkeys, const igx_agg *aggs,
                                  uint32_t naggs, uint64_t capacity, igx_table **out) {
    if (!ctx || !out || !key_widths || nkeys == 0 || nkeys > 16)
        return igx_fail(ctx, IGX_EINVAL, "groupby_create: bad key description");
    if (naggs > AMAX) return igx_fail(ctx, IGX_ENOTSUP, "groupby_create: more than %d aggregates", AMAX);
    for (uint32_t x = 0; x < naggs; ++x) {
        const uint32_t ow = aggs[x].out_width;
        if (ow != 0 && !igx_scalar_width(ow))
            return igx_fail(ctx, IGX_EINVAL, "groupby_create: aggregate %u out_width %u", x, ow);
        if (aggs[x].kind != IGX_AGG_COUNT && aggs[x].kind != IGX_AGG_SUM)
            return igx_fail(ctx, IGX_EINVAL, "groupby_create: aggregate %u kind %u", x, aggs[x].kind);
    }
    if (capacity == 0 || capacity > (1ull << 28)) return igx_fail(ctx, IGX_EINVAL, "groupby_create: bad capacity");
    uint32_t words = 0;
    for (uint32_t i = 0; i < nkeys; ++i) {
        const uint32_t w = key_widths[i];
        if (w == 0) return igx_fail(ctx, IGX_EINVAL, "groupby: key width 0");
        words += (w + 3) / 4;
    }
    if (words > KWMAX) return igx_fail(ctx, IGX_ENOTSUP, "groupby: key wider than %d bytes", KWMAX * 4);
    static const bool loaded = (gb_cached_load(), gb_direct_load(), gb_part_load(), true);   // once: see k_gb_table.h
    (void)loaded;
    auto *t = new igx_table();
    t->ctx = ctx;
    t->nkeys = nkeys;
    for (uint32_t i = 0; i < nkeys; ++i) t->key_widths[i] = key_widths[i];
    t->key_words = words;
    // the layout the kernels will use for this key description, and its record's key words.
    // gb_with_layout reads t->generic before it calls the functor: set here it only means "skip
    // the static layouts"; the functor then records what the chosen layout is, for every later call
    t->generic = std::getenv("IGX_GB_GENERIC") != nullptr;   // diagnostics: no static layout
    const int lrc = gb_with_layout(t, [&](auto tag) {
        using L = typename decltype(tag)::type;
        t->generic = !L::is_static;
        t->kw_rec = (uint32_t)L::KW;
        return (int)IGX_OK;
    });
    if (lrc) {
        delete t;
        return lrc;
    }
    t->koff = koff_of((int)t->kw_rec);
    t->krec_len = krec_bytes((int)t->kw_rec);
    if (const char *d = std::getenv("IGX_GB_KR16"))   // tuning knob: 16-B rounded key records
        if (std::strtoul(d, nullptr, 0)) t->krec_len = (uint32_t)igx_align(t->koff + 16, 16);
    t->vrec_len = vrec_bytes(naggs);
    t->naggs = naggs;
    for (uint32_t i = 0; i < naggs; ++i) t->aggs[i] = aggs[i];
    t->cap = capacity;
    // S >= slotf/4 x capacity (default 2x); a smaller table stays resident in the Infinity Cache
    uint64_t slotf = 8;
    if (const char *d = std::getenv("IGX_GB_SLOTF")) slotf = std::max<uint64_t>(5, std::strtoul(d, nullptr, 0));
    uint64_t ns = 1024;
    while (ns * 4 < slotf * capacity) ns <<= 1;
    t->nslots = ns;
    t->sbits = (uint32_t)__builtin_ctzll(ns);
    // probe regions of max(1024, S / 16384) slots: up to 16K regions, so a bucket of the
    // partitioned form can own whole regions
    t->rbits = std::max<uint32_t>(10, t->sbits > 14 ? t->sbits - 14 : 0);
    // key records past a buffer descriptor's 4 GiB: the wide instances (per-lane 64-bit addresses)
    t->wide = ns * t->krec_len >= (1ull << 32);
    if (const char *d = std::getenv("IGX_GB_WIDE"))   // A/B and test knob: wide instances on a narrow-sized table
        t->wide = t->wide || std::strtoul(d, nullptr, 0) != 0;
    const uint64_t tiles = (ns + CT - 1) / CT;
    hipError_t e = hipMalloc(&t->krec, ns * t->krec_len);
    if (e == hipSuccess) e = hipMemsetAsync(t->krec, 0, ns * t->krec_len, ctx->stream);
    if (e == hipSuccess) e = hipMalloc(&t->vrec, ns * t->vrec_len);
    if (e == hipSuccess) e = hipMalloc(&t->err, 128);   // error block, generation block, count, log counters
    if (e == hipSuccess) e = hipMemsetAsync(t->err, 0, 128, ctx->stream);
    if (e == hipSuccess) e = hipMalloc(&t->groups, ns * 4);
    if (e == hipSuccess) e = hipMalloc(&t->tile_cnt, tiles * 4);
    t->occ_words = (ns + 31) / 32;
    if (e == hipSuccess) e = hipMalloc(&t->occ, t->occ_words * 4);
    if (e == hipSuccess) e = hipMalloc(&t->occb, t->occ_words * 32);
    if (e == hipSuccess) e = hipMemsetAsync(t->occb, 0, t->occ_words * 32, ctx->stream);
    if (e == hipSuccess) t->n_groups = reinterpret_cast<uint64_t *>(t->err + 4);   // behind the error block
    if (e == hipSuccess) e = hipMalloc(&t->dbg_cnt, 256);
    if (e == hipSuccess)
        e = hipHostMalloc(reinterpret_cast<void **>(&t->fin_host), 128, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void **>(&t->fin_dev), t->fin_host, 0);
    if (e == hipSuccess) std::fill(t->fin_host, t->fin_host + 16, 0ull);
    if (e == hipSuccess) e = hipMemsetAsync(t->dbg_cnt, 0, 256, ctx->stream);
    if (e != hipSuccess) {
        igx_groupby_destroy(t);
        return igx_fail(ctx, IGX_ENOMEM, "groupby_create: %s", hipGetErrorString(e));
    }
    // tuning / A-B knob (tools/gpu/ab_modes.sh): the initial mode, as igx_groupby_set_mode
    if (const char *m = std::getenv("IGX_GB_MODE")) {
        const unsigned long v = std::strtoul(m, nullptr, 0);
        if (v <= IGX_GB_PART && !(t->wide && v == IGX_GB_CACHED)) t->mode = (uint32_t)v;   // no cached form on a wide table
    }
    if (const char *m = std::getenv("IGX_GB_PERSIST")) t->persist = std::strtoul(m, nullptr, 0) != 0;   // A/B knob
    if (const char *m = std::getenv("IGX_GB_SEED")) t->seed_on = std::strtoul(m, nullptr, 0) != 0;       // A/B knob
    *out = t;
    return igx_groupby_reset(t);
}

static bool fin_landed(const igx_table *t) {
    return __atomic_load_n(t->fin_host + 3, __ATOMIC_ACQUIRE) == t->fin_seq;
}

extern "C" int igx_groupby_reset(igx_table *t) {
    if (!t) return IGX_EINVAL;
    igx_ctx *ctx = t->ctx;
    // an asynchronous finalize whose read-back has landed is collected now (its AUTO
    // bookkeeping then steers this interval); one still in flight is collected by a later
    // call, so a reset never waits for the device.  A collected error is returned after the
    // reset is done.
    if (t->fin_pending && fin_landed(t)) (void)fin_collect(t, nullptr);
    const int pending_rc = t->fin_status;
    t->fin_status = IGX_OK;
    // A new interval is a new epoch: records of older epochs read as empty and a claimer
    // initialises its value record, so only the bitmap and the error word are cleared.
    bool wrapped = false;
    if (++t->ep > EP_MAX) {
        hipLaunchKernelGGL(k_table_clear, dim3(2048), dim3(256), 0, ctx->stream, t->krec, t->krec_len, t->koff,
                           t->nslots);
        IGX_HIP(ctx, hipGetLastError());
        t->ep = 1;
        wrapped = true;
        // Seeds are identified by their generation's first epoch (*seed_gep), and epochs repeat
        // after the wrap: a table's first generation and the one after the wrap both start at
        // epoch 1.  The cleared table holds none of the seeds' slots, so they end here -- not when
        // the wrapped interval's read-back is collected (fin_apply), which under asynchronous
        // finalizes is usually after the next interval has adopted them.
        t->nseeds = 0;
        t->seed_left = 0;
    }
    // The generation goes on (the device checks its key count) when the last interval's groups
    // were listed by a finalize after its last update and this interval is planned in the cached
    // form (the direct and partitioned forms start their own: k_gen_restart if the plan changes).
    ResetGen rg{};
    rg.gen = reinterpret_cast<uint64_t *>(t->err) + GEN_WORD;
    rg.ep = t->ep;
    // the most keys a generation may hold after an interval: 4/5 of the slots (a 1 024-slot probe
    // region then overflows only past 7 standard deviations of its expected fill)
    const uint64_t fill = t->nslots / 5 * 4;
    rg.limit = fill > t->cap ? fill - t->cap : 0;
    rg.groups = t->groups;
    rg.ng = t->n_groups;
    rg.vrec = t->vrec;
    rg.vw = t->vrec_len / 8;
    const bool planned_cached = !(t->wide || t->mode == IGX_GB_DIRECT || t->mode == IGX_GB_PART ||
                                  (t->mode == IGX_GB_AUTO && t->direct_left > 0));
    rg.may = t->persist && !wrapped && t->fin_since_update && rg.limit > 0 && planned_cached ? 1u : 0u;
    t->gen_planned = rg.may != 0;
    // the bitmap, the error bits and the LDS-miss count (and the byte map if it holds claims)
    const uint64_t nb16 = t->occb_dirty ? t->occ_words * 2 : 0;
    const uint64_t grid = rg.may ? 2048 : std::min<uint64_t>(1024, (std::max(t->occ_words / 4, nb16) + 255) / 256 + 1);
    hipLaunchKernelGGL(k_reset_clear, dim3((unsigned)grid), dim3(256), 0, ctx->stream, t->occ, t->occ_words, t->err,
                       reinterpret_cast<uint4 *>(t->occb), nb16, rg);
    t->occb_dirty = false;
    IGX_HIP(ctx, hipGetLastError());
    t->rows_fed = 0;
    t->host_groups = 0;
    t->fin_current = false;
    return pending_rc;
}

extern "C" int igx_groupby_destroy(igx_table *t) {
    if (!t) return IGX_OK;
    (void)hipStreamSynchronize(t->ctx->stream);
    (void)hipFree(t->krec);
    (void)hipFree(t->vrec);
    (void)hipFree(t->err);
    (void)hipFree(t->groups);
    (void)hipFree(t->tile_cnt);
    (void)hipFree(t->occ);
    (void)hipFree(t->occb);
    (void)hipFree(t->dbg_cnt);
    (void)hipFree(t->seeds);
    (void)hipFree(t->seed_slots);
    (void)hipFree(t->seed_gep);
    if (t->seed_tab) igx_groupby_destroy(t->seed_tab);
    (void)hipFree(t->p_recs);
    (void)hipFree(t->p_cnt);
    (void)hipFree(t->p_mask);
    (void)hipFree(t->lg_recs);
    (void)hipFree(t->lg_bk);
    (void)hipFree(t->lg_cnt);
    for (auto &h : t->tk) (void)hipFree(h.slots);
    (void)hipFree(t->tk_state);
    for (auto *p : t->text) (void)hipFree(p);
    if (t->fin_host) (void)hipHostFree(t->fin_host);
    delete t;
    return IGX_OK;
}

constexpr uint64_t DIRECT_MISS_PCT = 90;        // AUTO: LDS-miss share that selects the partitioned form
// LDS-miss share (per mille of rows) above which a loader wave becomes a prober, and below
// which it turns back: a band, so a stream near the threshold does not flip the roles every
// interval.  Measured: C5 (~42 % misses) 6.15 -> 5.95-6.02 ms with 7 loaders,
// C2 (~35 %) 3.69 -> 3.86 ms, so C2 keeps 8 -- the band sits between the two.
constexpr uint64_t MORE_PROBERS_ON_PM = 390;
constexpr uint64_t MORE_PROBERS_OFF_PM = 370;
constexpr uint32_t DIRECT_RUN = 16;             // ... for this many intervals
constexpr uint64_t PROBE_ROWS = 16u << 20;      // rows the re-probe replays (C4: 16M of 125M)
// the cached form's sample-seeded LDS cache (k_gb_cached.hip, gb_seeds_compute)
constexpr uint32_t SEED_EVERY = 16;   // round 6: 8 -> 16 and rows / 64 -> rows / 128 (profiles/r06/seed_period_ab.txt)
constexpr uint64_t SEED_MIN_ROWS = 8u << 20;    // smaller updates: no seeds (IGX_GB_SEED_MIN overrides)

// one update in the interval's form, over the table's key layout (each form's entry point
// dispatches over gb_with_layout in its own translation unit)
static int launch_form(igx_table *t, GbArgs &a) {
    igx_ctx *ctx = t->ctx;
    const uint64_t want = (a.n + GTB - 1) / GTB;
    const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)ctx->num_cus));
    if (t->interval_part && t->interval_probe && t->rows_fed == a.n) {
        t->probe_rows = std::min<uint64_t>(a.n, PROBE_ROWS);
        const int rc = gb_launch_estimate(t, a, blocks, t->probe_rows);
        if (rc) return rc;
    }
    if (t->interval_part) {
        const GbArgs saved = a;   // the partitioned form turns the fused predicates into a row mask
        const int rc = gb_launch_part(t, a);
        if (rc != IGX_ENOMEM || t->mode != IGX_GB_AUTO) return rc;
        // AUTO picked the partitioned form on its own and its scratch does not fit: this
        // update runs cached instead (the forms share the table protocol, so they may mix
        // within an interval), and AUTO measures again at the next interval
        (void)hipGetLastError();
        if (t->wide) {   // no cached form: the rest of the interval runs direct (finalize then also
            t->interval_part = false;   // reads the occupancy off the tags, OR-ed into the claimers' bits)
            t->interval_direct = true;
            a = saved;
            return gb_launch_direct(t, a);
        }
        if (t->interval_probe)   // the cached kernel measures this interval itself: drop the estimate
            IGX_HIP(ctx, hipMemsetAsync(t->err + 2, 0, 8, ctx->stream));
        t->interval_part = false;
        t->interval_probe = false;
        t->direct_left = 0;
        a = saved;
    }
    if (t->interval_direct) return gb_launch_direct(t, a);
    if (t->wide) return igx_fail(ctx, IGX_ENOTSUP, "groupby_update: no cached form on a wide table");
    t->occb_dirty = true;   // the cached form's claims mark the byte map
    if (t->rows_fed == a.n) {   // the interval's first update decides whether it is seeded
        uint64_t min_rows = SEED_MIN_ROWS;
        if (const char *m = std::getenv("IGX_GB_SEED_MIN")) min_rows = std::strtoull(m, nullptr, 0);
        t->interval_seeded = false;
        // static key layouts only (the reference's BPF key structs)
        // (a debug kernel runs unseeded, so that its ablations compare like with like -- except
        // when it only counts, bit 3: then it counts what the production kernel would see)
        if (!t->generic && t->seed_on && t->gen_planned && (!a.dbg || a.dbg == 8u) && a.n >= min_rows) {
            if (t->seed_left == 0 || !t->nseeds) {
                uint32_t every = SEED_EVERY;
                if (const char *e = std::getenv("IGX_GB_SEED_EVERY"))   // A/B knob
                    every = std::max<uint32_t>(1, (uint32_t)std::strtoul(e, nullptr, 0));
                if (gb_seeds_compute(t, a) == IGX_OK) t->seed_left = every;
                else t->nseeds = 0;   // no seeds this time (the sample table failed): plain cache
            }
            --t->seed_left;
            t->interval_seeded = t->nseeds > 0;
        }
    }
    if (t->interval_seeded) {
        a.seeds = t->seeds;
        a.seed_gep = t->seed_gep;
        a.nseeds = t->nseeds;
    }
    // the update log: the server waves stream the misses' sums, two passes add them (k_gb_log.hip)
    int rc = gb_log_prepare(t, a, blocks);
    if (rc) return rc;
    if ((rc = gb_launch_cached(t, a, blocks))) return rc;
    return gb_log_launch(t, a, blocks);
}

extern "C" int igx_groupby_set_mode(igx_table *t, uint32_t mode) {
    if (!t) return IGX_EINVAL;
    if (mode > IGX_GB_PART) return igx_fail(t->ctx, IGX_EINVAL, "groupby_set_mode: mode %u", mode);
    if (t->wide && mode == IGX_GB_CACHED)
        return igx_fail(t->ctx, IGX_ENOTSUP, "groupby_set_mode: the cached form is not available on a wide table "
                                             "(%llu slots x %u B of key records; 64-bit record addressing)",
                        (unsigned long long)t->nslots, t->krec_len);
    t->mode = mode;
    t->direct_left = 0;
    return IGX_OK;
}

extern "C" int igx_groupby_update(igx_table *t, const igx_col *cols, uint32_t ncols, const uint32_t *key_cols,
                                  const igx_pred *preds, uint32_t npreds, uint64_t nrows, uint64_t base_idx) {
    return igx_groupby_update_ex(t, cols, ncols, key_cols, preds, npreds, nullptr, IGX_NO_COL, nrows, base_idx);
}

// ---- one update's GbArgs, piece by piece (igx_groupby_update_ex calls them in this order) ----

// the key columns.  Key column 0 (a.kcol[0]) doubles as the dummy column: any readable dword
// for loads whose result is discarded (padding words, COUNT, no cond, unused predicate slots)
static int plan_keys(igx_table *t, const igx_col *cols, uint32_t ncols, const uint32_t *key_cols, GbArgs &a) {
    igx_ctx *ctx = t->ctx;
    uint32_t w = 0;
    for (uint32_t k = 0; k < t->nkeys; ++k) {
        const uint32_t ci = key_cols[k];
        if (ci >= ncols) return igx_fail(ctx, IGX_EINVAL, "groupby_update: key column %u out of range", ci);
        const igx_col &c = cols[ci];
        if (c.width != t->key_widths[k])
            return igx_fail(ctx, IGX_EINVAL, "groupby_update: key column %u width %u != %u", k, c.width,
                            t->key_widths[k]);
        const uint8_t *p = static_cast<const uint8_t *>(c.ptr);
        const bool odd = c.width > 2 && c.width % 4;   // 3, 5, 6, 7, 9, ... bytes: byte loads
        const uintptr_t need = odd ? 1 : (c.width >= 16 ? 16 : (c.width >= 4 ? 4 : c.width));
        if (reinterpret_cast<uintptr_t>(p) & (need - 1))
            return igx_fail(ctx, IGX_EINVAL, "groupby_update: key column %u misaligned", k);
        a.kcol[k] = p;
        const uint32_t nw = (c.width + 3) / 4;
        for (uint32_t j = 0; j < nw; ++j, ++w) {
            a.kptr[w] = p;
            a.kwidth[w] = c.width;
            a.koff[w] = 4 * j;
            a.kmask[w] = c.width >= 4 ? 0xFFFFFFFFu : ((1u << (8 * c.width)) - 1u);
            a.kbytes[w] = odd ? std::min<uint32_t>(4, c.width - 4 * j) : 0;
        }
    }
    for (; w < KWMAX; ++w) {
        a.kptr[w] = a.kcol[0];
        a.kwidth[w] = 0;
        a.koff[w] = 0;
        a.kmask[w] = 0;
    }
    return IGX_OK;
}

// Scalar columns other than keys (aggregate values and conditions, predicates, guards, the
// nil mask) are read as the aligned dwords that hold each row, formed from the column's
// base: a base off a 4-byte boundary would make them misaligned loads that run up to three
// bytes past the column's last 4-byte block.
static bool misaligned(const igx_col &c) {
    return (reinterpret_cast<uintptr_t>(c.ptr) & (c.width == 8 ? 7u : 3u)) != 0;
}

// the aggregates' value and condition columns, and which of them share a load
static int plan_aggs(igx_table *t, const igx_col *cols, uint32_t ncols, GbArgs &a) {
    igx_ctx *ctx = t->ctx;
    const uint8_t *dummy = a.kcol[0];
    a.naggs = t->naggs;
    for (uint32_t x = t->naggs; x < AMAX; ++x) {   // unused slots are still loaded (issue_row)
        a.vptr[x] = a.cptr[x] = dummy;
        a.vwidth[x] = a.cwidth[x] = 1;
    }
    for (uint32_t x = 0; x < t->naggs; ++x) {
        const igx_agg &g = t->aggs[x];
        a.vcount[x] = g.kind == IGX_AGG_COUNT;
        a.vptr[x] = dummy;
        a.vwidth[x] = 1;
        if (!a.vcount[x]) {
            if (g.col >= ncols) return igx_fail(ctx, IGX_EINVAL, "groupby_update: agg column out of range");
            a.vptr[x] = static_cast<const uint8_t *>(cols[g.col].ptr);
            a.vwidth[x] = cols[g.col].width;
            a.vsign[x] = cols[g.col].kind == IGX_KIND_INT;
            if (!igx_scalar_width(a.vwidth[x]))
                return igx_fail(ctx, IGX_ENOTSUP, "groupby_update: agg width %u", a.vwidth[x]);
            if (cols[g.col].kind == IGX_KIND_FLOAT)
                return igx_fail(ctx, IGX_ENOTSUP, "groupby_update: float sums are not supported");
            if (misaligned(cols[g.col]))
                return igx_fail(ctx, IGX_EINVAL, "groupby_update: value column of aggregate %u misaligned", x);
            if (g.divisor > 1) {
                if (a.vsign[x])
                    return igx_fail(ctx, IGX_ENOTSUP, "groupby_update: divisor on a signed column");
                a.vdiv[x] = g.divisor;
            }
        }
        a.cptr[x] = dummy;
        a.cwidth[x] = 1;
        if (g.cond_col != IGX_NO_COL) {
            if (g.cond_col >= ncols) return igx_fail(ctx, IGX_EINVAL, "groupby_update: cond column out of range");
            const uint32_t cw = cols[g.cond_col].width;
            if (!igx_scalar_width(cw))
                return igx_fail(ctx, IGX_ENOTSUP, "groupby_update: condition width %u", cw);
            if (misaligned(cols[g.cond_col]))
                return igx_fail(ctx, IGX_EINVAL, "groupby_update: condition column of aggregate %u misaligned", x);
            a.cptr[x] = static_cast<const uint8_t *>(cols[g.cond_col].ptr);
            a.cwidth[x] = cw;
            a.cval[x] = cw == 8 ? g.cond_val : (g.cond_val & ((1ull << (8 * cw)) - 1));
            a.hascond[x] = 1;
        }
    }
    for (uint32_t x = 0; x < AMAX; ++x) {
        a.vshare[x] = a.cshare[x] = AMAX;
        a.vload[x] = x < t->naggs && !a.vcount[x];
        a.cload[x] = x < t->naggs && a.hascond[x];
        for (uint32_t y = 0; y < x; ++y) {
            if (a.vload[x] && a.vshare[x] == AMAX && a.vload[y] && a.vptr[y] == a.vptr[x] && a.vwidth[y] == a.vwidth[x]) {
                a.vshare[x] = y;
                a.vload[x] = 0;
            }
            if (a.cload[x] && a.cshare[x] == AMAX && a.cload[y] && a.cptr[y] == a.cptr[x] && a.cwidth[y] == a.cwidth[x]) {
                a.cshare[x] = y;
                a.cload[x] = 0;
            }
        }
    }
    for (uint32_t x = 0; x < AMAX; ++x) {
        a.vldw[x] = a.vload[x] ? a.vwidth[x] : 0;
        a.cldw[x] = a.cload[x] ? a.cwidth[x] : 0;
        a.vhioff[x] = a.vload[x] && a.vwidth[x] == 8 ? 4 : 0;
        a.chioff[x] = a.cload[x] && a.cwidth[x] == 8 ? 4 : 0;
    }
    return IGX_OK;
}

// Up to PMAX scalar comparisons (and IN sets) are fused into the kernel; any others --
// more predicates, regex or string rules -- are AND-ed into a row mask first by a scan
// with the filter's predicate evaluator (k_common.h), which then masks rows like `valid`.
// (dry: plan only, nothing is launched -- predicates that would need the mask scan fail with IGX_ENOTSUP)
static int plan_preds(igx_table *t, const igx_col *cols, uint32_t ncols, const igx_pred *preds, uint32_t npreds,
                      const uint8_t *valid, uint64_t nrows, GbArgs &a, bool dry = false) {
    igx_ctx *ctx = t->ctx;
    const uint8_t *dummy = a.kcol[0];
    std::vector<igx_pred> fused, masked;
    // a guard is fused when it is the condition column of an aggregate (whose raw value the
    // kernel holds anyway): that aggregate's index, else AMAX
    auto guard_agg = [&](const igx_pred &q) -> uint32_t {
        const igx_col &g = cols[q.guard_col];
        for (uint32_t x = 0; x < t->naggs; ++x)
            if (a.hascond[x] && a.cptr[x] == static_cast<const uint8_t *>(g.ptr) && a.cwidth[x] == g.width) return x;
        return AMAX;
    };
    // a scalar comparison, or on such a column an IN set (or a comparison number past it, which
    // the fused plan below rejects by that number), unless a guard keeps it out
    auto fusable = [&](const igx_pred &q) {
        const igx_col &c = cols[q.col];
        return igx_scalar_cmp(c.kind, c.width, q.cmp >= IGX_CMP_IN ? (uint32_t)IGX_CMP_EQ : q.cmp) &&
               !(q.guard_len && guard_agg(q) == AMAX);
    };
    for (uint32_t p = 0; p < npreds; ++p) {
        if (preds[p].col >= ncols) return igx_fail(ctx, IGX_EINVAL, "groupby_update: predicate column out of range");
        if (preds[p].guard_len) {
            const int rc = igx_check_guard(ctx, cols, ncols, preds[p]);
            if (rc) return rc;
            if (misaligned(cols[preds[p].guard_col]))
                return igx_fail(ctx, IGX_EINVAL, "groupby_update: guard column of predicate %u misaligned", p);
        }
        if (cols[preds[p].col].kind != IGX_KIND_BYTES && misaligned(cols[preds[p].col]))
            return igx_fail(ctx, IGX_EINVAL, "groupby_update: predicate column %u misaligned", p);
        if (preds[p].cmp == IGX_CMP_IN && !fusable(preds[p])) {   // the mask scan has no set test
            if (preds[p].guard_len && guard_agg(preds[p]) == AMAX)
                return igx_fail(ctx, IGX_ENOTSUP, "groupby_update: IN predicate %u is guarded by a column that is no "
                                                  "aggregate's condition column (not supported)", p);
            return igx_fail(ctx, IGX_EINVAL, "groupby_update: IN predicate %u needs an integer column of 1, 2, 4 "
                                             "or 8 bytes", p);
        }
        (fusable(preds[p]) ? fused : masked).push_back(preds[p]);
    }
    while (fused.size() > PMAX) {   // overflow into the mask, set tests (IN) last: the mask scan has none
        auto it = std::find_if(fused.begin(), fused.end(), [](const igx_pred &q) { return q.cmp != IGX_CMP_IN; });
        if (it == fused.end())
            return igx_fail(ctx, IGX_ENOTSUP, "groupby_update: more than %d set-membership predicates", PMAX);
        masked.push_back(*it);
        fused.erase(it);
    }
    if (!masked.empty() && dry) return IGX_ENOTSUP;
    if (!masked.empty()) {
        int rc = grow(ctx, reinterpret_cast<void **>(&t->p_mask), &t->p_mask_bytes, igx_align(nrows, 256));
        if (rc) return rc;
        const uint8_t *in = valid;
        for (size_t b = 0; b < masked.size(); b += IGX_KMAX_PREDS) {
            DevPreds dp;
            rc = igx_build_preds(ctx, cols, ncols, masked.data() + b,
                                 (uint32_t)std::min<size_t>(IGX_KMAX_PREDS, masked.size() - b), &dp);
            if (rc) return rc;
            hipLaunchKernelGGL(k_pred_mask, dim3((unsigned)std::min<uint64_t>(4096, (nrows + 255) / 256)), dim3(256), 0,
                               ctx->stream, dp, in, nrows, t->p_mask);
            IGX_HIP(ctx, hipGetLastError());
            in = t->p_mask;
        }
        valid = t->p_mask;
    }
    preds = fused.data();
    npreds = (uint32_t)fused.size();
    for (uint32_t p = 0; p < npreds; ++p) {
        const igx_pred &q = preds[p];
        const igx_col &c = cols[q.col];
        if (q.cmp == IGX_CMP_IN) {
            if (q.ref_len == 0 || q.ref_len % c.width || q.ref_len > 8 || c.kind == IGX_KIND_FLOAT)
                return igx_fail(ctx, IGX_EINVAL, "groupby_update: IN predicate %u needs 1..8/width "
                                                 "integer values", p);
            a.pcnt[p] = q.ref_len / c.width;
        } else if (q.cmp > IGX_CMP_GE) {
            return igx_fail(ctx, IGX_EINVAL, "groupby_update: predicate %u comparison %u", p, q.cmp);
        }
        a.pptr[p] = static_cast<const uint8_t *>(c.ptr);
        a.pwidth[p] = c.width;
        a.pkind[p] = c.kind;
        a.pcmp[p] = q.cmp;
        a.pneg[p] = q.negate;
        a.pref[p] = igx_pack_ref(q.ref, q.cmp == IGX_CMP_IN ? q.ref_len : c.width);
        a.pldw[p] = c.width;
        a.pshare[p] = a.pguard[p] = AMAX;
        for (uint32_t x = 0; x < t->naggs; ++x)   // the value column of an aggregate: reuse its load
            if (a.pshare[p] == AMAX && !a.vcount[x] && a.vptr[x] == a.pptr[p] && a.vwidth[x] == c.width) {
                a.pshare[p] = x;
                a.pldw[p] = 0;
            }
        a.gptr[p] = dummy;
        if (q.guard_len) {
            a.pguard[p] = guard_agg(q);
            a.gptr[p] = static_cast<const uint8_t *>(cols[q.guard_col].ptr);
            a.gwidth[p] = q.guard_len;
            a.gref[p] = igx_pack_ref(q.guard_ref, q.guard_len);
        }
    }
    for (uint32_t p = npreds; p < PMAX; ++p) {
        a.pptr[p] = a.gptr[p] = dummy;
        a.pwidth[p] = a.pldw[p] = 0;
        a.pshare[p] = a.pguard[p] = AMAX;
    }
    for (uint32_t p = 0; p < PMAX; ++p) a.phioff[p] = a.pwidth[p] == 8 ? 4 : 0;
    a.npred = npreds;
    a.valid = valid;
    a.validp = valid ? valid : dummy;
    a.validw = valid ? 1 : 0;
    return IGX_OK;
}

// the rows' indices, the table's records and the per-call knobs
static int bind_table(igx_table *t, const igx_col *cols, uint32_t ncols, uint32_t idx_col, uint64_t nrows,
                      uint64_t base_idx, GbArgs &a) {
    igx_ctx *ctx = t->ctx;
    a.fidx = nullptr;
    if (idx_col != IGX_NO_COL) {
        if (idx_col >= ncols || cols[idx_col].width != 8)
            return igx_fail(ctx, IGX_EINVAL, "groupby_update: index column must be a u64 column");
        a.fidx = static_cast<const uint64_t *>(cols[idx_col].ptr);
    }
    a.n = nrows;
    a.base_idx = base_idx;
    bind_records(t, a);
    if (const char *d = std::getenv("IGX_GB_DEBUG")) a.dbg = (uint32_t)std::strtoul(d, nullptr, 0);
    t->rowplan_on = true;
    if (const char *d = std::getenv("IGX_GB_ROWPLAN")) t->rowplan_on = std::strtoul(d, nullptr, 0) != 0;   // A/B and test knob
    // one loader wave fewer (one prober more) after intervals that missed the cache on more
    // than MORE_PROBERS_ON_PM / 1000 of their rows (until one falls below MORE_PROBERS_OFF_PM)
    a.nl = t->more_probers ? NL_DEFAULT - 1 : NL_DEFAULT;
    if (const char *d = std::getenv("IGX_GB_LOADERS")) {   // tuning knob
        const unsigned long v = std::strtoul(d, nullptr, 0);
        if (v >= 1 && v <= NWAVES - 2) a.nl = (uint32_t)v;
    }
    a.admit_mask = 1;
    a.sm = t->prefer_sm ? 1u : 0u;
    a.direct = 0;
    if (const char *d = std::getenv("IGX_GB_DIRECT")) a.direct = std::strtoul(d, nullptr, 0) ? 1u : 0u;   // ablation
    if (const char *d = std::getenv("IGX_GB_PROBER")) a.sm = std::strtoul(d, nullptr, 0) ? 1u : 0u;   // ablation
    if (const char *d = std::getenv("IGX_GB_ADMIT"))   // ablation: 0 first-miss admission, k: on the (k+1)-th
        a.admit_mask = std::min<uint32_t>(3u, (uint32_t)std::strtoul(d, nullptr, 0));
    return IGX_OK;
}

// the interval's form is fixed by its first update (the LDS-miss count that drives AUTO
// is only meaningful for a whole interval of the cached form)
static int choose_form(igx_table *t, const GbArgs &a) {
    igx_ctx *ctx = t->ctx;
    if (t->rows_fed == a.n) {
        t->interval_direct = t->mode == IGX_GB_DIRECT;
        // a wide table has no cached form: AUTO plans every interval partitioned (no run to
        // count down, no re-probe of the stream)
        t->interval_part = t->mode == IGX_GB_PART || (t->mode == IGX_GB_AUTO && (t->wide || t->direct_left > 0));
        t->interval_probe = false;
        t->probe_rows = 0;
        if (t->mode == IGX_GB_AUTO && !t->wide && t->direct_left > 0) t->interval_probe = --t->direct_left == 0;
        t->interval_region = false;
        if (t->region_off > 0) --t->region_off;
    }
    if (std::getenv("IGX_GB_DEBUG") && !t->wide) t->interval_direct = t->interval_part = false;   // diagnostics: cached form
    if (t->gen_planned && (t->interval_direct || t->interval_part)) {
        hipLaunchKernelGGL(k_gen_restart, dim3(1), dim3(1), 0, ctx->stream, a.gen, t->ep);
        IGX_HIP(ctx, hipGetLastError());
        t->gen_planned = false;
    }
    return IGX_OK;
}

extern "C" int igx_groupby_update_ex(igx_table *t, const igx_col *cols, uint32_t ncols, const uint32_t *key_cols,
                                     const igx_pred *preds, uint32_t npreds, const uint8_t *valid, uint32_t idx_col,
                                     uint64_t nrows, uint64_t base_idx) {
    if (!t) return IGX_EINVAL;
    igx_ctx *ctx = t->ctx;
    if (nrows == 0) return IGX_OK;
    if (!cols || !key_cols) return igx_fail(ctx, IGX_EINVAL, "groupby_update: null columns");
    if (nrows >= (1ull << 32)) return igx_fail(ctx, IGX_EINVAL, "groupby_update: more than 2^32 rows in one call");
    // `ready` carries first_ins + 1 (a kept key's: index + 2) in 48 bits: the last row's index stays
    // below IDX_LIMIT (written so that a base_idx near 2^64 cannot wrap past the test)
    if (base_idx >= IDX_LIMIT || nrows > IDX_LIMIT - base_idx)
        return igx_fail(ctx, IGX_EINVAL, "groupby_update: event indices reach 2^48 (rebase the interval's indices)");
    t->rows_fed += nrows;
    t->fin_since_update = false;
    t->fin_current = false;
    GbArgs a{};
    int rc = plan_keys(t, cols, ncols, key_cols, a);
    if (rc) return rc;
    if (valid && (reinterpret_cast<uintptr_t>(valid) & 3u))
        return igx_fail(ctx, IGX_EINVAL, "groupby_update: valid mask misaligned");
    if ((rc = plan_aggs(t, cols, ncols, a))) return rc;
    if ((rc = plan_preds(t, cols, ncols, preds, npreds, valid, nrows, a))) return rc;
    if ((rc = bind_table(t, cols, ncols, idx_col, nrows, base_idx, a))) return rc;
    if ((rc = choose_form(t, a))) return rc;
    if ((rc = launch_form(t, a))) return rc;
    IGX_HIP(ctx, hipGetLastError());
    return IGX_OK;
}

extern "C" int igx_groupby_rowplan(igx_table *t) { return t ? t->rowplan_last : 0; }

// The registry's answer for an update described as igx_groupby_create and igx_groupby_update_ex
// describe it, without a table or a device: the update is planned as usual (column pointers are
// compared, never read) and matched as gb_launch_cached matches it.
extern "C" int igx_groupby_rowplan_match(const uint32_t *key_widths, uint32_t nkeys, const igx_agg *aggs,
                                         uint32_t naggs, const igx_col *cols, uint32_t ncols,
                                         const uint32_t *key_cols, const igx_pred *preds, uint32_t npreds,
                                         const uint8_t *valid, uint32_t idx_col) {
    if (!key_widths || !cols || !key_cols || nkeys == 0 || nkeys > 16 || naggs > AMAX || (naggs && !aggs)) return 0;
    igx_table t{};
    t.nkeys = nkeys;
    for (uint32_t k = 0; k < nkeys; ++k) {
        t.key_widths[k] = key_widths[k];
        t.key_words += (key_widths[k] + 3) / 4;
    }
    t.naggs = naggs;
    for (uint32_t x = 0; x < naggs; ++x) t.aggs[x] = aggs[x];
    GbArgs a{};
    if (plan_keys(&t, cols, ncols, key_cols, a) || plan_aggs(&t, cols, ncols, a) ||
        plan_preds(&t, cols, ncols, preds, npreds, valid, 0, a, true))
        return 0;
    if (idx_col != IGX_NO_COL) a.fidx = reinterpret_cast<const uint64_t *>(cols);   // present: any non-null value
    int plan = 0;
    (void)gb_with_layout(&t, [&](auto tag) {
        plan = plan_for_update<typename decltype(tag)::type>(a);
        return (int)IGX_OK;
    });
    return plan;
}

// finalize's device part: the occupied-slot list and the group count, then the count, the
// error word and the LDS-miss count copied to the table's pinned read-back buffer
static int fin_launch(igx_table *t) {
    igx_ctx *ctx = t->ctx;
    const uint64_t tiles = (t->nslots + CT - 1) / CT;
    if (t->interval_direct)
        hipLaunchKernelGGL(k_occ_from_tags, dim3((unsigned)((t->occ_words + 255) / 256)), dim3(256), 0, ctx->stream,
                           t->krec, t->krec_len, t->koff, t->nslots, t->ep, t->occ);
    hipLaunchKernelGGL(k_slots_count, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, t->occ, t->occ_words,
                       t->tile_cnt, t->occb_dirty ? t->occb : (uint8_t *)nullptr);
    t->occb_dirty = false;
    t->fin_since_update = true;
    t->fin_current = true;
    // the kernel that finds the group count also writes the read-back into fin_host
    const uint64_t seq = ++t->fin_seq;
    t->fin_snap.rows_fed = t->rows_fed;
    t->fin_snap.direct = t->interval_direct;
    t->fin_snap.part = t->interval_part;
    t->fin_snap.region = t->interval_region;
    t->fin_snap.probe = t->interval_part && t->interval_probe;
    t->fin_snap.sampled = t->probe_rows;
    if (tiles <= SLOTS_INLINE_TILES) {
        hipLaunchKernelGGL(k_slots_write, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, t->occ, t->occ_words,
                           (const uint32_t *)nullptr, t->tile_cnt, t->groups, t->n_groups, t->err, t->fin_dev, seq, t->ep);
    } else {
        hipLaunchKernelGGL(k_slots_scan, dim3(1), dim3(1024), 0, ctx->stream, t->tile_cnt, tiles, t->n_groups, t->err,
                           t->fin_dev, seq, t->ep);
        hipLaunchKernelGGL(k_slots_write, dim3((unsigned)tiles), dim3(256), 0, ctx->stream, t->occ, t->occ_words,
                           t->tile_cnt, (const uint32_t *)nullptr, t->groups, (uint64_t *)nullptr, t->err, t->fin_dev, seq, t->ep);
    }
    IGX_HIP(ctx, hipGetLastError());
    return IGX_OK;
}

static void fin_view(igx_table *t, igx_table_view *view, uint64_t ng) {
    if (!view) return;
    view->n_groups = ng;
    view->n_slots = t->nslots;
    view->key_bytes = t->key_words * 4;
    view->key_stride = t->krec_len;
    view->val_stride = t->vrec_len;
    view->naggs = t->naggs;
    view->keys = t->krec;
    for (uint32_t x = 0; x < 16; ++x) view->aggs[x] = x < t->naggs ? t->vrec + 1 + x : nullptr;
    view->first_idx = t->vrec;
    view->groups = t->groups;
    view->d_n_groups = t->n_groups;
}

// finalize's host part, once the read-back has landed: the count, the AUTO bookkeeping and
// the interval's status
static int fin_apply(igx_table *t) {
    igx_ctx *ctx = t->ctx;
    const uint64_t *h = t->fin_host;   // err block {bits, pad, LDS misses} | group count
    const uint32_t err = reinterpret_cast<const uint32_t *>(h)[0];
    const uint64_t misses = h[1];
    const uint64_t ng = h[2];
    const uint32_t spilled = reinterpret_cast<const uint32_t *>(h)[1];   // a region overflowed
    t->claims_last = h[4];
    t->gen_keys = h[5];
    for (int x = 0; x < 4; ++x) t->log_last[x] = h[LOG_STAT_WORD + x];
    if (h[4] == ng || h[5] == ~0ull) t->seed_left = 0;   // a generation started or ended: fresh seeds
    const auto &f = t->fin_snap;   // the interval this read-back belongs to
    if (spilled && f.region) t->region_off = DIRECT_RUN + 1;
    t->host_groups = ng;
    // Miss-heavy streams (most rows miss the LDS cache: near-uniform, high-cardinality keys)
    // go faster with the state-machine probers; hit-heavy ones with the batch probers.  When
    // nearly every row missed, the cache is pure overhead: AUTO runs the next DIRECT_RUN
    // intervals in the partitioned form (streamed passes instead of a random HBM probe per
    // row; C4: 4.1 vs 4.4 ms direct, 6.4 ms cached); the last of them re-probes the stream with
    // k_gb_estimate on a sample, and only a stream that has stopped missing goes cached again.
    if (f.rows_fed >= 1000000 && !f.direct && !f.part) {
        t->prefer_sm = misses * 10 > f.rows_fed * 7;
        t->miss_pm = (uint32_t)(misses * 1000 / f.rows_fed);
        t->more_probers = t->miss_pm > (t->more_probers ? MORE_PROBERS_OFF_PM : MORE_PROBERS_ON_PM);
        if (t->mode == IGX_GB_AUTO && misses * 100 > f.rows_fed * DIRECT_MISS_PCT) t->direct_left = DIRECT_RUN;
    }
    // the probe interval (partitioned, with k_gb_estimate on a sample): still nearly all misses
    // -> another run of partitioned intervals; otherwise the next interval runs cached and
    // measures the stream itself
    if (f.probe && f.sampled && t->mode == IGX_GB_AUTO && misses * 100 > f.sampled * DIRECT_MISS_PCT)
        t->direct_left = DIRECT_RUN;
    if (err) return igx_fail(ctx, IGX_ENOSPC, "groupby: table full or probe failure (err=%u)", err);
    if (ng > t->cap)
        return igx_fail(ctx, IGX_ENOSPC, "groupby: %llu distinct keys exceed capacity %llu",
                        (unsigned long long)ng, (unsigned long long)t->cap);
    return IGX_OK;
}

// waits for a pending asynchronous finalize and applies it; its status is kept in fin_status
// until a call returns it (igx_groupby_wait, reset, finalize)
int fin_collect(igx_table *t, uint64_t *n_groups) {
    if (t->fin_pending) {
        t->fin_pending = false;
        // poll the sequence number; once the stream has drained it must be there
        while (!fin_landed(t)) {
            const hipError_t q = hipStreamQuery(t->ctx->stream);
            if (q == hipSuccess) {
                if (fin_landed(t)) break;
                return t->fin_status = igx_fail(t->ctx, IGX_EIO, "groupby: finalize read-back did not land");
            }
            if (q != hipErrorNotReady) IGX_HIP(t->ctx, q);
            std::this_thread::yield();
        }
        const int rc = fin_apply(t);
        if (rc && !t->fin_status) {
            t->fin_status = rc;
            t->fin_status_seq = t->fin_seq;
        }
    }
    if (n_groups) *n_groups = t->host_groups;
    return t->fin_status;
}

extern "C" int igx_groupby_finalize(igx_table *t, igx_table_view *view) {
    if (!t) return IGX_EINVAL;
    igx_ctx *ctx = t->ctx;
    (void)fin_collect(t, nullptr);   // the read-back buffer is about to be reused
    int rc = fin_launch(t);
    if (rc) return rc;
    IGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    rc = fin_apply(t);
    fin_view(t, view, t->host_groups);
    if (!rc) rc = t->fin_status;     // an earlier asynchronous finalize's error is not lost
    t->fin_status = IGX_OK;
    return rc;
}

extern "C" int igx_groupby_finalize_async(igx_table *t, igx_table_view *view) {
    if (!t) return IGX_EINVAL;
    igx_ctx *ctx = t->ctx;
    // the previous interval's read-back (it precedes this interval) is collected first.  A
    // failure of that interval is returned by this call WITHOUT issuing this interval (the view
    // is left untouched), once: a non-zero return always means "not finalized", and calling
    // again issues the interval.  igx_groupby_wait reports an interval's own status only.
    (void)fin_collect(t, nullptr);
    if (const int earlier = t->fin_status) {
        const uint64_t earlier_seq = t->fin_status_seq;
        t->fin_status = IGX_OK;
        const std::string why = igx_last_error(ctx);   // the collected interval's message
        return igx_fail(ctx, earlier, "groupby: the previous interval (finalize %llu) failed: %s; this interval "
                                      "was not finalized",
                        (unsigned long long)earlier_seq, why.c_str());
    }
    const int rc = fin_launch(t);
    if (rc) return rc;
    t->fin_pending = true;
    fin_view(t, view, 0);
    return IGX_OK;
}

extern "C" int igx_groupby_wait(igx_table *t, uint64_t *n_groups) {
    if (!t) return IGX_EINVAL;
    int rc = fin_collect(t, n_groups);
    if (rc && t->fin_status_seq != t->fin_seq) rc = IGX_OK;   // an older interval's (never reached here)
    t->fin_status = IGX_OK;
    return rc;
}

extern "C" int igx_groupby_info(igx_table *t, igx_groupby_info_t *out) {
    if (!t || !out) return IGX_EINVAL;
    std::memset(out, 0, sizeof *out);
    if (t->rows_fed)
        out->form = t->interval_part ? IGX_GB_PART : (t->interval_direct ? IGX_GB_DIRECT : IGX_GB_CACHED);
    out->region = t->interval_part && t->interval_region ? 1u : 0u;
    out->part_left = t->direct_left;
    out->exact_left = t->region_off;
    out->sm_probers = t->prefer_sm ? 1u : 0u;
    out->loaders = t->more_probers ? NL_DEFAULT - 1 : NL_DEFAULT;
    out->miss_permille = t->miss_pm;
    out->rows = t->rows_fed;
    out->claims = t->claims_last;
    out->gen_keys = t->gen_keys;
    out->persist = t->persist ? 1u : 0u;
    return IGX_OK;
}

extern "C" int igx_groupby_log_stats(igx_table *t, igx_groupby_log_stats_t *out) {
    if (!t || !out) return IGX_EINVAL;
    out->logged = t->log_last[0];
    out->fallback_value = t->log_last[1];
    out->fallback_log_full = t->log_last[2];
    out->fallback_bucket_full = t->log_last[3];
    return IGX_OK;
}

// per aggregate: the mask that wraps it to its out_width, as (lo, hi) words
static uint64_t agg_out_mask(const igx_table *t, uint32_t x) {
    const uint32_t ow = t->aggs[x].out_width;
    return (ow == 0 || ow >= 8) ? ~0ull : ((1ull << (8 * ow)) - 1);
}
static AggMasks agg_masks(const igx_table *t) {
    AggMasks am{};
    for (uint32_t x = 0; x < t->naggs; ++x) {
        const uint64_t m = agg_out_mask(t, x);
        am.m[2 * x] = (uint32_t)m;
        am.m[2 * x + 1] = (uint32_t)(m >> 32);
    }
    return am;
}

extern "C" int igx_groupby_gather(igx_table *t, const uint32_t *idx, uint64_t k, uint8_t *out_rows) {
    if (!t) return IGX_EINVAL;
    igx_ctx *ctx = t->ctx;
    if (k == 0) return IGX_OK;
    if (!idx || !out_rows) return igx_fail(ctx, IGX_EINVAL, "groupby_gather: null argument");
    hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)k), dim3(64), 0, ctx->stream, t->krec, t->krec_len, t->vrec,
                       t->vrec_len / 8, t->key_words, t->naggs, agg_masks(t), idx, t->nslots, k, out_rows);
    IGX_HIP(ctx, hipGetLastError());
    return IGX_OK;
}

extern "C" int igx_groupby_select_ge(igx_table *t, uint32_t agg, uint64_t threshold, uint32_t *out_slots,
                                     uint64_t cap, uint64_t *d_count) {
    if (!t) return IGX_EINVAL;
    igx_ctx *ctx = t->ctx;
    if (!d_count || (cap && !out_slots)) return igx_fail(ctx, IGX_EINVAL, "groupby_select_ge: null argument");
    if (agg >= t->naggs) return igx_fail(ctx, IGX_EINVAL, "groupby_select_ge: aggregate %u of %u", agg, t->naggs);
    if (!t->fin_current) return igx_fail(ctx, IGX_EINVAL, "groupby_select_ge: the interval is not finalized");
    IGX_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(uint64_t), ctx->stream));
    // the group count is on the device: blocks for the most groups the table can list
    const uint64_t most = std::min<uint64_t>(t->cap, t->nslots);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((uint64_t)std::max(1, ctx->num_cus * 4), (most + 255) / 256);
    hipLaunchKernelGGL(k_select_ge, dim3(blocks), dim3(256), 0, ctx->stream, t->groups, t->n_groups, t->nslots, t->vrec,
                       t->vrec_len / 8, agg, agg_out_mask(t, agg), threshold, out_slots, cap,
                       reinterpret_cast<unsigned long long *>(d_count));
    IGX_HIP(ctx, hipGetLastError());
    return IGX_OK;
}

extern "C" int igx_groupby_lookup(igx_table *t, const uint8_t *keys, uint32_t key_stride, uint64_t n,
                                  uint8_t *out_rows, uint8_t *found) {
    if (!t) return IGX_EINVAL;
    igx_ctx *ctx = t->ctx;
    if (n == 0) return IGX_OK;
    if (!keys || !out_rows || !found) return igx_fail(ctx, IGX_EINVAL, "groupby_lookup: null argument");
    if (n >= (1ull << 32)) return igx_fail(ctx, IGX_EINVAL, "groupby_lookup: more than 2^32 keys");
    if (key_stride < t->key_words * 4 || (key_stride & 3) || (reinterpret_cast<uintptr_t>(keys) & 3) ||
        (reinterpret_cast<uintptr_t>(out_rows) & 3))
        return igx_fail(ctx, IGX_EINVAL, "groupby_lookup: keys must be 4-byte aligned, key_stride a multiple of 4 "
                                         "and at least %u", t->key_words * 4);
    if (!t->fin_current) return igx_fail(ctx, IGX_EINVAL, "groupby_lookup: the interval is not finalized");
    GbArgs a{};   // the table's side of the update kernels' arguments (the probe reads only part of it)
    a.naggs = t->naggs;
    bind_records(t, a);
    const AggMasks am = agg_masks(t);
    // the kernel over the table's key-record width: its layout's KW
    const int rc = gb_with_layout(t, [&](auto tag) {
        constexpr int KW = decltype(tag)::type::KW;
        hipLaunchKernelGGL(k_gb_lookup<KW>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, a, keys,
                           key_stride, n, t->key_words, am, out_rows, found);
        return (int)IGX_OK;
    });
    if (rc) return rc;
    IGX_HIP(ctx, hipGetLastError());
    return IGX_OK;
}

// Sort / top-K over the table's groups without materialising them (rows are the occupied
// slots; keys read through the slot list at the record stride).
extern "C" int igx_groupby_sort(igx_table *t, const igx_tsortkey *keys, uint32_t nkeys, uint32_t k,
                                uint32_t *out_slots) {
    if (!t) return IGX_EINVAL;
    igx_ctx *ctx = t->ctx;
    if (nkeys > 32) return igx_fail(ctx, IGX_ENOTSUP, "groupby_sort: more than 32 keys");
    // After an asynchronous finalize the group count is on the device: a top-K whose keys the
    // device selection handles (no float, no IP text) runs over at most min(capacity, slots)
    // rows bounded by that count; anything else waits for the count first.
    const uint64_t *d_count = nullptr;
    uint64_t nrows = t->host_groups;
    if (t->fin_pending) {
        bool dev_ok = k > 0 && k <= 4096 && 2ull * k < std::min<uint64_t>(t->cap, t->nslots);
        for (uint32_t i = 0; i < nkeys && dev_ok; ++i) {
            const igx_tsortkey &q = keys[i];
            if (q.src == IGX_TSRC_IPTEXT || (q.src == IGX_TSRC_KEY && q.kind == IGX_KIND_FLOAT)) dev_ok = false;
        }
        if (dev_ok) {
            d_count = t->n_groups;
            nrows = std::min<uint64_t>(t->cap, t->nslots);
        } else {
            (void)fin_collect(t, nullptr);   // its status stays for igx_groupby_wait / the next reset
            nrows = t->host_groups;
        }
    }
    igx_sortkey sk[32];
    uint32_t strides[32];
    uint32_t direct = 0;
    for (uint32_t i = 0; i < nkeys; ++i) {
        const igx_tsortkey &q = keys[i];
        sk[i] = igx_sortkey{};
        sk[i].desc = q.desc;
        strides[i] = t->vrec_len;
        if (q.src == IGX_TSRC_AGG) {
            if (q.index >= t->naggs) return igx_fail(ctx, IGX_EINVAL, "groupby_sort: aggregate %u", q.index);
            sk[i].ptr = t->vrec + 1 + q.index;   // little endian: the low out_width bytes
            sk[i].width = t->aggs[q.index].out_width ? t->aggs[q.index].out_width : 8;   // are the wrapped value
            sk[i].kind = IGX_KIND_UINT;
        } else if (q.src == IGX_TSRC_FIRST) {
            sk[i].ptr = t->vrec;
            sk[i].width = 8;
            sk[i].kind = IGX_KIND_UINT;
        } else if (q.src == IGX_TSRC_CONST) {
            sk[i].ptr = t->vrec;   // never read: width 0 marks a parity-only pass
            sk[i].width = 0;
            sk[i].kind = IGX_KIND_BYTES;
        } else if (q.src == IGX_TSRC_KEY) {
            if (q.offset + q.width > t->key_words * 4)
                return igx_fail(ctx, IGX_EINVAL, "groupby_sort: key bytes out of range");
            sk[i].ptr = t->krec + q.offset;
            strides[i] = t->krec_len;
            sk[i].width = q.width;
            sk[i].kind = q.kind;
        } else if (q.src == IGX_TSRC_IPTEXT) {
            // a Stats string column made from key bytes: render the groups' texts (in slot-list
            // order) and sort them as strings
            if (q.offset + 16 > t->key_words * 4 || q.index + 2 > t->key_words * 4)
                return igx_fail(ctx, IGX_EINVAL, "groupby_sort: address / family bytes out of range");
            const uint64_t ng = std::max<uint64_t>(t->host_groups, 1);
            if (t->text_rows[i] < ng) {
                (void)hipFree(t->text[i]);
                t->text[i] = nullptr;
                t->text_rows[i] = 0;
                IGX_HIP(ctx, hipMalloc(&t->text[i], ng * IGX_IPTEXT_WIDTH));
                t->text_rows[i] = ng;
            }
            const int rc = launch_ip_text(ctx, t->krec + q.offset, t->krec_len, t->krec + q.index, t->krec_len,
                                          t->groups, t->host_groups, t->text[i]);
            if (rc) return rc;
            sk[i].ptr = t->text[i];
            strides[i] = IGX_IPTEXT_WIDTH;
            sk[i].width = IGX_IPTEXT_WIDTH;
            sk[i].kind = IGX_KIND_BYTES;
            direct |= 1u << i;
        } else {
            return igx_fail(ctx, IGX_EINVAL, "groupby_sort: bad source");
        }
    }
    // the hint of the table's repeated top-K (k_sort.hip k_tk_*): any slots give an exact answer,
    // the last top-K's give a tight bound
    TopkHint hint{};
    igx_table::TkHint *th = nullptr;
    if (k > 0 && k <= TK_MAXK) {
        uint64_t sig = 0xcbf29ce484222325ull;   // FNV-1a over the sort's description
        auto mix = [&sig](uint64_t v) {
            for (int b = 0; b < 8; ++b) sig = (sig ^ ((v >> (8 * b)) & 0xFF)) * 0x100000001b3ull;
        };
        mix(k);
        mix(nkeys);
        for (uint32_t i = 0; i < nkeys; ++i) {
            const igx_tsortkey &q = keys[i];
            mix(q.src);
            mix(q.index);
            mix(q.desc);
            mix(q.offset);
            mix(q.width);
            mix(q.kind);
        }
        sig |= 1;
        for (auto &h : t->tk)
            if (h.sig == sig) th = &h;
        if (!th) {   // a new sort: the least recently used entry
            th = &t->tk[0];
            for (auto &h : t->tk)
                if (h.used < th->used) th = &h;
            th->sig = sig;
            th->nh = 0;
        }
        th->used = ++t->tk_clock;
        if (!th->slots) IGX_HIP(ctx, hipMalloc(&th->slots, TK_MAXK * 4));
        if (!t->tk_state) {
            IGX_HIP(ctx, hipMalloc(&t->tk_state, TK_STATE_BYTES));
            IGX_HIP(ctx, hipMemsetAsync(t->tk_state, 0, TK_STATE_BYTES, ctx->stream));
        }
        hint.slots = th->slots;
        hint.nh = th->nh;
        hint.occ = t->occ;
        hint.nslots = t->nslots;
        hint.state = t->tk_state;
    }
    const int rc = sort_common_rows(ctx, sk, strides, nkeys, nrows, t->groups, t->vrec, t->vrec_len, k, out_slots,
                                    direct, d_count, th ? &hint : nullptr);
    if (th) th->nh = rc == IGX_OK ? hint.nh : 0;
    return rc;
}

// Diagnostics: how the table's top-Ks were answered so far (synchronous).
extern "C" int igx_groupby_topk_counts(igx_table *t, uint64_t *out2) {
    if (!t || !out2) return IGX_EINVAL;
    igx_ctx *ctx = t->ctx;
    out2[0] = out2[1] = 0;
    if (!t->tk_state) return IGX_OK;
    uint32_t w[2];
    IGX_HIP(ctx, hipMemcpyAsync(w, t->tk_state + 14, 8, hipMemcpyDeviceToHost, ctx->stream));
    IGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    out2[0] = w[0];
    out2[1] = w[1];
    return IGX_OK;
}

// Diagnostics only: LDS-cache hit / miss counters collected when IGX_GB_DEBUG has bit 3.
extern "C" int igx_groupby_debug_counts(igx_table *t, uint64_t *out16) {   // out16: 32 words
    if (!t || !out16) return IGX_EINVAL;
    igx_ctx *ctx = t->ctx;
    IGX_HIP(ctx, hipMemcpyAsync(out16, t->dbg_cnt, 256, hipMemcpyDeviceToHost, ctx->stream));
    IGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    IGX_HIP(ctx, hipMemsetAsync(t->dbg_cnt, 0, 256, ctx->stream));
    return IGX_OK;
}
