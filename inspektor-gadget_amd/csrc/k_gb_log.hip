// k_gb_log.hip -- the cached form's update log ("The update log"): the sums of the
// rows that miss the LDS cache, streamed instead of issued as one memory-side atomic each.
//
// The cached kernel's server waves write their updates as 8-byte records {value, (slot << 2) |
// aggregate} into one log region per workgroup (ring_serve, k_gb_cached.hip).  Two passes on the
// same stream then apply them:
//   k_gbl_part    sorts tiles of the logs by bucket (slot >> bshift) in LDS and writes each
//                 bucket's records of a tile as one run into the bucket's region, reserved with
//                 one returning atomic per (tile, bucket);
//   k_gbl_reduce  one workgroup per bucket: 64-bit LDS accumulators per (slot, aggregate), records
//                 added with LDS atomics, every non-zero accumulator added to its value record.
// Counts are read on the device; neither kernel waits on another workgroup.  A record that finds
// its bucket region full is added from the partition pass, so the result is exact at any size.
#include "k_gb_table.h"

namespace {

constexpr uint32_t LOG_TILE = 16384;                 // records per partition tile (128 KB of LDS)
constexpr uint32_t LOG_TB = 1024;                    // threads of both kernels
constexpr uint32_t LOG_RPT = LOG_TILE / LOG_TB;      // records per thread of a tile
constexpr uint32_t LOG_NB_MAX = 1024;                // buckets (the partition's LDS counters)
constexpr size_t LOG_ACC_BYTES = 128 * 1024;         // LDS accumulators of one bucket
constexpr uint32_t LOG_CNT_WORDS = 4096;             // workgroup counters, then LOG_NB_MAX bucket counters
constexpr uint32_t LOG_BCNT_OFF = LOG_CNT_WORDS - LOG_NB_MAX;
constexpr uint64_t LOG_COLD_ROWS = 8192;             // sizing: rows per workgroup that may all miss
constexpr uint64_t LOG_BUCKET_SLACK = 16384;         // sizing: records per bucket beyond its share

struct LogArgs {
    const uint64_t *log;      // nwg regions of cap records
    const uint32_t *wcnt;     // records in each (nulls included)
    uint64_t *bk;             // nb regions of bcap records
    uint32_t *bcnt;           // records reserved in each (may pass bcap); the reduce pass zeroes it
    uint64_t *vrec;
    uint32_t *err;
    uint32_t cap, nwg, bcap, nb;
    uint32_t bshift;          // bucket = slot >> bshift
    uint32_t spb;             // slots per bucket (1 << bshift)
    uint32_t naggs, vrec_words;
    uint64_t nslots;
};

__device__ __forceinline__ unsigned long long *log_agg(const LogArgs &a, uint32_t slot, uint32_t x) {
    return reinterpret_cast<unsigned long long *>(a.vrec + (uint64_t)slot * a.vrec_words + 1 + x);
}

// tile t: records [ti * LOG_TILE, ...) of workgroup t % nwg's region (consecutive tiles come from
// different regions, so the regions' empty tails are spread over the grid)
__global__ __launch_bounds__(LOG_TB) void k_gbl_part(LogArgs a) {
    extern __shared__ uint64_t sorted[];   // LOG_TILE records
    __shared__ uint32_t cnt[LOG_NB_MAX], off[LOG_NB_MAX], gbase[LOG_NB_MAX], wsum[LOG_TB / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t wg = blockIdx.x % a.nwg, ti = blockIdx.x / a.nwg;
    const uint32_t have = min(a.wcnt[wg], a.cap);
    const uint64_t start = (uint64_t)ti * LOG_TILE;
    if (start >= have) return;
    const uint32_t m = (uint32_t)min((uint64_t)LOG_TILE, have - start);
    const uint64_t *src = a.log + (uint64_t)wg * a.cap + start;
    cnt[tid] = 0;
    __syncthreads();
    uint64_t rec[LOG_RPT];
    uint32_t rank[LOG_RPT];
#pragma unroll
    for (uint32_t k = 0; k < LOG_RPT; ++k) {
        const uint32_t i = k * LOG_TB + tid;
        rec[k] = i < m ? __builtin_nontemporal_load(src + i) : ~0ull;
    }
#pragma unroll
    for (uint32_t k = 0; k < LOG_RPT; ++k) {
        const uint32_t hi = (uint32_t)(rec[k] >> 32);
        rank[k] = 0;
        if (hi == LOG_NULL_HI) continue;
        if ((hi >> 2) >= a.nslots || (hi & 3u) >= a.naggs) {   // never expected: fail, do not write
            atomicOr(a.err, 16u);
            rec[k] = ~0ull;
            continue;
        }
        rank[k] = atomicAdd(&cnt[(hi >> 2) >> a.bshift], 1u);
    }
    __syncthreads();
    // one reservation per bucket with records, and the exclusive scan of the counts
    const uint32_t c = cnt[tid];
    gbase[tid] = c ? atomicAdd(&a.bcnt[tid], c) : 0u;
    uint32_t inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(inc, d);
        if ((int)lane >= d) inc += u;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < wave; ++w) before += wsum[w];
    off[tid] = before + inc - c;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < LOG_RPT; ++k) {
        const uint32_t hi = (uint32_t)(rec[k] >> 32);
        if (hi != LOG_NULL_HI) sorted[off[(hi >> 2) >> a.bshift] + rank[k]] = rec[k];
    }
    __syncthreads();
    const uint32_t total = off[LOG_NB_MAX - 1] + cnt[LOG_NB_MAX - 1];
    uint32_t nfull = 0;
    for (uint32_t i = tid; i < total; i += LOG_TB) {
        const uint64_t r = sorted[i];
        const uint32_t hi = (uint32_t)(r >> 32), b = (hi >> 2) >> a.bshift;
        const uint64_t j = (uint64_t)gbase[b] + (i - off[b]);
        if (j < a.bcap) {
            __builtin_nontemporal_store(r, a.bk + (uint64_t)b * a.bcap + j);
        } else {   // the bucket's region is full: add it here
            gadd(log_agg(a, hi >> 2, hi & 3u), (unsigned long long)(uint32_t)r);
            ++nfull;
        }
    }
    if (__ballot(nfull != 0)) {
        for (int o = 32; o > 0; o >>= 1) nfull += __shfl_xor(nfull, o);
        if (lane == 0)
            atomicAdd(reinterpret_cast<unsigned long long *>(a.err) + LOG_STAT_WORD + 3, (unsigned long long)nfull);
    }
}

__global__ __launch_bounds__(LOG_TB) void k_gbl_reduce(LogArgs a) {
    extern __shared__ uint64_t acc[];   // spb x naggs
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    const uint32_t nacc = a.spb * a.naggs;
    const uint32_t have = min(a.bcnt[b], a.bcap);
    if (!have) return;   // uniform: nothing reserved, nothing to zero
    for (uint32_t q = tid; q < nacc; q += LOG_TB) acc[q] = 0;
    __syncthreads();
    const uint64_t *src = a.bk + (uint64_t)b * a.bcap;
    constexpr uint32_t U = 4;
    for (uint32_t i0 = tid; i0 < have; i0 += U * LOG_TB) {
        uint64_t r[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t i = i0 + u * LOG_TB;
            r[u] = i < have ? __builtin_nontemporal_load(src + i) : ~0ull;
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t hi = (uint32_t)(r[u] >> 32);
            if (hi == LOG_NULL_HI) continue;
            const uint32_t q = ((hi >> 2) & (a.spb - 1)) * a.naggs + (hi & 3u);
            atomicAdd(reinterpret_cast<unsigned long long *>(&acc[q]), (unsigned long long)(uint32_t)r[u]);
        }
    }
    __syncthreads();
    // a record's aggregates from adjacent lanes: one memory-side request per value record
    for (uint32_t q = tid; q < nacc; q += LOG_TB) {
        const uint64_t v = acc[q];
        const uint32_t s = q / a.naggs, x = q - s * a.naggs;
        if (v) gadd(log_agg(a, b * a.spb + s, x), (unsigned long long)v);
    }
    if (tid == 0) a.bcnt[b] = 0;   // the next logged update starts from empty regions
}

// slots per bucket: the most (a power of two) whose accumulators fit LOG_ACC_BYTES
uint32_t log_spb(const igx_table *t) {
    uint32_t spb = 1;
    while ((size_t)spb * 2 * t->naggs * 8 <= LOG_ACC_BYTES) spb <<= 1;
    return (uint32_t)std::min<uint64_t>(spb, t->nslots);
}

}  // namespace

int gb_log_prepare(igx_table *t, GbArgs &a, uint32_t blocks) {
    a.log = nullptr;
    a.log_cnt = nullptr;
    a.log_cap = 0;
    if (t->wide || t->naggs < 1 || t->naggs > 4 || a.direct || a.dbg) return IGX_OK;
    if (t->nslots & (t->nslots - 1)) return IGX_OK;
    if (const char *d = std::getenv("IGX_GB_LOG"))
        if (std::strtoul(d, nullptr, 0) == 0) return IGX_OK;
    const uint32_t spb = log_spb(t);
    const uint64_t nb = t->nslots / spb;
    if (nb > LOG_NB_MAX || blocks > LOG_BCNT_OFF || t->nslots > LOG_SLOT_LIMIT) return IGX_OK;   // C5's 2^25 slots x 4: 8 192 buckets
    // Half a record per row covers the cached form's miss shares (above 90 % AUTO leaves the form).
    // A workgroup's first LOG_COLD_ROWS rows meet a cold cache and may miss every time, a record
    // per aggregate each: a short update (a thousand rows per workgroup) is nothing else.  What
    // does not fit goes out as atomics.
    const uint64_t rows_wg = (a.n + blocks - 1) / blocks;
    uint64_t cap = (rows_wg / 2 + std::min<uint64_t>(rows_wg, LOG_COLD_ROWS) * t->naggs + 63) & ~63ull;
    cap = std::max<uint64_t>(cap, 64);
    if (const char *d = std::getenv("IGX_GB_LOG_CAP")) cap = std::max<uint64_t>(1, std::strtoull(d, nullptr, 0));
    // a bucket's share of what the log can hold, a quarter more, and LOG_BUCKET_SLACK records for
    // the slots of hot keys (each workgroup logs a hot key a few times before its cache admits it)
    uint64_t bcap = (uint64_t)blocks * cap / nb * 5 / 4 + LOG_BUCKET_SLACK;
    if (const char *d = std::getenv("IGX_GB_LOG_BCAP")) bcap = std::max<uint64_t>(1, std::strtoull(d, nullptr, 0));
    if (cap >= (1ull << 31) || bcap >= (1ull << 31)) return IGX_OK;
    igx_ctx *ctx = t->ctx;
    if (!t->lg_cnt) {
        if (hipMalloc(&t->lg_cnt, LOG_CNT_WORDS * 4) != hipSuccess) {
            (void)hipGetLastError();
            t->lg_cnt = nullptr;
            return IGX_OK;
        }
        IGX_HIP(ctx, hipMemsetAsync(t->lg_cnt, 0, LOG_CNT_WORDS * 4, ctx->stream));
    }
    size_t have = t->lg_recs_bytes;
    if (grow(ctx, reinterpret_cast<void **>(&t->lg_recs), &have, (size_t)blocks * cap * 8) != IGX_OK) {
        (void)hipGetLastError();   // no room for the log: this update's sums go out as atomics
        t->lg_recs_bytes = 0;
        return IGX_OK;
    }
    t->lg_recs_bytes = have;
    have = t->lg_bk_bytes;
    if (grow(ctx, reinterpret_cast<void **>(&t->lg_bk), &have, (size_t)nb * bcap * 8) != IGX_OK) {
        (void)hipGetLastError();
        t->lg_bk_bytes = 0;
        return IGX_OK;
    }
    t->lg_bk_bytes = have;
    a.log = t->lg_recs;
    a.log_cnt = t->lg_cnt;
    a.log_cap = (uint32_t)cap;
    return IGX_OK;
}

int gb_log_launch(igx_table *t, const GbArgs &a, uint32_t blocks) {
    if (!a.log) return IGX_OK;
    igx_ctx *ctx = t->ctx;
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_gbl_part), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  LOG_TILE * 8);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_gbl_reduce),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, LOG_ACC_BYTES);
        attr = true;
    }
    LogArgs l{};
    l.log = a.log;
    l.wcnt = a.log_cnt;
    l.bk = t->lg_bk;
    l.bcnt = t->lg_cnt + LOG_BCNT_OFF;
    l.vrec = t->vrec;
    l.err = t->err;
    l.cap = a.log_cap;
    l.nwg = blocks;
    l.spb = log_spb(t);
    l.nb = (uint32_t)(t->nslots / l.spb);
    l.bshift = (uint32_t)__builtin_ctz(l.spb);
    l.naggs = t->naggs;
    l.vrec_words = t->vrec_len / 8;
    l.nslots = t->nslots;
    // the bucket regions are sized by gb_log_prepare for this update; a kept, larger allocation
    // only leaves more room per bucket
    l.bcap = (uint32_t)std::min<uint64_t>(t->lg_bk_bytes / 8 / l.nb, (1u << 31) - 1);
    if (const char *d = std::getenv("IGX_GB_LOG_BCAP"))
        l.bcap = (uint32_t)std::min<uint64_t>(l.bcap, std::max<uint64_t>(1, std::strtoull(d, nullptr, 0)));
    const uint32_t tiles = (a.log_cap + LOG_TILE - 1) / LOG_TILE;
    hipLaunchKernelGGL(k_gbl_part, dim3(blocks * tiles), dim3(LOG_TB), LOG_TILE * 8, ctx->stream, l);
    hipLaunchKernelGGL(k_gbl_reduce, dim3(l.nb), dim3(LOG_TB), (size_t)l.spb * l.naggs * 8, ctx->stream, l);
    IGX_HIP(ctx, hipGetLastError());
    return IGX_OK;
}
