// k_join.hip -- the pipeline that the sorted-run joins by key share (k_reqjoin.hip, k_lwjoin.hip
// and through it k_chainjoin.hip): everything but the summary and the four passes that use it.
//
//   join_mark   scratch layout, the stable sort of the row ids by key, then the join's own
//               code / summary / carry / apply passes; leaves one flag byte per row
//               (JOIN_F_EMIT with the row's pair, JOIN_F_LIVE, or 0)
//   join_emit   count / scan / compact: the flagged rows written out in stream order, as
//               k_filter.hip does, the two classes side by side and the counts on the device
//
// Every launch is a plain grid; no workgroup waits on another.
#include "k_scan.h"

namespace {

constexpr int TB = 256;
constexpr int CRPT = 4;
constexpr int CTILE = TB * CRPT;      // 1024 rows per compaction tile
constexpr int CGROUPS = CTILE / 64;   // wave-row groups per compaction tile
constexpr uint8_t F_EMIT = JOIN_F_EMIT, F_LIVE = JOIN_F_LIVE;

__global__ __launch_bounds__(TB) void k_join_count(const uint8_t *__restrict__ flags, uint64_t n,
                                                   uint32_t *__restrict__ cnt_e, uint32_t *__restrict__ cnt_p) {
    __shared__ uint32_t we[TB / 64], wp[TB / 64];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t e = 0, p = 0;
#pragma unroll
    for (int j = 0; j < CRPT; ++j) {
        const uint64_t row = (uint64_t)blockIdx.x * CTILE + (uint64_t)j * TB + threadIdx.x;
        const uint32_t f = row < n ? flags[row] : 0u;
        e += __popcll(__ballot(f == F_EMIT));
        p += __popcll(__ballot(f == F_LIVE));
    }
    if (lane == 0) {
        we[wave] = e;
        wp[wave] = p;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t se = 0, sp = 0;
        for (int w = 0; w < TB / 64; ++w) {
            se += we[w];
            sp += wp[w];
        }
        cnt_e[blockIdx.x] = se;
        cnt_p[blockIdx.x] = sp;
    }
}

// block 0 the emitting counts, block 1 the live counts (each one workgroup of 1024 on its own array)
__global__ __launch_bounds__(1024) void k_join_scan(const uint32_t *__restrict__ cnt_e,
                                                    const uint32_t *__restrict__ cnt_p, uint64_t m,
                                                    uint64_t *__restrict__ off_e, uint64_t *__restrict__ off_p,
                                                    uint64_t *__restrict__ tot_e, uint64_t *__restrict__ tot_p) {
    const uint64_t total = scan_counts(blockIdx.x ? cnt_p : cnt_e, m, blockIdx.x ? off_p : off_e);
    if (threadIdx.x == 1023) *(blockIdx.x ? tot_p : tot_e) = total;
}

// what an emission writes beside its three rows: nothing, or the time since its A row
struct NoDelta {
    __device__ __forceinline__ void operator()(uint64_t, uint32_t, uint32_t) const {}
};
struct TsDelta {
    const uint64_t *__restrict__ ts;
    uint64_t *__restrict__ delta;
    __device__ __forceinline__ void operator()(uint64_t o, uint32_t row, uint32_t a) const { delta[o] = ts[row] - ts[a]; }
};

template <class Extra>
__global__ __launch_bounds__(TB) void k_join_compact(const uint8_t *__restrict__ flags, uint64_t n,
                                                     const uint64_t *__restrict__ off_e,
                                                     const uint64_t *__restrict__ off_p,
                                                     const uint2 *__restrict__ pair, uint32_t *__restrict__ emit_row,
                                                     uint32_t *__restrict__ a_row, uint32_t *__restrict__ b_row,
                                                     uint32_t *__restrict__ pend_row, uint64_t pend_cap, Extra extra) {
    __shared__ uint32_t ge[CGROUPS], gp[CGROUPS];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t f[CRPT];
    uint64_t be[CRPT], bp[CRPT];
#pragma unroll
    for (int j = 0; j < CRPT; ++j) {
        const uint64_t row = (uint64_t)blockIdx.x * CTILE + (uint64_t)j * TB + threadIdx.x;
        f[j] = row < n ? flags[row] : 0u;
        be[j] = __ballot(f[j] == F_EMIT);
        bp[j] = __ballot(f[j] == F_LIVE);
        if (lane == 0) {   // group j * 4 + wave holds rows [64 * group, 64 * group + 64) of the tile
            ge[j * (TB / 64) + wave] = __popcll(be[j]);
            gp[j * (TB / 64) + wave] = __popcll(bp[j]);
        }
    }
    __syncthreads();
    const uint64_t base_e = off_e[blockIdx.x], base_p = off_p[blockIdx.x];
#pragma unroll
    for (int j = 0; j < CRPT; ++j) {
        if (f[j] == 0) continue;
        const uint32_t g = j * (TB / 64) + wave;
        const uint32_t row = (uint32_t)((uint64_t)blockIdx.x * CTILE + (uint64_t)j * TB + threadIdx.x);
        uint32_t pre = 0;
        if (f[j] == F_EMIT) {
            for (uint32_t w = 0; w < g; ++w) pre += ge[w];
            const uint64_t o = base_e + pre + __popcll(be[j] & lanemask_lt());
            const uint2 pr = pair[row];
            emit_row[o] = row;
            a_row[o] = pr.x;
            b_row[o] = pr.y;
            extra(o, row, pr.x);
        } else {
            for (uint32_t w = 0; w < g; ++w) pre += gp[w];
            const uint64_t o = base_p + pre + __popcll(bp[j] & lanemask_lt());
            if (o < pend_cap) pend_row[o] = row;
        }
    }
}

// code | flags | pairs | tile summaries | carries | 2 x tile counts | 2 x tile offsets
JoinWork join_carve(IgxCarve &c, uint64_t nrows, size_t sum_bytes) {
    const uint64_t ntiles = (nrows + SCAN_TILE - 1) / SCAN_TILE, ctiles = (nrows + CTILE - 1) / CTILE;
    JoinWork w;
    w.code = c.take<uint8_t>(ntiles * SCAN_TILE);
    w.flags = c.take<uint8_t>(nrows);
    w.pair = c.take<uint2>(nrows * 8);
    w.sums = c.take<void>(ntiles * sum_bytes);
    w.carry = c.take<void>(ntiles * sum_bytes);
    w.cnt_e = c.take<uint32_t>(ctiles * 4);
    w.cnt_p = c.take<uint32_t>(ctiles * 4);
    w.off_e = c.take<uint64_t>(ctiles * 8);
    w.off_p = c.take<uint64_t>(ctiles * 8);
    return w;
}

}  // namespace

int join_mark(igx_ctx *ctx, size_t sum_bytes, JoinPasses passes, const uint64_t *key, const uint8_t *kind,
              const uint8_t *valid, uint64_t nrows, uint32_t *perm, JoinWork *w) {
    IgxCarve need{nullptr};
    (void)join_carve(need, nrows, sum_bytes);
    void *s;
    // ask before the sort, so that an arena that has to grow does it before the order exists
    int rc = igx_scratch(ctx, need.used, &s);
    if (rc) return rc;
    const SortPlanKey sk = sort_key_u64(key);
    rc = launch_sort_perm(ctx, &sk, 1, nrows, nullptr, false, nullptr, perm, 0, nullptr);
    if (rc) return rc;
    rc = igx_scratch(ctx, need.used, &s);
    if (rc) return rc;
    IgxCarve c{reinterpret_cast<char *>(s)};
    *w = join_carve(c, nrows, sum_bytes);
    IGX_HIP(ctx, hipMemsetAsync(w->flags, 0, igx_align(nrows, 256), ctx->stream));
    passes(ctx->stream, key, kind, valid, perm, nrows, *w);
    return IGX_OK;
}

int join_emit(igx_ctx *ctx, const JoinWork *w, uint64_t nrows, uint32_t *emit_row, uint32_t *a_row, uint32_t *b_row,
              uint64_t *d_nemit, uint32_t *pend_row, uint64_t pend_cap, uint64_t *d_npend, const uint64_t *ts,
              uint64_t *delta) {
    const dim3 ctiles((unsigned)((nrows + CTILE - 1) / CTILE));
    hipLaunchKernelGGL(k_join_count, ctiles, dim3(TB), 0, ctx->stream, w->flags, nrows, w->cnt_e, w->cnt_p);
    hipLaunchKernelGGL(k_join_scan, dim3(2), dim3(1024), 0, ctx->stream, w->cnt_e, w->cnt_p, (uint64_t)ctiles.x,
                       w->off_e, w->off_p, d_nemit, d_npend);
    const auto compact = [&](auto extra) {
        hipLaunchKernelGGL(k_join_compact<decltype(extra)>, ctiles, dim3(TB), 0, ctx->stream, w->flags, nrows,
                           w->off_e, w->off_p, w->pair, emit_row, a_row, b_row, pend_row, pend_cap, extra);
    };
    if (delta) compact(TsDelta{ts, delta});
    else compact(NoDelta{});
    IGX_HIP(ctx, hipGetLastError());
    return IGX_OK;
}
