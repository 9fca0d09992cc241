// k_scan.h -- the scans the sorted-run joins share (k_reqjoin.hip, k_lwjoin.hip, k_traceloop.hip)
// and the scan of per-tile counts that every stream-order compaction runs (k_join.hip,
// k_filter.hip, k_stack.hip).  Device code.
//
// A summary scan is written against an operator struct beside the join's kernels:
//   struct Op {
//       using T = ...;                            // the summary (k_reqjoin.h, k_lwjoin.h, k_traceloop.h)
//       static T identity();
//       static T combine(const T &x, const T &y); // x's range, then y's
//       static T shfl_up(const T &v, int o);      // field by field: the pad words stay where they are
//   };
#pragma once

#include "k_common.h"

constexpr int SCAN_TB = 256;                  // threads of a tile's workgroup
constexpr int SCAN_RPT = 8;                   // consecutive positions per thread
constexpr int SCAN_TILE = SCAN_TB * SCAN_RPT; // 2048 positions per scan tile

// Exclusive scan of the threads' summaries over a workgroup of SCAN_TB; wsum holds one summary
// per wave, and *total is the tile's summary (valid in every thread).
template <class Op>
__device__ __forceinline__ typename Op::T block_scan(const typename Op::T &mine, typename Op::T *wsum,
                                                     typename Op::T *total) {
    using T = typename Op::T;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T lo = Op::shfl_up(inc, o);
        if (lane >= (uint32_t)o) inc = Op::combine(lo, inc);
    }
    if (lane == 63) wsum[wave] = inc;
    T exc = Op::shfl_up(inc, 1);
    if (lane == 0) exc = Op::identity();
    __syncthreads();
    T pre = Op::identity(), tot = Op::identity();
#pragma unroll
    for (int w = 0; w < SCAN_TB / 64; ++w) {
        if ((uint32_t)w == wave) pre = tot;
        tot = Op::combine(tot, wsum[w]);
    }
    *total = tot;
    return Op::combine(pre, exc);
}

// carry[t] = the summary of tiles [0, t); the body of a kernel of one workgroup of NT threads
template <class Op, int NT>
__device__ __forceinline__ void tile_carry(const typename Op::T *__restrict__ sums, uint64_t m,
                                           typename Op::T *__restrict__ carry) {
    using T = typename Op::T;
    __shared__ T part[NT];
    const uint64_t per = (m + NT - 1) / NT;
    const uint64_t b = min(m, (uint64_t)threadIdx.x * per), e = min(m, b + per);
    T s = Op::identity();
    for (uint64_t i = b; i < e; ++i) s = Op::combine(s, sums[i]);
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
        T lo = Op::identity();
        if (threadIdx.x >= (unsigned)d) lo = part[threadIdx.x - d];
        __syncthreads();
        if (threadIdx.x >= (unsigned)d) part[threadIdx.x] = Op::combine(lo, part[threadIdx.x]);
        __syncthreads();
    }
    T run = threadIdx.x ? part[threadIdx.x - 1] : Op::identity();
    for (uint64_t i = b; i < e; ++i) {
        carry[i] = run;
        run = Op::combine(run, sums[i]);
    }
}

// Exclusive scan of cnt[0..m) -> off[0..m) by one workgroup of 1024.  Returns the sum through
// the calling thread's share of cnt: in thread 1023, the total.
__device__ __forceinline__ uint64_t scan_counts(const uint32_t *__restrict__ cnt, uint64_t m,
                                                uint64_t *__restrict__ off) {
    __shared__ uint64_t part[1024];
    const uint64_t per = (m + 1023) / 1024;
    const uint64_t b = min(m, (uint64_t)threadIdx.x * per), e = min(m, b + per);
    uint64_t s = 0;
    for (uint64_t i = b; i < e; ++i) s += cnt[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const uint64_t v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t run = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (uint64_t i = b; i < e; ++i) {
        off[i] = run;
        run += cnt[i];
    }
    return part[threadIdx.x];
}
