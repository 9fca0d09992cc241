// k_reqjoin.hip -- block-I/O request pairing: the start / issue / done join by `struct request *`.
//
// Restates the map logic of top block-io (biotop.bpf.c:41-130: whobyreq and start keyed by the
// request, looked up and deleted by blk_account_io_done) and profile block-io
// (biolatency.bpf.c:47-154) over a batch of probe rows in stream order; include/igx.h has the
// contract.  No row walks its run: the state a row sees is an associative summary (k_reqjoin.h),
// scanned reduce-then-scan over the rows sorted by request.
//
//   sort     stable order of the row ids by req (launch_sort_perm: the LSD passes skip the
//            bytes that do not vary, and request pointers share their high bytes)
//   code     one byte per sorted position: the row's kind (or "does not exist") and whether
//            it starts a run of equal req -- the only pass that gathers req / kind / valid
//   summary  one RjSum per tile of RJ_TILE positions
//   carry    one workgroup: exclusive scan of the tile summaries
//   apply    per tile, from its carry: every DONE's outcome (its issue and who rows, one 8-byte
//            store at the done row) and, at the last row of each run, the run's live rows;
//            one flag byte per row
//   count / scan / compact   the flagged rows written out in stream order, as k_filter.hip does
//
// Every launch is a plain grid; no workgroup waits on another.  Algorithmic bytes per row:
// DESIGN.md §4.
#include "k_common.h"
#include "k_reqjoin.h"

namespace {

constexpr int TB = 256;
constexpr int RPT = 8;                // consecutive positions per thread
constexpr int RJ_TILE = TB * RPT;     // 2048 positions per scan tile
constexpr int CRPT = 4;
constexpr int CTILE = TB * CRPT;      // 1024 rows per compaction tile
constexpr int CGROUPS = CTILE / 64;   // wave-row groups per compaction tile
constexpr uint8_t F_DONE = 1, F_LIVE = 2;

__device__ __forceinline__ RjSum rj_shfl_up(const RjSum &v, int o) {
    RjSum r;
    r.id = __shfl_up((unsigned long long)v.id, o);
    r.s = __shfl_up(v.s, o);
    r.h = __shfl_up(v.h, o);
    r.ok = __shfl_up(v.ok, o);
    r.ld = __shfl_up(v.ld, o);
    r.lh = __shfl_up(v.lh, o);
    r.pad = 0;
    return r;
}

__global__ __launch_bounds__(TB) void k_rj_code(const uint64_t *__restrict__ req, const uint8_t *__restrict__ kind,
                                                const uint8_t *__restrict__ valid,
                                                const uint32_t *__restrict__ perm, uint64_t n,
                                                uint8_t *__restrict__ code) {
    const uint64_t p = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (p >= n) return;
    const uint32_t r = perm[p];
    const uint32_t k = kind[r];
    const bool live = k <= IGX_REQ_DONE && (!valid || valid[r] != 0);
    const bool head = p == 0 || req[r] != req[perm[p - 1]];
    code[p] = (uint8_t)((live ? k : RJ_NONE) | (head ? RJ_HEAD : 0u));
}

// The tile's RPT codes of this thread (RJ_NONE past n) and their summary.
__device__ __forceinline__ RjSum rj_thread_sum(const uint8_t *__restrict__ code, uint64_t p0, uint64_t n,
                                               uint32_t (&c)[RPT]) {
    // code is allocated to a multiple of RJ_TILE, so the 8-byte load stays inside it
    const uint64_t w = *reinterpret_cast<const uint64_t *>(code + p0);
    RjSum acc{};
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        c[j] = p0 + j < n ? (uint32_t)(w >> (8 * j)) & 7u : RJ_NONE;
        acc = rj_combine(acc, rj_elem((uint32_t)(p0 + j), c[j]));
    }
    return acc;
}

// Exclusive scan of the threads' summaries over the workgroup; *total is the tile's summary
// (valid in every thread).
__device__ __forceinline__ RjSum rj_block_scan(const RjSum &mine, RjSum *wsum, RjSum *total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    RjSum inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const RjSum lo = rj_shfl_up(inc, o);
        if (lane >= (uint32_t)o) inc = rj_combine(lo, inc);
    }
    if (lane == 63) wsum[wave] = inc;
    RjSum exc = rj_shfl_up(inc, 1);
    if (lane == 0) exc = RjSum{};
    __syncthreads();
    RjSum pre{}, tot{};
#pragma unroll
    for (int w = 0; w < TB / 64; ++w) {
        if ((uint32_t)w == wave) pre = tot;
        tot = rj_combine(tot, wsum[w]);
    }
    *total = tot;
    return rj_combine(pre, exc);
}

__global__ __launch_bounds__(TB) void k_rj_summary(const uint8_t *__restrict__ code, uint64_t n,
                                                   RjSum *__restrict__ sums) {
    __shared__ RjSum wsum[TB / 64];
    uint32_t c[RPT];
    const uint64_t p0 = (uint64_t)blockIdx.x * RJ_TILE + (uint64_t)threadIdx.x * RPT;
    const RjSum mine = rj_thread_sum(code, p0, n, c);
    RjSum total;
    (void)rj_block_scan(mine, wsum, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// carry[t] = the summary of tiles [0, t); one workgroup of 1024
__global__ __launch_bounds__(1024) void k_rj_carry(const RjSum *__restrict__ sums, uint64_t m,
                                                   RjSum *__restrict__ carry) {
    __shared__ RjSum part[1024];
    const uint64_t per = (m + 1023) / 1024;
    const uint64_t b = min(m, (uint64_t)threadIdx.x * per), e = min(m, b + per);
    RjSum s{};
    for (uint64_t i = b; i < e; ++i) s = rj_combine(s, sums[i]);
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        RjSum lo{};
        if (threadIdx.x >= (unsigned)d) lo = part[threadIdx.x - d];
        __syncthreads();
        if (threadIdx.x >= (unsigned)d) part[threadIdx.x] = rj_combine(lo, part[threadIdx.x]);
        __syncthreads();
    }
    RjSum run = threadIdx.x ? part[threadIdx.x - 1] : RjSum{};
    for (uint64_t i = b; i < e; ++i) {
        carry[i] = run;
        run = rj_combine(run, sums[i]);
    }
}

__global__ __launch_bounds__(TB) void k_rj_apply(const uint8_t *__restrict__ code,
                                                 const uint32_t *__restrict__ perm, uint64_t n,
                                                 const RjSum *__restrict__ carry, uint8_t *__restrict__ flags,
                                                 uint2 *__restrict__ t_pair) {
    __shared__ RjSum wsum[TB / 64];
    uint32_t c[RPT];
    const uint64_t p0 = (uint64_t)blockIdx.x * RJ_TILE + (uint64_t)threadIdx.x * RPT;
    const RjSum mine = rj_thread_sum(code, p0, n, c);
    RjSum total;
    const RjSum exc = rj_block_scan(mine, wsum, &total);
    if (p0 >= n) return;
    RjSum st = rj_combine(carry[blockIdx.x], exc);
    // the code after this thread's last one says whether that one ends its run
    const uint32_t after = p0 + RPT < n ? code[p0 + RPT] : RJ_HEAD;
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        const uint64_t p = p0 + j;
        if (p >= n) break;
        uint32_t issue = 0, who = 0;
        if (rj_step(st, (uint32_t)p, c[j], &issue, &who)) {
            const uint32_t r = perm[p];
            flags[r] = F_DONE;
            t_pair[r] = make_uint2(perm[issue - 1], who ? perm[who - 1] : IGX_NO_COL);
        }
        const uint32_t next = p + 1 >= n ? RJ_HEAD : (j + 1 < RPT ? c[(j + 1) % RPT] : after);
        if (next & RJ_HEAD) {
            uint32_t li, ls;
            rj_live(st, &li, &ls);
            if (li) flags[perm[li - 1]] = F_LIVE;
            if (ls) flags[perm[ls - 1]] = F_LIVE;
        }
    }
}

// ---- the flagged rows in stream order ---------------------------------------------------------
__global__ __launch_bounds__(TB) void k_rj_count(const uint8_t *__restrict__ flags, uint64_t n,
                                                 uint32_t *__restrict__ cnt_d, uint32_t *__restrict__ cnt_p) {
    __shared__ uint32_t wd[TB / 64], wp[TB / 64];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t d = 0, p = 0;
#pragma unroll
    for (int j = 0; j < CRPT; ++j) {
        const uint64_t row = (uint64_t)blockIdx.x * CTILE + (uint64_t)j * TB + threadIdx.x;
        const uint32_t f = row < n ? flags[row] : 0u;
        d += __popcll(__ballot(f == F_DONE));
        p += __popcll(__ballot(f == F_LIVE));
    }
    if (lane == 0) {
        wd[wave] = d;
        wp[wave] = p;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sd = 0, sp = 0;
        for (int w = 0; w < TB / 64; ++w) {
            sd += wd[w];
            sp += wp[w];
        }
        cnt_d[blockIdx.x] = sd;
        cnt_p[blockIdx.x] = sp;
    }
}

// exclusive scan of cnt[0..m) -> off[0..m), total -> *total; block 0 the DONE counts, block 1
// the live counts (each one workgroup of 1024 on its own array)
__global__ __launch_bounds__(1024) void k_rj_scan(const uint32_t *__restrict__ cnt_d,
                                                  const uint32_t *__restrict__ cnt_p, uint64_t m,
                                                  uint64_t *__restrict__ off_d, uint64_t *__restrict__ off_p,
                                                  uint64_t *__restrict__ tot_d, uint64_t *__restrict__ tot_p) {
    __shared__ uint64_t part[1024];
    const uint32_t *cnt = blockIdx.x ? cnt_p : cnt_d;
    uint64_t *off = blockIdx.x ? off_p : off_d;
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
    if (threadIdx.x == 1023) *(blockIdx.x ? tot_p : tot_d) = part[1023];
}

__global__ __launch_bounds__(TB) void k_rj_compact(const uint8_t *__restrict__ flags, uint64_t n,
                                                   const uint64_t *__restrict__ off_d,
                                                   const uint64_t *__restrict__ off_p,
                                                   const uint2 *__restrict__ t_pair,
                                                   const uint64_t *__restrict__ ts, uint32_t *__restrict__ done_row,
                                                   uint32_t *__restrict__ issue_row, uint32_t *__restrict__ who_row,
                                                   uint64_t *__restrict__ delta, uint32_t *__restrict__ pend_row,
                                                   uint64_t pend_cap) {
    __shared__ uint32_t gd[CGROUPS], gp[CGROUPS];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t f[CRPT];
    uint64_t bd[CRPT], bp[CRPT];
#pragma unroll
    for (int j = 0; j < CRPT; ++j) {
        const uint64_t row = (uint64_t)blockIdx.x * CTILE + (uint64_t)j * TB + threadIdx.x;
        f[j] = row < n ? flags[row] : 0u;
        bd[j] = __ballot(f[j] == F_DONE);
        bp[j] = __ballot(f[j] == F_LIVE);
        if (lane == 0) {   // group j * 4 + wave holds rows [64 * group, 64 * group + 64) of the tile
            gd[j * (TB / 64) + wave] = __popcll(bd[j]);
            gp[j * (TB / 64) + wave] = __popcll(bp[j]);
        }
    }
    __syncthreads();
    const uint64_t base_d = off_d[blockIdx.x], base_p = off_p[blockIdx.x];
#pragma unroll
    for (int j = 0; j < CRPT; ++j) {
        if (f[j] == 0) continue;
        const uint32_t g = j * (TB / 64) + wave;
        const uint32_t row = (uint32_t)((uint64_t)blockIdx.x * CTILE + (uint64_t)j * TB + threadIdx.x);
        uint32_t pre = 0;
        if (f[j] == F_DONE) {
            for (uint32_t w = 0; w < g; ++w) pre += gd[w];
            const uint64_t o = base_d + pre + __popcll(bd[j] & lanemask_lt());
            const uint2 pr = t_pair[row];
            done_row[o] = row;
            issue_row[o] = pr.x;
            who_row[o] = pr.y;
            delta[o] = ts[row] - ts[pr.x];
        } else {
            for (uint32_t w = 0; w < g; ++w) pre += gp[w];
            const uint64_t o = base_p + pre + __popcll(bp[j] & lanemask_lt());
            if (o < pend_cap) pend_row[o] = row;
        }
    }
}

}  // namespace

extern "C" int igx_req_join_tile(void) { return RJ_TILE; }

extern "C" int igx_req_join(igx_ctx *ctx, const uint64_t *req, const uint8_t *kind, const uint64_t *ts,
                            const uint8_t *valid, uint64_t nrows, uint32_t *done_row, uint32_t *issue_row,
                            uint32_t *who_row, uint64_t *delta, uint64_t *d_ndone, uint32_t *pend_row,
                            uint64_t pend_cap, uint64_t *d_npend) {
    if (!ctx) return IGX_EINVAL;
    if (nrows > 0xFFFFFFFEull) return igx_fail(ctx, IGX_EINVAL, "req_join: more than 2^32 - 2 rows");
    if (!d_ndone || !d_npend) return igx_fail(ctx, IGX_EINVAL, "req_join: null count");
    if (((uintptr_t)d_ndone | (uintptr_t)d_npend) & 7)
        return igx_fail(ctx, IGX_EINVAL, "req_join: counts not 8-byte aligned");
    if (nrows == 0) {
        IGX_HIP(ctx, hipMemsetAsync(d_ndone, 0, 8, ctx->stream));
        IGX_HIP(ctx, hipMemsetAsync(d_npend, 0, 8, ctx->stream));
        return IGX_OK;
    }
    if (!req || !kind || !ts || !done_row || !issue_row || !who_row || !delta || (pend_cap && !pend_row))
        return igx_fail(ctx, IGX_EINVAL, "req_join: null argument");
    if (((uintptr_t)req | (uintptr_t)ts | (uintptr_t)delta) & 7)
        return igx_fail(ctx, IGX_EINVAL, "req_join: req, ts and delta must be 8-byte aligned");
    if (((uintptr_t)done_row | (uintptr_t)issue_row | (uintptr_t)who_row | (uintptr_t)pend_row) & 3)
        return igx_fail(ctx, IGX_EINVAL, "req_join: row outputs must be 4-byte aligned");

    const uint64_t ntiles = (nrows + RJ_TILE - 1) / RJ_TILE, ctiles = (nrows + CTILE - 1) / CTILE;
    const size_t code_b = igx_align(ntiles * RJ_TILE, 256), flag_b = igx_align(nrows, 256);
    const size_t pair_b = igx_align(nrows * 8, 256), sum_b = igx_align(ntiles * sizeof(RjSum), 256);
    const size_t cnt_b = igx_align(ctiles * 4, 256), off_b = igx_align(ctiles * 8, 256);
    const size_t need = code_b + flag_b + pair_b + 2 * sum_b + 2 * cnt_b + 2 * off_b;
    void *s;
    // ask before the sort, so that an arena that has to grow does it before the order exists
    int rc = igx_scratch(ctx, need, &s);
    if (rc) return rc;
    // The order lives in delta (8 bytes per row, written last) while the scratch arena, which
    // the sort uses too, is handed from the sort to the passes below.
    uint32_t *perm = reinterpret_cast<uint32_t *>(delta);
    SortPlanKey key{};
    key.ptr = reinterpret_cast<const uint8_t *>(req);
    key.width = 8;
    key.kind = IGX_KIND_UINT;
    key.words = 2;
    key.stride = 8;
    rc = launch_sort_perm(ctx, &key, 1, nrows, nullptr, false, nullptr, perm, 0, nullptr);
    if (rc) return rc;
    rc = igx_scratch(ctx, need, &s);
    if (rc) return rc;
    char *c = reinterpret_cast<char *>(s);
    uint8_t *code = reinterpret_cast<uint8_t *>(c);
    uint8_t *flags = reinterpret_cast<uint8_t *>(c + code_b);
    uint2 *t_pair = reinterpret_cast<uint2 *>(c + code_b + flag_b);
    RjSum *sums = reinterpret_cast<RjSum *>(c + code_b + flag_b + pair_b);
    RjSum *carry = reinterpret_cast<RjSum *>(c + code_b + flag_b + pair_b + sum_b);
    char *q = c + code_b + flag_b + pair_b + 2 * sum_b;
    uint32_t *cnt_d = reinterpret_cast<uint32_t *>(q), *cnt_p = reinterpret_cast<uint32_t *>(q + cnt_b);
    uint64_t *off_d = reinterpret_cast<uint64_t *>(q + 2 * cnt_b);
    uint64_t *off_p = reinterpret_cast<uint64_t *>(q + 2 * cnt_b + off_b);

    IGX_HIP(ctx, hipMemsetAsync(flags, 0, flag_b, ctx->stream));
    hipLaunchKernelGGL(k_rj_code, dim3((unsigned)((nrows + TB - 1) / TB)), dim3(TB), 0, ctx->stream, req, kind, valid,
                       perm, nrows, code);
    hipLaunchKernelGGL(k_rj_summary, dim3((unsigned)ntiles), dim3(TB), 0, ctx->stream, code, nrows, sums);
    hipLaunchKernelGGL(k_rj_carry, dim3(1), dim3(1024), 0, ctx->stream, sums, ntiles, carry);
    hipLaunchKernelGGL(k_rj_apply, dim3((unsigned)ntiles), dim3(TB), 0, ctx->stream, code, perm, nrows, carry, flags,
                       t_pair);
    hipLaunchKernelGGL(k_rj_count, dim3((unsigned)ctiles), dim3(TB), 0, ctx->stream, flags, nrows, cnt_d, cnt_p);
    hipLaunchKernelGGL(k_rj_scan, dim3(2), dim3(1024), 0, ctx->stream, cnt_d, cnt_p, ctiles, off_d, off_p, d_ndone,
                       d_npend);
    hipLaunchKernelGGL(k_rj_compact, dim3((unsigned)ctiles), dim3(TB), 0, ctx->stream, flags, nrows, off_d, off_p,
                       t_pair, ts, done_row, issue_row, who_row, delta, pend_row, pend_cap);
    IGX_HIP(ctx, hipGetLastError());
    return IGX_OK;
}
