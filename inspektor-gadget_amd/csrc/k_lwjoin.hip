// k_lwjoin.hip -- the two-register last-writer join by key: what a kprobe / kretprobe pair does
// through hash maps keyed by the thread.
//
// Restates the map logic of trace capabilities (capable.bpf.c:87-248: `start` written by the
// cap_capable kprobe, read and deleted by its kretprobe; `current_syscall` written by sys_enter,
// deleted by sys_exit and only read by the kretprobe) over a batch of probe rows in stream order;
// include/igx.h has the contract.  No row walks its run: the state a row sees is an associative
// summary (k_lwjoin.h), scanned reduce-then-scan over the rows sorted by key.  The pipeline is the
// one of k_reqjoin.hip:
//
//   sort     stable order of the row ids by key (launch_sort_perm)
//   code     one byte per sorted position: the row's kind (or "does not exist") and whether
//            it starts a run of equal key -- the only pass that gathers key / kind / valid
//   summary  one LwSum per tile of LW_TILE positions
//   carry    one workgroup: exclusive scan of the tile summaries
//   apply    per tile, from its carry: every TAKE_A's outcome (its A and B rows, one 8-byte
//            store at the take row) and, at the last row of each run, the rows the registers
//            hold; one flag byte per row
//   count / scan / compact   the flagged rows written out in stream order
//
// Every launch is a plain grid; no workgroup waits on another.  Algorithmic bytes per row:
// DESIGN.md §4.  The pipeline is callable in two halves (igx_internal.h: lw_join_mark through
// apply, lw_join_emit from count on) for the joins composed of it (k_chainjoin.hip); igx_lw_join
// is the two back to back.
#include "k_common.h"
#include "k_lwjoin.h"

static_assert(IGX_LW_SET_A == LW_SET_A && IGX_LW_SET_B == LW_SET_B && IGX_LW_CLEAR_B == LW_CLEAR_B &&
                  IGX_LW_TAKE_A == LW_TAKE_A,
              "enum igx_lw_kind and the codes of k_lwjoin.h");

namespace {

constexpr int TB = 256;
constexpr int RPT = 8;                // consecutive positions per thread
constexpr int LW_TILE = TB * RPT;     // 2048 positions per scan tile
constexpr int CRPT = 4;
constexpr int CTILE = TB * CRPT;      // 1024 rows per compaction tile
constexpr int CGROUPS = CTILE / 64;   // wave-row groups per compaction tile
constexpr uint8_t F_TAKE = LW_F_TAKE, F_LIVE = LW_F_LIVE;

__device__ __forceinline__ LwSum lw_shfl_up(const LwSum &v, int o) {
    LwSum r;
    r.a = __shfl_up((unsigned long long)v.a, o);
    r.b = __shfl_up((unsigned long long)v.b, o);
    r.h = __shfl_up(v.h, o);
    r.pad = 0;
    return r;
}

__global__ __launch_bounds__(TB) void k_lw_code(const uint64_t *__restrict__ key, const uint8_t *__restrict__ kind,
                                                const uint8_t *__restrict__ valid,
                                                const uint32_t *__restrict__ perm, uint64_t n,
                                                uint8_t *__restrict__ code) {
    const uint64_t p = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (p >= n) return;
    const uint32_t r = perm[p];
    const uint32_t k = kind[r];
    const bool live = k <= IGX_LW_TAKE_A && (!valid || valid[r] != 0);
    const bool head = p == 0 || key[r] != key[perm[p - 1]];
    code[p] = (uint8_t)((live ? k : LW_NONE) | (head ? LW_HEAD : 0u));
}

// The tile's RPT codes of this thread (LW_NONE past n) and their summary.
__device__ __forceinline__ LwSum lw_thread_sum(const uint8_t *__restrict__ code, uint64_t p0, uint64_t n,
                                               uint32_t (&c)[RPT]) {
    // code is allocated to a multiple of LW_TILE, so the 8-byte load stays inside it
    const uint64_t w = *reinterpret_cast<const uint64_t *>(code + p0);
    LwSum acc{};
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        c[j] = p0 + j < n ? (uint32_t)(w >> (8 * j)) & 15u : LW_NONE;
        acc = lw_combine(acc, lw_elem((uint32_t)(p0 + j), c[j]));
    }
    return acc;
}

// Exclusive scan of the threads' summaries over the workgroup; *total is the tile's summary
// (valid in every thread).
__device__ __forceinline__ LwSum lw_block_scan(const LwSum &mine, LwSum *wsum, LwSum *total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    LwSum inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const LwSum lo = lw_shfl_up(inc, o);
        if (lane >= (uint32_t)o) inc = lw_combine(lo, inc);
    }
    if (lane == 63) wsum[wave] = inc;
    LwSum exc = lw_shfl_up(inc, 1);
    if (lane == 0) exc = LwSum{};
    __syncthreads();
    LwSum pre{}, tot{};
#pragma unroll
    for (int w = 0; w < TB / 64; ++w) {
        if ((uint32_t)w == wave) pre = tot;
        tot = lw_combine(tot, wsum[w]);
    }
    *total = tot;
    return lw_combine(pre, exc);
}

__global__ __launch_bounds__(TB) void k_lw_summary(const uint8_t *__restrict__ code, uint64_t n,
                                                   LwSum *__restrict__ sums) {
    __shared__ LwSum wsum[TB / 64];
    uint32_t c[RPT];
    const uint64_t p0 = (uint64_t)blockIdx.x * LW_TILE + (uint64_t)threadIdx.x * RPT;
    const LwSum mine = lw_thread_sum(code, p0, n, c);
    LwSum total;
    (void)lw_block_scan(mine, wsum, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// carry[t] = the summary of tiles [0, t); one workgroup of 1024
__global__ __launch_bounds__(1024) void k_lw_carry(const LwSum *__restrict__ sums, uint64_t m,
                                                   LwSum *__restrict__ carry) {
    __shared__ LwSum part[1024];
    const uint64_t per = (m + 1023) / 1024;
    const uint64_t b = min(m, (uint64_t)threadIdx.x * per), e = min(m, b + per);
    LwSum s{};
    for (uint64_t i = b; i < e; ++i) s = lw_combine(s, sums[i]);
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        LwSum lo{};
        if (threadIdx.x >= (unsigned)d) lo = part[threadIdx.x - d];
        __syncthreads();
        if (threadIdx.x >= (unsigned)d) part[threadIdx.x] = lw_combine(lo, part[threadIdx.x]);
        __syncthreads();
    }
    LwSum run = threadIdx.x ? part[threadIdx.x - 1] : LwSum{};
    for (uint64_t i = b; i < e; ++i) {
        carry[i] = run;
        run = lw_combine(run, sums[i]);
    }
}

__global__ __launch_bounds__(TB) void k_lw_apply(const uint8_t *__restrict__ code,
                                                 const uint32_t *__restrict__ perm, uint64_t n,
                                                 const LwSum *__restrict__ carry, uint8_t *__restrict__ flags,
                                                 uint2 *__restrict__ t_pair) {
    __shared__ LwSum wsum[TB / 64];
    uint32_t c[RPT];
    const uint64_t p0 = (uint64_t)blockIdx.x * LW_TILE + (uint64_t)threadIdx.x * RPT;
    const LwSum mine = lw_thread_sum(code, p0, n, c);
    LwSum total;
    const LwSum exc = lw_block_scan(mine, wsum, &total);
    if (p0 >= n) return;
    LwSum st = lw_combine(carry[blockIdx.x], exc);
    // the code after this thread's last one says whether that one ends its run
    const uint32_t after = p0 + RPT < n ? code[p0 + RPT] : LW_HEAD;
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        const uint64_t p = p0 + j;
        if (p >= n) break;
        uint32_t ra = 0, rb = 0;
        if (lw_step(st, (uint32_t)p, c[j], &ra, &rb)) {
            const uint32_t r = perm[p];
            flags[r] = F_TAKE;
            t_pair[r] = make_uint2(perm[ra - 1], rb ? perm[rb - 1] : IGX_NO_COL);
        }
        const uint32_t next = p + 1 >= n ? LW_HEAD : (j + 1 < RPT ? c[(j + 1) % RPT] : after);
        if (next & LW_HEAD) {
            uint32_t la, lb;
            lw_live(st, &la, &lb);
            if (la) flags[perm[la - 1]] = F_LIVE;
            if (lb) flags[perm[lb - 1]] = F_LIVE;
        }
    }
}

// ---- the flagged rows in stream order ---------------------------------------------------------
__global__ __launch_bounds__(TB) void k_lw_count(const uint8_t *__restrict__ flags, uint64_t n,
                                                 uint32_t *__restrict__ cnt_t, uint32_t *__restrict__ cnt_p) {
    __shared__ uint32_t wt[TB / 64], wp[TB / 64];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t t = 0, p = 0;
#pragma unroll
    for (int j = 0; j < CRPT; ++j) {
        const uint64_t row = (uint64_t)blockIdx.x * CTILE + (uint64_t)j * TB + threadIdx.x;
        const uint32_t f = row < n ? flags[row] : 0u;
        t += __popcll(__ballot(f == F_TAKE));
        p += __popcll(__ballot(f == F_LIVE));
    }
    if (lane == 0) {
        wt[wave] = t;
        wp[wave] = p;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t st = 0, sp = 0;
        for (int w = 0; w < TB / 64; ++w) {
            st += wt[w];
            sp += wp[w];
        }
        cnt_t[blockIdx.x] = st;
        cnt_p[blockIdx.x] = sp;
    }
}

// exclusive scan of cnt[0..m) -> off[0..m), total -> *total; block 0 the TAKE counts, block 1
// the live counts (each one workgroup of 1024 on its own array)
__global__ __launch_bounds__(1024) void k_lw_scan(const uint32_t *__restrict__ cnt_t,
                                                  const uint32_t *__restrict__ cnt_p, uint64_t m,
                                                  uint64_t *__restrict__ off_t, uint64_t *__restrict__ off_p,
                                                  uint64_t *__restrict__ tot_t, uint64_t *__restrict__ tot_p) {
    __shared__ uint64_t part[1024];
    const uint32_t *cnt = blockIdx.x ? cnt_p : cnt_t;
    uint64_t *off = blockIdx.x ? off_p : off_t;
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
    if (threadIdx.x == 1023) *(blockIdx.x ? tot_p : tot_t) = part[1023];
}

__global__ __launch_bounds__(TB) void k_lw_compact(const uint8_t *__restrict__ flags, uint64_t n,
                                                   const uint64_t *__restrict__ off_t,
                                                   const uint64_t *__restrict__ off_p,
                                                   const uint2 *__restrict__ t_pair, uint32_t *__restrict__ take_row,
                                                   uint32_t *__restrict__ a_row, uint32_t *__restrict__ b_row,
                                                   uint32_t *__restrict__ pend_row, uint64_t pend_cap) {
    __shared__ uint32_t gt[CGROUPS], gp[CGROUPS];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t f[CRPT];
    uint64_t bt[CRPT], bp[CRPT];
#pragma unroll
    for (int j = 0; j < CRPT; ++j) {
        const uint64_t row = (uint64_t)blockIdx.x * CTILE + (uint64_t)j * TB + threadIdx.x;
        f[j] = row < n ? flags[row] : 0u;
        bt[j] = __ballot(f[j] == F_TAKE);
        bp[j] = __ballot(f[j] == F_LIVE);
        if (lane == 0) {   // group j * 4 + wave holds rows [64 * group, 64 * group + 64) of the tile
            gt[j * (TB / 64) + wave] = __popcll(bt[j]);
            gp[j * (TB / 64) + wave] = __popcll(bp[j]);
        }
    }
    __syncthreads();
    const uint64_t base_t = off_t[blockIdx.x], base_p = off_p[blockIdx.x];
#pragma unroll
    for (int j = 0; j < CRPT; ++j) {
        if (f[j] == 0) continue;
        const uint32_t g = j * (TB / 64) + wave;
        const uint32_t row = (uint32_t)((uint64_t)blockIdx.x * CTILE + (uint64_t)j * TB + threadIdx.x);
        uint32_t pre = 0;
        if (f[j] == F_TAKE) {
            for (uint32_t w = 0; w < g; ++w) pre += gt[w];
            const uint64_t o = base_t + pre + __popcll(bt[j] & lanemask_lt());
            const uint2 pr = t_pair[row];
            take_row[o] = row;
            a_row[o] = pr.x;
            b_row[o] = pr.y;
        } else {
            for (uint32_t w = 0; w < g; ++w) pre += gp[w];
            const uint64_t o = base_p + pre + __popcll(bp[j] & lanemask_lt());
            if (o < pend_cap) pend_row[o] = row;
        }
    }
}

}  // namespace

extern "C" int igx_lw_join_tile(void) { return LW_TILE; }

// The pipeline through the apply pass: w->flags[r] says what row r ended as (LW_F_TAKE: an emitting
// TAKE_A, with its A and B rows in w->t_pair[r]; LW_F_LIVE: still held in a register), all of it in
// the scratch arena.  perm (nrows entries) holds the order and must outlive lw_join_emit.
int lw_join_mark(igx_ctx *ctx, const uint64_t *key, const uint8_t *kind, const uint8_t *valid, uint64_t nrows,
                 uint32_t *perm, LwWork *w) {
    const uint64_t ntiles = (nrows + LW_TILE - 1) / LW_TILE, ctiles = (nrows + CTILE - 1) / CTILE;
    const size_t code_b = igx_align(ntiles * LW_TILE, 256), flag_b = igx_align(nrows, 256);
    const size_t pair_b = igx_align(nrows * 8, 256), sum_b = igx_align(ntiles * sizeof(LwSum), 256);
    const size_t cnt_b = igx_align(ctiles * 4, 256), off_b = igx_align(ctiles * 8, 256);
    const size_t need = code_b + flag_b + pair_b + 2 * sum_b + 2 * cnt_b + 2 * off_b;
    void *s;
    // ask before the sort, so that an arena that has to grow does it before the order exists
    int rc = igx_scratch(ctx, need, &s);
    if (rc) return rc;
    SortPlanKey sk{};
    sk.ptr = reinterpret_cast<const uint8_t *>(key);
    sk.width = 8;
    sk.kind = IGX_KIND_UINT;
    sk.words = 2;
    sk.stride = 8;
    rc = launch_sort_perm(ctx, &sk, 1, nrows, nullptr, false, nullptr, perm, 0, nullptr);
    if (rc) return rc;
    rc = igx_scratch(ctx, need, &s);
    if (rc) return rc;
    char *c = reinterpret_cast<char *>(s);
    uint8_t *code = reinterpret_cast<uint8_t *>(c);
    uint8_t *flags = reinterpret_cast<uint8_t *>(c + code_b);
    uint2 *t_pair = reinterpret_cast<uint2 *>(c + code_b + flag_b);
    LwSum *sums = reinterpret_cast<LwSum *>(c + code_b + flag_b + pair_b);
    LwSum *carry = reinterpret_cast<LwSum *>(c + code_b + flag_b + pair_b + sum_b);
    char *q = c + code_b + flag_b + pair_b + 2 * sum_b;
    w->flags = flags;
    w->t_pair = t_pair;
    w->perm = perm;
    w->cnt_t = reinterpret_cast<uint32_t *>(q);
    w->cnt_p = reinterpret_cast<uint32_t *>(q + cnt_b);
    w->off_t = reinterpret_cast<uint64_t *>(q + 2 * cnt_b);
    w->off_p = reinterpret_cast<uint64_t *>(q + 2 * cnt_b + off_b);

    IGX_HIP(ctx, hipMemsetAsync(flags, 0, flag_b, ctx->stream));
    hipLaunchKernelGGL(k_lw_code, dim3((unsigned)((nrows + TB - 1) / TB)), dim3(TB), 0, ctx->stream, key, kind, valid,
                       perm, nrows, code);
    hipLaunchKernelGGL(k_lw_summary, dim3((unsigned)ntiles), dim3(TB), 0, ctx->stream, code, nrows, sums);
    hipLaunchKernelGGL(k_lw_carry, dim3(1), dim3(1024), 0, ctx->stream, sums, ntiles, carry);
    hipLaunchKernelGGL(k_lw_apply, dim3((unsigned)ntiles), dim3(TB), 0, ctx->stream, code, perm, nrows, carry, flags,
                       t_pair);
    return IGX_OK;
}

// The flagged rows of w written out in stream order; b_row may be the perm that lw_join_mark used.
int lw_join_emit(igx_ctx *ctx, const LwWork *w, uint64_t nrows, uint32_t *take_row, uint32_t *a_row,
                 uint32_t *b_row, uint64_t *d_ntake, uint32_t *pend_row, uint64_t pend_cap, uint64_t *d_npend) {
    const uint64_t ctiles = (nrows + CTILE - 1) / CTILE;
    hipLaunchKernelGGL(k_lw_count, dim3((unsigned)ctiles), dim3(TB), 0, ctx->stream, w->flags, nrows, w->cnt_t,
                       w->cnt_p);
    hipLaunchKernelGGL(k_lw_scan, dim3(2), dim3(1024), 0, ctx->stream, w->cnt_t, w->cnt_p, ctiles, w->off_t, w->off_p,
                       d_ntake, d_npend);
    hipLaunchKernelGGL(k_lw_compact, dim3((unsigned)ctiles), dim3(TB), 0, ctx->stream, w->flags, nrows, w->off_t,
                       w->off_p, w->t_pair, take_row, a_row, b_row, pend_row, pend_cap);
    IGX_HIP(ctx, hipGetLastError());
    return IGX_OK;
}

extern "C" int igx_lw_join(igx_ctx *ctx, const uint64_t *key, const uint8_t *kind, const uint8_t *valid,
                           uint64_t nrows, uint32_t *take_row, uint32_t *a_row, uint32_t *b_row, uint64_t *d_ntake,
                           uint32_t *pend_row, uint64_t pend_cap, uint64_t *d_npend) {
    if (!ctx) return IGX_EINVAL;
    if (nrows > 0xFFFFFFFEull) return igx_fail(ctx, IGX_EINVAL, "lw_join: more than 2^32 - 2 rows");
    if (!d_ntake || !d_npend) return igx_fail(ctx, IGX_EINVAL, "lw_join: null count");
    if (((uintptr_t)d_ntake | (uintptr_t)d_npend) & 7)
        return igx_fail(ctx, IGX_EINVAL, "lw_join: counts not 8-byte aligned");
    if (nrows == 0) {
        IGX_HIP(ctx, hipMemsetAsync(d_ntake, 0, 8, ctx->stream));
        IGX_HIP(ctx, hipMemsetAsync(d_npend, 0, 8, ctx->stream));
        return IGX_OK;
    }
    if (!key || !kind || !take_row || !a_row || !b_row || (pend_cap && !pend_row))
        return igx_fail(ctx, IGX_EINVAL, "lw_join: null argument");
    if ((uintptr_t)key & 7) return igx_fail(ctx, IGX_EINVAL, "lw_join: key must be 8-byte aligned");
    if (((uintptr_t)take_row | (uintptr_t)a_row | (uintptr_t)b_row | (uintptr_t)pend_row) & 3)
        return igx_fail(ctx, IGX_EINVAL, "lw_join: row outputs must be 4-byte aligned");
    // The order lives in b_row (read by the code and apply passes, written by the compaction,
    // which no longer needs it) while the scratch arena, which the sort uses too, is handed from
    // the sort to the passes.
    LwWork w;
    const int rc = lw_join_mark(ctx, key, kind, valid, nrows, b_row, &w);
    if (rc) return rc;
    return lw_join_emit(ctx, &w, nrows, take_row, a_row, b_row, d_ntake, pend_row, pend_cap, d_npend);
}
