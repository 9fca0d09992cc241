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
//   count / scan / compact   the flagged rows written out in stream order (k_join.hip)
//
// Every launch is a plain grid; no workgroup waits on another.  Algorithmic bytes per row:
// DESIGN.md §4.  The pipeline is callable in two halves (igx_internal.h: lw_join_mark through
// apply, join_emit from count on) for the joins composed of it (k_chainjoin.hip); igx_lw_join
// is the two back to back.
#include "k_scan.h"
#include "k_lwjoin.h"

static_assert(IGX_LW_SET_A == LW_SET_A && IGX_LW_SET_B == LW_SET_B && IGX_LW_CLEAR_B == LW_CLEAR_B &&
                  IGX_LW_TAKE_A == LW_TAKE_A,
              "enum igx_lw_kind and the codes of k_lwjoin.h");

namespace {

constexpr int TB = SCAN_TB, RPT = SCAN_RPT, LW_TILE = SCAN_TILE;
constexpr uint8_t F_TAKE = LW_F_TAKE, F_LIVE = LW_F_LIVE;

__device__ __forceinline__ LwSum lw_shfl_up(const LwSum &v, int o) {
    LwSum r;
    r.a = __shfl_up((unsigned long long)v.a, o);
    r.b = __shfl_up((unsigned long long)v.b, o);
    r.h = __shfl_up(v.h, o);
    r.pad = 0;
    return r;
}

struct LwOp {
    using T = LwSum;
    static __device__ __forceinline__ T identity() { return T{}; }
    static __device__ __forceinline__ T combine(const T &x, const T &y) { return lw_combine(x, y); }
    static __device__ __forceinline__ T shfl_up(const T &v, int o) { return lw_shfl_up(v, o); }
};

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

__global__ __launch_bounds__(TB) void k_lw_summary(const uint8_t *__restrict__ code, uint64_t n,
                                                   LwSum *__restrict__ sums) {
    __shared__ LwSum wsum[TB / 64];
    uint32_t c[RPT];
    const uint64_t p0 = (uint64_t)blockIdx.x * LW_TILE + (uint64_t)threadIdx.x * RPT;
    const LwSum mine = lw_thread_sum(code, p0, n, c);
    LwSum total;
    (void)block_scan<LwOp>(mine, wsum, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// carry[t] = the summary of tiles [0, t); one workgroup of 1024
__global__ __launch_bounds__(1024) void k_lw_carry(const LwSum *__restrict__ sums, uint64_t m,
                                                   LwSum *__restrict__ carry) {
    tile_carry<LwOp, 1024>(sums, m, carry);
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
    const LwSum exc = block_scan<LwOp>(mine, wsum, &total);
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

// the four passes of join_mark
void lw_passes(hipStream_t st, const uint64_t *key, const uint8_t *kind, const uint8_t *valid, const uint32_t *perm,
               uint64_t nrows, const JoinWork &w) {
    const dim3 tiles((unsigned)((nrows + LW_TILE - 1) / LW_TILE));
    LwSum *sums = static_cast<LwSum *>(w.sums), *carry = static_cast<LwSum *>(w.carry);
    hipLaunchKernelGGL(k_lw_code, dim3((unsigned)((nrows + TB - 1) / TB)), dim3(TB), 0, st, key, kind, valid, perm,
                       nrows, w.code);
    hipLaunchKernelGGL(k_lw_summary, tiles, dim3(TB), 0, st, w.code, nrows, sums);
    hipLaunchKernelGGL(k_lw_carry, dim3(1), dim3(1024), 0, st, sums, (uint64_t)tiles.x, carry);
    hipLaunchKernelGGL(k_lw_apply, tiles, dim3(TB), 0, st, w.code, perm, nrows, carry, w.flags, w.pair);
}

}  // namespace

extern "C" int igx_lw_join_tile(void) { return LW_TILE; }

// The pipeline through the apply pass: w->flags[r] says what row r ended as (LW_F_TAKE: an emitting
// TAKE_A, with its A and B rows in w->pair[r]; LW_F_LIVE: still held in a register).
int lw_join_mark(igx_ctx *ctx, const uint64_t *key, const uint8_t *kind, const uint8_t *valid, uint64_t nrows,
                 uint32_t *perm, JoinWork *w) {
    return join_mark(ctx, sizeof(LwSum), lw_passes, key, kind, valid, nrows, perm, w);
}

extern "C" int igx_lw_join(igx_ctx *ctx, const uint64_t *key, const uint8_t *kind, const uint8_t *valid,
                           uint64_t nrows, uint32_t *take_row, uint32_t *a_row, uint32_t *b_row, uint64_t *d_ntake,
                           uint32_t *pend_row, uint64_t pend_cap, uint64_t *d_npend) {
    if (!ctx) return IGX_EINVAL;
    int rc = igx_join_begin(ctx, "lw_join", nrows, d_ntake, d_npend);
    if (rc || nrows == 0) return rc;
    if (!key || !kind || !take_row || !a_row || !b_row || (pend_cap && !pend_row))
        return igx_fail(ctx, IGX_EINVAL, "lw_join: null argument");
    if ((uintptr_t)key & 7) return igx_fail(ctx, IGX_EINVAL, "lw_join: key must be 8-byte aligned");
    if (((uintptr_t)take_row | (uintptr_t)a_row | (uintptr_t)b_row | (uintptr_t)pend_row) & 3)
        return igx_fail(ctx, IGX_EINVAL, "lw_join: row outputs must be 4-byte aligned");
    // The order lives in b_row (read by the code and apply passes, written by the compaction,
    // which no longer needs it) while the scratch arena, which the sort uses too, is handed from
    // the sort to the passes.
    JoinWork w;
    rc = lw_join_mark(ctx, key, kind, valid, nrows, b_row, &w);
    if (rc) return rc;
    return join_emit(ctx, &w, nrows, take_row, a_row, b_row, d_ntake, pend_row, pend_cap, d_npend);
}
