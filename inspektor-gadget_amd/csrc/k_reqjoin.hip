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
//   count / scan / compact   the flagged rows written out in stream order (k_join.hip)
//
// Every launch is a plain grid; no workgroup waits on another.  Algorithmic bytes per row:
// DESIGN.md §4.  Everything around the four passes in the middle is join_mark / join_emit.
#include "k_scan.h"
#include "k_reqjoin.h"

namespace {

constexpr int TB = SCAN_TB, RPT = SCAN_RPT, RJ_TILE = SCAN_TILE;
constexpr uint8_t F_DONE = JOIN_F_EMIT, F_LIVE = JOIN_F_LIVE;

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

struct RjOp {
    using T = RjSum;
    static __device__ __forceinline__ T identity() { return T{}; }
    static __device__ __forceinline__ T combine(const T &x, const T &y) { return rj_combine(x, y); }
    static __device__ __forceinline__ T shfl_up(const T &v, int o) { return rj_shfl_up(v, o); }
};

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

__global__ __launch_bounds__(TB) void k_rj_summary(const uint8_t *__restrict__ code, uint64_t n,
                                                   RjSum *__restrict__ sums) {
    __shared__ RjSum wsum[TB / 64];
    uint32_t c[RPT];
    const uint64_t p0 = (uint64_t)blockIdx.x * RJ_TILE + (uint64_t)threadIdx.x * RPT;
    const RjSum mine = rj_thread_sum(code, p0, n, c);
    RjSum total;
    (void)block_scan<RjOp>(mine, wsum, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// carry[t] = the summary of tiles [0, t); one workgroup of 1024
__global__ __launch_bounds__(1024) void k_rj_carry(const RjSum *__restrict__ sums, uint64_t m,
                                                   RjSum *__restrict__ carry) {
    tile_carry<RjOp, 1024>(sums, m, carry);
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
    const RjSum exc = block_scan<RjOp>(mine, wsum, &total);
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

// the four passes of join_mark
void rj_passes(hipStream_t st, const uint64_t *req, const uint8_t *kind, const uint8_t *valid, const uint32_t *perm,
               uint64_t nrows, const JoinWork &w) {
    const dim3 tiles((unsigned)((nrows + RJ_TILE - 1) / RJ_TILE));
    RjSum *sums = static_cast<RjSum *>(w.sums), *carry = static_cast<RjSum *>(w.carry);
    hipLaunchKernelGGL(k_rj_code, dim3((unsigned)((nrows + TB - 1) / TB)), dim3(TB), 0, st, req, kind, valid, perm,
                       nrows, w.code);
    hipLaunchKernelGGL(k_rj_summary, tiles, dim3(TB), 0, st, w.code, nrows, sums);
    hipLaunchKernelGGL(k_rj_carry, dim3(1), dim3(1024), 0, st, sums, (uint64_t)tiles.x, carry);
    hipLaunchKernelGGL(k_rj_apply, tiles, dim3(TB), 0, st, w.code, perm, nrows, carry, w.flags, w.pair);
}

}  // namespace

extern "C" int igx_req_join_tile(void) { return RJ_TILE; }

extern "C" int igx_req_join(igx_ctx *ctx, const uint64_t *req, const uint8_t *kind, const uint64_t *ts,
                            const uint8_t *valid, uint64_t nrows, uint32_t *done_row, uint32_t *issue_row,
                            uint32_t *who_row, uint64_t *delta, uint64_t *d_ndone, uint32_t *pend_row,
                            uint64_t pend_cap, uint64_t *d_npend) {
    if (!ctx) return IGX_EINVAL;
    int rc = igx_join_begin(ctx, "req_join", nrows, d_ndone, d_npend);
    if (rc || nrows == 0) return rc;
    if (!req || !kind || !ts || !done_row || !issue_row || !who_row || !delta || (pend_cap && !pend_row))
        return igx_fail(ctx, IGX_EINVAL, "req_join: null argument");
    if (((uintptr_t)req | (uintptr_t)ts | (uintptr_t)delta) & 7)
        return igx_fail(ctx, IGX_EINVAL, "req_join: req, ts and delta must be 8-byte aligned");
    if (((uintptr_t)done_row | (uintptr_t)issue_row | (uintptr_t)who_row | (uintptr_t)pend_row) & 3)
        return igx_fail(ctx, IGX_EINVAL, "req_join: row outputs must be 4-byte aligned");
    // The order lives in delta (8 bytes per row, written last) while the scratch arena, which
    // the sort uses too, is handed from the sort to the passes.
    JoinWork w;
    rc = join_mark(ctx, sizeof(RjSum), rj_passes, req, kind, valid, nrows, reinterpret_cast<uint32_t *>(delta), &w);
    if (rc) return rc;
    return join_emit(ctx, &w, nrows, done_row, issue_row, who_row, d_ndone, pend_row, pend_cap, d_npend, ts, delta);
}
