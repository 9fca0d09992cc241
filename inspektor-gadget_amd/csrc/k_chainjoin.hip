// k_chainjoin.hip -- the chained join through two maps: what trace tcp does with its connect probes
// (tcptracer.bpf.c: `sockets` keyed by the thread, then `tuplepid` keyed by the tuple).
// include/igx.h has the contract.
//
// No new scan: both stages are the last-writer join of k_lwjoin.hip (lw_join_mark), over the same
// row index space.
//
//   stage 1  on key1: ENTER = SET_A, PASS / ABORT = TAKE_A.  A PASS that emits found its ENTER;
//            an ENTER still live is pending.
//   hand-over (k_cj_handover) writes stage 2's kind column from stage 1's flags:
//            an emitting PASS or a HELD row = SET_A, TAKE / DROP = TAKE_A, everything else does
//            not exist; a pending ENTER is remembered in the same byte (CJ_PEND1).
//   stage 2  on key2.  A DROP is a TAKE_A whose emission nobody wants: the register is empty
//            afterwards either way, which is all a delete has to do.
//   merge    (k_cj_merge) in place on stage 2's flags: an emitting DROP loses its flag, a pending
//            ENTER gets the live flag, and the joins' compaction (join_emit, k_join.hip) writes
//            emissions and both maps' pending rows out in stream order.
//
// The kind column and the order live in the side arena (a sort owns the scratch arena while it
// runs); stage 1's flags are consumed before stage 2's sort starts.  Every launch is a plain grid
// and the counts stay on the device.
#include "k_common.h"
#include "k_lwjoin.h"

namespace {

constexpr int TB = 256;
constexpr uint8_t CJ_NONE = 255;      // not a kind of igx_lw_join: the row does not exist for it
constexpr uint8_t CJ_PEND1 = 0x80;    // likewise, and: an ENTER that stage 1 left in map 1

__global__ __launch_bounds__(TB) void k_cj_stage1(const uint8_t *__restrict__ kind, const uint8_t *__restrict__ valid,
                                                  uint64_t n, uint8_t *__restrict__ k1) {
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = kind[i];
    uint8_t o = CJ_NONE;
    if (!valid || valid[i] != 0) {
        if (k == IGX_CJ_ENTER) o = IGX_LW_SET_A;
        if (k == IGX_CJ_PASS || k == IGX_CJ_ABORT) o = IGX_LW_TAKE_A;
    }
    k1[i] = o;
}

// k12 holds stage 1's kinds on entry and stage 2's on return (each lane rewrites its own byte)
__global__ __launch_bounds__(TB) void k_cj_handover(const uint8_t *__restrict__ kind,
                                                    const uint8_t *__restrict__ valid,
                                                    const uint8_t *__restrict__ flags1, uint64_t n,
                                                    uint8_t *__restrict__ k12) {
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = kind[i], f = flags1[i];
    uint8_t o = CJ_NONE;
    if (!valid || valid[i] != 0) {
        if ((k == IGX_CJ_PASS && f == LW_F_TAKE) || k == IGX_CJ_HELD) o = IGX_LW_SET_A;
        if (k == IGX_CJ_TAKE || k == IGX_CJ_DROP) o = IGX_LW_TAKE_A;
        if (k == IGX_CJ_ENTER && f == LW_F_LIVE) o = CJ_PEND1;
    }
    k12[i] = o;
}

__global__ __launch_bounds__(TB) void k_cj_merge(const uint8_t *__restrict__ kind, const uint8_t *__restrict__ k2,
                                                 uint64_t n, uint8_t *__restrict__ flags2) {
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = flags2[i];
    uint8_t o = 0;
    if (f == LW_F_TAKE && kind[i] == IGX_CJ_TAKE) o = LW_F_TAKE;
    if (f == LW_F_LIVE || k2[i] == CJ_PEND1) o = LW_F_LIVE;
    flags2[i] = o;
}

}  // namespace

extern "C" int igx_chain_join_tile(void) { return igx_lw_join_tile(); }

extern "C" int igx_chain_join(igx_ctx *ctx, const uint64_t *key1, const uint64_t *key2, const uint8_t *kind,
                              const uint8_t *valid, uint64_t nrows, uint32_t *take_row, uint32_t *pass_row,
                              uint64_t *d_ntake, uint32_t *pend_row, uint64_t pend_cap, uint64_t *d_npend) {
    if (!ctx) return IGX_EINVAL;
    int rc = igx_join_begin(ctx, "chain_join", nrows, d_ntake, d_npend);
    if (rc || nrows == 0) return rc;
    if (!key1 || !key2 || !kind || !take_row || !pass_row || (pend_cap && !pend_row))
        return igx_fail(ctx, IGX_EINVAL, "chain_join: null argument");
    if (((uintptr_t)key1 | (uintptr_t)key2) & 7)
        return igx_fail(ctx, IGX_EINVAL, "chain_join: keys must be 8-byte aligned");
    if (((uintptr_t)take_row | (uintptr_t)pass_row | (uintptr_t)pend_row) & 3)
        return igx_fail(ctx, IGX_EINVAL, "chain_join: row outputs must be 4-byte aligned");

    const size_t kind_b = igx_align(nrows, 256);
    void *sd;
    rc = igx_side(ctx, kind_b + igx_align(nrows * 4, 256), &sd);
    if (rc) return rc;
    uint8_t *k12 = reinterpret_cast<uint8_t *>(sd);
    // the order of each stage, and where the compaction puts the B rows nobody reads
    uint32_t *perm = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(sd) + kind_b);
    const dim3 grid((unsigned)((nrows + TB - 1) / TB));

    JoinWork w;
    hipLaunchKernelGGL(k_cj_stage1, grid, dim3(TB), 0, ctx->stream, kind, valid, nrows, k12);
    rc = lw_join_mark(ctx, key1, k12, nullptr, nrows, perm, &w);
    if (rc) return igx_side_drop(ctx, rc);
    hipLaunchKernelGGL(k_cj_handover, grid, dim3(TB), 0, ctx->stream, kind, valid, w.flags, nrows, k12);
    rc = lw_join_mark(ctx, key2, k12, nullptr, nrows, perm, &w);
    if (rc) return igx_side_drop(ctx, rc);
    hipLaunchKernelGGL(k_cj_merge, grid, dim3(TB), 0, ctx->stream, kind, k12, nrows, w.flags);
    return join_emit(ctx, &w, nrows, take_row, pass_row, perm, d_ntake, pend_row, pend_cap, d_npend);
}
