// k_gb_direct.hip -- the group-by's direct form: every row probes the HBM table (k_gb_table.h)
// itself, no LDS cache.  k_groupby_direct, its launchers and gb_launch_direct.
#include "k_gb_table.h"

namespace {

#ifndef IGX_GB_DIRECT_U
#define IGX_GB_DIRECT_U 2
#endif

// ---- direct form: no LDS cache ---------------------------------------------------------
// For near-uniform, high-cardinality streams (C4's distinct tuples: nearly every row misses
// any per-CU cache) the LDS cache, its rings and its roles only add work: every row goes
// to HBM anyway.  Here each lane takes rows of a grid-stride sweep (so the whole grid
// advances through the stream in index order and first indices arrive nearly in order --
// the atomicMin on `first` is then rare) and resolves each one itself: probe, compare,
// claim, atomics.  The throughput is the chip's random-access rate (~45-50 G probes/s over
// a 1 GiB table, tools/micro/randacc.hip); occupancy, not a pipeline, hides the latency.
// WIDE: the table's record addressing (probe_issue); the wide instance keeps the shape -- its
// probes' loads are in flight together and probe_wait retires them before the first resolve.
template <class L, int NA, bool WIDE = false>
__global__ __launch_bounds__(256) void k_groupby_direct(GbArgs a) {
    constexpr int KW = L::KW;
    constexpr int U = IGX_GB_DIRECT_U;   // rows in flight per lane: all rows' loads, then all probes
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t row0 = (uint64_t)blockIdx.x * 256 + threadIdx.x; row0 < a.n; row0 += U * stride) {
        RowRaw<L, NA> R[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t row = row0 + u * stride;
            issue_row<L, NA>(a, row < a.n ? row : row0, R[u]);
        }
        uint32_t k[U][KW];
        uint64_t v[U][NA], h[U];
        bool ok[U];
        probe_regs<KW, WIDE> d[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t row = row0 + u * stride;
            ok[u] = row < a.n && decode_row<L, NA>(a, row, R[u], k[u], v[u]);
            h[u] = hash_key<KW>(k[u]);
            if constexpr (WIDE) {   // every lane loads (a dropped row: slot 0), so every d is defined
                probe_issue<KW, true>(a, ok[u] ? h[u] : 0ull, d[u]);
            } else {
                if (ok[u]) probe_issue<KW>(a, h[u], d[u]);
            }
        }
        if constexpr (WIDE) {
#pragma unroll
            for (int u = 0; u < U; ++u) probe_wait<KW, true>(d[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!ok[u]) continue;
            const uint64_t gidx = row_gidx(a, row0 + u * stride);
            uint64_t first_ins = 0;
            bool claimed = false;
            // no occupancy bit: finalize rebuilds the bitmap from the tags (k_occ_from_tags),
            // one streaming pass instead of a memory-side atomic per claim
            const uint32_t gs = find_or_insert<KW, false, NA, WIDE>(a, k[u], h[u], gidx, first_ins, d[u], v[u], claimed);
            if (gs == SLOT_OVF || claimed) continue;
#pragma unroll
            for (int x = 0; x < NA; ++x)
                if (x < (int)a.naggs && v[u][x]) gadd(rec_agg(a, gs, x), (unsigned long long)v[u][x]);
            if (gidx < first_ins) gmin(rec_first(a, gs), (unsigned long long)gidx);
        }
    }
}

// The grid is exactly the blocks that are resident at once (the occupancy the kernel's
// registers allow): every block sweeps a fixed share of the rows, so a block that had to wait
// for a free slot would run its whole share after the others -- a tail of up to 1/8 of the time.
template <class L, int NA, bool WIDE = false>
void launch_direct_as(igx_ctx *ctx, GbArgs &a) {
    static int per_cu = 0;
    if (!per_cu) {
        int b = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, reinterpret_cast<const void *>(k_groupby_direct<L, NA, WIDE>),
                                                         256, 0) != hipSuccess || b < 1)
            b = 4;
        per_cu = std::min(b, 8);
    }
    const uint64_t want = (a.n + 255) / 256;
    const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)ctx->num_cus * per_cu));
    hipLaunchKernelGGL((k_groupby_direct<L, NA, WIDE>), dim3(blocks), dim3(256), 0, ctx->stream, a);
}

template <class L, bool WIDE = false>
void launch_direct(igx_ctx *ctx, GbArgs &a) {
    if (a.naggs <= 2) launch_direct_as<L, 2, WIDE>(ctx, a);
    else launch_direct_as<L, AMAX, WIDE>(ctx, a);
}

}  // namespace

void gb_direct_load() {
    hipFuncAttributes fa;
    (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_groupby_direct<TcpKey, 2, false>));
}

int gb_launch_direct(igx_table *t, GbArgs &a) {
    return gb_with_layout(t, [&](auto tag) {
        using L = typename decltype(tag)::type;
        if (t->wide) launch_direct<L, true>(t->ctx, a);
        else launch_direct<L>(t->ctx, a);
        return (int)IGX_OK;
    });
}
