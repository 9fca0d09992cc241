// k_gb_part_c.hip -- pass C of the group-by's partitioned form: this unit instantiates k_gbp_c
// (k_groupby_part.h: AggTab, hbm_merge, flush_owned, wave_combine) behind one launch function.
// The pass is more than a third of the group-by's kernel instances, hence a unit of its own.
#include "k_gb_part.h"

namespace {

#include "k_groupby_part.h"

// pass C over layout L for records of NV loaded columns: with aggregates, distinct-only (no
// aggregate decode or accumulate in the per-record path), or distinct-only with packed entries
// (C4).  The dynamic LDS granted so far is kept per instance.
template <class L, int NV, bool WIDE>
int launch_c_as(igx_table *t, const GbArgs &a, const PartArgs &p, size_t lds_c) {
    igx_ctx *ctx = t->ctx;
    constexpr bool PEK = pack_words<L>() <= 3;   // a packed-entry pass C exists for this layout
    using Kern = void (*)(GbArgs, PartArgs);
    const Kern kern[3] = {k_gbp_c<L, NV, AMAX, false, WIDE>, k_gbp_c<L, NV, 0, false, WIDE>,
                          k_gbp_c<L, NV, 0, PEK, WIDE>};
    static size_t lds_set[3] = {0, 0, 0};
    const int i = t->naggs ? 0 : (PEK && p.pe ? 2 : 1);
    if (lds_c > lds_set[i]) {
        IGX_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kern[i]),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_c));
        lds_set[i] = lds_c;
    }
    hipLaunchKernelGGL(kern[i], dim3(2 * (uint32_t)ctx->num_cus), dim3(PTC), lds_c, ctx->stream, a, p);
    return IGX_OK;
}

}  // namespace

void gbp_c_load() {
    hipFuncAttributes fa;
    (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_gbp_c<TcpKey, 0, 0, false, false>));
}

int gbp_launch_c(igx_table *t, const GbArgs &a, const PartArgs &p, size_t lds_c) {
    return gb_with_layout(t, [&](auto tag) {
        using L = typename decltype(tag)::type;
        return part_with_shape(p.nv, t->wide, [&](auto nvc, auto wide) {
            return launch_c_as<L, decltype(nvc)::value, decltype(wide)::value>(t, a, p, lds_c);
        });
    });
}
