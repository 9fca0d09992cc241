// k_gb_part.hip -- the group-by's partitioned form, passes K, O, S, A and B: this unit instantiates
// k_gbp_count / k_gbp_a / k_gbp_b (k_groupby_part.h), holds the form's plain kernels and the plan
// of an update -- the record layout, the bucket counts, the scratch and every pass's launch
// (gb_launch_part).  Pass C is k_gb_part_c.hip.
#include "k_gb_part.h"

namespace {

#include "k_groupby_part.h"

// Fused predicates of an update in the partitioned form: evaluated once into a row mask
// (AND-ed with the nil mask), which the passes then read like `valid`.
__global__ __launch_bounds__(256) void k_gbp_mask(GbArgs a, uint8_t *out) {
    for (uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x; row < a.n; row += (uint64_t)gridDim.x * 256) {
        bool ok = !a.valid || a.valid[row] != 0;
        for (uint32_t q = 0; q < a.npred && q < PMAX; ++q)
            ok = ok && ((a.gwidth[q] && ld_val(a.gptr[q], row, a.gwidth[q]) != a.gref[q]) ||
                        pred_scalar(ld_val(a.pptr[q], row, a.pwidth[q]), a.pref[q], a.pwidth[q], a.pkind[q],
                                    a.pcmp[q], a.pneg[q], a.pcnt[q]));
        out[row] = ok ? 1 : 0;
    }
}

// O1: per chunk of CHT A tiles, rows per first-level bucket
__global__ __launch_bounds__(PTA) void k_gbp_csum(PartArgs p) {
    const uint32_t F1 = 1u << p.f1, c = blockIdx.x;
    if (threadIdx.x >= F1) return;
    const uint32_t t0 = c * CHT, t1 = min(p.tiles_a, t0 + CHT);
    uint32_t s = 0;
    for (uint32_t t = t0; t < t1; ++t) s += p.cnt1[(uint64_t)t * F1 + threadIdx.x];
    p.csum[(uint64_t)c * F1 + threadIdx.x] = s;
}

// ---- S: bucket starts, cursors, chunk offsets, B tiles, C work items (one block) -----------
__global__ __launch_bounds__(1024) void k_gbp_scan(PartArgs p) {
    __shared__ uint32_t wsum[17];
    __shared__ uint32_t ts[PART_F_MAX + 1];
    const uint32_t NB = 1u << p.lb, F1 = 1u << p.f1, F2 = 1u << p.f2;
    const uint32_t per = (NB + 1023) / 1024, b0 = threadIdx.x * per;
    uint32_t s = 0, si = 0;
    for (uint32_t i = 0; i < per; ++i) {
        const uint32_t b = b0 + i;
        const uint32_t c = b < NB ? p.hist[b] : 0u;
        s += c;
        si += (c + p.ch - 1) / p.ch;
    }
    uint32_t tot, toti;
    uint32_t run = block_excl_scan(s, wsum, tot);
    uint32_t runi = block_excl_scan(si, wsum, toti);
    for (uint32_t i = 0; i < per; ++i) {
        const uint32_t b = b0 + i;
        if (b >= NB) break;
        const uint32_t c = p.hist[b], ni = (c + p.ch - 1) / p.ch;
        p.start2[b] = run;
        p.cur2[b] = run;
        p.istart[b] = runi;
        for (uint32_t k = 0; k < ni; ++k) p.itfb[runi + k] = b;
        run += c;
        runi += ni;
    }
    // first-level buckets: record counts, starts (= start2 of their first final bucket),
    // chunk offsets and B tiles
    uint32_t c1 = 0;
    if (threadIdx.x < F1)
        for (uint32_t b2 = 0; b2 < F2; ++b2) c1 += p.hist[threadIdx.x * F2 + b2];
    uint32_t tot1, tott;
    const uint32_t st1 = block_excl_scan(c1, wsum, tot1);
    const uint32_t nt = (c1 + p.trb - 1) / p.trb;
    const uint32_t tst = block_excl_scan(nt, wsum, tott);
    if (threadIdx.x < F1) {
        scan_column(p.csum + threadIdx.x, F1, p.nchunk, st1);
        p.tstart[threadIdx.x] = tst;
        ts[threadIdx.x] = tst;
    }
    if (threadIdx.x == 0) {
        p.start2[NB] = tot;
        p.istart[NB] = toti;
        p.tstart[F1] = tott;
        ts[F1] = tott;
        p.ctl[0] = 0;
        p.ctl[1] = tott;
        p.ctl[2] = toti;
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < tott; t += 1024) p.bt[t] = upper_bound_u32(ts, 0, F1 + 1, t) - 1;
}

// O2: each A tile's exact output position per first-level bucket (cnt1 in place)
__global__ __launch_bounds__(PTA) void k_gbp_offs(PartArgs p) {
    const uint32_t F1 = 1u << p.f1, c = blockIdx.x;
    if (threadIdx.x >= F1) return;
    const uint32_t t0 = c * CHT, t1 = min(p.tiles_a, t0 + CHT);
    scan_column(p.cnt1 + (uint64_t)t0 * F1 + threadIdx.x, F1, t1 - t0, p.csum[(uint64_t)c * F1 + threadIdx.x]);
}

// region variant, between A and B: B tiles of each first-level slice (tstart, bt, ctl[1])
__global__ __launch_bounds__(1024) void k_gbr_tiles(PartArgs p) {
    __shared__ uint32_t wsum[17];
    __shared__ uint32_t ts[PART_U1_MAX + 1];
    const uint32_t U1 = 1u << (p.f1 + p.s1log);
    const uint32_t per = (U1 + 1023) / 1024, u0 = threadIdx.x * per;
    uint32_t nt = 0;
    for (uint32_t i = 0; i < per; ++i)
        if (u0 + i < U1) nt += (min(p.rc1[(u0 + i) * RC1_PAD], p.reg1) + p.trb - 1) / p.trb;
    uint32_t tot;
    uint32_t st = block_excl_scan(nt, wsum, tot);
    for (uint32_t i = 0; i < per && u0 + i < U1; ++i) {
        p.tstart[u0 + i] = st;
        ts[u0 + i] = st;
        st += (min(p.rc1[(u0 + i) * RC1_PAD], p.reg1) + p.trb - 1) / p.trb;
    }
    if (threadIdx.x == 0) {
        p.tstart[U1] = tot;
        ts[U1] = tot;
        p.ctl[1] = tot;
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < tot; t += 1024) p.bt[t] = upper_bound_u32(ts, 0, U1 + 1, t) - 1;
}

// region variant, after B: C work items from the final regions' fills (a final bucket larger
// than ch is split)
__global__ __launch_bounds__(1024) void k_gbr_items(PartArgs p) {
    __shared__ uint32_t wsum[17];
    const uint32_t NB = 1u << p.lb;
    const uint32_t per = (NB + 1023) / 1024, b0 = threadIdx.x * per;
    uint32_t si = 0;
    for (uint32_t i = 0; i < per; ++i) {
        const uint32_t b = b0 + i;
        const uint32_t c = b < NB ? min(p.rc2[b * p.c2pad], p.reg2) : 0u;
        si += (c + p.ch - 1) / p.ch;
    }
    uint32_t toti;
    uint32_t runi = block_excl_scan(si, wsum, toti);
    for (uint32_t i = 0; i < per; ++i) {
        const uint32_t b = b0 + i;
        if (b >= NB) break;
        const uint32_t c = min(p.rc2[b * p.c2pad], p.reg2), ni = (c + p.ch - 1) / p.ch;
        p.istart[b] = runi;
        for (uint32_t k = 0; k < ni; ++k) p.itfb[runi + k] = b;
        runi += ni;
    }
    if (threadIdx.x == 0) {
        p.istart[NB] = toti;
        p.ctl[0] = 0;
        p.ctl[2] = toti;
    }
}

// The partitioned form (k_groupby_part.h): passes K, O, S, A, B, C -- or, in the region
// variant (AUTO's miss-heavy intervals), A, T, B, I, C: no count pass, buckets filled through
// cursors into regions of 1.25x their share of the rows.
template <class L, int NV, bool WIDE = false>
int launch_part_as(igx_table *t, igx_ctx *ctx, GbArgs &a, PartArgs &p, bool region) {
    constexpr int KW = L::KW;
    constexpr uint32_t TRA = PTA * part_rows<KW, NV>();
    if (4 * p.rq > (uint32_t)part_w<KW, NV>()) return igx_fail(ctx, IGX_EINVAL, "groupby_update: record layout");
    // final buckets: enough that a bucket's share of the capacity fills at most ~60% of the
    // C block's LDS table; each bucket owns whole probe regions of the table
    // pass C's packed entries (c_row_pe): distinct-only, a static key of <= 3 packed words,
    // row-offset indices; IGX_GBP_NOPE=1 keeps the general table (A/B)
    p.pe = pack_words<L>() <= 3 && t->naggs == 0 && p.iw == 1 &&
           !std::getenv("IGX_GBP_COMBINE") && !std::getenv("IGX_GBP_NOPE");
    const size_t entry = p.pe ? 17 : agg_entry_bytes(KW, t->naggs);
    p.uc = p.rq <= 1 ? 2 : 1;
    if (const char *d = std::getenv("IGX_GBP_UC"))   // tuning knob: records per thread and round of pass C
        p.uc = std::max<uint32_t>(1, std::min<uint32_t>(UCMAX, (uint32_t)std::strtoul(d, nullptr, 0)));
    const size_t stage_c = (size_t)p.uc * PTC * p.rq * 16;
    const uint32_t lb_max = std::min<uint32_t>(PART_LB_MAX, t->sbits - t->rbits);
    auto entries = [&](uint32_t lb, size_t esz) {
        const int64_t occw = (int64_t)1 << (t->sbits - lb - 5);
        const int64_t room = (int64_t)PART_AGG_LDS - (int64_t)stage_c - 8 * occw - 16;
        if (room < (int64_t)(8 * esz)) return 0u;
        // whole 8-way sets, E a multiple of 16: the byte tags keep what follows them 16-B aligned
        return (uint32_t)std::min<int64_t>(65520, room / (int64_t)esz) & ~15u;
    };
    // the bucket count follows the general entry size, so packed entries only lower the load
    // factor (IGX_GBP_PE_LB=1: let them halve the bucket count instead)
    const size_t lb_entry = std::getenv("IGX_GBP_PE_LB") ? entry : agg_entry_bytes(KW, t->naggs);
    uint32_t lb = 0;
    while (lb < lb_max && (double)(t->cap >> lb) > 0.9 * entries(lb, lb_entry)) ++lb;
    p.lb = lb;
    p.f1 = (lb + 1) / 2;
    if (const char *d = std::getenv("IGX_GBP_F1"))   // tuning knob: first-level bucket bits
        p.f1 = std::min<uint32_t>(std::min<uint32_t>(lb, 8u), (uint32_t)std::strtoul(d, nullptr, 0));
    p.f1 = std::max<uint32_t>(p.f1, lb > 8 ? lb - 8 : 0u);   // both levels <= 256 buckets
    p.f2 = lb - p.f1;
    p.sb_log = t->sbits - lb;
    p.occw = 1u << (p.sb_log - 5);
    p.E = entries(lb, entry);
    if (p.E < 16) return igx_fail(ctx, IGX_ENOTSUP, "groupby_update: key of %u words too wide for the partitioned form", KW);
    if (const char *d = std::getenv("IGX_GBP_ENTRIES"))   // tests: a small LDS table overflows
        p.E = std::max<uint32_t>(16, std::min<uint32_t>(p.E, (uint32_t)std::strtoul(d, nullptr, 0))) & ~15u;
    p.maxp = std::min<uint32_t>(p.E / 8, 32);   // sets probed before a row takes the HBM path
    p.combine = 0;   // wave pre-combine: measured slower on C4 and C5
    if (const char *d = std::getenv("IGX_GBP_COMBINE")) p.combine = (uint32_t)std::strtoul(d, nullptr, 0);
    if (const char *d = std::getenv("IGX_GBP_DEBUG")) p.dbg = (uint32_t)std::strtoul(d, nullptr, 0);
    const uint32_t F1 = 1u << p.f1, F2 = 1u << p.f2, NB = 1u << lb;
    // B tiles: as many records (a multiple of PTA, at most 4096) as the tile LDS holds
    uint32_t trb = 4096;
    // (sized for the LDS-order path; the register path then stages 17 B per record in
    // ~52 KB, three blocks per CU: 4 096-record tiles measured 1.06 ms against 0.89 on C4)
    while (trb > PTA && (size_t)trb * (16 * p.rq + 6) + 12 * PART_F_MAX + 72 > PART_TILE_LDS) trb -= PTA;
    if (const char *d = std::getenv("IGX_GBP_TRB"))   // tuning knob: records per B tile (a multiple of PTA)
        trb = std::max<uint32_t>(PTA, std::min<uint32_t>(trb, (uint32_t)std::strtoul(d, nullptr, 0) / PTA * PTA));
    p.trb = trb;
    p.ch = (uint32_t)std::max<uint64_t>(8192, 4 * (a.n / NB + 1));
    p.tiles_a = (uint32_t)((a.n + TRA - 1) / TRA);
    p.nchunk = (p.tiles_a + CHT - 1) / CHT;
    const uint32_t S1 = region ? 1u << PART_S1_LOG : 1u, U1 = F1 * S1;   // first-level runs (slices)
    const uint64_t tiles_b = a.n / trb + U1 + 1;
    uint32_t c2pad = 16;   // final-region cursors one 64-B line apart (pass B's atomics)
    if (const char *d = std::getenv("IGX_GBP_C2PAD")) c2pad = std::max<uint32_t>(1, (uint32_t)std::strtoul(d, nullptr, 0));
    const uint64_t items_max = NB + a.n / p.ch + 1;
    uint64_t r1 = a.n * 5 / 4 / U1 + TRA, r2 = a.n * 5 / 4 / NB + 1024;   // region records
    if (const char *d = std::getenv("IGX_GBP_REGSIZE"))   // tests: small regions overflow
        r1 = r2 = std::max<uint64_t>(1, std::strtoull(d, nullptr, 0));
    if (region && (r1 * U1 >= (1ull << 31) || r2 * NB >= (1ull << 31))) region = false;
    if (region) {
        p.reg1 = (uint32_t)r1;
        p.reg2 = (uint32_t)r2;
        p.s1log = PART_S1_LOG;
        p.c2pad = c2pad;
        // scratch: rc1 | rc2 | tstart | bt | istart | itfb | ctl (u32 words)
        const uint64_t words = U1 * RC1_PAD + NB * c2pad + (U1 + 1) + tiles_b + (NB + 1) + items_max + 4;
        int rc = grow(ctx, reinterpret_cast<void **>(&t->p_cnt), &t->p_cnt_bytes, 4 * words);
        if (!rc) rc = grow(ctx, reinterpret_cast<void **>(&t->p_recs), &t->p_recs_bytes,
                           (size_t)16 * p.rq * (r1 * U1 + r2 * NB));
        if (rc) return rc;
        p.rc1 = t->p_cnt;
        p.rc2 = p.rc1 + U1 * RC1_PAD;
        p.tstart = p.rc2 + NB * c2pad;
        p.bt = p.tstart + U1 + 1;
        p.istart = p.bt + tiles_b;
        p.itfb = p.istart + NB + 1;
        p.ctl = p.itfb + items_max;
        p.recs1 = t->p_recs;
        p.recs2 = t->p_recs + r1 * U1 * p.rq * 4;
    }
    // scratch: cnt1 | csum | hist | start2 | cur2 | tstart | bt | istart | itfb | ctl (u32 words)
    const uint64_t w_cnt1 = (uint64_t)p.tiles_a * F1, w_csum = (uint64_t)p.nchunk * F1;
    const uint64_t words = w_cnt1 + w_csum + NB + (NB + 1) + NB + (F1 + 1) + tiles_b + (NB + 1) + items_max + 4;
    int rc = region ? IGX_OK : grow(ctx, reinterpret_cast<void **>(&t->p_cnt), &t->p_cnt_bytes, 4 * words);
    const size_t rec_bytes = (size_t)16 * p.rq;
    if (!rc && !region) rc = grow(ctx, reinterpret_cast<void **>(&t->p_recs), &t->p_recs_bytes, 2 * rec_bytes * a.n);
    if (rc) return rc;
    if (!region) {
    p.cnt1 = t->p_cnt;
    p.csum = p.cnt1 + w_cnt1;
    p.hist = p.csum + w_csum;
    p.start2 = p.hist + NB;
    p.cur2 = p.start2 + NB + 1;
    p.tstart = p.cur2 + NB;
    p.bt = p.tstart + F1 + 1;
    p.istart = p.bt + tiles_b;
    p.itfb = p.istart + NB + 1;
    p.ctl = p.itfb + items_max;
    p.recs1 = t->p_recs;
    p.recs2 = t->p_recs + (uint64_t)a.n * p.rq * 4;
    }
    const size_t lds_k = 4 * ((size_t)NB + F1);
    const size_t lds_a = (size_t)TRA * (16 * p.rq + 1) + 12 * (size_t)F1 + 4 * 17;
    const size_t lds_b = PackKey<L>::known && L::KW <= 8 && gbp_b_regs(p) ? (size_t)trb * (16 * p.rq + 1) + 12 * (size_t)F2 + 4 * 17
                                                            : (size_t)trb * (16 * p.rq + 6) + 12 * (size_t)F2 + 4 * 17;
    const size_t lds_c = (size_t)p.E * entry + 8 * (size_t)p.occw + 16 + stage_c;
    // dynamic LDS granted to each kernel so far (pass C keeps its own: gbp_launch_c)
    static size_t lds_set[3] = {0, 0, 0};
    const void *kern[3] = {reinterpret_cast<const void *>(k_gbp_count<L, NV>),
                           reinterpret_cast<const void *>(k_gbp_a<L, NV, WIDE>),
                           reinterpret_cast<const void *>(k_gbp_b<L, NV, WIDE>)};
    const size_t need[3] = {lds_k, lds_a, lds_b};
    for (int i = 0; i < 3; ++i) {
        if (need[i] > lds_set[i]) {
            IGX_HIP(ctx, hipFuncSetAttribute(kern[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)need[i]));
            lds_set[i] = need[i];
        }
    }
    const uint32_t cus = (uint32_t)ctx->num_cus;
    if (region) {
        IGX_HIP(ctx, hipMemsetAsync(p.rc1, 0, 4ull * (U1 * RC1_PAD + NB * p.c2pad), ctx->stream));
        hipLaunchKernelGGL((k_gbp_a<L, NV, WIDE>), dim3(p.tiles_a), dim3(PTA), lds_a, ctx->stream, a, p);
        if (p.dbg & 256u) return IGX_OK;   // diagnostics: stop after pass A (the table is left unset)
        hipLaunchKernelGGL(k_gbr_tiles, dim3(1), dim3(1024), 0, ctx->stream, p);
        hipLaunchKernelGGL((k_gbp_b<L, NV, WIDE>), dim3((unsigned)tiles_b), dim3(PTA), lds_b, ctx->stream, a, p);
        if (p.dbg & 512u) return IGX_OK;   // ... after pass B
        hipLaunchKernelGGL(k_gbr_items, dim3(1), dim3(1024), 0, ctx->stream, p);
    }
    if (!region) {
    IGX_HIP(ctx, hipMemsetAsync(p.hist, 0, 4ull * NB, ctx->stream));
    hipLaunchKernelGGL((k_gbp_count<L, NV>), dim3(std::min<uint32_t>(p.tiles_a, 2 * cus)), dim3(PTA), lds_k,
                       ctx->stream, a, p);
    hipLaunchKernelGGL(k_gbp_csum, dim3(p.nchunk), dim3(PTA), 0, ctx->stream, p);
    hipLaunchKernelGGL(k_gbp_scan, dim3(1), dim3(1024), 0, ctx->stream, p);
    hipLaunchKernelGGL(k_gbp_offs, dim3(p.nchunk), dim3(PTA), 0, ctx->stream, p);
    if (p.dbg & 1024u) return IGX_OK;   // diagnostics: stop after the count and the scans
    hipLaunchKernelGGL((k_gbp_a<L, NV, WIDE>), dim3(p.tiles_a), dim3(PTA), lds_a, ctx->stream, a, p);
    if (p.dbg & 256u) return IGX_OK;   // diagnostics: stop after pass A (the table is left unset)
    hipLaunchKernelGGL((k_gbp_b<L, NV, WIDE>), dim3((unsigned)tiles_b), dim3(PTA), lds_b, ctx->stream, a, p);
    if (p.dbg & 512u) return IGX_OK;   // ... after pass B
    }
    return gbp_launch_c(t, a, p, lds_c);
}

// record layout and the loaded columns; predicates become a row mask first
template <class L>
int launch_part(igx_table *t, igx_ctx *ctx, GbArgs &a) {
    PartArgs p{};
    // packed key words: 1- and 2-byte columns share words, other columns keep theirs
    uint32_t wp = 0, used = 4, shared = 0, w = 0;
    for (uint32_t c = 0; c < t->nkeys; ++c) {
        const uint32_t cw = t->key_widths[c];
        if (cw <= 2) {
            if (used + cw > 4) {
                shared = wp++;
                used = 0;
            }
            p.kpw[w] = shared;
            p.ksh[w] = 8 * used;
            p.kmsk[w] = cw == 1 ? 0xFFu : 0xFFFFu;
            used += cw;
            ++w;
        } else {
            for (uint32_t j = 0; j < (cw + 3) / 4; ++j, ++w) {
                p.kpw[w] = wp++;
                p.ksh[w] = 0;
                p.kmsk[w] = 0xFFFFFFFFu;
            }
        }
    }
    if (w != t->key_words) return igx_fail(ctx, IGX_EINVAL, "groupby_update: internal key packing mismatch");
    p.kpn = wp;
    // each distinct value / condition column once
    uint32_t nv = 0;
    auto col_of = [&](const uint8_t *ptr, uint32_t width) {
        for (uint32_t j = 0; j < nv; ++j)
            if (p.vcol[j] == ptr && p.vcw[j] == width) return j;
        p.vcol[nv] = ptr;
        p.vcw[nv] = width;
        p.vchi[nv] = width == 8 ? 4 : 0;
        return nv++;
    };
    for (uint32_t x = 0; x < AMAX; ++x) {
        p.vsrc[x] = p.csrc[x] = PNV;
        if (x >= t->naggs) continue;
        if (!a.vcount[x]) p.vsrc[x] = col_of(a.vptr[x], a.vwidth[x]);
        if (a.hascond[x]) p.csrc[x] = col_of(a.cptr[x], a.cwidth[x]);
    }
    for (uint32_t j = 0; j < nv; ++j) {
        p.rpos[j] = wp;
        p.rw2[j] = p.vcw[j] == 8;
        wp += 1 + p.rw2[j];
    }
    p.nv = nv;
    for (uint32_t x = 0; x < AMAX; ++x) {
        p.avp[x] = p.vsrc[x] < PNV ? p.rpos[p.vsrc[x]] : 0xFFFFu;
        p.av2[x] = p.vsrc[x] < PNV ? p.rw2[p.vsrc[x]] : 0u;
        p.acp[x] = p.csrc[x] < PNV ? p.rpos[p.csrc[x]] : 0xFFFFu;
        p.ac2[x] = p.csrc[x] < PNV ? p.rw2[p.csrc[x]] : 0u;
    }
    for (uint32_t j = nv; j < PNV; ++j) {   // unused: dword 0 of a readable column
        p.vcol[j] = a.kcol[0];
        p.vcw[j] = 0;
        p.vchi[j] = 0;
        p.rpos[j] = 0;
        p.rw2[j] = 0;
    }
    p.iw = a.fidx ? 2 : 1;
    p.ipos = wp;
    wp += p.iw;
    p.rq = (wp + 3) / 4;
    p.rq_magic = p.rq > 1 ? (uint32_t)((0x100000000ull + p.rq - 1) / p.rq) : 0u;
    if (a.npred) {
        int rc = grow(ctx, reinterpret_cast<void **>(&t->p_mask), &t->p_mask_bytes, igx_align(a.n, 256));
        if (rc) return rc;
        hipLaunchKernelGGL(k_gbp_mask, dim3((unsigned)std::min<uint64_t>(4096, (a.n + 255) / 256)), dim3(256), 0,
                           ctx->stream, a, t->p_mask);
        a.valid = a.validp = t->p_mask;
        a.validw = 1;
        a.npred = 0;
    }
    // AUTO's miss-heavy intervals run the region variant (no count pass); IGX_GB_PART keeps
    // exact runs, whose split work items also take heavily skewed streams in stride
    // The region variant sizes each bucket's region at 1.25x its share of the rows; a bucket
    // past it merges its extra records into the table directly (exact; a wave's spilled
    // records are pre-combined per key first, region_spill).  An interval that overflowed a
    // region switches AUTO to the exact variant for the rest of the partitioned run.
    const bool region = (t->mode == IGX_GB_AUTO || std::getenv("IGX_GBP_REGION")) && !std::getenv("IGX_GBP_EXACT") &&
                        t->region_off == 0;
    t->interval_region = t->interval_region || region;
    return part_with_shape(nv, t->wide, [&](auto nvc, auto wide) {
        return launch_part_as<L, decltype(nvc)::value, decltype(wide)::value>(t, ctx, a, p, region);
    });
}

}  // namespace

void gb_part_load() {
    hipFuncAttributes fa;
    (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_gbp_csum));
    gbp_c_load();
}

int gb_launch_part(igx_table *t, GbArgs &a) {
    return gb_with_layout(t, [&](auto tag) { return launch_part<typename decltype(tag)::type>(t, t->ctx, a); });
}
