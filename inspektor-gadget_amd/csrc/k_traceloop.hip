// k_traceloop.hip -- traceloop: the sys_enter / sys_exit / cont join by monotonic timestamp.
//
// Restates Tracer.Read (pkg/gadgets/traceloop/tracer/tracer.go:246-545: three maps of slices keyed
// by the timestamp, the publishing loops, the sort by event time) over the two record streams of
// a batch; include/igx.h has the contract and DESIGN.md the closed form.  No row walks its group:
// what a group comes to is an associative summary (k_traceloop.h) scanned reduce-then-scan over
// the rows of both streams sorted by (mntns, mono_ts, key).
//
//   pack     one u64 key per row of either stream beside its mntns and mono_ts: the only pass
//            that reads typ / id / pid / valid / index, all of it coalesced
//   sort     stable order of the row ids by (mntns, mono_ts, key) (launch_sort_perm)
//   code     one byte per sorted position: kind, cont index, group head, subgroup head
//   summary  one TlSum per tile of TL_TILE positions
//   carry    one workgroup: exclusive scan of the tile summaries
//   groups   per tile, from its carry: at the last position of every group, what the group
//            comes to (16 bytes, and its six first conts if it has any), indexed by group number
//   class    per tile: every syscall row's group number (a count of heads) and from the group's
//            result its event class; the number of events
//   sort     the syscall rows by (no event, sort_ts), ties by row: the events come first
//   emit     the output columns of event j from its row and its group's result
//
// Every launch is a plain grid; no workgroup waits on another, and the only atomic is the integer
// add of the event count.  Algorithmic bytes per row: DESIGN.md §4.
#include "k_scan.h"
#include "k_traceloop.h"

namespace {

constexpr int TB = SCAN_TB, RPT = SCAN_RPT, TL_TILE = SCAN_TILE;
constexpr int CARRY_T = 512;

struct TlIn {
    const uint64_t *mntns, *mono_ts;
    const uint8_t *typ;
    const uint16_t *id;
    const uint32_t *pid;
    const uint8_t *valid;
    uint64_t ns;
    const uint64_t *c_mntns, *c_mono_ts;
    const uint8_t *c_index, *c_valid;
    uint64_t nc;
};

__global__ __launch_bounds__(TB) void k_tl_pack(TlIn in, uint64_t *__restrict__ k_mn, uint64_t *__restrict__ k_ts,
                                                uint64_t *__restrict__ k_sub) {
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= in.ns + in.nc) return;
    if (i < in.ns) {
        if (k_mn) k_mn[i] = in.mntns[i];
        k_ts[i] = in.mono_ts[i];
        k_sub[i] = tl_key_sys(in.pid[i], in.id[i], in.typ[i], !in.valid || in.valid[i] != 0);
    } else {
        const uint64_t j = i - in.ns;
        if (k_mn) k_mn[i] = in.c_mntns[j];
        k_ts[i] = in.c_mono_ts[j];
        k_sub[i] = tl_key_cont(in.c_index[j], !in.c_valid || in.c_valid[j] != 0);
    }
}

__global__ __launch_bounds__(TB) void k_tl_code(const uint64_t *__restrict__ k_mn, const uint64_t *__restrict__ k_ts,
                                                const uint64_t *__restrict__ k_sub,
                                                const uint32_t *__restrict__ perm, uint64_t n, uint16_t nr_exit,
                                                uint16_t nr_exit_group, uint16_t nr_rt_sigreturn,
                                                uint8_t *__restrict__ code) {
    const uint64_t p = (uint64_t)blockIdx.x * TB + threadIdx.x;
    const bool in = p < n;
    // each lane gathers its own row's keys and takes its left neighbour's from the lane below;
    // lane 0 gathers that row too
    uint64_t key = 0, ts = 0, mn = 0;
    if (in) {
        const uint32_t r = perm[p];
        key = k_sub[r];
        ts = k_ts[r];
        if (k_mn) mn = k_mn[r];
    }
    uint64_t qkey = __shfl_up((unsigned long long)key, 1), qts = __shfl_up((unsigned long long)ts, 1);
    uint64_t qmn = __shfl_up((unsigned long long)mn, 1);
    if (!in) return;
    if ((threadIdx.x & 63) == 0 && p > 0) {
        const uint32_t q = perm[p - 1];
        qkey = k_sub[q];
        qts = k_ts[q];
        qmn = k_mn ? k_mn[q] : 0;
    }
    const bool gh = p == 0 || ts != qts || mn != qmn;
    const bool sh = (key >> 2) != (qkey >> 2);
    code[p] = (uint8_t)(tl_kind(key, nr_exit, nr_exit_group, nr_rt_sigreturn) | (gh ? TL_CODE_GH : 0u) |
                        (gh || sh ? TL_CODE_SH : 0u));
}

__device__ __forceinline__ TlSum tl_shfl_up(const TlSum &v, int o) {
    TlSum r;
    r.ng = __shfl_up(v.ng, o);
    r.flags = __shfl_up(v.flags, o);
    r.e0 = __shfl_up(v.e0, o);
    r.m = __shfl_up(v.m, o);
    r.mx = __shfl_up(v.mx, o);
    r.te = __shfl_up(v.te, o);
    r.tx = __shfl_up(v.tx, o);
    r.le = __shfl_up(v.le, o);
    r.lx = __shfl_up(v.lx, o);
#pragma unroll
    for (int i = 0; i < TL_PARAMS; ++i) r.c[i] = __shfl_up(v.c[i], o);
    r.pad = 0;
    return r;
}

// The tile's RPT codes and rows of this thread (TL_NONE past n) and their summary.
__device__ __forceinline__ TlSum tl_thread_sum(const uint8_t *__restrict__ code, const uint32_t *__restrict__ perm,
                                               uint64_t p0, uint64_t n, uint32_t (&c)[RPT], uint32_t (&row)[RPT]) {
    // code is allocated to a multiple of TL_TILE, so the 8-byte load stays inside it
    const uint64_t w = *reinterpret_cast<const uint64_t *>(code + p0);
    TlSum acc = tl_identity();
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        const bool in = p0 + j < n;
        c[j] = in ? (uint32_t)(w >> (8 * j)) & 0xFFu : TL_NONE;
        row[j] = in ? perm[p0 + j] : 0u;
        acc = tl_combine(acc, tl_elem(row[j], c[j]));
    }
    return acc;
}

struct TlOp {
    using T = TlSum;
    static __device__ __forceinline__ T identity() { return tl_identity(); }
    static __device__ __forceinline__ T combine(const T &x, const T &y) { return tl_combine(x, y); }
    static __device__ __forceinline__ T shfl_up(const T &v, int o) { return tl_shfl_up(v, o); }
};

__global__ __launch_bounds__(TB) void k_tl_summary(const uint8_t *__restrict__ code,
                                                   const uint32_t *__restrict__ perm, uint64_t n,
                                                   TlSum *__restrict__ sums) {
    __shared__ TlSum wsum[TB / 64];
    uint32_t c[RPT], row[RPT];
    const uint64_t p0 = (uint64_t)blockIdx.x * TL_TILE + (uint64_t)threadIdx.x * RPT;
    const TlSum mine = tl_thread_sum(code, perm, p0, n, c, row);
    TlSum total;
    (void)block_scan<TlOp>(mine, wsum, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// carry[t] = the summary of tiles [0, t); one workgroup
__global__ __launch_bounds__(CARRY_T) void k_tl_carry(const TlSum *__restrict__ sums, uint64_t m,
                                                      TlSum *__restrict__ carry) {
    tile_carry<TlOp, CARRY_T>(sums, m, carry);
}

// At the last position of every group: what the group comes to, at its number.
__global__ __launch_bounds__(TB) void k_tl_groups(const uint8_t *__restrict__ code,
                                                  const uint32_t *__restrict__ perm, uint64_t n,
                                                  const TlSum *__restrict__ carry, uint4 *__restrict__ gsum,
                                                  uint32_t *__restrict__ gcont) {
    __shared__ TlSum wsum[TB / 64];
    uint32_t c[RPT], row[RPT];
    const uint64_t p0 = (uint64_t)blockIdx.x * TL_TILE + (uint64_t)threadIdx.x * RPT;
    const TlSum mine = tl_thread_sum(code, perm, p0, n, c, row);
    TlSum total;
    const TlSum exc = block_scan<TlOp>(mine, wsum, &total);
    if (p0 >= n) return;
    TlSum st = tl_combine(carry[blockIdx.x], exc);
    // the code after this thread's last one says whether that one ends its group
    const uint32_t after = p0 + RPT < n ? code[p0 + RPT] : TL_CODE_GH;
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        const uint64_t p = p0 + j;
        if (p >= n) break;
        st = tl_combine(st, tl_elem(row[j], c[j]));
        const uint32_t next = p + 1 >= n ? TL_CODE_GH : (j + 1 < RPT ? c[(j + 1) % RPT] : after);
        if (next & TL_CODE_GH) {
            const TlGroup g = tl_final(st);
            const uint64_t gid = st.ng - 1;   // position 0 is a head, so ng >= 1; gid < n
            gsum[gid] = make_uint4(g.e0, g.m, g.mx, g.flags);
            if (g.flags & TL_HASCONT) {
#pragma unroll
                for (int i = 0; i < TL_PARAMS; ++i) gcont[gid * TL_PARAMS + i] = st.c[i];
            }
        }
    }
}

// Every syscall row's event class from its group's result; rows that emit get their class, a
// zero "no event" byte and their group number.  *d_nev accumulates the number of events.
__global__ __launch_bounds__(TB) void k_tl_class(const uint8_t *__restrict__ code,
                                                 const uint32_t *__restrict__ perm, uint64_t n,
                                                 const TlSum *__restrict__ carry, const uint4 *__restrict__ gsum,
                                                 uint8_t *__restrict__ cls, uint8_t *__restrict__ nf,
                                                 uint32_t *__restrict__ t_gid,
                                                 unsigned long long *__restrict__ d_nev) {
    __shared__ uint32_t wh[TB / 64], wc[TB / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t p0 = (uint64_t)blockIdx.x * TL_TILE + (uint64_t)threadIdx.x * RPT;
    const uint64_t w = *reinterpret_cast<const uint64_t *>(code + p0);
    uint32_t c[RPT], heads = 0;
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        c[j] = p0 + j < n ? (uint32_t)(w >> (8 * j)) & 0xFFu : TL_NONE;
        heads += (c[j] & TL_CODE_GH) ? 1u : 0u;
    }
    uint32_t inc = heads;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t lo = __shfl_up(inc, o);
        if (lane >= (uint32_t)o) inc += lo;
    }
    if (lane == 63) wh[wave] = inc;
    __syncthreads();
    uint32_t g = carry[blockIdx.x].ng + inc - heads;   // group heads before this thread's positions
    for (uint32_t v = 0; v < wave; ++v) g += wh[v];
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        if (p0 + j >= n) break;
        if (c[j] & TL_CODE_GH) ++g;
        const uint32_t k = c[j] & 7u;
        if (k != TL_ENTER && k != TL_ENTER_SKIP && k != TL_EXIT) continue;
        const uint32_t r = perm[p0 + j], gid = g - 1;
        const uint4 q = gsum[gid];
        TlGroup grp;
        grp.e0 = q.x;
        grp.m = q.y;
        grp.mx = q.z;
        grp.flags = q.w;
        const uint32_t cl = tl_class(grp, r, k);
        if (cl == TL_DROP) continue;
        cls[r] = (uint8_t)cl;
        nf[r] = 0;
        t_gid[r] = gid;
        ++cnt;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
    if (lane == 0) wc[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int v = 0; v < TB / 64; ++v) s += wc[v];
        if (s) atomicAdd(d_nev, (unsigned long long)s);
    }
}

__global__ __launch_bounds__(TB) void k_tl_emit(uint64_t ns, const uint64_t *__restrict__ d_nev,
                                                const uint8_t *__restrict__ cls,
                                                const uint32_t *__restrict__ t_gid,
                                                const uint4 *__restrict__ gsum, const uint32_t *__restrict__ gcont,
                                                uint32_t *__restrict__ ev_row, uint32_t *__restrict__ ev_exit,
                                                uint8_t *__restrict__ ev_class, uint32_t *__restrict__ ev_cont) {
    const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (j >= ns) return;
    uint32_t row = IGX_NO_COL, ex = IGX_NO_COL, cl = 0xFF, cont[TL_PARAMS];
#pragma unroll
    for (int i = 0; i < TL_PARAMS; ++i) cont[i] = IGX_NO_COL;
    if (j < *d_nev) {
        row = ev_row[j];   // the second sort's order: the rows with an event first
        cl = cls[row];
        const uint32_t gid = t_gid[row];
        const uint4 q = gsum[gid];
        if (cl == 0 && q.y == row) ex = q.z;
        if (cl == 0 && q.x == row && (q.w & TL_HASCONT)) {
#pragma unroll
            for (int i = 0; i < TL_PARAMS; ++i) {
                const uint32_t v = gcont[(uint64_t)gid * TL_PARAMS + i];
                cont[i] = v == TL_NO ? IGX_NO_COL : (uint32_t)(v - ns);
            }
        }
    }
    ev_row[j] = row;
    ev_exit[j] = ex;
    ev_class[j] = (uint8_t)cl;
#pragma unroll
    for (int i = 0; i < TL_PARAMS; ++i) ev_cont[j * TL_PARAMS + i] = cont[i];
}

}  // namespace

extern "C" int igx_traceloop_tile(void) { return TL_TILE; }

extern "C" int igx_traceloop_join(igx_ctx *ctx, const uint64_t *mntns, const uint64_t *mono_ts,
                                  const uint64_t *sort_ts, const uint8_t *typ, const uint16_t *id,
                                  const uint32_t *pid, const uint8_t *valid, uint64_t ns, const uint64_t *c_mntns,
                                  const uint64_t *c_mono_ts, const uint8_t *c_index, const uint8_t *c_valid,
                                  uint64_t nc, uint16_t nr_exit, uint16_t nr_exit_group, uint16_t nr_rt_sigreturn,
                                  uint32_t *ev_row, uint32_t *ev_exit, uint8_t *ev_class, uint32_t *ev_cont,
                                  uint64_t *d_nev) {
    if (!ctx) return IGX_EINVAL;
    int rc = igx_check_rows(ctx, "traceloop_join", ns, nc);
    if (rc) return rc;
    if (!d_nev) return igx_fail(ctx, IGX_EINVAL, "traceloop_join: null count");
    if ((uintptr_t)d_nev & 7) return igx_fail(ctx, IGX_EINVAL, "traceloop_join: count not 8-byte aligned");
    if (ns && (!mono_ts || !sort_ts || !typ || !id || !pid || !ev_row || !ev_exit || !ev_class || !ev_cont))
        return igx_fail(ctx, IGX_EINVAL, "traceloop_join: null argument");
    if (nc && (!c_mono_ts || !c_index)) return igx_fail(ctx, IGX_EINVAL, "traceloop_join: null cont column");
    if (ns && nc && (mntns == nullptr) != (c_mntns == nullptr))
        return igx_fail(ctx, IGX_EINVAL, "traceloop_join: mntns on one stream only");
    if (((uintptr_t)mntns | (uintptr_t)mono_ts | (uintptr_t)sort_ts | (uintptr_t)c_mntns | (uintptr_t)c_mono_ts) & 7)
        return igx_fail(ctx, IGX_EINVAL, "traceloop_join: mntns and timestamps must be 8-byte aligned");
    if (((uintptr_t)pid | (uintptr_t)ev_row | (uintptr_t)ev_exit | (uintptr_t)ev_cont) & 3)
        return igx_fail(ctx, IGX_EINVAL, "traceloop_join: pid and row outputs must be 4-byte aligned");
    if ((uintptr_t)id & 1) return igx_fail(ctx, IGX_EINVAL, "traceloop_join: id must be 2-byte aligned");
    IGX_HIP(ctx, hipMemsetAsync(d_nev, 0, 8, ctx->stream));
    if (ns == 0) return IGX_OK;   // conts alone publish nothing (tracer.go:362: the loops run over enters and exits)

    const uint64_t n = ns + nc;
    const bool has_mn = mntns != nullptr;
    const uint64_t ntiles = (n + TL_TILE - 1) / TL_TILE;
    // side arena: keys (3 x 8n; the groups' conts, 24 bytes a group, take their place once the
    // code pass has read them) | order | group results | per syscall row: class, no-event, group
    const size_t key_b = igx_align(n * 8, 256), perm_b = igx_align(n * 4, 256), gsum_b = igx_align(n * 16, 256);
    const size_t byte_b = igx_align(ns, 256), gid_b = igx_align(ns * 4, 256);
    const size_t side_need = 3 * key_b + perm_b + gsum_b + 2 * byte_b + gid_b;
    // scratch arena (the sorts' while they run): code | tile summaries | carries
    uint8_t *code;
    TlSum *sums, *carry;
    const auto carve = [&](void *base) {
        IgxCarve c{reinterpret_cast<char *>(base)};
        code = c.take<uint8_t>(ntiles * TL_TILE);
        sums = c.take<TlSum>(ntiles * sizeof(TlSum));
        carry = c.take<TlSum>(ntiles * sizeof(TlSum));
        return c.used;
    };
    const size_t need = carve(nullptr);
    void *s, *sd;
    rc = igx_side(ctx, side_need, &sd);
    if (rc) return rc;
    // ask before the sort, so that an arena that has to grow does it before the order exists
    rc = igx_scratch(ctx, need, &s);
    if (rc) return igx_side_drop(ctx, rc);
    char *d = reinterpret_cast<char *>(sd);
    uint64_t *k_mn = has_mn ? reinterpret_cast<uint64_t *>(d) : nullptr;
    uint64_t *k_ts = reinterpret_cast<uint64_t *>(d + key_b), *k_sub = reinterpret_cast<uint64_t *>(d + 2 * key_b);
    uint32_t *gcont = reinterpret_cast<uint32_t *>(d);   // 24 bytes x groups <= 3 x key_b
    uint32_t *perm = reinterpret_cast<uint32_t *>(d + 3 * key_b);
    uint4 *gsum = reinterpret_cast<uint4 *>(d + 3 * key_b + perm_b);
    uint8_t *cls = reinterpret_cast<uint8_t *>(d + 3 * key_b + perm_b + gsum_b);
    uint8_t *nf = cls + byte_b;
    uint32_t *t_gid = reinterpret_cast<uint32_t *>(nf + byte_b);

    TlIn in{mntns, mono_ts, typ, id, pid, valid, ns, c_mntns, c_mono_ts, c_index, c_valid, nc};
    hipLaunchKernelGGL(k_tl_pack, dim3((unsigned)((n + TB - 1) / TB)), dim3(TB), 0, ctx->stream, in, k_mn, k_ts, k_sub);
    IGX_HIP(ctx, hipGetLastError());
    const SortPlanKey key[3] = {sort_key_u64(k_mn), sort_key_u64(k_ts), sort_key_u64(k_sub)};
    const int k0 = has_mn ? 0 : 1;
    rc = launch_sort_perm(ctx, key + k0, 3 - k0, n, nullptr, false, nullptr, perm, 0, nullptr);
    if (rc) return rc;
    rc = igx_scratch(ctx, need, &s);
    if (rc) return rc;
    (void)carve(s);

    IGX_HIP(ctx, hipMemsetAsync(cls, 0xFF, byte_b, ctx->stream));
    IGX_HIP(ctx, hipMemsetAsync(nf, 1, byte_b, ctx->stream));
    hipLaunchKernelGGL(k_tl_code, dim3((unsigned)((n + TB - 1) / TB)), dim3(TB), 0, ctx->stream, k_mn, k_ts, k_sub, perm,
                       n, nr_exit, nr_exit_group, nr_rt_sigreturn, code);
    hipLaunchKernelGGL(k_tl_summary, dim3((unsigned)ntiles), dim3(TB), 0, ctx->stream, code, perm, n, sums);
    hipLaunchKernelGGL(k_tl_carry, dim3(1), dim3(CARRY_T), 0, ctx->stream, sums, ntiles, carry);
    hipLaunchKernelGGL(k_tl_groups, dim3((unsigned)ntiles), dim3(TB), 0, ctx->stream, code, perm, n, carry, gsum, gcont);
    hipLaunchKernelGGL(k_tl_class, dim3((unsigned)ntiles), dim3(TB), 0, ctx->stream, code, perm, n, carry, gsum, cls, nf,
                       t_gid, reinterpret_cast<unsigned long long *>(d_nev));
    IGX_HIP(ctx, hipGetLastError());
    // the events in output order: the rows with an event first, by sort_ts, ties by row (the
    // sort is stable); the order lands in ev_row
    SortPlanKey k2[2] = {};
    k2[0].ptr = nf;
    k2[0].width = 1;
    k2[0].kind = IGX_KIND_UINT;
    k2[0].words = 1;
    k2[0].stride = 1;
    k2[1] = sort_key_u64(sort_ts);
    rc = launch_sort_perm(ctx, k2, 2, ns, nullptr, false, nullptr, ev_row, 0, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tl_emit, dim3((unsigned)((ns + TB - 1) / TB)), dim3(TB), 0, ctx->stream, ns, d_nev, cls, t_gid,
                       gsum, gcont, ev_row, ev_exit, ev_class, ev_cont);
    IGX_HIP(ctx, hipGetLastError());
    return IGX_OK;
}
