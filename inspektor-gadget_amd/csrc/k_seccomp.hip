// k_seccomp.hip -- advise seccomp-profile on the device: the per-mount-namespace syscall sets of
// ig_seccomp_e (advise/seccomp/tracer/bpf/seccomp.bpf.c:67-139).  include/igx.h has the contracts,
// k_seccomp.h the row classifier, the hash and the per-row code.
//
// The table is open-addressed over the u64 mntns (0 = empty), linear probing from sc_home, S a
// power of two >= 2 x capacity.  Per slot: the key, a 64-byte bitmap (bit id), a u64 gate (the
// global stream index of the namespace's first arming row, SC_NO_GATE for none) and a live byte.
// A key, once claimed, stays for the object's life (Delete clears the rest), so probe chains never
// break.  igx_seccomp_update is two plain grids on the context's stream:
//   gate  one lane per row: classify; find the key's slot or claim an empty one (CAS after an
//         agent-scope read); set live if it reads 0; an ARM row lowers the slot's gate with
//         atomicMin, only after a read shows the gate higher; write the row's u32 code.
//   mark  one lane per four codes: a PLAIN row records, an ARM or GATED row records when its index
//         is past the slot's gate -- complete, because the gate launch has ended.  Bits only ever
//         rise within a launch, so a stale read of a bitmap word can cause a redundant atomic but
//         never a lost bit: every atomicOr follows a read that found the bit missing.
//         LDS form (S <= LDS_SLOTS): the workgroup ORs into a private LDS copy of all bitmaps and
//         at the end commits only the words that add bits to the global word.
//         Global form: read-before-atomic straight to memory.
// No lane waits for another's store, no workgroup for another; every probe loop ends after S
// slots.  Overflow (more than capacity keys claimed, or no slot found) marks the object dead:
// codes of later rows are DROP, nothing is written out of bounds.
#include <algorithm>

#include "k_common.h"
#include "k_seccomp.h"

struct igx_seccomp {
    igx_ctx *ctx = nullptr;
    uint64_t cap = 0, nslots = 0;
    uint32_t nr_prctl = 0, nr_seccomp = 0;
    uint64_t rows_fed = 0;      // stream index of the next update's first row
    bool dead = false;          // igx_seccomp_count has seen the overflow
    uint64_t *keys = nullptr;   // nslots
    uint64_t *gate = nullptr;   // nslots
    uint32_t *bits = nullptr;   // nslots x SC_WORDS
    uint8_t *live = nullptr;    // nslots
    uint64_t *state = nullptr;  // ST_* words
};

namespace {

constexpr int TB = 256;                 // gate, global mark: rows per workgroup pass
constexpr int TBL = 1024;               // LDS mark: lanes per workgroup
constexpr int CPL = 4;                  // mark: codes per lane per pass (one 16-byte load)
constexpr uint64_t LDS_SLOTS = 2048;    // 128 KiB of bitmaps
constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;
constexpr int ST_KEYS = 0;   // slots claimed so far (deleted keys included)
constexpr int ST_DEAD = 1;   // capacity overflowed
constexpr int ST_LIVE = 2;   // scratch of the count / list kernel
constexpr size_t ST_BYTES = 64;

__device__ __forceinline__ uint32_t ld_comm4(const uint8_t *p, bool aligned) {
    if (aligned) return *reinterpret_cast<const uint32_t *>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

struct GateArgs {
    const uint64_t *mntns;
    const uint32_t *id;
    const uint64_t *arg0;
    const uint8_t *comm;
    uint64_t comm_stride;
    const uint8_t *compat, *valid;   // nullable
    uint64_t nrows, base;
    uint32_t nr_prctl, nr_seccomp, comm_aligned;
    uint64_t *keys, smask, *gate;
    uint8_t *live;
    uint64_t *state, cap;
    uint32_t *code;
};

__global__ __launch_bounds__(TB) void k_sc_gate(GateArgs a) {
    const bool dead = a.state[ST_DEAD] != 0;
    const uint64_t step = (uint64_t)gridDim.x * TB;
    for (uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x; i < a.nrows; i += step) {
        uint32_t c = 0;
        if (!dead && (!a.valid || a.valid[i] != 0)) {
            const uint64_t m = a.mntns[i];
            const uint32_t id = a.id[i];
            const uint32_t cls = sc_classify(m, id, a.arg0[i], ld_comm4(a.comm + i * a.comm_stride, a.comm_aligned != 0),
                                             a.compat ? a.compat[i] : 0u, a.nr_prctl, a.nr_seccomp);
            if (cls != SC_DROP) {
                uint64_t s = sc_home(m, a.smask + 1);
                bool found = false;
                for (uint64_t j = 0; j <= a.smask; ++j, s = (s + 1) & a.smask) {
                    unsigned long long k = ld_agent(a.keys + s);
                    if (k == 0) {
                        k = atomicCAS(reinterpret_cast<unsigned long long *>(a.keys + s), 0ull, (unsigned long long)m);
                        if (k == 0) {   // claimed
                            k = m;
                            const unsigned long long had =
                                atomicAdd(reinterpret_cast<unsigned long long *>(a.state + ST_KEYS), 1ull);
                            if (had + 1 > a.cap) st_agent(a.state + ST_DEAD, 1ull);
                        }
                    }
                    if (k == m) {
                        found = true;
                        break;
                    }
                }
                if (found) {
                    if (a.live[s] == 0) a.live[s] = 1;
                    if (cls == SC_ARM) {
                        const uint64_t idx = a.base + i;
                        if (ld_agent(a.gate + s) > idx)
                            atomicMin(reinterpret_cast<unsigned long long *>(a.gate + s), (unsigned long long)idx);
                    }
                    c = sc_pack((uint32_t)s, id, cls);
                } else {
                    st_agent(a.state + ST_DEAD, 1ull);
                }
            }
        }
        a.code[i] = c;
    }
}

// The bitmap word and bit a code marks, if its row records.  code is 16-byte aligned and padded
// to a multiple of four codes.
__device__ __forceinline__ bool mark_of(uint32_t c, uint64_t idx, const uint64_t *__restrict__ gate, uint32_t &word,
                                        uint32_t &bit) {
    const uint32_t cls = sc_code_class(c);
    if (cls == SC_DROP || cls == SC_TOUCH) return false;
    const uint32_t slot = sc_code_slot(c), id = sc_code_id(c);
    if (cls != SC_PLAIN && !sc_records(cls, idx, gate[slot])) return false;
    word = slot * SC_WORDS + (id >> 5);
    bit = 1u << (id & 31);
    return true;
}

__global__ __launch_bounds__(TBL) void k_sc_mark_lds(const uint32_t *__restrict__ code, uint64_t nrows, uint64_t base,
                                                     const uint64_t *__restrict__ gate, uint32_t *bits,
                                                     uint32_t nwords) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lb[];
    for (uint32_t w = threadIdx.x; w < nwords; w += TBL) lb[w] = 0;
    __syncthreads();
    const uint64_t nquads = (nrows + CPL - 1) / CPL, step = (uint64_t)gridDim.x * TBL;
    for (uint64_t q = (uint64_t)blockIdx.x * TBL + threadIdx.x; q < nquads; q += step) {
        const uint4 v = reinterpret_cast<const uint4 *>(code)[q];
        const uint32_t c[CPL] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const uint64_t row = q * CPL + k;
            uint32_t word, bit;
            if (row < nrows && mark_of(c[k], base + row, gate, word, bit) && !(lb[word] & bit))
                atomicOr(&lb[word], bit);
        }
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < nwords; w += TBL) {
        const uint32_t v = lb[w];
        if (v != 0 && (v & ~bits[w]) != 0) atomicOr(bits + w, v);
    }
}

__global__ __launch_bounds__(TB) void k_sc_mark_global(const uint32_t *__restrict__ code, uint64_t nrows,
                                                       uint64_t base, const uint64_t *__restrict__ gate,
                                                       uint32_t *bits) {
    const uint64_t nquads = (nrows + CPL - 1) / CPL, step = (uint64_t)gridDim.x * TB;
    for (uint64_t q = (uint64_t)blockIdx.x * TB + threadIdx.x; q < nquads; q += step) {
        const uint4 v = reinterpret_cast<const uint4 *>(code)[q];
        const uint32_t c[CPL] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const uint64_t row = q * CPL + k;
            uint32_t word, bit;
            if (row < nrows && mark_of(c[k], base + row, gate, word, bit) && !(bits[word] & bit))
                atomicOr(bits + word, bit);
        }
    }
}

// The slot that holds m, or NO_SLOT; claims nothing.  An empty slot ends the chain.
__device__ __forceinline__ uint32_t find_slot(const uint64_t *__restrict__ keys, uint64_t smask, uint64_t m) {
    if (m == 0) return NO_SLOT;
    uint64_t s = sc_home(m, smask + 1);
    for (uint64_t j = 0; j <= smask; ++j, s = (s + 1) & smask) {
        const uint64_t k = keys[s];
        if (k == m) return (uint32_t)s;
        if (k == 0) break;
    }
    return NO_SLOT;
}

// one workgroup per queried namespace: SC_VALUE_BYTES bytes and a found byte
__global__ __launch_bounds__(512) void k_sc_peek(const uint64_t *__restrict__ q_mntns, uint64_t n,
                                                 const uint64_t *__restrict__ keys, uint64_t smask,
                                                 const uint64_t *__restrict__ gate, const uint8_t *__restrict__ live,
                                                 const uint32_t *__restrict__ bits, uint8_t *__restrict__ out,
                                                 uint8_t *__restrict__ found) {
    __shared__ uint32_t sh_slot;
    for (uint64_t q = blockIdx.x; q < n; q += gridDim.x) {
        if (threadIdx.x == 0) {
            const uint64_t m = q_mntns[q];
            uint32_t s = find_slot(keys, smask, m);
            if (s != NO_SLOT && live[s] == 0) s = NO_SLOT;
            sh_slot = s;
            found[q] = (m == 0 || s != NO_SLOT) ? 1 : 0;   // key 0 holds the reference's blank value
        }
        __syncthreads();
        const uint32_t s = sh_slot, t = threadIdx.x;
        if (t < SC_VALUE_BYTES) {
            uint8_t v = 0;
            if (s != NO_SLOT)
                v = t < SC_SYSCALLS ? (bits[(uint64_t)s * SC_WORDS + (t >> 5)] >> (t & 31)) & 1u
                                    : (gate[s] != SC_NO_GATE ? 1 : 0);
            out[q * SC_VALUE_BYTES + t] = v;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(TB) void k_sc_delete(const uint64_t *__restrict__ q_mntns, uint64_t n,
                                                  const uint64_t *__restrict__ keys, uint64_t smask, uint64_t *gate,
                                                  uint8_t *live, uint32_t *bits) {
    const uint64_t q = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (q >= n) return;
    const uint32_t s = find_slot(keys, smask, q_mntns[q]);
    if (s == NO_SLOT) return;
    // a namespace listed twice gets the same stores twice
    for (uint32_t w = 0; w < SC_WORDS; ++w) bits[(uint64_t)s * SC_WORDS + w] = 0;
    gate[s] = SC_NO_GATE;
    live[s] = 0;
}

// counts the live slots into state[ST_LIVE]; with out, also lists their keys (in no order)
__global__ __launch_bounds__(TB) void k_sc_list(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ live,
                                                uint64_t nslots, uint64_t *__restrict__ out, uint64_t cap,
                                                uint64_t *state) {
    const uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (s >= nslots || live[s] == 0) return;
    const uint64_t pos = atomicAdd(reinterpret_cast<unsigned long long *>(state + ST_LIVE), 1ull);
    if (out && pos < cap) out[pos] = keys[s];
}

int live_count(igx_seccomp *t, uint64_t *out, uint64_t cap, uint64_t *n, const char *what) {
    igx_ctx *ctx = t->ctx;
    IGX_HIP(ctx, hipMemsetAsync(t->state + ST_LIVE, 0, 8, ctx->stream));
    hipLaunchKernelGGL(k_sc_list, dim3((unsigned)((t->nslots + TB - 1) / TB)), dim3(TB), 0, ctx->stream, t->keys,
                       t->live, t->nslots, out, cap, t->state);
    IGX_HIP(ctx, hipGetLastError());
    uint64_t st[4] = {0, 0, 0, 0};
    IGX_HIP(ctx, hipMemcpyAsync(st, t->state, sizeof st, hipMemcpyDeviceToHost, ctx->stream));
    IGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n = st[ST_LIVE];
    if (st[ST_DEAD]) {
        t->dead = true;
        return igx_fail(ctx, IGX_ENOSPC, "%s: more than %llu mount namespaces", what, (unsigned long long)t->cap);
    }
    return IGX_OK;
}

}  // namespace

extern "C" int igx_seccomp_destroy(igx_seccomp *t) {
    if (!t) return IGX_OK;
    (void)hipStreamSynchronize(t->ctx->stream);
    (void)hipFree(t->keys);
    (void)hipFree(t->gate);
    (void)hipFree(t->bits);
    (void)hipFree(t->live);
    (void)hipFree(t->state);
    delete t;
    return IGX_OK;
}

extern "C" int igx_seccomp_create(igx_ctx *ctx, uint64_t capacity, uint32_t nr_prctl, uint32_t nr_seccomp,
                                  igx_seccomp **out) {
    if (!ctx) return IGX_EINVAL;
    if (!out) return igx_fail(ctx, IGX_EINVAL, "seccomp_create: null out");
    *out = nullptr;
    if (capacity == 0 || capacity > SC_MAX_SLOTS / 2)
        return igx_fail(ctx, IGX_EINVAL, "seccomp_create: capacity must be in 1..2^19");
    auto *t = new igx_seccomp();
    t->ctx = ctx;
    t->cap = capacity;
    t->nr_prctl = nr_prctl;
    t->nr_seccomp = nr_seccomp;
    uint64_t ns = 2;
    while (ns < 2 * capacity) ns <<= 1;
    t->nslots = ns;
    hipError_t e = hipMalloc(&t->keys, ns * 8);
    if (e == hipSuccess) e = hipMalloc(&t->gate, ns * 8);
    if (e == hipSuccess) e = hipMalloc(&t->bits, ns * SC_WORDS * 4);
    if (e == hipSuccess) e = hipMalloc(&t->live, ns);
    if (e == hipSuccess) e = hipMalloc(&t->state, ST_BYTES);
    if (e == hipSuccess) e = hipMemsetAsync(t->keys, 0, ns * 8, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->gate, 0xFF, ns * 8, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->bits, 0, ns * SC_WORDS * 4, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->live, 0, ns, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->state, 0, ST_BYTES, ctx->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        igx_seccomp_destroy(t);
        return igx_fail(ctx, IGX_ENOMEM, "seccomp_create: %s", hipGetErrorString(e));
    }
    *out = t;
    return IGX_OK;
}

extern "C" int igx_seccomp_update(igx_seccomp *t, const uint64_t *mntns, const uint32_t *id, const uint64_t *arg0,
                                  const void *comm, uint64_t comm_stride, const uint8_t *compat, const uint8_t *valid,
                                  uint64_t nrows) {
    if (!t) return IGX_EINVAL;
    igx_ctx *ctx = t->ctx;
    if (nrows > 0x7FFFFFFFull) return igx_fail(ctx, IGX_EINVAL, "seccomp_update: more than 2^31 - 1 rows");
    if (comm_stride < 4) return igx_fail(ctx, IGX_EINVAL, "seccomp_update: comm_stride must be at least 4");
    if (nrows && (!mntns || !id || !arg0 || !comm)) return igx_fail(ctx, IGX_EINVAL, "seccomp_update: null column");
    if ((((uintptr_t)mntns | (uintptr_t)arg0) & 7) || ((uintptr_t)id & 3))
        return igx_fail(ctx, IGX_EINVAL, "seccomp_update: mntns and arg0 must be 8-byte, id 4-byte aligned");
    if (t->dead) return igx_fail(ctx, IGX_ENOSPC, "seccomp_update: the map has overflowed its capacity");
    if (nrows == 0) return IGX_OK;

    void *s;
    const int rc = igx_scratch(ctx, igx_align(nrows * 4, 256), &s);
    if (rc) return rc;
    GateArgs a;
    a.mntns = mntns;
    a.id = id;
    a.arg0 = arg0;
    a.comm = reinterpret_cast<const uint8_t *>(comm);
    a.comm_stride = comm_stride;
    a.compat = compat;
    a.valid = valid;
    a.nrows = nrows;
    a.base = t->rows_fed;
    a.nr_prctl = t->nr_prctl;
    a.nr_seccomp = t->nr_seccomp;
    a.comm_aligned = (((uintptr_t)comm | comm_stride) & 3) == 0;
    a.keys = t->keys;
    a.smask = t->nslots - 1;
    a.gate = t->gate;
    a.live = t->live;
    a.state = t->state;
    a.cap = t->cap;
    a.code = reinterpret_cast<uint32_t *>(s);
    const uint64_t fill = (uint64_t)ctx->num_cus;
    const unsigned g1 = (unsigned)std::max<uint64_t>(1, std::min((nrows + TB - 1) / TB, fill * 8));
    hipLaunchKernelGGL(k_sc_gate, dim3(g1), dim3(TB), 0, ctx->stream, a);
    if (t->nslots <= LDS_SLOTS) {
        static bool attr_set = false;
        if (!attr_set) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_sc_mark_lds),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS_SLOTS * SC_WORDS * 4));
            attr_set = true;
        }
        const uint32_t nwords = (uint32_t)(t->nslots * SC_WORDS);
        const unsigned g2 = (unsigned)std::max<uint64_t>(1, std::min((nrows + TBL * CPL - 1) / (TBL * CPL), fill));
        hipLaunchKernelGGL(k_sc_mark_lds, dim3(g2), dim3(TBL), nwords * 4, ctx->stream, a.code, nrows, a.base, t->gate,
                           t->bits, nwords);
    } else {
        const unsigned g2 = (unsigned)std::max<uint64_t>(1, std::min((nrows + TB * CPL - 1) / (TB * CPL), fill * 8));
        hipLaunchKernelGGL(k_sc_mark_global, dim3(g2), dim3(TB), 0, ctx->stream, a.code, nrows, a.base, t->gate,
                           t->bits);
    }
    IGX_HIP(ctx, hipGetLastError());
    t->rows_fed += nrows;
    return IGX_OK;
}

extern "C" int igx_seccomp_peek(igx_seccomp *t, const uint64_t *mntns, uint64_t n, uint8_t *out, uint8_t *found) {
    if (!t) return IGX_EINVAL;
    igx_ctx *ctx = t->ctx;
    if (n == 0) return IGX_OK;
    if (!mntns || !out || !found) return igx_fail(ctx, IGX_EINVAL, "seccomp_peek: null argument");
    if ((uintptr_t)mntns & 7) return igx_fail(ctx, IGX_EINVAL, "seccomp_peek: mntns must be 8-byte aligned");
    hipLaunchKernelGGL(k_sc_peek, dim3((unsigned)std::min<uint64_t>(n, 65536)), dim3(512), 0, ctx->stream, mntns, n,
                       t->keys, t->nslots - 1, t->gate, t->live, t->bits, out, found);
    IGX_HIP(ctx, hipGetLastError());
    return IGX_OK;
}

extern "C" int igx_seccomp_delete(igx_seccomp *t, const uint64_t *mntns, uint64_t n) {
    if (!t) return IGX_EINVAL;
    igx_ctx *ctx = t->ctx;
    if (n > 0xFFFFFFFFull) return igx_fail(ctx, IGX_EINVAL, "seccomp_delete: too many namespaces");
    if (n == 0) return IGX_OK;
    if (!mntns) return igx_fail(ctx, IGX_EINVAL, "seccomp_delete: null argument");
    if ((uintptr_t)mntns & 7) return igx_fail(ctx, IGX_EINVAL, "seccomp_delete: mntns must be 8-byte aligned");
    hipLaunchKernelGGL(k_sc_delete, dim3((unsigned)((n + TB - 1) / TB)), dim3(TB), 0, ctx->stream, mntns, n, t->keys,
                       t->nslots - 1, t->gate, t->live, t->bits);
    IGX_HIP(ctx, hipGetLastError());
    return IGX_OK;
}

extern "C" int igx_seccomp_list(igx_seccomp *t, uint64_t *out, uint64_t cap, uint64_t *n) {
    if (!t || !n) return IGX_EINVAL;
    if (cap && !out) return igx_fail(t->ctx, IGX_EINVAL, "seccomp_list: null out");
    if ((uintptr_t)out & 7) return igx_fail(t->ctx, IGX_EINVAL, "seccomp_list: out must be 8-byte aligned");
    return live_count(t, cap ? out : nullptr, cap, n, "seccomp_list");
}

extern "C" int igx_seccomp_count(igx_seccomp *t, uint64_t *n) {
    if (!t || !n) return IGX_EINVAL;
    return live_count(t, nullptr, 0, n, "seccomp_count");
}

extern "C" int igx_seccomp_slots(igx_seccomp *t, uint64_t *n_slots) {
    if (!t || !n_slots) return IGX_EINVAL;
    *n_slots = t->nslots;
    return IGX_OK;
}

extern "C" int igx_seccomp_home(uint64_t mntns, uint64_t nslots, uint64_t *home) {
    if (!home || nslots == 0 || (nslots & (nslots - 1))) return IGX_EINVAL;
    *home = sc_home(mntns, nslots);
    return IGX_OK;
}
