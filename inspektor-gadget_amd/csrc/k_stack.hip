// k_stack.hip -- profile cpu on the device: row interning (what bpf_get_stackid and the kernel's
// stack map do for profile.bpf.c:90-98) and the kernel symbol search (findKernelSymbol,
// tracer.go:184-208).  include/igx.h has the contracts, k_stack.h the hash and the search.
//
// igx_intern_add, every launch a plain grid on the context's stream:
//   insert  one wave per row: lane l holds the 16 bytes at l * 16 (8 where the row ends on a
//           half), the wave sums the lanes' word hashes, then probes linearly from the home
//           slot.  A slot is one u64, tag (hash >> 32) over a reference: a stored id, or with
//           bit 31 set a row of this batch.  An empty slot is claimed by CAS; a slot with the
//           row's tag has its row compared (the same load and a ballot); an equal batch row
//           that comes later in the batch is lowered to this row with atomicMin -- only after
//           the slot was read and found higher, so the hottest stack of a skewed stream costs
//           reads, not atomics.  Once claimed, a slot's content never changes in the launch and
//           its reference only falls, so it ends as the content's first row.  The slot a row
//           ended at goes to out_ids.
//   flag    a row is new when its slot still refers to it; one byte per row, counts per tile
//   scan    one workgroup: exclusive scan of the tile counts, the id base and the new count;
//           overflow (count past capacity, or a row that found no slot) marks the object dead
//   assign  a new row's rank is its position among the new rows in row order; its slot becomes
//           tag | id, and the row joins the list of new rows
//   copy    one wave per new row: the row is appended to the store
//   gather  out_ids[i] = the id in the slot that out_ids[i] named
// Row content is only ever read from memory that no workgroup writes in the same launch: the
// batch, or the store as earlier launches left it (a CU's L1 is not refreshed by another CU's
// stores).  Within a launch only the slot words are shared, through device-scope atomics.  No
// lane waits for another's store; every probe loop ends after S slots.
#include <algorithm>

#include "k_scan.h"
#include "k_stack.h"

struct igx_intern {
    igx_ctx *ctx = nullptr;
    uint32_t row_bytes = 0;
    uint64_t cap = 0, nslots = 0;
    uint8_t *store = nullptr;    // cap x row_bytes: row id at id * row_bytes
    uint64_t *slots = nullptr;   // nslots words
    uint64_t *state = nullptr;   // ST_* words
};

namespace {

constexpr int TB = 256;
constexpr int WPB = TB / 64;          // rows per workgroup pass of the wave-per-row kernels
constexpr int CRPT = 4;
constexpr int CTILE = TB * CRPT;      // rows per tile of the rank scan
constexpr uint64_t SLOT_EMPTY = ~0ull;
constexpr uint32_t REF_BATCH = 0x80000000u;   // the reference is a row of the batch
// the object's device words
constexpr int ST_COUNT = 0;    // distinct rows stored (the capacity once dead)
constexpr int ST_BASE = 1;     // the count before the add in flight
constexpr int ST_NEW = 2;      // rows the add in flight appends
constexpr int ST_DEAD = 3;     // capacity overflowed: later adds intern nothing
constexpr int ST_NOSLOT = 4;   // a row of the insert in flight found no slot
constexpr size_t ST_BYTES = 64;

// The lane's part of a row: a = word 2 * lane, b = word 2 * lane + 1, zero past the row.  Rows
// are 8-byte aligned, so the 16-byte access is told no more than that.
__device__ __forceinline__ void row_load(const uint8_t *row, uint32_t row_bytes, uint32_t lane, uint64_t &a,
                                         uint64_t &b) {
    const uint32_t off = lane * 16;
    a = 0;
    b = 0;
    if (off + 16 <= row_bytes) {
        uint64_t v[2];
        __builtin_memcpy(v, __builtin_assume_aligned(row + off, 8), 16);
        a = v[0];
        b = v[1];
    } else if (off + 8 <= row_bytes) {
        a = *reinterpret_cast<const uint64_t *>(row + off);
    }
}

__device__ __forceinline__ void row_store(uint8_t *row, uint32_t row_bytes, uint32_t lane, uint64_t a, uint64_t b) {
    const uint32_t off = lane * 16;
    if (off + 16 <= row_bytes) {
        const uint64_t v[2] = {a, b};
        __builtin_memcpy(__builtin_assume_aligned(row + off, 8), v, 16);
    } else if (off + 8 <= row_bytes) {
        *reinterpret_cast<uint64_t *>(row + off) = a;
    }
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor((unsigned long long)v, o);
    return v;
}

__global__ __launch_bounds__(TB) void k_st_insert(const uint8_t *__restrict__ rows, uint64_t stride,
                                                  const uint8_t *__restrict__ valid, uint64_t nrows,
                                                  uint32_t row_bytes, const uint8_t *__restrict__ store,
                                                  uint64_t *slots, uint64_t smask, uint64_t *state,
                                                  uint32_t *__restrict__ out_slot) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = (uint64_t)gridDim.x * WPB;
    const bool dead = state[ST_DEAD] != 0;   // set by an earlier add's scan only
    for (uint64_t i = (uint64_t)blockIdx.x * WPB + (threadIdx.x >> 6); i < nrows; i += nwaves) {
        if (dead || (valid && valid[i] == 0)) {
            if (lane == 0) out_slot[i] = IGX_NO_COL;
            continue;
        }
        uint64_t a, b;
        row_load(rows + i * stride, row_bytes, lane, a, b);
        uint64_t part = 0;
        if (lane * 16 + 8 <= row_bytes) part = st_word(a, 2 * lane);
        if (lane * 16 + 16 <= row_bytes) part += st_word(b, 2 * lane + 1);
        const uint64_t h = st_finish(wave_sum(part), row_bytes);
        const uint64_t tag = h >> 32, mine = (tag << 32) | REF_BATCH | (uint32_t)i;
        uint64_t s = h & smask;
        uint32_t res = IGX_NO_COL;
        for (uint64_t j = 0; j <= smask; ++j, s = (s + 1) & smask) {
            unsigned long long v = 0;
            if (lane == 0) {
                v = ld_agent(slots + s);
                if (v == SLOT_EMPTY) {
                    v = atomicCAS(reinterpret_cast<unsigned long long *>(slots + s), SLOT_EMPTY, mine);
                    if (v == SLOT_EMPTY) v = mine;
                }
            }
            v = __shfl(v, 0);
            if (v == mine) {   // claimed
                res = (uint32_t)s;
                break;
            }
            if ((v >> 32) != tag) continue;
            const uint32_t ref = (uint32_t)v;
            const uint8_t *cand = (ref & REF_BATCH) ? rows + (uint64_t)(ref & ~REF_BATCH) * stride
                                                    : store + (uint64_t)ref * row_bytes;
            uint64_t ca, cb;
            row_load(cand, row_bytes, lane, ca, cb);
            if (__ballot(ca != a || cb != b)) continue;
            if (lane == 0 && (ref & REF_BATCH) && (ref & ~REF_BATCH) > (uint32_t)i)
                atomicMin(reinterpret_cast<unsigned long long *>(slots + s), (unsigned long long)mine);
            res = (uint32_t)s;
            break;
        }
        if (lane == 0) {
            out_slot[i] = res;
            if (res == IGX_NO_COL) st_agent(state + ST_NOSLOT, 1ull);
        }
    }
}

__global__ __launch_bounds__(TB) void k_st_flag(const uint32_t *__restrict__ out_slot,
                                                const uint64_t *__restrict__ slots, uint64_t nrows,
                                                uint8_t *__restrict__ flags, uint32_t *__restrict__ cnt) {
    __shared__ uint32_t wc[TB / 64];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < CRPT; ++j) {
        const uint64_t row = (uint64_t)blockIdx.x * CTILE + (uint64_t)j * TB + threadIdx.x;
        bool f = false;
        if (row < nrows) {
            const uint32_t s = out_slot[row];
            f = s != IGX_NO_COL && (uint32_t)slots[s] == (REF_BATCH | (uint32_t)row);
            flags[row] = f ? 1 : 0;
        }
        c += __popcll(__ballot(f));
    }
    if (lane == 0) wc[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < TB / 64; ++w) s += wc[w];
        cnt[blockIdx.x] = s;
    }
}

// exclusive scan of cnt[0..m) -> off[0..m) (one workgroup of 1024), then the add's bookkeeping
__global__ __launch_bounds__(1024) void k_st_scan(const uint32_t *__restrict__ cnt, uint64_t m,
                                                  uint64_t *__restrict__ off, uint64_t *state, uint64_t cap) {
    const uint64_t total = scan_counts(cnt, m, off);
    if (threadIdx.x == 1023) {
        const uint64_t base = state[ST_COUNT], fresh = total;
        const bool over = state[ST_NOSLOT] != 0 || base + fresh > cap;
        state[ST_BASE] = base;
        state[ST_NEW] = fresh;
        state[ST_COUNT] = over ? cap : base + fresh;
        if (over) state[ST_DEAD] = 1;
        state[ST_NOSLOT] = 0;
    }
}

__global__ __launch_bounds__(TB) void k_st_assign(const uint8_t *__restrict__ flags,
                                                  const uint32_t *__restrict__ out_slot, uint64_t nrows,
                                                  const uint64_t *__restrict__ off,
                                                  const uint64_t *__restrict__ state, uint64_t cap, uint64_t *slots,
                                                  uint32_t *__restrict__ newrows) {
    __shared__ uint32_t g[CTILE / 64];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    bool f[CRPT];
    uint64_t bal[CRPT];
#pragma unroll
    for (int j = 0; j < CRPT; ++j) {
        const uint64_t row = (uint64_t)blockIdx.x * CTILE + (uint64_t)j * TB + threadIdx.x;
        f[j] = row < nrows && flags[row] != 0;
        bal[j] = __ballot(f[j]);
        if (lane == 0) g[j * (TB / 64) + wave] = __popcll(bal[j]);   // group: 64 consecutive rows
    }
    __syncthreads();
    const uint64_t base = state[ST_BASE], tile_off = off[blockIdx.x];
#pragma unroll
    for (int j = 0; j < CRPT; ++j) {
        if (!f[j]) continue;
        const uint32_t grp = j * (TB / 64) + wave;
        uint32_t pre = 0;
        for (uint32_t w = 0; w < grp; ++w) pre += g[w];
        const uint64_t rank = tile_off + pre + __popcll(bal[j] & lanemask_lt());
        const uint64_t row = (uint64_t)blockIdx.x * CTILE + (uint64_t)j * TB + threadIdx.x;
        const uint64_t id = base + rank;
        // the one writer of this slot in this launch; no other thread reads it here
        uint64_t *sp = slots + out_slot[row];
        *sp = id < cap ? ((*sp >> 32) << 32) | id : SLOT_EMPTY;
        newrows[rank] = (uint32_t)row;
    }
}

__global__ __launch_bounds__(TB) void k_st_copy(const uint8_t *__restrict__ rows, uint64_t stride, uint32_t row_bytes,
                                                const uint32_t *__restrict__ newrows,
                                                const uint64_t *__restrict__ state, uint64_t cap,
                                                uint8_t *__restrict__ store) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = (uint64_t)gridDim.x * WPB;
    const uint64_t base = state[ST_BASE], fresh = state[ST_NEW];
    for (uint64_t r = (uint64_t)blockIdx.x * WPB + (threadIdx.x >> 6); r < fresh; r += nwaves) {
        const uint64_t id = base + r;
        if (id >= cap) break;
        uint64_t a, b;
        row_load(rows + (uint64_t)newrows[r] * stride, row_bytes, lane, a, b);
        row_store(store + id * row_bytes, row_bytes, lane, a, b);
    }
}

__global__ __launch_bounds__(TB) void k_st_gather(const uint64_t *__restrict__ slots, uint64_t nrows,
                                                  uint32_t *__restrict__ out_ids) {
    const uint64_t row = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (row >= nrows) return;
    const uint32_t s = out_ids[row];
    // a slot that overflowed was emptied: its low half reads IGX_NO_COL
    if (s != IGX_NO_COL) out_ids[row] = (uint32_t)slots[s];
}

__global__ __launch_bounds__(TB) void k_st_rows(const uint8_t *__restrict__ store, uint32_t row_bytes,
                                                const uint64_t *__restrict__ state,
                                                const uint32_t *__restrict__ ids, uint64_t k,
                                                uint8_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = (uint64_t)gridDim.x * WPB;
    const uint64_t count = state[ST_COUNT];
    for (uint64_t r = (uint64_t)blockIdx.x * WPB + (threadIdx.x >> 6); r < k; r += nwaves) {
        const uint32_t id = ids[r];
        uint64_t a = 0, b = 0;
        if (id != IGX_NO_COL && id < count) row_load(store + (uint64_t)id * row_bytes, row_bytes, lane, a, b);
        row_store(out + r * row_bytes, row_bytes, lane, a, b);
    }
}

__global__ __launch_bounds__(TB) void k_ksym(const uint64_t *__restrict__ sym, uint64_t nsyms,
                                             const uint64_t *__restrict__ ips, uint64_t n,
                                             uint32_t *__restrict__ out_idx) {
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i < n) out_idx[i] = st_ksym_find(sym, nsyms, ips[i]);
}

// workgroups of a wave-per-row grid: enough to fill the chip, rows beyond that by stride
unsigned wave_grid(const igx_ctx *ctx, uint64_t nrows) {
    const uint64_t need = (nrows + WPB - 1) / WPB, fill = (uint64_t)ctx->num_cus * 16;
    return (unsigned)std::max<uint64_t>(1, std::min(need, fill));
}

}  // namespace

extern "C" int igx_intern_destroy(igx_intern *t) {
    if (!t) return IGX_OK;
    (void)hipStreamSynchronize(t->ctx->stream);
    (void)hipFree(t->store);
    (void)hipFree(t->slots);
    (void)hipFree(t->state);
    delete t;
    return IGX_OK;
}

extern "C" int igx_intern_create(igx_ctx *ctx, uint32_t row_bytes, uint64_t capacity, igx_intern **out) {
    if (!ctx) return IGX_EINVAL;
    if (!out) return igx_fail(ctx, IGX_EINVAL, "intern_create: null out");
    *out = nullptr;
    if (row_bytes < 8 || row_bytes > 1024 || (row_bytes & 7))
        return igx_fail(ctx, IGX_EINVAL, "intern_create: row_bytes %u is not a multiple of 8 in 8..1024", row_bytes);
    if (capacity == 0 || capacity > (1ull << 28)) return igx_fail(ctx, IGX_EINVAL, "intern_create: bad capacity");
    auto *t = new igx_intern();
    t->ctx = ctx;
    t->row_bytes = row_bytes;
    t->cap = capacity;
    uint64_t ns = 2;
    while (ns < 2 * capacity) ns <<= 1;
    t->nslots = ns;
    hipError_t e = hipMalloc(&t->store, capacity * row_bytes);
    if (e == hipSuccess) e = hipMalloc(&t->slots, ns * 8);
    if (e == hipSuccess) e = hipMalloc(&t->state, ST_BYTES);
    if (e == hipSuccess) e = hipMemsetAsync(t->slots, 0xFF, ns * 8, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->state, 0, ST_BYTES, ctx->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        igx_intern_destroy(t);
        return igx_fail(ctx, IGX_ENOMEM, "intern_create: %s", hipGetErrorString(e));
    }
    *out = t;
    return IGX_OK;
}

extern "C" int igx_intern_slots(igx_intern *t, uint64_t *n_slots) {
    if (!t || !n_slots) return IGX_EINVAL;
    *n_slots = t->nslots;
    return IGX_OK;
}

// igx_intern_add and igx_intern_add_first.  The flag pass already marks a content's first
// occurrence over the whole stream (the row its slot still refers to): with out_first the flags
// are written there instead of to scratch.  Without out_ids the slot numbers go to scratch and
// the last pass, which turns them into ids, is left out.
static int intern_add(igx_intern *t, const void *rows, uint64_t row_stride, const uint8_t *valid, uint64_t nrows,
                      uint32_t *out_ids, uint8_t *out_first, bool want_first) {
    if (!t) return IGX_EINVAL;
    igx_ctx *ctx = t->ctx;
    if (nrows > 0x7FFFFFFFull) return igx_fail(ctx, IGX_EINVAL, "intern_add: more than 2^31 - 1 rows");
    if ((row_stride & 7) || row_stride < t->row_bytes)
        return igx_fail(ctx, IGX_EINVAL, "intern_add: row_stride must be a multiple of 8 and at least row_bytes");
    if ((uintptr_t)rows & 7) return igx_fail(ctx, IGX_EINVAL, "intern_add: rows must be 8-byte aligned");
    if ((uintptr_t)out_ids & 3) return igx_fail(ctx, IGX_EINVAL, "intern_add: out_ids must be 4-byte aligned");
    if (nrows == 0) return IGX_OK;
    if (!rows || (want_first ? !out_first : !out_ids)) return igx_fail(ctx, IGX_EINVAL, "intern_add: null argument");

    const uint64_t tiles = (nrows + CTILE - 1) / CTILE;
    const size_t flag_b = igx_align(nrows, 256), cnt_b = igx_align(tiles * 4, 256);
    const size_t off_b = igx_align(tiles * 8, 256), new_b = igx_align(nrows * 4, 256);
    const size_t slot_b = out_ids ? 0 : new_b;
    void *s;
    const int rc = igx_scratch(ctx, flag_b + cnt_b + off_b + new_b + slot_b, &s);
    if (rc) return rc;
    char *c = reinterpret_cast<char *>(s);
    uint8_t *flags = out_first ? out_first : reinterpret_cast<uint8_t *>(c);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(c + flag_b);
    uint64_t *off = reinterpret_cast<uint64_t *>(c + flag_b + cnt_b);
    uint32_t *newrows = reinterpret_cast<uint32_t *>(c + flag_b + cnt_b + off_b);
    const bool ids = out_ids != nullptr;
    if (!ids) out_ids = reinterpret_cast<uint32_t *>(c + flag_b + cnt_b + off_b + new_b);
    const uint8_t *in = reinterpret_cast<const uint8_t *>(rows);

    hipLaunchKernelGGL(k_st_insert, dim3(wave_grid(ctx, nrows)), dim3(TB), 0, ctx->stream, in, row_stride, valid, nrows,
                       t->row_bytes, t->store, t->slots, t->nslots - 1, t->state, out_ids);
    hipLaunchKernelGGL(k_st_flag, dim3((unsigned)tiles), dim3(TB), 0, ctx->stream, out_ids, t->slots, nrows, flags, cnt);
    hipLaunchKernelGGL(k_st_scan, dim3(1), dim3(1024), 0, ctx->stream, cnt, tiles, off, t->state, t->cap);
    hipLaunchKernelGGL(k_st_assign, dim3((unsigned)tiles), dim3(TB), 0, ctx->stream, flags, out_ids, nrows, off,
                       t->state, t->cap, t->slots, newrows);
    hipLaunchKernelGGL(k_st_copy, dim3(wave_grid(ctx, std::min(nrows, t->cap))), dim3(TB), 0, ctx->stream, in,
                       row_stride, t->row_bytes, newrows, t->state, t->cap, t->store);
    if (ids)
        hipLaunchKernelGGL(k_st_gather, dim3((unsigned)((nrows + TB - 1) / TB)), dim3(TB), 0, ctx->stream, t->slots,
                           nrows, out_ids);
    IGX_HIP(ctx, hipGetLastError());
    return IGX_OK;
}

extern "C" int igx_intern_add(igx_intern *t, const void *rows, uint64_t row_stride, const uint8_t *valid,
                              uint64_t nrows, uint32_t *out_ids) {
    return intern_add(t, rows, row_stride, valid, nrows, out_ids, nullptr, false);
}

extern "C" int igx_intern_add_first(igx_intern *t, const void *rows, uint64_t row_stride, const uint8_t *valid,
                                    uint64_t nrows, uint32_t *out_ids, uint8_t *out_first) {
    return intern_add(t, rows, row_stride, valid, nrows, out_ids, out_first, true);
}

extern "C" int igx_intern_count(igx_intern *t, uint64_t *n_distinct) {
    if (!t || !n_distinct) return IGX_EINVAL;
    igx_ctx *ctx = t->ctx;
    uint64_t st[4] = {0, 0, 0, 0};
    IGX_HIP(ctx, hipMemcpyAsync(st, t->state, sizeof st, hipMemcpyDeviceToHost, ctx->stream));
    IGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_distinct = st[ST_COUNT];
    if (st[ST_DEAD]) return igx_fail(ctx, IGX_ENOSPC, "intern: more than %llu distinct rows", (unsigned long long)t->cap);
    return IGX_OK;
}

extern "C" int igx_intern_rows(igx_intern *t, const uint32_t *ids, uint64_t k, void *out) {
    if (!t) return IGX_EINVAL;
    igx_ctx *ctx = t->ctx;
    if (k == 0) return IGX_OK;
    if (!ids || !out) return igx_fail(ctx, IGX_EINVAL, "intern_rows: null argument");
    if (((uintptr_t)ids & 3) || ((uintptr_t)out & 7))
        return igx_fail(ctx, IGX_EINVAL, "intern_rows: ids must be 4-byte and out 8-byte aligned");
    hipLaunchKernelGGL(k_st_rows, dim3(wave_grid(ctx, k)), dim3(TB), 0, ctx->stream, t->store, t->row_bytes, t->state,
                       ids, k, reinterpret_cast<uint8_t *>(out));
    IGX_HIP(ctx, hipGetLastError());
    return IGX_OK;
}

extern "C" int igx_intern_hash_rows(const void *rows, uint32_t row_bytes, uint64_t row_stride, uint64_t n,
                                    uint64_t *out) {
    if (row_bytes < 8 || row_bytes > 1024 || (row_bytes & 7) || row_stride < row_bytes) return IGX_EINVAL;
    if (n && (!rows || !out)) return IGX_EINVAL;
    const uint8_t *p = reinterpret_cast<const uint8_t *>(rows);
    for (uint64_t i = 0; i < n; ++i) out[i] = st_hash_row(p + i * row_stride, row_bytes);
    return IGX_OK;
}

extern "C" int igx_ksym_lookup(igx_ctx *ctx, const uint64_t *sym_addr, uint64_t nsyms, const uint64_t *ips, uint64_t n,
                               uint32_t *out_idx) {
    if (!ctx) return IGX_EINVAL;
    if (nsyms > 0xFFFFFFFEull) return igx_fail(ctx, IGX_EINVAL, "ksym_lookup: more than 2^32 - 2 symbols");
    if (n > 0xFFFFFFFFull * TB) return igx_fail(ctx, IGX_EINVAL, "ksym_lookup: too many addresses");
    if (n == 0) return IGX_OK;
    if (!ips || !out_idx || (nsyms && !sym_addr)) return igx_fail(ctx, IGX_EINVAL, "ksym_lookup: null argument");
    if (((uintptr_t)sym_addr | (uintptr_t)ips) & 7)
        return igx_fail(ctx, IGX_EINVAL, "ksym_lookup: sym_addr and ips must be 8-byte aligned");
    if ((uintptr_t)out_idx & 3) return igx_fail(ctx, IGX_EINVAL, "ksym_lookup: out_idx must be 4-byte aligned");
    hipLaunchKernelGGL(k_ksym, dim3((unsigned)((n + TB - 1) / TB)), dim3(TB), 0, ctx->stream, sym_addr, nsyms, ips, n,
                       out_idx);
    IGX_HIP(ctx, hipGetLastError());
    return IGX_OK;
}
