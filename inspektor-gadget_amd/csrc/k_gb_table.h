// k_gb_table.h -- the group-by's HBM table: what every translation unit of the group-by shares.
// k_groupby.hip (create / reset / finalize / lookup / sort), k_gb_cached.hip, k_gb_direct.hip and
// the partitioned form (k_gb_part.hip, k_gb_part_c.hip) include it: the kernel arguments, the key
// hash and the key layouts, the record addressing and the claim protocol, the row decoders,
// struct igx_table, the one list of key layouts (gb_with_layout) and the forms' host entry points.
//
// HBM table: S = 2^k slots (S >= 2 x capacity), open addressing with linear probing.
// Each slot has a key record (KR = 32..256 B, one cache line for every built-in layout):
//     [0, KOFF)            key words (KW x u32, packed; each key column padded to 4 B)
//     KOFF                 u64 tag   (hash bits 16..63 | generation; another generation = empty)
//     KOFF + 8             u64 ready (epoch << 48 | first_ins + 1.  An epoch before the
//                          generation's = key not yet published; the interval's own epoch =
//                          first_ins is this interval's: an upper bound of the group's first,
//                          whose value record holds first <= first_ins (or will, once the
//                          interval's atomics land); an earlier epoch of the generation = a
//                          key kept from an earlier interval, not yet seen in this one)
// and a value record (VR = 8 x 2^m B):  u64 first (first-occurrence event index), then
// u64 aggregate a at 8 + 8a.  The two are kept apart because 64-bit atomics execute at
// the memory side and drop their line from L2 (MI355X_MICROARCH.md, store flavours and
// global atomics): key records are written once per interval and stay L2-resident for
// the probes, value records only ever receive fire-and-forget atomics.
// The slot index IS the group id; igx_groupby_finalize lists the occupied slots from a
// bitmap (one bit per slot, so the list costs S/8 bytes, not a walk of every key record):
// the partitioned form's claimers set it, the cached form's mark a byte map with plain byte
// stores that finalize folds into it, the direct form's are read off the tags.  A reset bumps the epoch instead of rewriting the table: records of an
// older epoch read as empty and the claimer initialises its value record (first =
// first_ins, aggregates 0) before it publishes `ready`.
// Keys outlive their interval (a *generation* spans intervals): the reference drains its BPF
// map every interval (tcp/tracer/tracer.go:154-171) and re-inserts every recurring key, here a
// reset that continues the generation only returns the previous interval's groups' value
// records to (first = UINT64_MAX, sums 0), from finalize's slot list.  The first miss of a kept
// key in an interval finds it (no CAS, no key or value-record stores): it re-stamps `ready`
// with the interval's epoch and first_ins = its index + 1 (so its own first-index minimum is
// pushed like any earlier event's) and marks the occupancy byte.  So the interval's output is
// still exactly its own groups, sums and first indices.  A generation ends (the next interval
// starts an empty one: tag bits = that interval's epoch) when the keys it holds plus a full
// interval's capacity would pass 4/5 of the slots, after a failed interval, when the
// interval runs the direct or partitioned form, or at the epoch counter's wrap.
// A new key claims a record with a 64-bit CAS on the tag, writes its key with write-through
// (sc1) stores and publishes `ready` with an sc1 store after `s_waitcnt vmcnt(0)`; readers
// load the key record with 16-byte sc1 buffer loads (one round trip) and compare the key
// in registers (MI355X_MICROARCH.md §Workgroup dispatch, hand-off table row 1).
#pragma once

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <string>
#include <utility>
#include <vector>

#include <thread>

#include "k_common.h"

// event-stream loads of the group-by kernels: non-temporal (read once; IGX_GB_STREAM_NT=0
// builds a plain-load variant for cache-residency experiments)
#ifndef IGX_GB_STREAM_NT
#define IGX_GB_STREAM_NT 1
#endif
#if IGX_GB_STREAM_NT
#define IGX_STREAM_LOAD(p) __builtin_nontemporal_load(p)
#else
#define IGX_STREAM_LOAD(p) (*(p))
#endif
// a stream load, non-temporal (IGX_STREAM_LOAD) unless the caller asks for a plain one
template <bool NT, class T>
__device__ __forceinline__ T stream_ld(const T *p) {
    if constexpr (NT) return IGX_STREAM_LOAD(p);
    else return *p;
}

constexpr uint32_t SLOT_OVF = 0xFFFFFFFFu;
constexpr int KWMAX = 32;
constexpr int AMAX = 4;   // top file needs 4 (reads, rbytes, writes, wbytes)
constexpr int PMAX = 2;   // more predicates: run igx_filter first
constexpr int GTB = 1024;
constexpr uint64_t EP_MAX = 0xFFFF;              // epoch bits in a tag / in `ready`
constexpr uint64_t READY_IDX = (1ull << 48) - 1;  // `ready` = epoch << 48 | (first_ins + 1)
// Event indices stay below IDX_LIMIT on every path (include/igx.h, igx_groupby_update): a kept key's
// re-stamp stores index + 2 in `ready`'s 48 bits, one more than a claim does, so the claims, the
// re-stamp and the host's row-index guard all compare against this one constant and a fresh and a
// kept key accept and reject the same values.
constexpr uint64_t IDX_LIMIT = READY_IDX - 1;
// Every wait on another wave is bounded: a wait that never ends sets err bit 4
// (igx_groupby_finalize then fails with IGX_ENOSPC) instead of hanging the GPU.
constexpr uint32_t SPIN_LIMIT = 1u << 24;
// wave roles in a workgroup of the cached form: a.nl loaders stream rows, the next 15 - a.nl
// waves (probers) resolve LDS misses against HBM, and the last wave serves the HBM-update ring
constexpr uint32_t NWAVES = GTB / 64;
constexpr uint32_t NL_DEFAULT = 8;    // loader waves (7 probers + 1 server); IGX_GB_LOADERS sweeps

__device__ __forceinline__ bool ready_ok(uint64_t ready, uint64_t ep) { return (ready >> 48) == ep; }
// published in the generation that started at epoch gep (the interval's epoch is ep >= gep;
// epochs only grow within a generation: the counter's wrap clears the table)
__device__ __forceinline__ bool ready_pub(uint64_t ready, uint32_t gep, uint64_t ep) {
    const uint64_t r = ready >> 48;
    return r >= gep && r <= ep;
}
// the device generation block behind the error block (u64 words of igx_table::err):
// [3] the generation's first epoch (tag bits), [4] keys claimed in the generation before this
// interval (~0: end it), [5] keys claimed in this interval
constexpr int GEN_WORD = 3;

__host__ __device__ constexpr uint32_t koff_of(int kw) { return (uint32_t)((4 * kw + 7) & ~7); }
__host__ __device__ constexpr uint32_t pow2_at_least(uint32_t b) {
    uint32_t r = 8;
    while (r < b) r <<= 1;
    return r;
}
__host__ __device__ constexpr uint32_t krec_bytes(int kw) { return pow2_at_least(koff_of(kw) + 16); }
__host__ __device__ constexpr uint32_t vrec_bytes(uint32_t naggs) { return pow2_at_least(8 + 8 * naggs); }

// Every input byte is fetched with an unconditional load (no load sits behind a runtime
// branch), so all of a row's loads issue back to back and retire under one wait.
struct GbArgs {
    // static layouts: one base pointer per key column
    const uint8_t *kcol[16];
    // generic layout: word w = (dword at kptr[w] + row*kwidth[w] + koff[w]) & kmask[w], or,
    // for a column whose width is neither 1, 2 nor a multiple of 4, its kbytes[w] bytes
    // loaded one by one (such a column is not dword aligned)
    const uint8_t *kptr[KWMAX];
    uint32_t kwidth[KWMAX];
    uint32_t koff[KWMAX];
    uint32_t kmask[KWMAX];
    uint32_t kbytes[KWMAX];
    // aggregates: value = SUM column (vwidth bytes) or 1 (COUNT), if cond column == cval
    const uint8_t *vptr[AMAX];
    const uint8_t *cptr[AMAX];
    uint64_t cval[AMAX];
    uint64_t vdiv[AMAX];    // 0: plain value, else value / vdiv (unsigned)
    uint32_t vwidth[AMAX], vsign[AMAX], vcount[AMAX], cwidth[AMAX], hascond[AMAX];
    // per aggregate: load its value / condition column (1), or reuse aggregate vshare /
    // cshare's dwords (same column; AMAX = not shared)
    uint32_t vload[AMAX], cload[AMAX], vshare[AMAX], cshare[AMAX];
    // load geometry: row stride (0 = nothing to load: dword 0 of the pointer) and the
    // offset of the high dword (4 for 8-byte columns, else 0)
    uint32_t vldw[AMAX], cldw[AMAX], vhioff[AMAX], chioff[AMAX], phioff[PMAX], validw;
    uint32_t naggs;
    // scalar predicates (FilterSpec on a <= 8-byte column), AND-ed.  pldw: load stride (0 when
    // pshare < AMAX: the column is aggregate pshare's value column, whose raw value is reused).
    // A guarded predicate applies to the rows whose guard column equals gref; the fused
    // kernels read the guard as aggregate pguard's condition value (a guard on any other
    // column goes to the row mask), the mask kernel loads it from gptr (gwidth bytes).
    const uint8_t *pptr[PMAX];
    const uint8_t *gptr[PMAX];
    uint64_t pref[PMAX], gref[PMAX];
    uint32_t pwidth[PMAX], pkind[PMAX], pcmp[PMAX], pneg[PMAX], pcnt[PMAX];
    uint32_t pldw[PMAX], pshare[PMAX], pguard[PMAX], gwidth[PMAX];
    uint32_t npred;
    uint32_t lds_entries;   // E (8 x sets)
    uint32_t direct;        // 1: probers issue their HBM atomics; the server wave probes too
    uint32_t sm;            // 1: state-machine probers (IGX_GB_PROBER=0: batch probers)
    uint32_t admit_mask;    // LDS admission on a key's (admit_mask + 1)-th miss (ghost_admit), 0: on the first
    uint32_t nl;            // loader waves (1..14)
    // input
    const uint8_t *valid;   // nullable: rows with 0 are skipped (nil / filtered entries)
    const uint8_t *validp;  // valid, or the dummy column when there is none (always loaded)
    const uint64_t *fidx;   // nullable: per-row global event index (merging partial groups)
    uint64_t n, base_idx;
    // table
    uint8_t *krec;          // key records
    uint64_t *vrec;         // value records
    uint32_t krec_len;      // KR
    uint32_t krec_total;    // S x KR of a narrow table (< 2^32); 0 on a wide one (no descriptor reaches it)
    uint32_t vrec_words;    // VR / 8
    uint32_t vrec_total;    // S x VR when below 4 GiB (16-B buffer stores of a claim), else 0
    uint32_t *err;
    uint32_t *occ;          // occupancy bitmap, one bit per slot (set by the partitioned form's claimers)
    uint8_t *occb;          // occupancy byte map, one byte per slot: the cached form's claimers store
                            // 1 with a plain byte store (no atomic: one claimer per slot), finalize
                            // folds it into the bitmap (k_slots_count)
    uint64_t ep;            // the interval's epoch (1..EP_MAX): tags and `ready` of older
                            // epochs read as empty (the direct and partitioned forms, which
                            // always start a generation: their generation is ep)
    uint64_t *gen;          // the device generation block (GEN_WORD): the cached form reads its
                            // generation there and counts its claims into it
    uint64_t rmask;         // probe region slots - 1 (probing wraps inside a region)
    uint32_t sshift;        // home slot = h >> sshift (the hash's top bits)
    uint32_t max_probe;
    // diagnostics (IGX_GB_DEBUG; compiled into the top-tcp key's debug kernel only):
    // bit0 stop after load+hash, bit1 drop LDS misses, bit10 probers drop the cells they take, bit2 drop HBM atomics, bit3 count
    // hits/misses, bit8 no HBM probe (a hash-derived slot), bit9 no LDS accumulate on hits
    uint32_t dbg;
    unsigned long long *dbg_cnt;
    // sample-seeded LDS cache (cached form, kept keys): nseeds records of seed_words u32 each
    // (key words padded to quads | HBM slot | pad | hash) that every workgroup adopts into its
    // cache before the stream starts, when they belong to the current generation (*seed_gep)
    const uint32_t *seeds;
    const uint64_t *seed_gep;
    uint32_t nseeds;
    // update log (cached form with the server wave; k_gb_log.hip): null = every update goes out as
    // an atomic.  Workgroup w's server wave writes 8-byte records {value, (slot << 2) | aggregate}
    // at log + w * log_cap and its record count (nulls included) to log_cnt[w].
    uint32_t log_cap;
    uint64_t *log;
    uint32_t *log_cnt;
};

// ---- the update log's records and counters (k_gb_cached.hip writes, k_gb_log.hip reads) ----
constexpr uint32_t LOG_NULL_HI = 0xFFFFFFFFu;          // a position whose entry went out as an atomic
constexpr uint32_t LOG_SLOT_LIMIT = (1u << 30) - 1;    // slots below it fit a record
// u64 words of the error block (igx_table::err) counted per interval: records logged, and the
// entries that fell back to atomics because of their value, a full log region, a full bucket region
constexpr int LOG_STAT_WORD = 8;
__device__ __forceinline__ uint64_t log_record(uint32_t slot, uint32_t agg, uint32_t value) {
    return ((uint64_t)((slot << 2) | agg) << 32) | value;
}

// Key hash: NH (the UMAC inner hash) over the key's word pairs -- one 32x32->64 multiply
// per 8 key bytes, sum(( k[2i] + K[2i]) * (k[2i+1] + K[2i+1])) mod 2^64 -- then the murmur3
// 64-bit finaliser.  Exactness never depends on it (keys are compared in full); it only
// spreads slots, LDS sets and tags.
__device__ __forceinline__ uint32_t nh_const(int i) {
    return 0x9E3779B9u * (uint32_t)(2 * i + 1) + 0x7F4A7C15u;   // odd, distinct per word
}

template <int KW>
__device__ __forceinline__ uint64_t hash_key(const uint32_t (&k)[KW]) {
    uint64_t h = 0x243F6A8885A308D3ull ^ (uint64_t)KW;
#pragma unroll
    for (int w = 0; w < KW; w += 2) {
        const uint32_t a = k[w] + nh_const(w);
        const uint32_t b = ((w + 1 < KW) ? k[w + 1] : 0u) + nh_const(w + 1);
        h += (uint64_t)a * (uint64_t)b;
    }
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 33;
    return h;
}

// aligned dword containing byte `off`, shifted so that byte lands in bits 0..7; the
// dword containing a column's last byte never crosses its last 4-byte block (no overrun)
__device__ __forceinline__ uint32_t ldw(const uint8_t *base, uint64_t off) {
    const uint32_t d = *reinterpret_cast<const uint32_t *>(base + (off & ~3ull));
    return d >> ((uint32_t)(off & 3u) * 8u);
}

// zero-extended little-endian value of `width` (1, 2, 4 or 8) bytes at row; branch-free
[[maybe_unused]] __device__ __forceinline__ uint64_t ld_val(const uint8_t *base, uint64_t row, uint32_t width) {
    const uint64_t b = row * width;
    const uint32_t lomask = width >= 4 ? 0xFFFFFFFFu : ((1u << (8 * width)) - 1u);
    const uint32_t lo = ldw(base, b) & lomask;
    const uint32_t hi = ldw(base, b + (width == 8 ? 4u : 0u));
    return (uint64_t)lo | ((uint64_t)(width == 8 ? hi : 0u) << 32);
}

// Key layouts.  StaticLayout<W...> fixes the key column widths at compile time (the
// reference's BPF key structs: ip_key_t, file_id, the advisor tuple, single columns), so
// every key load is one typed load (dwordx4 for a 16-byte column) with no descriptors in
// registers.  GenericLayout<KW> handles any other layout from per-word descriptors.
template <int... W>
struct StaticLayout {
    static constexpr int NC = sizeof...(W);
    static constexpr int Ws[NC] = {W...};
    static constexpr int words(int c) { return (Ws[c] + 3) / 4; }
    static constexpr int off(int c) {
        int o = 0;
        for (int i = 0; i < c; ++i) o += words(i);
        return o;
    }
    static constexpr int KW = off(NC);
    static constexpr bool is_static = true;

    template <int c, bool NT>
    __device__ __forceinline__ static void load_col(const GbArgs &a, uint64_t row, uint32_t *k) {
        constexpr int w = Ws[c];
        constexpr int o = off(c);
        const uint8_t *p = a.kcol[c];
        // the event stream is read once: non-temporal loads, so it does not push the
        // table's key records out of the caches
        if constexpr (w == 16) {
            typedef unsigned int v4u __attribute__((ext_vector_type(4)));
            const v4u q = stream_ld<NT>(reinterpret_cast<const v4u *>(p) + row);
            k[o] = q.x; k[o + 1] = q.y; k[o + 2] = q.z; k[o + 3] = q.w;
        } else if constexpr (w == 8) {
            typedef unsigned int v2u __attribute__((ext_vector_type(2)));
            const v2u q = stream_ld<NT>(reinterpret_cast<const v2u *>(p) + row);
            k[o] = q.x; k[o + 1] = q.y;
        } else if constexpr (w == 4) {
            k[o] = stream_ld<NT>(reinterpret_cast<const uint32_t *>(p) + row);
        } else if constexpr (w == 2) {
            k[o] = stream_ld<NT>(reinterpret_cast<const uint16_t *>(p) + row);
        } else if constexpr (w == 1) {
            k[o] = stream_ld<NT>(p + row);
        } else {
            static_assert(w % 4 == 0, "key widths other than 1/2 must be multiples of 4");
#pragma unroll
            for (int j = 0; j < w / 4; ++j) k[o + j] = reinterpret_cast<const uint32_t *>(p + row * w)[j];
        }
    }
    template <bool NT, size_t... I>
    __device__ __forceinline__ static void load_all(const GbArgs &a, uint64_t row, uint32_t *k,
                                                    std::index_sequence<I...>) {
        (load_col<(int)I, NT>(a, row, k), ...);
    }
    template <bool NT = true>
    __device__ __forceinline__ static void load(const GbArgs &a, uint64_t row, uint32_t (&k)[KW]) {
        load_all<NT>(a, row, k, std::make_index_sequence<NC>{});
    }
};

template <int KWG>
struct GenericLayout {
    static constexpr int KW = KWG;
    static constexpr bool is_static = false;
    template <bool NT = true>
    __device__ __forceinline__ static void load(const GbArgs &a, uint64_t row, uint32_t (&k)[KW]) {
#pragma unroll
        for (int w = 0; w < KW; ++w) {
            const uint64_t off = row * a.kwidth[w] + a.koff[w];
            if (a.kbytes[w]) {   // an unaligned column: byte loads (uniform branch)
                uint32_t v = 0;
                for (uint32_t b = 0; b < a.kbytes[w]; ++b) v |= (uint32_t)a.kptr[w][off + b] << (8 * b);
                k[w] = v;
            } else {
                k[w] = ldw(a.kptr[w], off) & a.kmask[w];
            }
        }
    }
};

// A key's home slot is the hash's top bits and linear probing wraps inside the slot's
// region (table.rbits): a bucket of the partitioned form (also the hash's top bits) then owns
// whole regions of the table, in every form alike.
__device__ __forceinline__ uint64_t home_slot(const GbArgs &a, uint64_t h) { return h >> a.sshift; }
__device__ __forceinline__ uint64_t next_slot(const GbArgs &a, uint64_t s) {
    return (s & ~a.rmask) | ((s + 1) & a.rmask);
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rec_rsrc(const GbArgs &a) {
    return __builtin_amdgcn_make_buffer_rsrc(a.krec, (short)0, (int)a.krec_total, 0x00020000);
}

typedef unsigned int u4v __attribute__((ext_vector_type(4)));

// the first 16*NQ bytes of a key record (key, tag, ready) as sc1 loads (L2-served)
template <int NQ>
__device__ __forceinline__ void load_rec(__amdgpu_buffer_rsrc_t rs, uint32_t off, uint32_t (&d)[NQ * 4]) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const u4v q = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16 * i, 0, 16 /* sc1 */);
        d[4 * i] = q.x; d[4 * i + 1] = q.y; d[4 * i + 2] = q.z; d[4 * i + 3] = q.w;
    }
}

// lookup-or-insert in the HBM table; returns the slot (SLOT_OVF: table full) and the
// slot's first_ins (claiming event index).  An event with a larger index never needs the
// atomicMin on the value record's first: the group's first is min(first_ins, that field).
template <int KW>
constexpr int probe_quads() { return (int)((koff_of(KW) + 16 + 15) / 16); }   // key, tag, ready

// Record addressing.  A narrow table (S x KR < 4 GiB) addresses its key records
// through one raw buffer descriptor and a 32-bit byte offset.  A wide table (WIDE = true: S x KR
// >= 4 GiB, or IGX_GB_WIDE=1) addresses them per lane, krec + slot * KR in 64 bits, with the
// global forms of the same 16-byte write-through (sc1) loads and stores.  Those have no builtin,
// so they are inline asm, which the compiler does not count: a wide load's registers hold its
// data only after probe_wait.  The policy is a template parameter: the narrow instances carry
// none of the wide code.
template <int KW, bool WIDE = false>
using probe_regs = std::conditional_t<WIDE, u4v[probe_quads<KW>()], uint32_t[probe_quads<KW>() * 4]>;

// word i (a compile-time index) of a probed record
template <bool WIDE, class D>
__device__ __forceinline__ uint32_t rec_word(const D &d, int i) {
    if constexpr (WIDE) return d[i / 4][i % 4];
    else return d[i];
}

template <int I>
__device__ __forceinline__ void wide_load_quad(const uint8_t *p, u4v &q) {
    asm volatile("global_load_dwordx4 %0, %1, off offset:%2 sc1" : "=v"(q) : "v"(p), "i"(16 * I) : "memory");
}
template <int NQ, size_t... I>
__device__ __forceinline__ void wide_load_quads(const uint8_t *p, u4v (&d)[NQ], std::index_sequence<I...>) {
    (wide_load_quad<(int)I>(p, d[I]), ...);
}
// issues the loads of a record's first NQ quads; d is undefined until wide_wait_rec<NQ>(d)
template <int NQ>
__device__ __forceinline__ void wide_issue_rec(const uint8_t *p, u4v (&d)[NQ]) {
    wide_load_quads<NQ>(p, d, std::make_index_sequence<NQ>{});
}
// the wait names every destination: no use of d is scheduled above it
template <int NQ>
__device__ __forceinline__ void wide_wait_rec(u4v (&d)[NQ]) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(d[0]) : : "memory");
#pragma unroll
    for (int i = 1; i < NQ; ++i) asm volatile("" : "+v"(d[i]));
}
template <int NQ>
__device__ __forceinline__ void wide_load_rec(const uint8_t *p, u4v (&d)[NQ]) {
    wide_issue_rec<NQ>(p, d);
    wide_wait_rec<NQ>(d);
}
// 16 bytes, written through; the trailing nop keeps the data registers until the store has read them
__device__ __forceinline__ void wide_store_quad(uint8_t *p, u4v q) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(q) : "memory");
}

// the home slot's record, issued early so its round trip overlaps other work (wide: probe_wait
// before find_or_insert)
template <int KW, bool WIDE = false>
__device__ __forceinline__ void probe_issue(const GbArgs &a, uint64_t h, probe_regs<KW, WIDE> &d) {
    if constexpr (WIDE) wide_issue_rec<probe_quads<KW>()>(a.krec + home_slot(a, h) * a.krec_len, d);
    else load_rec<probe_quads<KW>()>(rec_rsrc(a), (uint32_t)(home_slot(a, h) * a.krec_len), d);
}
template <int KW, bool WIDE = false>
__device__ __forceinline__ void probe_wait(probe_regs<KW, WIDE> &d) {
    if constexpr (WIDE) wide_wait_rec<probe_quads<KW>()>(d);
}

// A claimer's value record: first = its event index, aggregate x = vinit[x] (the claiming
// event's own values, so they need no atomic; null: 0), written through (sc1) as 16-B stores
// where the record array allows buffer addressing -- a claim's stores are memory-side write
// requests each, and they are the largest share of a high-cardinality interval's requests.
// The padding words of the record are never read and not written.
// (All indices are compile-time: a register array indexed at run time would live in scratch.)
template <int NV>
__device__ __forceinline__ void vrec_init(const GbArgs &a, uint64_t s, uint64_t gidx, const uint64_t (&v)[NV]) {
    uint64_t w[NV + 2];
    w[0] = gidx;
#pragma unroll
    for (int x = 0; x < NV; ++x) w[1 + x] = v[x];
    w[NV + 1] = 0;
    uint64_t *vr = a.vrec + s * a.vrec_words;
    const uint32_t nw = 1 + a.naggs;   // <= 1 + NV
    if (a.vrec_total) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.vrec, (short)0, (int)a.vrec_total, 0x00020000);
        const uint32_t off = (uint32_t)(s * a.vrec_words * 8);
#pragma unroll
        for (int j = 0; j < NV + 1; j += 2) {
            if ((uint32_t)j >= nw) break;
            if ((uint32_t)j + 1 < nw) {
                const u4v q = {(uint32_t)w[j], (uint32_t)(w[j] >> 32), (uint32_t)w[j + 1], (uint32_t)(w[j + 1] >> 32)};
                __builtin_amdgcn_raw_buffer_store_b128(q, rs, off + 8 * j, 0, 16 /* sc1 */);
            } else {
                st_agent(vr + j, w[j]);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < NV + 1; ++j)
            if ((uint32_t)j < nw) st_agent(vr + j, w[j]);
    }
}

// d holds the home slot's record (probe_issue).  vinit: the event's aggregate values, written
// into the value record when this call claims the slot (claimed = true; the caller then adds
// them nowhere else).
template <int KW, bool SET_OCC, int NV, bool WIDE = false>
__device__ __forceinline__ uint32_t find_or_insert(const GbArgs &a, const uint32_t (&k)[KW], uint64_t h,
                                                   uint64_t gidx, uint64_t &first_ins,
                                                   probe_regs<KW, WIDE> &d,
                                                   const uint64_t (&vinit)[NV], bool &claimed) {
    constexpr uint32_t KOFF = koff_of(KW);
    constexpr int NQ = probe_quads<KW>();
    const uint64_t tag = (h & ~EP_MAX) | a.ep;
    [[maybe_unused]] const auto rs = [&] {   // narrow: the records' descriptor
        if constexpr (WIDE) return 0;
        else return rec_rsrc(a);
    }();
    // the record at byte offset off (narrow) / at r (wide), complete when this returns
    auto reload = [&](uint32_t off, const uint8_t *r) {
        if constexpr (WIDE) wide_load_rec<NQ>(r, d);
        else load_rec<NQ>(rs, off, d);
    };
    uint64_t s = home_slot(a, h);
    for (uint32_t probe = 0; probe < a.max_probe; ++probe) {
        const uint32_t off = (uint32_t)(s * a.krec_len);   // narrow only
        uint8_t *r;
        if constexpr (WIDE) r = a.krec + s * a.krec_len;
        else r = a.krec + off;
        if (probe) reload(off, r);
        uint64_t t = (uint64_t)rec_word<WIDE>(d, KOFF / 4) | ((uint64_t)rec_word<WIDE>(d, KOFF / 4 + 1) << 32);
        uint64_t ready = (uint64_t)rec_word<WIDE>(d, KOFF / 4 + 2) | ((uint64_t)rec_word<WIDE>(d, KOFF / 4 + 3) << 32);
        if ((t & EP_MAX) != a.ep) {   // empty in this interval (never claimed, or an older epoch's)
            if (gidx >= IDX_LIMIT) {   // an index column value that `ready` cannot carry
                atomicOr(a.err, 8u);
                return SLOT_OVF;
            }
            const uint64_t old = atomicCAS(reinterpret_cast<unsigned long long *>(r + KOFF),
                                           (unsigned long long)t, (unsigned long long)tag);
            if (old == t) {
                // key words as 16-byte write-through stores (each store is one memory-side write)
#pragma unroll
                for (int w = 0; w < KW; w += 4) {
                    if (w + 3 < KW) {
                        const u4v q = {k[w], k[w + 1], k[w + 2], k[w + 3]};
                        if constexpr (WIDE) wide_store_quad(r + 4 * w, q);
                        else __builtin_amdgcn_raw_buffer_store_b128(q, rs, off + 4 * w, 0, 16 /* sc1 */);
                    } else if (w + 1 < KW) {
                        st_agent(reinterpret_cast<uint64_t *>(r + 4 * w), (uint64_t)k[w] | ((uint64_t)k[w + 1] << 32));
                        if (w + 2 < KW) st_agent(reinterpret_cast<uint32_t *>(r + 4 * w + 8), k[w + 2]);
                    } else {
                        st_agent(reinterpret_cast<uint32_t *>(r + 4 * w), k[w]);
                    }
                }
                // the value record starts at first = first_ins and the claimer's own values
                // (no reset pass)
                vrec_init<NV>(a, s, gidx, vinit);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                st_agent(reinterpret_cast<uint64_t *>(r + KOFF + 8), (a.ep << 48) | (gidx + 1));
                if (SET_OCC) atomicOr(a.occ + (s >> 5), 1u << (s & 31));
                first_ins = gidx;
                claimed = true;
                return (uint32_t)s;
            }
            t = old;
            ready = 0;   // the claimer may still be writing the key
        }
        if (t == tag) {
            if (!ready_ok(ready, a.ep)) {
                uint32_t spins = 0;
                while (!ready_ok(ld_agent(reinterpret_cast<const uint64_t *>(r + KOFF + 8)), a.ep)) {
                    __builtin_amdgcn_s_sleep(1);
                    if (++spins > (1u << 22)) {
                        atomicOr(a.err, 2u);
                        return SLOT_OVF;
                    }
                }
                reload(off, r);
            }
            bool eq = true;
#pragma unroll
            for (int w = 0; w < KW; ++w) eq = eq && (rec_word<WIDE>(d, w) == k[w]);
            if (!eq) {
                // The quads of one snapshot are separate loads: `ready` may have been sampled
                // after the key quads, so a tag hit with a key mismatch is re-read once, now
                // ordered after the ready observation (genuine 64-bit tag collisions are rare).
                reload(off, r);
                eq = true;
#pragma unroll
                for (int w = 0; w < KW; ++w) eq = eq && (rec_word<WIDE>(d, w) == k[w]);
            }
            if (eq) {
                first_ins = (((uint64_t)rec_word<WIDE>(d, KOFF / 4 + 2) | ((uint64_t)rec_word<WIDE>(d, KOFF / 4 + 3) << 32)) & READY_IDX) - 1;
                return (uint32_t)s;
            }
        }
        s = next_slot(a, s);
    }
    atomicOr(a.err, 4u);
    return SLOT_OVF;
}

// ---- per-row pieces ------------------------------------------------------------------
// Every input dword of the row is loaded unconditionally first (unused predicate and
// aggregate slots point at a readable dummy column, set up by the host), and only then
// combined.  A load whose value is used inside a branch forces the wait into that branch,
// so each guarded column used to cost a memory round trip of its own; issued together
// they retire under one wait.
template <bool NT = true>
__device__ __forceinline__ uint32_t ldd(const uint8_t *base, uint64_t off) {
    return stream_ld<NT>(reinterpret_cast<const uint32_t *>(base + (off & ~3ull)));
}

// zero-extended value of `width` bytes from the aligned dwords lo (holding its first byte)
// and hi (the next dword; used for width 8 only)
__device__ __forceinline__ uint64_t assemble(uint32_t lo, uint32_t hi, uint64_t off, uint32_t width) {
    const uint32_t lomask = width >= 4 ? 0xFFFFFFFFu : ((1u << (8 * width)) - 1u);
    const uint32_t l = (lo >> ((uint32_t)(off & 3u) * 8u)) & lomask;
    return (uint64_t)l | ((uint64_t)(width == 8 ? hi : 0u) << 32);
}

// The raw dwords of one row: issued by issue_row, combined by decode_row.  The main loop
// issues row i+1 before it waits for row i's HBM probe, so the two round trips overlap.
// NA is the number of aggregate slots the kernel carries (2 or 4).
template <class L, int NA>
struct RowRaw {
    uint32_t k[L::KW];
    uint32_t vraw, plo[PMAX], phi[PMAX], vlo[NA], vhi[NA], clo[NA], chi[NA];
};

// ---- row plans -------------------------------------------------------------------------
// The row pieces below read an update's shape from GbArgs at run time: every column's width,
// sign, sharing, every predicate's kind and comparison.  A RowPlan fixes that shape at compile
// time for the plans shipped gadgets build ("Row plans"): an instance over a
// plan loads each distinct column once, at its own width, loads no dummy column, and evaluates
// values and predicates with constant widths, kinds and comparisons.  Of GbArgs it reads the
// column pointers, the reference values (pref, gref, cval) and the table fields; the reference
// *values* stay run-time.  RowPlanRT is the run-time shape: today's code, unchanged.
struct PlanAgg {
    bool count;              // COUNT (adds 1), else SUM of the value column
    uint8_t vwidth;          // value column bytes (SUM)
    bool vsign;              // value column is signed
    bool cond;               // adds only where the condition column holds cval
    uint8_t cwidth;          // condition column bytes
    int8_t vshare, cshare;   // the earlier aggregate whose value / condition load it reuses (-1: its own)
};
struct PlanPred {
    uint8_t width, kind, cmp;
    bool neg;
    uint8_t cnt;             // reference values of an IN set (else 0)
    int8_t share;            // the aggregate whose value load it reuses (-1: its own load)
    int8_t guard;            // the aggregate whose condition value guards it (-1: unguarded)
};
struct RowPlanDesc {
    int id;                  // what igx_groupby_rowplan reports (0 is the run-time shape)
    int naggs, npred;
    bool valid, index;       // a valid column / an index column is present
    PlanAgg agg[AMAX];
    PlanPred pred[PMAX];
};
struct RowPlanRT {
    static constexpr bool RT = true;
};
// gadgets.TopTcpTracer (and the headline benchmark): ip_key_t, sent / received = SUM(size) where
// dir == 0 / 1, family IN {..} (two 2-byte values), `int copied` (size's memory) > ref where dir == gref
struct TopTcpPlan {
    static constexpr bool RT = false;
    static constexpr RowPlanDesc D = {1, 2, 2, false, false,
                                      {{false, 4, false, true, 1, -1, -1}, {false, 4, false, true, 1, 0, 0}},
                                      {{2, IGX_KIND_UINT, IGX_CMP_IN, false, 2, -1, -1},
                                       {4, IGX_KIND_INT, IGX_CMP_GT, false, 0, 0, 0}}};
};
// gadgets.TopFileTracer(AllFiles=True): file_id, reads / rbytes / writes / wbytes = COUNT and
// SUM(count) where op == 0 / 1, no predicate
struct TopFilePlan {
    static constexpr bool RT = false;
    static constexpr RowPlanDesc D = {2, 4, 0, false, false,
                                      {{true, 0, false, true, 1, -1, -1}, {false, 4, false, true, 1, -1, 0},
                                       {true, 0, false, true, 1, -1, 0}, {false, 4, false, true, 1, 1, 0}},
                                      {}};
};

// f(std::integral_constant<int, i>) for i in [0, N): loops whose index is a constant expression
template <class F, size_t... I>
__device__ __forceinline__ void plan_each(F &f, std::index_sequence<I...>) {
    (f(std::integral_constant<int, (int)I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void plan_for(F &&f) {
    plan_each(f, std::make_index_sequence<N>{});
}

// a plan's column load: W (1, 2, 4 or 8) bytes of the row at their own width, zero-extended into
// lo (hi: the upper dword of an 8-byte column).  Columns are aligned to their width (plan_aggs,
// plan_preds), so no shift by the row's phase in a dword is needed.
template <int W, bool NT>
__device__ __forceinline__ void plan_ld(const uint8_t *p, uint64_t row, uint32_t &lo, uint32_t &hi) {
    static_assert(W == 1 || W == 2 || W == 4 || W == 8, "scalar column widths");
    if constexpr (W == 8) {
        typedef unsigned int v2u __attribute__((ext_vector_type(2)));
        const v2u q = stream_ld<NT>(reinterpret_cast<const v2u *>(p) + row);
        lo = q.x;
        hi = q.y;
    } else if constexpr (W == 4) {
        lo = stream_ld<NT>(reinterpret_cast<const uint32_t *>(p) + row);
    } else if constexpr (W == 2) {
        lo = stream_ld<NT>(reinterpret_cast<const uint16_t *>(p) + row);
    } else {
        lo = stream_ld<NT>(p + row);
    }
}
template <int W>
__device__ __forceinline__ uint64_t plan_val(uint32_t lo, uint32_t hi) {
    return (uint64_t)lo | (W == 8 ? (uint64_t)hi << 32 : 0ull);
}

template <class L, int NA, bool NT = true, class P = RowPlanRT>
__device__ __forceinline__ void issue_row(const GbArgs &a, uint64_t row, RowRaw<L, NA> &R) {
    if constexpr (!P::RT) {
        // the plan's distinct columns, each once (the slots it leaves alone are never read)
        static_assert(P::D.naggs <= NA && !P::D.valid && !P::D.index, "plan does not fit this instance");
        plan_for<PMAX>([&](auto I) __attribute__((always_inline)) {
            constexpr int p = decltype(I)::value;
            if constexpr (p < P::D.npred && P::D.pred[p].share < 0)
                plan_ld<P::D.pred[p].width, NT>(a.pptr[p], row, R.plo[p], R.phi[p]);
        });
        L::template load<NT>(a, row, R.k);
        plan_for<NA>([&](auto I) __attribute__((always_inline)) {
            constexpr int x = decltype(I)::value;
            if constexpr (x < P::D.naggs) {
                if constexpr (!P::D.agg[x].count && P::D.agg[x].vshare < 0)
                    plan_ld<P::D.agg[x].vwidth, NT>(a.vptr[x], row, R.vlo[x], R.vhi[x]);
                if constexpr (P::D.agg[x].cond && P::D.agg[x].cshare < 0)
                    plan_ld<P::D.agg[x].cwidth, NT>(a.cptr[x], row, R.clo[x], R.chi[x]);
            }
        });
    } else {
        // unconditional loads; slots with nothing to load read dword 0 of the dummy column
        // (width 0: one cached line for the whole wave)
        R.vraw = ldd<NT>(a.validp, row * a.validw);
#pragma unroll
        for (int p = 0; p < PMAX; ++p) {
            const uint64_t b = row * a.pldw[p];
            R.plo[p] = ldd<NT>(a.pptr[p], b);
            R.phi[p] = ldd<NT>(a.pptr[p], b + a.phioff[p]);
        }
        L::template load<NT>(a, row, R.k);
#pragma unroll
        for (int x = 0; x < NA; ++x) {
            const uint64_t bv = row * a.vldw[x], bc = row * a.cldw[x];
            R.vlo[x] = ldd<NT>(a.vptr[x], bv);
            R.vhi[x] = ldd<NT>(a.vptr[x], bv + a.vhioff[x]);
            R.clo[x] = ldd<NT>(a.cptr[x], bc);
            R.chi[x] = ldd<NT>(a.cptr[x], bc + a.chioff[x]);
        }
    }
}

// aggregates reading a column an earlier one already loaded reuse its value
template <int NA>
__device__ __forceinline__ void share_raw(const GbArgs &a, uint64_t (&rv)[NA], uint64_t (&rc)[NA]) {
#pragma unroll
    for (int x = 1; x < NA; ++x) {
#pragma unroll
        for (int y = 0; y < x; ++y) {
            if (a.vshare[x] == (uint32_t)y) rv[x] = rv[y];
            if (a.cshare[x] == (uint32_t)y) rc[x] = rc[y];
        }
    }
}

// the value each aggregate adds: 1 (COUNT) or the column's value (sign-extended, divided),
// 0 when its condition column does not hold cval
template <int NA, class P = RowPlanRT>
__device__ __forceinline__ void vals_from_raw(const GbArgs &a, const uint64_t (&rv)[NA], const uint64_t (&rc)[NA],
                                              uint64_t (&v)[NA]) {
    if constexpr (!P::RT) {   // a plan has no divisor
        plan_for<NA>([&](auto I) __attribute__((always_inline)) {
            constexpr int x = decltype(I)::value;
            uint64_t val = 0;
            if constexpr (x < P::D.naggs) {
                val = P::D.agg[x].count ? 1ull : (P::D.agg[x].vsign ? sext(rv[x], P::D.agg[x].vwidth) : rv[x]);
                if (P::D.agg[x].cond && rc[x] != a.cval[x]) val = 0;
            }
            v[x] = val;
        });
    } else {
#pragma unroll
        for (int x = 0; x < NA; ++x) {
            uint64_t val = 0;
            if (x < (int)a.naggs) {
                val = a.vcount[x] ? 1ull : (a.vsign[x] ? sext(rv[x], a.vwidth[x]) : rv[x]);
                if (a.vdiv[x]) val /= a.vdiv[x];
                if (a.hascond[x] && rc[x] != a.cval[x]) val = 0;
            }
            v[x] = val;
        }
    }
}

// A row's key words, whether it is kept (valid and predicates), and the zero-extended raw
// value / condition column values of its aggregates (an aggregate that shares another's
// column takes that one's value).  vals_from_raw turns them into the added values; the
// partitioned form stores the raw values of the loaded columns in its records.
template <class L, int NA, class P = RowPlanRT>
__device__ __forceinline__ bool row_raw(const GbArgs &a, uint64_t row, const RowRaw<L, NA> &R,
                                        uint32_t (&k)[L::KW], uint64_t (&rv)[NA], uint64_t (&rc)[NA]) {
#pragma unroll
    for (int w = 0; w < L::KW; ++w) k[w] = R.k[w];
    if constexpr (!P::RT) {
        plan_for<NA>([&](auto I) __attribute__((always_inline)) {
            constexpr int x = decltype(I)::value;
            rv[x] = rc[x] = 0;
            if constexpr (x < P::D.naggs) {
                constexpr PlanAgg g = P::D.agg[x];
                if constexpr (!g.count) rv[x] = g.vshare >= 0 ? rv[g.vshare < 0 ? 0 : g.vshare] : plan_val<g.vwidth>(R.vlo[x], R.vhi[x]);
                if constexpr (g.cond) rc[x] = g.cshare >= 0 ? rc[g.cshare < 0 ? 0 : g.cshare] : plan_val<g.cwidth>(R.clo[x], R.chi[x]);
            }
        });
        bool ok = true;
        plan_for<PMAX>([&](auto I) __attribute__((always_inline)) {
            constexpr int p = decltype(I)::value;
            if constexpr (p < P::D.npred) {
                constexpr PlanPred q = P::D.pred[p];
                const uint64_t pv = q.share >= 0 ? rv[q.share < 0 ? 0 : q.share] : plan_val<q.width>(R.plo[p], R.phi[p]);
                bool r = pred_scalar(pv, a.pref[p], q.width, q.kind, q.cmp, q.neg, q.cnt);
                if constexpr (q.guard >= 0) r = r || rc[q.guard] != a.gref[p];
                ok = ok && r;
            }
        });
        return ok;
    }
#pragma unroll
    for (int x = 0; x < NA; ++x) {
        rv[x] = assemble(R.vlo[x], R.vhi[x], row * a.vwidth[x], a.vwidth[x]);
        rc[x] = assemble(R.clo[x], R.chi[x], row * a.cwidth[x], a.cwidth[x]);
    }
    share_raw<NA>(a, rv, rc);
    bool ok = !a.valid || ((R.vraw >> ((uint32_t)(row & 3u) * 8u)) & 0xFFu) != 0;
#pragma unroll
    for (int p = 0; p < PMAX; ++p) {
        if (p < (int)a.npred) {
            uint64_t pv = assemble(R.plo[p], R.phi[p], row * a.pwidth[p], a.pwidth[p]);
#pragma unroll
            for (int x = 0; x < NA; ++x)
                if (a.pshare[p] == (uint32_t)x) pv = rv[x];
            bool r = pred_scalar(pv, a.pref[p], a.pwidth[p], a.pkind[p], a.pcmp[p], a.pneg[p], a.pcnt[p]);
#pragma unroll
            for (int x = 0; x < NA; ++x)
                if (a.pguard[p] == (uint32_t)x) r = r || rc[x] != a.gref[p];
            ok = ok && r;
        }
    }
    return ok;
}

template <class L, int NA, class P = RowPlanRT>
__device__ __forceinline__ bool decode_row(const GbArgs &a, uint64_t row, const RowRaw<L, NA> &R,
                                           uint32_t (&k)[L::KW], uint64_t (&v)[NA]) {
    uint64_t rv[NA], rc[NA];
    const bool ok = row_raw<L, NA, P>(a, row, R, k, rv, rc);
    vals_from_raw<NA, P>(a, rv, rc, v);
    return ok;
}

// ---- the plan registry (host) ------------------------------------------------------------
// A plan is registered when a shipped gadget builds it.  An update runs a plan's instance only
// when its GbArgs match the plan field by field: every aggregate's and predicate's shape, the
// natural packed strides (each column loaded at its own width), no divisor, no valid column and
// no index column.  Anything else runs the run-time shape.
inline bool plan_matches(const RowPlanDesc &d, const GbArgs &a) {
    if ((int)a.naggs != d.naggs || (int)a.npred != d.npred) return false;
    if ((a.valid != nullptr) != d.valid || (a.fidx != nullptr) != d.index) return false;
    for (int x = 0; x < d.naggs; ++x) {
        const PlanAgg &g = d.agg[x];
        if ((a.vcount[x] != 0) != g.count || (a.hascond[x] != 0) != g.cond || a.vdiv[x]) return false;
        if (!g.count) {
            if (a.vwidth[x] != g.vwidth || (a.vsign[x] != 0) != g.vsign) return false;
            if (a.vshare[x] != (g.vshare < 0 ? (uint32_t)AMAX : (uint32_t)g.vshare)) return false;
            if (a.vldw[x] != (g.vshare < 0 ? g.vwidth : 0u)) return false;
        }
        if (g.cond) {
            if (a.cwidth[x] != g.cwidth) return false;
            if (a.cshare[x] != (g.cshare < 0 ? (uint32_t)AMAX : (uint32_t)g.cshare)) return false;
            if (a.cldw[x] != (g.cshare < 0 ? g.cwidth : 0u)) return false;
        }
    }
    for (int p = 0; p < d.npred; ++p) {
        const PlanPred &q = d.pred[p];
        if (a.pwidth[p] != q.width || a.pkind[p] != q.kind || a.pcmp[p] != q.cmp || (a.pneg[p] != 0) != q.neg)
            return false;
        if (q.cmp == IGX_CMP_IN && a.pcnt[p] != q.cnt) return false;
        if (a.pshare[p] != (q.share < 0 ? (uint32_t)AMAX : (uint32_t)q.share)) return false;
        if (a.pldw[p] != (q.share < 0 ? q.width : 0u)) return false;
        if (a.pguard[p] != (q.guard < 0 ? (uint32_t)AMAX : (uint32_t)q.guard)) return false;
    }
    return true;
}
// the registered plan (its id) an update of key layout L with arguments a runs, 0: none
template <class L>
int plan_for_update(const GbArgs &a) {
    if constexpr (std::is_same<L, StaticLayout<16, 16, 8, 4, 16, 2, 2, 2>>::value)
        return plan_matches(TopTcpPlan::D, a) ? TopTcpPlan::D.id : 0;
    else if constexpr (std::is_same<L, StaticLayout<8, 4, 4, 4>>::value)
        return plan_matches(TopFilePlan::D, a) ? TopFilePlan::D.id : 0;
    else
        return 0;
}

__device__ __forceinline__ uint64_t row_gidx(const GbArgs &a, uint64_t row) {
    return a.fidx ? a.fidx[row] : a.base_idx + row;
}

// value-record words as global (address space 1) pointers, so their atomics are global_*
// instructions: a flat atomic also counts in lgkmcnt and stalls the next LDS wait
__device__ __forceinline__ unsigned long long *rec_first(const GbArgs &a, uint32_t gs) {
    return reinterpret_cast<unsigned long long *>(a.vrec + (uint64_t)gs * a.vrec_words);
}
__device__ __forceinline__ unsigned long long *rec_agg(const GbArgs &a, uint32_t gs, int x) {
    return reinterpret_cast<unsigned long long *>(a.vrec + (uint64_t)gs * a.vrec_words + 1 + x);
}
#if defined(__HIP_DEVICE_COMPILE__)
typedef __attribute__((address_space(1))) unsigned long long gu64;
__device__ __forceinline__ void gadd(unsigned long long *p, unsigned long long v) {
    __hip_atomic_fetch_add((gu64 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void gmin(unsigned long long *p, unsigned long long v) {
    __hip_atomic_fetch_min((gu64 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#else
__device__ inline void gadd(unsigned long long *, unsigned long long) {}   // host pass: never called
__device__ inline void gmin(unsigned long long *, unsigned long long) {}
#endif

// ---------------------------------------------------------------------------------------
// host side of the table
// ---------------------------------------------------------------------------------------
struct igx_table {
    igx_ctx *ctx = nullptr;
    uint32_t nkeys = 0;
    uint32_t key_widths[32] = {};
    uint32_t key_words = 0;      // packed words (each column padded to 4 B)
    uint32_t kw_rec = 0;         // key words as the kernel lays them out (static KW or generic width)
    uint32_t koff = 0, krec_len = 0, vrec_len = 0;
    bool generic = false;        // no compile-time layout (or IGX_GB_GENERIC at create)
    igx_agg aggs[AMAX] = {};
    uint32_t naggs = 0;
    uint64_t cap = 0;            // distinct keys promised by the caller
    uint64_t nslots = 0;
    bool wide = false;           // S x KR >= 4 GiB (or IGX_GB_WIDE=1): 64-bit record addressing, no cached form
    uint32_t sbits = 0;          // log2 nslots
    uint32_t rbits = 0;          // log2 probe-region slots (probing wraps inside a region)
    uint8_t *krec = nullptr;
    uint64_t *vrec = nullptr;
    uint32_t *err = nullptr;
    uint32_t *groups = nullptr;  // occupied slots after finalize
    uint32_t *tile_cnt = nullptr;
    uint32_t *occ = nullptr;     // occupancy bitmap (nslots bits)
    uint8_t *occb = nullptr;     // occupancy byte map (32 x occ_words bytes)
    bool occb_dirty = false;     // cached-form claims since the byte map was last folded / cleared
    uint64_t occ_words = 0;
    uint64_t ep = 0;             // current epoch (1..EP_MAX)
    bool persist = true;         // keys outlive their interval (IGX_GB_PERSIST=0: every reset starts a generation)
    bool fin_since_update = false;   // a finalize listed the groups after the last update
    bool fin_current = false;    // ... and no reset since: the slot list and the bitmap are the interval's
    bool gen_planned = false;    // the reset let the interval continue the generation (device decides by key count)
    bool seed_on = true;         // sample-seeded LDS cache for kept keys (IGX_GB_SEED=0: off)
    igx_table *seed_tab = nullptr;   // the row sample's counting table
    uint32_t *seeds = nullptr;   // seed records (device), nseeds of them
    uint32_t *seed_slots = nullptr;  // the sample table's top-E slots (device)
    uint64_t *seed_gep = nullptr;    // device: the generation the seeds were looked up in
    uint32_t nseeds = 0, seeds_cap = 0;
    uint32_t seed_left = 0;      // seeded intervals before the seeds are recomputed
    bool interval_seeded = false;    // this interval's cached updates adopt the seeds
    uint64_t claims_last = 0;    // the last collected finalize: keys its interval claimed
    uint64_t gen_keys = 0;       // ... and the keys its generation held after it (~0: ended)
    uint64_t *n_groups = nullptr;
    uint64_t rows_fed = 0;       // rows given to update since the last reset
    bool prefer_sm = false;      // the last interval missed the LDS cache on most rows
    bool more_probers = false;   // ... on more than MORE_PROBERS_ON_PM / 1000 of its rows (hysteresis below)
    uint32_t miss_pm = 0;        // LDS misses per 1000 rows of the last measured cached interval
    bool rowplan_on = true;      // cached updates of a registered shape run its plan's instance (IGX_GB_ROWPLAN=0: never)
    int rowplan_last = 0;        // the plan the last cached update ran (igx_groupby_rowplan; 0: the run-time shape)
    uint32_t mode = IGX_GB_AUTO; // igx_groupby_set_mode
    uint32_t direct_left = 0;    // AUTO: intervals to run in the direct form before re-measuring
    uint32_t region_off = 0;     // AUTO: intervals to partition exactly after a region overflowed
    bool interval_region = false;   // the interval ran the region variant
    bool interval_direct = false;// the current interval's updates run the direct form
    bool interval_part = false;  // ... the partitioned form
    // partitioned form scratch (grow-only)
    uint32_t *p_recs = nullptr;
    size_t p_recs_bytes = 0;
    uint32_t *p_cnt = nullptr;   // counts / offsets, then scan tile sums, then work items
    size_t p_cnt_bytes = 0;
    uint8_t *p_mask = nullptr;   // row mask of the predicates that are not fused (grow-only)
    size_t p_mask_bytes = 0;
    // update log scratch (k_gb_log.hip; first use, grow-only): the workgroups' log regions, the
    // bucket regions, and the counters (one per workgroup, then one per bucket)
    uint64_t *lg_recs = nullptr;
    size_t lg_recs_bytes = 0;
    uint64_t *lg_bk = nullptr;
    size_t lg_bk_bytes = 0;
    uint32_t *lg_cnt = nullptr;
    uint64_t log_last[4] = {};   // the last collected finalize's log counters (igx_groupby_log_stats)
    uint64_t host_groups = 0;
    uint64_t *fin_host = nullptr;   // pinned, coherent: error word, LDS misses, group count (finalize read-back)
    uint64_t *fin_dev = nullptr;    // the same buffer as the kernels address it
    uint64_t fin_seq = 0;           // the last finalize's number (fin_host[3] once it has landed)
    bool fin_pending = false;       // igx_groupby_finalize_async not yet collected
    int fin_status = 0;             // status of a collected asynchronous finalize, not yet returned
    uint64_t fin_status_seq = 0;    // ... and the finalize it belongs to
    // the finalized interval's own bookkeeping, taken when its finalize is issued: the read-back
    // may be collected after the next interval's reset and updates changed the live fields
    struct {
        uint64_t rows_fed;
        bool direct, part, region, probe;
        uint64_t sampled;   // probe: rows the estimator replayed
    } fin_snap{};
    bool interval_probe = false;   // AUTO: the last partitioned interval of a run (k_gb_estimate)
    uint64_t probe_rows = 0;       // ... the rows its estimator replayed
    unsigned long long *dbg_cnt = nullptr;
    // the last top-K's slots per sort (keys + k): the next same top-K's hint (TopkHint)
    struct TkHint {
        uint64_t sig = 0, used = 0;
        uint32_t *slots = nullptr;
        uint32_t nh = 0;
    } tk[4];
    uint32_t *tk_state = nullptr;
    uint64_t tk_clock = 0;
    uint8_t *text[32] = {};      // IP text of the groups, per IGX_TSRC_IPTEXT sort key
    uint64_t text_rows[32] = {};
};

// compile-time key layouts: the reference's BPF key structs + single-column keys
using TcpKey = StaticLayout<16, 16, 8, 4, 16, 2, 2, 2>;   // ip_key_t (tcptop.h:8-17)
using FileKey = StaticLayout<8, 4, 4, 4>;                 // file_id (filetop.h:13-18)
using NetPolicyKey = StaticLayout<4, 1, 4, 2>;            // (src, direction, peer, port)
using BioKey = StaticLayout<8, 4, 4, 4, 4, 16>;           // info_t (biotop.h:24-32)

template <class L>
static bool layout_is(const uint32_t *widths, uint32_t nkeys) {
    if constexpr (L::is_static) {
        if (nkeys != (uint32_t)L::NC) return false;
        for (int c = 0; c < L::NC; ++c)
            if ((int)widths[c] != L::Ws[c]) return false;
        return true;
    }
    return false;
}

// ---- the one list of key layouts -------------------------------------------------------
// Every kernel instance over a key layout comes from these two lists: a key description that
// matches a static layout column by column runs it, any other (or every one, under
// IGX_GB_GENERIC at create) the first generic layout that holds its packed words.  The record
// width chosen at create, every form's launch, the seeds, the estimate and the lookup kernel's
// KW all go through gb_with_layout, so a layout is added here and nowhere else.
template <class L>
struct GbLayoutTag {
    using type = L;
};
template <class... L>
struct GbLayouts {};
#ifdef IGX_DEV_FAST   // development builds: the bench's key layouts only (fast kernel iteration)
using GbStaticLayouts = GbLayouts<TcpKey, FileKey, NetPolicyKey>;
using GbGenericLayouts = GbLayouts<>;
#else
using GbStaticLayouts = GbLayouts<TcpKey, FileKey, NetPolicyKey, BioKey, StaticLayout<1>, StaticLayout<2>,
                                  StaticLayout<4>, StaticLayout<8>, StaticLayout<16>>;
using GbGenericLayouts = GbLayouts<GenericLayout<2>, GenericLayout<4>, GenericLayout<6>, GenericLayout<8>,
                                   GenericLayout<12>, GenericLayout<18>, GenericLayout<24>, GenericLayout<32>>;
#endif

template <class F, class... L>
static bool gb_visit_static(const igx_table *t, F &f, int &rc, GbLayouts<L...>) {
    return ((layout_is<L>(t->key_widths, t->nkeys) && ((rc = f(GbLayoutTag<L>{})), true)) || ...);
}
template <class F, class... L>
static bool gb_visit_generic(const igx_table *t, F &f, int &rc, GbLayouts<L...>) {
    return (((uint32_t)L::KW >= t->key_words && ((rc = f(GbLayoutTag<L>{})), true)) || ...);
}
// calls f(GbLayoutTag<L>{}) for the layout L of the table's key description (key_widths, nkeys,
// key_words, generic) and returns its status
template <class F>
static int gb_with_layout(const igx_table *t, F &&f) {
    int rc = IGX_OK;
    if ((!t->generic && gb_visit_static(t, f, rc, GbStaticLayouts{})) || gb_visit_generic(t, f, rc, GbGenericLayouts{}))
        return rc;
    return igx_fail(t->ctx, IGX_ENOTSUP, "groupby: no kernel for this key layout (%u key words) in this build",
                    t->key_words);
}

// a table's records, occupancy maps, epoch and probe geometry as the kernels read them
inline void bind_records(const igx_table *t, GbArgs &a) {
    a.krec = t->krec;
    a.vrec = t->vrec;
    a.krec_len = t->krec_len;
    a.krec_total = t->wide ? 0u : (uint32_t)(t->nslots * t->krec_len);
    a.vrec_words = t->vrec_len / 8;
    a.vrec_total = t->nslots * t->vrec_len < (1ull << 32) ? (uint32_t)(t->nslots * t->vrec_len) : 0u;
    a.err = t->err;
    a.occ = t->occ;
    a.occb = t->occb;
    a.ep = t->ep;
    a.gen = reinterpret_cast<uint64_t *>(t->err) + GEN_WORD;
    a.sshift = 64 - t->sbits;
    a.rmask = (1ull << t->rbits) - 1;
    a.max_probe = 1u << t->rbits;
    a.dbg_cnt = t->dbg_cnt;
}

// a grow-only device scratch buffer of the table (the row mask, the partitioned form's records)
inline int grow(igx_ctx *ctx, void **p, size_t *have, size_t need) {
    if (*have >= need) return IGX_OK;
    IGX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the old buffer may still be in use
    (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
    IGX_HIP(ctx, hipMalloc(p, need));
    *have = need;
    return IGX_OK;
}

// ---- the forms' host entry points --------------------------------------------------------
// One update's launches over the table's key layout; each dispatches over gb_with_layout in
// its own translation unit, so a change to one form recompiles that form.
// k_gb_cached.hip: the cached kernel, AUTO's estimate of its LDS-miss share over the first
// nsample rows, and the seeds of its LDS cache (IGX_ENOTSUP: a generic layout has none)
int gb_launch_cached(igx_table *t, GbArgs &a, uint32_t blocks);
int gb_launch_estimate(igx_table *t, const GbArgs &a, uint32_t blocks, uint64_t nsample);
int gb_seeds_compute(igx_table *t, const GbArgs &a);
// k_gb_log.hip: the update log of a cached update over `blocks` workgroups.  gb_log_prepare
// decides whether the update logs (0: it does not) and then allocates the scratch and points the
// arguments at it; gb_log_launch, after the cached kernel, runs the partition and reduce passes.
int gb_log_prepare(igx_table *t, GbArgs &a, uint32_t blocks);
int gb_log_launch(igx_table *t, const GbArgs &a, uint32_t blocks);
// k_gb_direct.hip
int gb_launch_direct(igx_table *t, GbArgs &a);
// k_gb_part.hip: passes K, O, S, A, B and the plan, then pass C (k_gb_part_c.hip)
int gb_launch_part(igx_table *t, GbArgs &a);
// The runtime loads a translation unit's code object at the first use of one of its kernels
// (tens of milliseconds for the partitioned form's).  igx_groupby_create asks for every form's, as
// when the group-by was one code object, so that no interval's first update in a form pays it.
void gb_cached_load();
void gb_direct_load();
void gb_part_load();
// k_groupby.hip: the read-back of an asynchronous finalize (the seeds' sample table collects its own)
int fin_collect(igx_table *t, uint64_t *n_groups);
