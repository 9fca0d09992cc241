// k_gb_part.h -- what the two translation units of the group-by's partitioned form share at file
// scope: the form's constants, PartArgs (it crosses from the plan in k_gb_part.hip to pass C's
// launch in k_gb_part_c.hip) and that launch's declaration.  The form itself is described, and its
// device code held, in k_groupby_part.h, which both units include in their anonymous namespace.
#pragma once

#include "k_gb_table.h"

constexpr uint32_t PTA = 256;                  // threads per block of passes K, A and B
constexpr uint32_t PTC = 512;                  // ... of the aggregate pass (two blocks per CU)
constexpr size_t PART_TILE_LDS = 72 * 1024;    // a B tile: records + 6 B each
constexpr size_t PART_AGG_LDS = 80 * 1024;     // the C block: LDS table + one round of records
constexpr uint32_t PART_LB_MAX = 15;           // final buckets <= 2^15 (count-pass LDS histogram)
constexpr uint32_t PART_F_MAX = 256;           // buckets per scatter level (one per thread)
constexpr uint32_t PNV = 2 * AMAX;             // distinct value / condition columns a record carries
constexpr uint32_t CHT = 64;                   // A tiles per chunk of the offset scan
constexpr uint32_t RC1_PAD = 16;               // words between two slice cursors of pass A
constexpr uint32_t PART_S1_LOG = 3;            // slices per first-level region (regions)
constexpr uint32_t PART_U1_MAX = PART_F_MAX << PART_S1_LOG;

struct PartArgs {
    uint32_t *recs1, *recs2;   // records after pass A / pass B (rq quads each)
    uint32_t *cnt1;            // tiles_a x F1: an A tile's rows per first-level bucket, then the
                               // exact output position of that run (pass O)
    uint32_t *csum;            // nchunk x F1: the same per chunk of CHT A tiles
    uint32_t *hist;            // NB: rows per final bucket (pass K)
    uint32_t *start2;          // NB + 1: first record of each final bucket (prefix of hist)
    uint32_t *cur2;            // NB: pass B's write cursors (final buckets)
    uint32_t *tstart;          // F1 + 1 (regions: U1 + 1): first B tile of each first-level bucket
                               // (regions: of each slice)
    uint32_t *bt;              // B tile -> first-level bucket
    uint32_t *istart;          // NB + 1: first C work item of each final bucket
    uint32_t *itfb;            // C work item -> final bucket
    uint32_t *ctl;             // [0] C work-item dequeue, [1] B tiles, [2] C work items
    // the row's value / condition columns, each loaded once (aggregates sharing a column
    // share it): pointer, width (0 = unused: dword 0 of a readable column) and high-dword
    // offset (4 for 8-byte columns)
    const uint8_t *vcol[PNV];
    uint32_t vcw[PNV], vchi[PNV];
    uint32_t rpos[PNV], rw2[PNV];      // record word of column j's raw value (+1 when 8 bytes)
    uint32_t nv;                       // loaded columns
    uint32_t vsrc[AMAX], csrc[AMAX];   // column of aggregate x's value / condition (PNV = none)
    uint32_t avp[AMAX], acp[AMAX];     // ... its record word (0xFFFF = none) ...
    uint32_t av2[AMAX], ac2[AMAX];     // ... and 1 when it is 8 bytes wide
    uint32_t tiles_a, nchunk;  // A tiles (PTA x rows-per-thread rows each), chunks of CHT tiles
    uint32_t trb;              // records per B tile
    uint32_t f1, f2, lb;       // bucket bits of the two levels, lb = f1 + f2
    uint32_t sb_log;           // log2 table slots per final bucket
    uint32_t occw;             // occupancy bitmap words per final bucket (slots / 32)
    uint32_t rq, rq_magic;     // record quads (16 B); ceil(2^32 / rq) for quad -> record
    uint32_t kpw[KWMAX];       // key word w lives in record word kpw[w] ...
    uint32_t ksh[KWMAX];       // ... at this bit shift (1- and 2-byte columns share words)
    uint32_t kmsk[KWMAX];      // ... with this mask (0 = a padding word)
    uint32_t kpn;              // packed key words
    uint32_t iw, ipos;         // index words (1 = row offset, 2 = global index column) and their word
    uint32_t ch;               // records per C work item (larger buckets are split)
    uint32_t E;                // LDS table entries
    uint32_t uc;               // records per thread and round of pass C
    uint32_t maxp;             // LDS probes before a row takes the HBM path
    uint32_t combine;          // wave pre-combine rounds per 64 records (0 = off)
    uint32_t dbg;              // diagnostics (IGX_GBP_DEBUG): phases to skip, results invalid
    // region variant (no count pass): bucket b's records fill a fixed region of reg records
    // through a cursor (one atomic per (tile, bucket)); a record past its region merges into
    // the table directly (find-or-insert + atomics: exact on any stream)
    // Pass A's cursors are the most contended words of the form (every A tile adds to each of
    // the F1): a first-level region is cut into 2^s1log slices, A tile t fills slice
    // t mod 2^s1log, and each slice's cursor has a 64-B line of its own (RC1_PAD words)
    uint32_t *rc1, *rc2;       // U1 = F1 << s1log slice cursors (stride RC1_PAD) / NB final-region
                               // cursors (records reserved; may pass the region)
    uint32_t reg1, reg2;       // records per first-level slice / final region (0: exact runs)
    uint32_t s1log;            // log2 slices per first-level region (0 in the exact form)
    uint32_t c2pad;            // words between two final-region cursors (rc2)
    uint32_t pe;               // pass C keeps 16-B packed entries (distinct-only, see c_row_pe)
};

// The record's loaded-column count class (0, <= 2, PNV) and the table's record addressing as
// compile-time tags: f(std::integral_constant<int, NV>{}, std::bool_constant<WIDE>{}).  Passes
// K, A, B and pass C are instantiated over the same (NV, WIDE) pairs through it.
template <class F>
int part_with_shape(uint32_t nv, bool wide, F &&f) {
    auto addr = [&](auto nvc) {
        return wide ? f(nvc, std::true_type{}) : f(nvc, std::false_type{});
    };
    if (nv == 0) return addr(std::integral_constant<int, 0>{});
    if (nv <= 2) return addr(std::integral_constant<int, 2>{});
    return addr(std::integral_constant<int, (int)PNV>{});
}

// k_gb_part_c.hip: pass C of one update over the plan p (lds_c bytes of dynamic LDS)
int gbp_launch_c(igx_table *t, const GbArgs &a, const PartArgs &p, size_t lds_c);
void gbp_c_load();   // its code object (gb_part_load calls it)
