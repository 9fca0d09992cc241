/*
 * igx.h -- C ABI of the MI355X-native Inspektor Gadget event-aggregation path.
 *
 * One shared library, libigx.so (HIP kernels for gfx950 + host C++), built in-tree at
 * inspektor-gadget_amd/libigx.so.  Plain pointers and sizes only; nothing here knows
 * about torch or Go types, so the reference's Go packages can bind it with cgo
 * (INTEGRATION.md shows the binding).
 *
 * Reference interfaces replaced (paths relative to the reference repository root):
 *   igx_filter_parse        filter.GetFilterFromString       pkg/columns/filter/filter.go:91-172
 *                           (+ getValueFromFilterSpec :53-87)
 *   igx_filter              filter.FilterEntries / FilterSpecs.MatchAll
 *                                                             pkg/columns/filter/filter.go:266-325
 *   igx_sort_prepare        sort.Prepare / FilterSortableColumns / CanSortBy
 *                                                             pkg/columns/sort/sort.go:87-111,139-178
 *   igx_sort_perm           ColumnSorterCollection.Sort / SortEntries
 *                                                             pkg/columns/sort/sort.go:35-83,116-123
 *   igx_topk                top.SortStats + stats[:MaxRows]  pkg/gadgets/top/top.go:39-41,
 *                                                             pkg/gadgets/top/tcp/tracer/tracer.go:249-253
 *   igx_groupby_*           BPF hash-map keyed aggregation + nextStats drain
 *                                                             pkg/gadgets/top/tcp/tracer/bpf/tcptop.bpf.c:33-110,
 *                                                             pkg/gadgets/top/tcp/tracer/tracer.go:147-226,
 *                                                             pkg/gadgets/top/file/tracer/bpf/filetop.bpf.c:39-94,
 *                                                             pkg/gadgets/top/block-io/tracer/bpf/biotop.bpf.c:85-130,
 *                                                             pkg/gadgets/trace/network/tracer/bpf/graph.c:102-114
 *                           and group.GroupEntries (one column per call)
 *                                                             pkg/columns/group/group.go:51-121
 *   igx_hist_log2           biolatency histogram              pkg/gadgets/profile/block-io/tracer/bpf/biolatency.bpf.c:100-154
 *                                                             pkg/gadgets/profile/block-io/tracer/bpf/bits.bpf.h:8-29
 *
 * Conventions
 *   - Return codes: IGX_OK (0) or a negative errno-style code.  The message of the last
 *     failure on a context is igx_last_error(ctx); host-only parsers write theirs into
 *     a caller buffer (the Go `error` text, e.g. `could not apply filter: column "x" not
 *     found`).
 *   - "device" pointers are HIP device allocations (igx_malloc or any HIP allocator);
 *     "host" pointers are plain memory.  Nothing is retained past the call except by
 *     igx_table objects, which own their device storage (cgo pointer rules).
 *   - Every device operation is enqueued on the context's stream (igx_set_stream to share
 *     a caller's stream) and is asynchronous unless documented as synchronising.
 */
#ifndef IGX_H
#define IGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGX_OK 0
#define IGX_ENOENT (-2)
#define IGX_EIO (-5)
#define IGX_ENOMEM (-12)
#define IGX_EINVAL (-22)
#define IGX_ENOSPC (-28)
#define IGX_ENOTSUP (-95)

/* Column kind classes (Go reflect kinds collapsed by arithmetic).  Strings are fixed-width
 * zero-padded byte columns: bytewise unsigned compare == Go string compare because
 * gadgets.FromCString never yields NUL (pkg/gadgets/helpers.go:76-83). */
enum igx_kind {
    IGX_KIND_INT = 0,   /* int, int8..int64 (two's complement, little-endian) */
    IGX_KIND_UINT = 1,  /* uint, uint8..uint64 */
    IGX_KIND_FLOAT = 2, /* float32 / float64 */
    IGX_KIND_BYTES = 3, /* string as fixed-width bytes */
    IGX_KIND_BOOL = 4,  /* bool: not filterable (filter.go:54-85), not sortable (sort.go:77-78) */
    IGX_KIND_OTHER = 5  /* struct and everything else */
};

enum igx_cmp { IGX_CMP_EQ = 0, IGX_CMP_REGEX = 1, IGX_CMP_LT = 2, IGX_CMP_LE = 3,
               IGX_CMP_GT = 4, IGX_CMP_GE = 5,
               /* group-by predicates only (a BPF probe's set test, e.g. tcptop.bpf.c:54
                * `family != AF_INET && family != AF_INET6` -> drop): the field equals one
                * of the ref_len / width values packed in ref (at most 8 bytes) */
               IGX_CMP_IN = 6 };

#define IGX_COL_VIRTUAL 1u   /* columns.AddColumn virtual column (columns.go:282-309) */
#define IGX_COL_EXTRACTOR 2u /* column with SetExtractor (columns.go:320-332) */
#define IGX_NO_COL 0xFFFFFFFFu
#define IGX_MAX_REF 256
#define IGX_MAX_KEY_BYTES 128

/* Schema entry: one column of the event struct T, as derived by columns.NewColumns. */
typedef struct {
    const char *name; /* column name; matched case-insensitively (columns.go:83-86) */
    uint32_t kind;    /* enum igx_kind */
    uint32_t width;   /* bytes per row in the SoA batch */
    uint32_t flags;   /* IGX_COL_* */
    uint32_t raw_kind;/* kind used for sorting extractor columns (sort.go:46-48) */
} igx_schema_col;

/* Device column: row i lives at ptr + i*width. */
typedef struct {
    const void *ptr;
    uint32_t width;
    uint32_t kind;
} igx_col;

/* One compiled filter (FilterSpec).  ref holds the reference value already converted to
 * the column type (reflect Convert truncation, filter.go:64,74). */
typedef struct {
    uint32_t col;     /* index into the schema / column array */
    uint32_t cmp;     /* enum igx_cmp */
    uint32_t negate;
    uint32_t ref_len; /* valid bytes in ref */
    uint8_t ref[IGX_MAX_REF];
    /* Group-by predicates only: a guard restricts the test to the rows whose guard column
     * (guard_col, an integer column of guard_len = 1/2/4/8 bytes) equals guard_ref; the other
     * rows pass.  A BPF program with one probe per event kind checks some fields on one kind
     * only, e.g. top tcp's receive probe drops `copied <= 0` (tcptop.bpf.c:124-130) while the
     * send probe has no such check (:112-116): {col = size as int32, GT 0, guard dir == 1}.
     * guard_len 0 = unguarded (what igx_filter_parse emits; igx_filter rejects guards). */
    uint32_t guard_col;
    uint32_t guard_len;
    uint8_t guard_ref[8];
} igx_pred;

/* One sort key as Prepare emits it, in sortBy order (first = highest priority). */
typedef struct {
    const void *ptr;  /* device column (igx_sort_perm) or unused (igx_sort_prepare) */
    uint32_t width;
    uint32_t kind;
    uint32_t desc;    /* 1 when the sortBy entry had the '-' prefix */
    uint32_t col;     /* schema index (igx_sort_prepare output) */
} igx_sortkey;

typedef struct igx_ctx igx_ctx;
typedef struct igx_table igx_table;

/* ---- context ------------------------------------------------------------------------ */
int igx_open(int device, uint32_t flags, igx_ctx **out);
int igx_close(igx_ctx *ctx);
const char *igx_last_error(igx_ctx *ctx);
/* Share a caller's hipStream_t (NULL = HIP's default/null stream, which is what torch's
 * default stream is).  Until the first call the context uses a stream of its own. */
int igx_set_stream(igx_ctx *ctx, void *hip_stream);
void *igx_get_stream(igx_ctx *ctx);
int igx_sync(igx_ctx *ctx);
int igx_malloc(igx_ctx *ctx, size_t bytes, void **out);
int igx_free(igx_ctx *ctx, void *p);
int igx_memcpy_h2d(igx_ctx *ctx, void *dst, const void *src, size_t bytes);   /* sync */
int igx_memcpy_d2h(igx_ctx *ctx, void *dst, const void *src, size_t bytes);   /* sync */
int igx_memcpy_d2d(igx_ctx *ctx, void *dst, const void *src, size_t bytes);   /* async */
int igx_version(void);

/* ---- filter (host parser + device scan) -------------------------------------------- */
/* GetFilterFromString: parses "col[:[!][~|>=|>|<=|<]value]".  Host only, no GPU needed.
 * Regex rules are returned with cmp=IGX_CMP_REGEX and value = the pattern; igx_filter
 * compiles and runs them (below).  errbuf receives the Go error text.  Numbers parse as
 * strconv does: ParseInt / ParseUint base 10 (a sign on int columns only), ParseFloat with hex
 * floats only when they carry a 'p' exponent ("0x1" is rejected) and a sign on inf / infinity
 * but not on nan ("+nan" is rejected).  A string column may be wider than IGX_MAX_REF: the
 * reference then reads as zero bytes past IGX_MAX_REF. */
int igx_filter_parse(const igx_schema_col *cols, uint32_t ncols, const char *filter,
                     igx_pred *out, char *errbuf, size_t errlen);

/* Regex rules (IGX_CMP_REGEX, on string columns) run on the device: the pattern is compiled
 * on the host to a DFA over rune classes with Go regexp semantics (RE2 syntax incl. \b \B
 * \A \z, (?m) (?i) (?s), \p{..} general categories and scripts of Unicode 13.0.0, POSIX
 * classes; UTF-8 decoded like utf8.DecodeRune; unanchored MatchString).  A pattern whose
 * automaton would exceed the device limits (255 rune classes, 2048 states) returns
 * IGX_ENOTSUP.  igx_regex_compile_blob exposes the compiled automaton (for tests and tools). */
int igx_regex_compile_blob(const char *pattern, size_t len, uint8_t *out, size_t cap,
                           size_t *out_len, char *errbuf, size_t errlen);

/* FilterEntries' per-filter pass (filter.go:301-322): AND of preds (any number) over rows
 * [0,nrows), order-preserving.  valid (device, nullable): 0 marks a nil entry, which is
 * skipped (:310-314).  out_idx (device) receives the selected row ids; *out_n (device u64)
 * their count.  Asynchronous. */
int igx_filter(igx_ctx *ctx, const igx_col *cols, uint32_t ncols, const igx_pred *preds,
               uint32_t npreds, const uint8_t *valid, uint64_t nrows, uint32_t *out_idx,
               uint64_t *out_n);
/* FilterSpecs.MatchAny (filter.go:276-283): OR of preds (any number); zero preds select
 * nothing; a nil row matches iff some pred is negated (Match(nil) == negate, :286-291).
 * Outputs as igx_filter.  Asynchronous. */
int igx_filter_any(igx_ctx *ctx, const igx_col *cols, uint32_t ncols, const igx_pred *preds,
                   uint32_t npreds, const uint8_t *valid, uint64_t nrows, uint32_t *out_idx,
                   uint64_t *out_n);
/* The general form.  flags:
 *   IGX_FILTER_ANY        OR of preds (MatchAny) instead of AND (MatchAll);
 *   IGX_FILTER_NIL_MATCH  a nil row yields Match(nil) == negate for every pred (filter.go:
 *                         286-291), combined like the other rows: FilterSpecs.MatchAll keeps a
 *                         nil row iff every pred is negated (or there are none), MatchAny iff
 *                         one is -- what parser.eventHandlerArray relies on (parser.go:209-218).
 *                         Without it nil rows are skipped (FilterEntries).
 * igx_filter == flags 0; igx_filter_any == IGX_FILTER_ANY | IGX_FILTER_NIL_MATCH. */
#define IGX_FILTER_ANY 1u
#define IGX_FILTER_NIL_MATCH 2u
int igx_filter_ex(igx_ctx *ctx, const igx_col *cols, uint32_t ncols, const igx_pred *preds,
                  uint32_t npreds, const uint8_t *valid, uint64_t nrows, uint32_t flags,
                  uint32_t *out_idx, uint64_t *out_n);
/* The compacted batch FilterEntries returns (filter.go:294-325 builds a fresh slice of the
 * selected entries): rows idx[0..k) (device u32, e.g. igx_filter's out_idx) of every column
 * gathered into out[c] (device, k * cols[c].width bytes, rows packed).  Indices >= nrows
 * yield zero rows.  Asynchronous. */
int igx_take(igx_ctx *ctx, const igx_col *cols, uint32_t ncols, uint64_t nrows,
             const uint32_t *idx, uint64_t k, void *const *out);

/* ---- sort / top-K -------------------------------------------------------------------- */
/* Prepare + FilterSortableColumns: keeps valid keys in sortBy order (unknown, empty and
 * virtual columns dropped).  *out_n = number of valid keys; *out_invalid = dropped ones.
 * Bool / unsupported kinds stay in the list (the Go code skips them at Sort time,
 * sort.go:77-78) and are skipped by igx_sort_perm.  Host only. */
int igx_sort_prepare(const igx_schema_col *cols, uint32_t ncols, const char *const *sort_by,
                     uint32_t n, igx_sortkey *out, uint32_t *out_n, uint32_t *out_invalid);

/* Sort permutation with the exact tie order of Go 1.19 sort.SliceStable under
 * getLessFunc (SURVEY.md §0.3 closed form).  pos (device u64, nullable): pre-sort position
 * of each row (NULL = row index).  valid (device, nullable): nil rows sort last.
 * Float keys compare as Go's `<` does: -0 == +0, -Inf < finite < +Inf; a NaN in a float key
 * of a non-nil row makes the comparison unordered (no strict weak order, so SliceStable's
 * output depends on its merge steps) and the call returns IGX_ENOTSUP.
 * out_perm (device u32, nrows).  Synchronises once: the digit plan's read-back (which bytes of
 * the composed key vary, the NaN flag, a device row count); IGX_SORT_DEVPLAN=1 plans full sorts
 * of at most 8 composed words without float keys on the device instead (no read-back; slower
 * at 1M rows).  String keys of 5..32 bytes in full sorts of >= 65 536 rows sort
 * by their rank in a dictionary of their distinct values (at most 4 096; 2 048 for 32 bytes),
 * built on the device -- the same order, a few radix passes instead of one per live byte;
 * more distinct values: the raw bytes, after one more read-back.  IGX_SORT_DICT=0 turns the
 * dictionaries off. */
int igx_sort_perm(igx_ctx *ctx, const igx_sortkey *keys, uint32_t nkeys, uint64_t nrows,
                  const uint64_t *pos, const uint8_t *valid, uint32_t *out_perm);

/* igx_sort_perm over a selection vector: row i of the slice is row rowmap[i] (device u32) of
 * the key columns -- FilterEntries' result is a slice of pointers into the caller's entries
 * (filter.go:294-325), and SortEntries sorts that slice (sort.go:116-123) without moving the
 * entries.  pos (nullable: slice index) and valid (nullable) are read at rowmap[i].  out_perm
 * receives the rowmap values (base rows) in sorted order: the sorted slice.  rowmap NULL ==
 * igx_sort_perm. */
int igx_sort_perm_ex(igx_ctx *ctx, const igx_sortkey *keys, uint32_t nkeys, uint64_t nrows,
                     const uint64_t *pos, const uint8_t *valid, const uint32_t *rowmap, uint32_t *out_perm);

/* igx_sort_perm_ex when the row count lives on the device: the slice is rows [0, *d_nrows) of
 * the selection vector, nrows_max its upper bound (d_nrows: device u64, e.g. igx_filter's
 * out_n) -- FilterEntries' count feeds SortEntries without a read-back of its own: it rides
 * the digit plan's read-back (none with IGX_SORT_DEVPLAN=1).  No float key (a NaN would need
 * the host's decision before the count is known), and a top-K needs a slot list and no nil
 * mask: otherwise IGX_EINVAL.  out_perm (device u32, nrows_max) holds the sorted rowmap values
 * in its first *d_nrows entries. */
int igx_sort_perm_dn(igx_ctx *ctx, const igx_sortkey *keys, uint32_t nkeys, uint64_t nrows_max,
                     const uint64_t *d_nrows, const uint64_t *pos, const uint8_t *valid, const uint32_t *rowmap,
                     uint32_t *out_perm);

/* First k rows of the igx_sort_perm order (SortStats + truncate to max-rows).
 * out_idx (device u32, k).  Asynchronous. */
int igx_topk(igx_ctx *ctx, const igx_sortkey *keys, uint32_t nkeys, uint64_t nrows,
             const uint64_t *pos, uint32_t k, uint32_t *out_idx);

/* ---- keyed aggregation (group-by) ------------------------------------------------------ */
enum igx_agg_kind { IGX_AGG_COUNT = 0, IGX_AGG_SUM = 1 };

typedef struct {
    uint32_t kind;      /* enum igx_agg_kind */
    uint32_t col;       /* value column index (SUM) */
    uint32_t cond_col;  /* IGX_NO_COL or column whose value must equal cond_val */
    uint32_t out_width; /* result wraps to this many bytes (1,2,4,8) */
    uint64_t cond_val;
    uint64_t divisor;   /* SUM of an unsigned column: add value / divisor per event (0, 1 =
                         * plain sum), e.g. biotop's `us += delta_ns / 1000`
                         * (pkg/gadgets/top/block-io/tracer/bpf/biotop.bpf.c:98,119) */
} igx_agg;

/* The table is an open-addressing array of n_slots slots; a group's id is its slot.
 * Slot s has a key record at keys + s*key_stride (the packed key) and a value record at
 * first_idx + s*val_stride bytes (u64 first-occurrence index, then the u64 aggregates;
 * aggs[a] points at slot 0's aggregate a).  Aggregates are kept as u64 sums; they wrap to
 * their out_width when read (the low out_width bytes, little-endian).  groups[0..n_groups)
 * lists the occupied slots in ascending slot order (the canonical pre-sort order is
 * first_idx, not this). */
typedef struct {
    uint64_t n_groups;        /* host copy, valid after igx_groupby_finalize */
    uint64_t n_slots;
    uint32_t key_bytes;       /* packed key bytes per group (each key column padded to 4) */
    uint32_t key_stride;      /* key record size: bytes between consecutive slots' keys */
    uint32_t val_stride;      /* value record size: bytes between consecutive slots' values */
    uint32_t naggs;
    const uint8_t *keys;      /* device: slot 0's packed key */
    const uint64_t *aggs[16]; /* device: slot 0's aggregate a; stride val_stride */
    const uint64_t *first_idx;/* device: slot 0's first-occurrence index; stride val_stride */
    const uint32_t *groups;   /* device: occupied slots, n_groups entries */
    const uint64_t *d_n_groups;/* device: group count */
} igx_table_view;

/* Sort key over a table's columns (igx_groupby_sort). */
/* IGX_TSRC_CONST: a column that holds the same value for every group (e.g. the
 * CommonData enrichment strings when nothing enriches).  Go still runs a SliceStable pass
 * for it, so it orders nothing but its '-' flips the tie parity. */
/* IGX_TSRC_IPTEXT: the text of a 16-byte address in the key (offset) under the u16 family
 * in the key (index = its byte offset), as IPStringFromBytes renders it (helpers.go:111-120,
 * top/tcp/tracer/tracer.go:199-206): the Saddr / Daddr string columns of the Stats rows. */
enum igx_tsrc { IGX_TSRC_AGG = 0, IGX_TSRC_FIRST = 1, IGX_TSRC_KEY = 2, IGX_TSRC_CONST = 3, IGX_TSRC_IPTEXT = 4 };
typedef struct {
    uint32_t src;    /* enum igx_tsrc */
    uint32_t index;  /* aggregate index (IGX_TSRC_AGG); family byte offset (IGX_TSRC_IPTEXT) */
    uint32_t offset; /* byte offset in the packed key (IGX_TSRC_KEY, IGX_TSRC_IPTEXT) */
    uint32_t width;  /* bytes (IGX_TSRC_KEY) */
    uint32_t kind;   /* enum igx_kind (IGX_TSRC_KEY) */
    uint32_t desc;   /* '-' prefix */
} igx_tsortkey;

/* capacity = maximum number of distinct groups (at most 2^28, the only limit on it).
 * key_widths: byte width of each key column, any width (packed, each padded to a multiple of 4;
 * at most IGX_MAX_KEY_BYTES padded bytes in all).
 * Memory: S slots, S the power of two >= 2 x capacity (>= 1024).  A slot takes a key record
 * (igx_table_view.key_stride: 32..256 B, the padded key + 16 B rounded up to a power of two --
 * 128 B for the 72-B ip_key_t, 64 B for top file's key), a value record (val_stride: 8 + 8 x
 * naggs B rounded up to a power of two) and 5 1/8 B of slot list and occupancy maps; the
 * partitioned form adds scratch per update (igx_groupby_set_mode).  Device memory that cannot
 * be had is IGX_ENOMEM and nothing stays allocated.
 * A table whose key records reach 4 GiB (S x key_stride >= 2^32) is *wide*.  Up to there
 * (8.39M ip_key_t groups, 4.19M groups of a 128-byte key, 16.7M of top file's) a table is
 * narrow and runs as it always did.  A wide table addresses its key records with per-lane
 * 64-bit addresses in place of one buffer descriptor; it runs the direct and the partitioned
 * form, and IGX_GB_AUTO plans every interval of it partitioned (such a table is the
 * high-cardinality case that form is for; no interval is measured in the cached form, so keys
 * are not kept across its intervals either).  The cached form is not offered on a wide table
 * yet (igx_groupby_set_mode).  Everything that reads a table -- finalize, sort, gather,
 * select_ge, lookup, igx_partition_groups -- works on both kinds alike, and results are
 * identical.  IGX_GB_WIDE=1 in the environment at create gives a narrow-sized table the wide
 * kernels (A/B measurements and tests). */
int igx_groupby_create(igx_ctx *ctx, const uint32_t *key_widths, uint32_t nkeys,
                       const igx_agg *aggs, uint32_t naggs, uint64_t capacity,
                       igx_table **out);
/* Aggregate rows [0,nrows) of cols into the table; key_cols selects the key columns
 * (in the table's key order); preds are AND-ed filters applied first (the BPF probe
 * checks): any number, of any kind igx_filter takes plus IGX_CMP_IN sets (up to two scalar
 * comparisons / sets are fused into the aggregation kernel, the others -- regex, string
 * rules, more comparisons -- first become a device row mask).  An IGX_CMP_IN set is only ever
 * evaluated in the aggregation kernel: more than two of them in one update return
 * IGX_ENOTSUP, and so does a guarded set whose guard column is not the cond_col of one of the
 * table's aggregates (a guard on any other column is evaluated by the row mask, which has no
 * set test); a set on a float or string column, or with ref_len not a multiple of the column
 * width, returns IGX_EINVAL.
 * Alignment (IGX_EINVAL otherwise): a key column of 1 or 2 bytes is aligned to its width, one
 * of 4, 8 or 12 bytes to 4, a wider multiple of 4 to 16; other widths take any address.  Every other scalar column the update reads -- aggregate value and
 * condition columns, predicate columns of a non-string kind, guard columns -- and `valid` are
 * read as the aligned 4-byte words that hold each row, counted from the column's base, so
 * the base must be 4-byte aligned (8-byte aligned for an 8-byte column): a 1- or 2-byte
 * column that starts at an odd row of a larger buffer is rejected with IGX_EINVAL (its words
 * would be misaligned and would run up to three bytes past its last row); copy such a slice
 * first.  The bytes up to the next 4-byte boundary after a column's last row are read and must
 * be readable, which holds for any HIP allocation.  String predicate columns take any address.
 * base_idx is the global index of row 0 (first-occurrence order).  Event indices must stay
 * below 2^48 - 2 on every path: the table stores an index in 48 bits next to the interval's
 * epoch, a new key's as index + 1 and a kept key's (igx_groupby_reset's generations) as
 * index + 2, and the one limit is the smaller of the two, so a key accepts and rejects the same
 * values whether the interval inserts it or finds it kept.  A row index that would reach the
 * limit (base_idx + nrows - 1 >= 2^48 - 2) returns IGX_EINVAL and nothing is issued; an index
 * column value (igx_groupby_update_ex) at or above it fails the interval with IGX_ENOSPC at
 * finalize -- in the cached form on any row, in the direct and partitioned forms where it would
 * become a group's stored index -- and the next interval is unaffected.  Long-running streams
 * rebase their indices per interval.  Async. */
int igx_groupby_update(igx_table *t, const igx_col *cols, uint32_t ncols,
                       const uint32_t *key_cols, const igx_pred *preds, uint32_t npreds,
                       uint64_t nrows, uint64_t base_idx);
/* igx_groupby_update with two more inputs (either may be absent):
 *   valid   (device u8, nullable): rows with 0 are skipped -- nil entries, or a mask from
 *           igx_np_mark;
 *   idx_col (IGX_NO_COL = row index + base_idx): a u64 column giving each row's global
 *           event index.  Used to merge partial groups from other shards: key columns +
 *           one u64 column per partial aggregate (summed by SUM aggregates) + their first
 *           index, so first = min over shards (SURVEY.md §8(e) group-by exchange). */
int igx_groupby_update_ex(igx_table *t, const igx_col *cols, uint32_t ncols,
                          const uint32_t *key_cols, const igx_pred *preds, uint32_t npreds,
                          const uint8_t *valid, uint32_t idx_col, uint64_t nrows,
                          uint64_t base_idx);
/* Synchronises; fills the view; IGX_ENOSPC if capacity was exceeded. */
int igx_groupby_finalize(igx_table *t, igx_table_view *view);
/* Diagnostics: the form the current interval runs in and AUTO's plan for the next ones. */
typedef struct {
    uint32_t form;       /* IGX_GB_CACHED / IGX_GB_DIRECT / IGX_GB_PART (0 before the interval's first update) */
    uint32_t region;     /* 1: the interval's partitioned updates run the region variant */
    uint32_t part_left;  /* AUTO: intervals still planned in the partitioned form */
    uint32_t exact_left; /* AUTO: intervals partitioned exactly after a region overflowed */
    uint32_t sm_probers; /* the cached form's probers: 1 state machine, 0 batch */
    uint32_t loaders;    /* the cached form's loader waves for the next update (8, or 7 after intervals
                            that missed the LDS cache on > 39 % of their rows, until one falls below 37 %) */
    uint64_t rows;       /* rows fed to the interval so far */
    uint32_t miss_permille;  /* LDS misses per 1000 rows of the last measured cached interval */
    uint32_t persist;    /* 1: keys are kept across intervals (a generation; igx_groupby_reset) */
    uint64_t claims;     /* the last collected finalize: keys its interval inserted (the others were kept) */
    uint64_t gen_keys;   /* ... keys the table's generation held after it (UINT64_MAX: it ended) */
} igx_groupby_info_t;
int igx_groupby_info(igx_table *t, igx_groupby_info_t *out);
/* The update log: a cached update of a table that is not wide, has 1-4 aggregates
 * and at most 128 MiB of (slot, aggregate) sums streams the sums of the rows that miss the LDS
 * cache to a log and adds them per slot bucket in LDS, instead of one atomic each.  Counters of
 * the last collected finalize's interval (they ride its read-back): records logged, and updates
 * that went out as atomics instead because their value was 2^32 or more, their workgroup's log
 * region was full, or their bucket's region was full.  All 0: the interval did not log. */
typedef struct {
    uint64_t logged;
    uint64_t fallback_value;
    uint64_t fallback_log_full;
    uint64_t fallback_bucket_full;
} igx_groupby_log_stats_t;
int igx_groupby_log_stats(igx_table *t, igx_groupby_log_stats_t *out);
/* Row plans: a cached update whose shape -- key layout, aggregates, fused
 * predicates, no valid mask, no index column, no divisor -- is exactly the one a shipped gadget
 * builds runs a kernel instance compiled for that shape; any other update, and every update under
 * IGX_GB_ROWPLAN=0, runs the general kernel.  Results are identical.
 * igx_groupby_rowplan: the plan the table's last cached update ran: 0 general, 1 top tcp, 2 top file.
 * igx_groupby_rowplan_match: the plan an update described as for igx_groupby_create and
 * igx_groupby_update_ex would run, 0 when none (or the description is invalid).  Host only: no
 * context, no device; column pointers are compared, never read. */
int igx_groupby_rowplan(igx_table *t);
int igx_groupby_rowplan_match(const uint32_t *key_widths, uint32_t nkeys, const igx_agg *aggs,
                              uint32_t naggs, const igx_col *cols, uint32_t ncols,
                              const uint32_t *key_cols, const igx_pred *preds, uint32_t npreds,
                              const uint8_t *valid, uint32_t idx_col);
/* igx_groupby_finalize without its host synchronisation: the occupied-slot list is built on
 * the device and the group count stays there (view->d_n_groups; view->n_groups is 0 until
 * igx_groupby_wait).  igx_groupby_sort's top-K of such a table (0 < k <= 4096, no float or
 * IP-text key) reads the count on the device, so a whole interval -- reset, update,
 * finalize, sort, gather -- is issued without a host round trip (nextStats' drain,
 * tracer.go:177-226, with no wait in it).  The count and the status igx_groupby_finalize
 * would have returned (IGX_ENOSPC) come back from igx_groupby_wait, or from the first
 * igx_groupby_reset / igx_groupby_finalize that finds the read-back landed (a reset never
 * waits for the device), or, when the next interval's igx_groupby_finalize_async collects it,
 * from that call, which then does NOT issue its own interval (the error text names the failed
 * finalize; calling it again finalizes this interval: a non-zero return always means "not
 * finalized") -- igx_groupby_wait only ever reports the last finalize's own status.  The
 * read-back is written by the kernel that counts the groups into
 * the table's coherent pinned buffer, followed by a sequence number the host polls (no copy
 * and no event on the stream); igx_groupby_wait polls it, and fails with IGX_EIO if the
 * stream drains without it.  Asynchronous. */
int igx_groupby_finalize_async(igx_table *t, igx_table_view *view);
/* Waits for the last igx_groupby_finalize_async: *n_groups (nullable) = its group count;
 * returns its status.  IGX_OK (and the last known count) when none is pending. */
int igx_groupby_wait(igx_table *t, uint64_t *n_groups);
/* Materialise groups idx[0..k) (device u32, e.g. igx_topk output) as packed rows of
 * key_bytes | naggs x u64 | first_idx u64 into out_rows (device) -- the Stats rows
 * nextStats builds (pkg/gadgets/top/tcp/tracer/tracer.go:186-219).  Call after
 * igx_groupby_finalize.  Asynchronous. */
int igx_groupby_gather(igx_table *t, const uint32_t *idx, uint64_t k, uint8_t *out_rows);
/* The two table steps of the cross-rank threshold top-K.  Both follow
 * igx_groupby_finalize or _async of the interval (IGX_EINVAL after a later update or reset),
 * read the table only, and are asynchronous.
 * igx_groupby_select_ge: the interval's group slots whose aggregate `agg`, wrapped to its
 * out_width as igx_groupby_gather wraps it, is >= threshold, in no particular order.  The group
 * count is read on the device.  *d_count (device u64) receives how many qualify; the first cap
 * of them go to out_slots (device u32, cap entries; nothing past cap is written, and d_count may
 * exceed cap: the list is then incomplete). */
int igx_groupby_select_ge(igx_table *t, uint32_t agg, uint64_t threshold, uint32_t *out_slots,
                          uint64_t cap, uint64_t *d_count);
/* igx_groupby_lookup: keys (device, 4-byte aligned) holds n packed keys in the table's key
 * layout (key_bytes, each column padded to 4 with zeros), key_stride bytes apart (a multiple of
 * 4) -- rows of igx_groupby_gather can be passed as they are.  For a key that is a group of the
 * finalized interval, out_rows[i] (device, n rows of igx_groupby_gather's layout, not
 * overlapping keys) is the row igx_groupby_gather gives for its slot and found[i] (device u8)
 * is 1; for any other key -- never inserted, or kept in the table from an earlier interval of
 * the generation without an event in this one (igx_groupby_reset) -- the row is zero and
 * found[i] is 0.  Duplicate keys are allowed.  A read-only probe of at most the table's probe
 * region per key, in every form (cached, direct, partitioned). */
int igx_groupby_lookup(igx_table *t, const uint8_t *keys, uint32_t key_stride, uint64_t n,
                       uint8_t *out_rows, uint8_t *found);
/* Per-interval reset (nextStats' Delete loop, tracer.go:154-171): the next interval's groups,
 * sums and first indices are its own.  Keys themselves are kept across intervals while the
 * table runs its cached form: a recurring key is found instead of inserted again, and only the
 * last interval's groups' value records are cleared.  The kept keys end (the next interval
 * starts an empty table) when they plus `capacity` new ones would fill more than 4/5 of the
 * slots, after a failed interval, when an interval runs the direct or partitioned form, or
 * with IGX_GB_PERSIST=0.  Asynchronous. */
int igx_groupby_reset(igx_table *t);
/* How updates run (results are identical in every mode):
 *   IGX_GB_CACHED  one workgroup per CU with an LDS cache of hot keys (Zipf-like streams:
 *                  most rows never leave the CU);
 *   IGX_GB_DIRECT  every row probes the HBM table itself (near-uniform, high-cardinality
 *                  streams, where nearly every row would miss the cache);
 *   IGX_GB_PART    rows are radix-partitioned by key hash in two streamed passes and each
 *                  final bucket is aggregated in LDS, then written to the table with plain
 *                  stores (no atomics; DESIGN.md §4 has its measured cost).  Scratch: two
 *                  record buffers of nrows x 16..128 B;
 *   IGX_GB_AUTO    (default) cached; an interval in which more than 90% of the rows missed
 *                  the cache switches the next 16 intervals to partitioned, then measures
 *                  again.
 * The mode of an interval is fixed by its first update.
 * On a wide table (igx_groupby_create) IGX_GB_AUTO runs every interval partitioned, and
 * IGX_GB_CACHED is refused: IGX_ENOTSUP, the message says why, the table keeps its mode and
 * goes on working (nor do IGX_GB_MODE=1 or IGX_GB_DEBUG force it).  The cached kernel's probers
 * address key records through a buffer descriptor; a wide prober within its register budget is
 * the follow-up. */
enum igx_gb_mode { IGX_GB_AUTO = 0, IGX_GB_CACHED = 1, IGX_GB_DIRECT = 2, IGX_GB_PART = 3 };
int igx_groupby_set_mode(igx_table *t, uint32_t mode);
/* SortStats over the table's groups (same order as igx_sort_perm with pos = first_idx);
 * writes the first k (0 = all) group slots to out_slots (device u32).  Call after
 * igx_groupby_finalize.  Asynchronous. */
int igx_groupby_sort(igx_table *t, const igx_tsortkey *keys, uint32_t nkeys, uint32_t k,
                     uint32_t *out_slots);
/* Diagnostics (synchronous): out2[0] = top-Ks of this table answered by the hinted path (the
 * slots of the same sort's last top-K bound the k-th key; only the groups at or below the bound
 * are ranked), out2[1] = top-Ks answered by the full selection.  Both give the same slots. */
int igx_groupby_topk_counts(igx_table *t, uint64_t *out2);
int igx_groupby_destroy(igx_table *t);
/* Diagnostics only (IGX_GB_DEBUG env), 32 words: out[0..1] LDS-cache hits / misses, out[2] the
 * misses that found their set closed (bit 3);
 * out[4..7] sleep counts of loaders on a full miss ring, probers on an empty one, probers on a
 * full update ring, the idle server (bit 16); bit 18, the memory-side atomics: out[8..11] the
 * server wave's updates, of them minima, distinct (value record, opcode) pairs per instruction,
 * distinct (128-B line, opcode) pairs; [12] instructions whose first record continues the
 * previous one's last; [13..15] the distinct (record, opcode) pairs within each 32-, 16- and
 * 8-lane group of the instruction; [16..19] the same four as [8..11] for the final LDS flush's
 * aggregate updates, [20] its minima.  Counters since the last call. */
int igx_groupby_debug_counts(igx_table *t, uint64_t *out32);

/* ---- advise network-policy -------------------------------------------------------------- */
/* keep[i] = 1 iff the advisor would consider event i (advisor.go:279-292): type == normal
 * (0), pkt (PACKET_* code) is HOST (0) or OUTGOING (4), and not (HOST and hostip == raddr).
 * typ/pkt/keep 4-byte aligned, hostip/raddr 16-byte aligned (device).  Asynchronous. */
int igx_np_mark(igx_ctx *ctx, const uint8_t *typ, const uint8_t *pkt, const uint32_t *hostip,
                const uint32_t *raddr, uint64_t nrows, uint8_t *keep);

/* ---- log2 latency histograms ---------------------------------------------------------- */
/* hist[(dev_index(dev)*ncont + cont) * nslots + slot] += 1 for every row with delta >= 0
 * (delta is s64 ns), slot = min(log2l(delta/divisor), nslots-1).  devs (host, ndev <= 64)
 * lists the device numbers (dev_index = position); rows with other devs are ignored.
 * ndev == 0 is the shipped gadget's keying (no targ_per_disk / targ_per_flag): every row
 * is device index 0 and dev may be NULL.  cont may be NULL (ncont must then be 1).
 * hist (device u32, max(ndev,1)*ncont*nslots) accumulates.  Async. */
int igx_hist_log2(igx_ctx *ctx, const uint32_t *dev, const uint32_t *cont,
                  const int64_t *delta, uint64_t nrows, const uint32_t *devs, uint32_t ndev,
                  uint32_t ncont, uint64_t divisor, uint32_t nslots, uint32_t *hist);

/* The raw-key form of the same histograms: biolatency keys its map by hist_key{cmd_flags, dev}
 * when targ_per_flag / targ_per_disk are set (biolatency.bpf.c:116-131), with any values.  Per
 * event, slot[i] = min(log2l(delta[i] / divisor), nslots - 1) and keep[i] = delta[i] >= 0;
 * a group-by with key (cmd_flags, dev, slot) and a COUNT of out_width 4 (the u32 slots) then
 * holds every key's histogram (engine.hist_log2_keyed).  Asynchronous. */
int igx_log2_slots(igx_ctx *ctx, const int64_t *delta, uint64_t nrows, uint64_t divisor, uint32_t nslots,
                   uint8_t *slot, uint8_t *keep);

/* ---- block-I/O request pairing ----------------------------------------------------------- */
/* The start / issue / done join that top block-io and profile block-io run through hash maps
 * keyed by `struct request *`: biotop.bpf.c:41-130 (blk_account_io_start stores who_t in
 * whobyreq, blk_mq_start_request stores start_req_t{ts, data_len} in start, blk_account_io_done
 * looks both up, forms delta_us and deletes both) and biolatency.bpf.c:47-154 (block_rq_insert /
 * block_rq_issue store ts, block_rq_complete looks it up, forms the latency and deletes it).
 *
 * A batch is nrows probe rows in stream order (row i before row i + 1): req (u64, the request
 * pointer), kind (u8, enum igx_req_kind), ts (u64, ktime ns); rows with valid[i] == 0 (valid
 * nullable) or any other kind do not exist for the join (the filters a probe applies before it
 * touches the maps).  Every req starts the batch with neither entry.  Per req, in row order:
 *   IGX_REQ_START  who := this row (overwrites)
 *   IGX_REQ_ISSUE  issue := this row (overwrites)
 *   IGX_REQ_DONE   without an issue entry: nothing, and who is kept (biotop.bpf.c:97-99);
 *                  else emit (this row, the issue row, the who row or IGX_NO_COL,
 *                  delta = ts[this] - ts[issue] mod 2^64) and delete both entries
 * done_row, issue_row, who_row, delta (device, nrows entries each): entry j describes the j-th
 * emitting DONE in stream order; igx_take of a who_row of IGX_NO_COL yields a zero row, the
 * reference's zero-initialised info_t.  *d_ndone (device u64) is their number.  The START and
 * ISSUE rows whose entries are still there at the end of the batch go to pend_row in stream
 * order: nothing is written past pend_cap entries, and *d_npend (device u64) is their true
 * number, which may exceed pend_cap (as igx_groupby_select_ge's count).  State crosses a batch
 * boundary in band: put those rows, every column, in that order, in front of the next batch.
 * The maps' max_entries is not reproduced.  biolatency's negative delta (:115-117) is an
 * emitting DONE like any other; igx_log2_slots' keep drops it.
 *
 * nrows <= 2^32 - 2 (IGX_EINVAL otherwise, checked before anything else is looked at); 0 is
 * valid.  req, ts, delta and the counts are 8-byte aligned, the row outputs 4-byte aligned
 * (IGX_EINVAL otherwise).  The outputs may not overlap the inputs or each other.  Work per row
 * does not depend on how long a req's run is; scratch of about 10 bytes per row beside the
 * sort's (IGX_ENOMEM if it cannot be had).  One host synchronisation (the sort's digit plan);
 * the counts stay on the device.  igx_req_join_tile: the rows per tile of the device scan
 * (sizes around it are where tiles hand state over). */
enum igx_req_kind { IGX_REQ_START = 0, IGX_REQ_ISSUE = 1, IGX_REQ_DONE = 2 };
int igx_req_join(igx_ctx *ctx, const uint64_t *req, const uint8_t *kind, const uint64_t *ts,
                 const uint8_t *valid /*nullable*/, uint64_t nrows,
                 uint32_t *done_row, uint32_t *issue_row, uint32_t *who_row, uint64_t *delta,
                 uint64_t *d_ndone,
                 uint32_t *pend_row, uint64_t pend_cap, uint64_t *d_npend);
int igx_req_join_tile(void);

/* ---- the two-register last-writer join ---------------------------------------------------- */
/* The join that the gadgets of pkg/gadgets/trace/ run when they pair a kprobe with its kretprobe
 * through hash maps keyed by the thread.  trace capabilities
 * (pkg/gadgets/trace/capabilities/tracer/bpf/capable.bpf.c) keeps two maps under pid_tgid:
 * `start` (:40-45) holds the arguments of the pending cap_capable call -- the kprobe writes it
 * (:147), the kretprobe looks it up (:162-164: without it, "missed entry", it returns at once)
 * and deletes it (:193); `current_syscall` (:80-85) holds the syscall the thread is in --
 * sys_enter writes it (:237), sys_exit deletes it (:246), and the kretprobe only reads it
 * (:184-189).  Unlike igx_req_join's who entry, the second entry survives any number of reads,
 * and nothing here is deleted conditionally: it is a last-writer machine with two registers, A
 * and B, per key.
 *
 * A batch is nrows rows in stream order (row i before row i + 1): key (u64), kind (u8, enum
 * igx_lw_kind); rows with valid[i] == 0 (valid nullable) or any other kind do not exist for the
 * join (the filters a probe applies before it touches the maps).  Every key starts the batch with
 * both registers empty.  Per key, in row order:
 *   IGX_LW_SET_A    A := this row (overwrites; capable.bpf.c:147)
 *   IGX_LW_SET_B    B := this row (overwrites; :237)
 *   IGX_LW_CLEAR_B  B := empty (:246)
 *   IGX_LW_TAKE_A   with A empty: nothing, and B is untouched (:162-164); else emit (this row,
 *                   the A row, the B row or IGX_NO_COL) and A := empty (:193); B is not changed
 * take_row, a_row, b_row (device, nrows entries each): entry j describes the j-th emitting TAKE_A
 * in stream order; igx_take of a b_row of IGX_NO_COL yields a zero row, so a caller for whom zero
 * is a value (syscall 0) masks on b_row itself.  *d_ntake (device u64) is their number; entries
 * at and past it are unspecified.  The rows still held in a register at the end of the batch --
 * per key at most one A row and one B row -- go to pend_row in stream order: nothing is written
 * past pend_cap entries, and *d_npend (device u64) is their true number, which may exceed
 * pend_cap.  State crosses a batch boundary in band: put those rows, every column, in that order,
 * in front of the next batch.  The maps' max_entries are not reproduced.  The one-register
 * gadgets of the family are the special case SET_A / TAKE_A.
 *
 * nrows <= 2^32 - 2 (IGX_EINVAL otherwise, checked before anything else is looked at); 0 is
 * valid.  key and the counts are 8-byte aligned, the row outputs 4-byte aligned (IGX_EINVAL
 * otherwise).  The outputs may not overlap the inputs or each other.  Work per row does not
 * depend on how long a key's run is; scratch of about 10 bytes per row beside the sort's
 * (IGX_ENOMEM if it cannot be had, and nothing stays allocated).  One host synchronisation (the
 * sort's digit plan); the counts stay on the device.  igx_lw_join_tile: the rows per tile of the
 * device scan (sizes around it are where tiles hand state over). */
enum igx_lw_kind { IGX_LW_SET_A = 0, IGX_LW_SET_B = 1, IGX_LW_CLEAR_B = 2, IGX_LW_TAKE_A = 3 };
int igx_lw_join(igx_ctx *ctx, const uint64_t *key, const uint8_t *kind,
                const uint8_t *valid /*nullable*/, uint64_t nrows,
                uint32_t *take_row, uint32_t *a_row, uint32_t *b_row, uint64_t *d_ntake,
                uint32_t *pend_row, uint64_t pend_cap, uint64_t *d_npend);
int igx_lw_join_tile(void);

/* ---- the chained join through two maps ---------------------------------------------------- */
/* The join that trace tcp (pkg/gadgets/trace/tcp/tracer/bpf/tcptracer.bpf.c) runs its connect
 * events through: two hash maps one after the other, keyed by different things.  `sockets`
 * (:59-64) is keyed by the thread: the tcp_v4/v6_connect kprobe writes it after filter_event
 * (:182-185), the kretprobe looks it up and always deletes it (:203-205, :225).  `tuplepid`
 * (:52-57) is keyed by the tuple: a kretprobe that found its `sockets` entry, returned 0 and could
 * fill the tuple stores the connecting task there (:207-222); tcp_set_state, which runs in some
 * other context and knows only the tuple, looks it up on TCP_ESTABLISHED and emits the connect
 * event with what is stored (:314-324), and deletes the entry on TCP_ESTABLISHED and TCP_CLOSE
 * (:326-327).  Whether a row writes the second map depends on what the first join found, and the
 * gadget's filters reach the event only through the first map.
 *
 * A batch is nrows rows in stream order (row i before row i + 1): key1 (u64, the thread), key2
 * (u64, an id of the tuple: equal tuples, equal ids), kind (u8, enum igx_cj_kind); rows with
 * valid[i] == 0 (valid nullable) or any other kind do not exist for the join.  Every key of
 * either map starts the batch with no entry.  In row order:
 *   IGX_CJ_ENTER  map1[key1] := this row (overwrites; :185)
 *   IGX_CJ_PASS   without map1[key1]: nothing (:203-205); else delete it and map2[key2] := this
 *                 row (overwrites; :207-225 with ret == 0 and a complete tuple)
 *   IGX_CJ_ABORT  delete map1[key1] if there is one, nothing else (:207-213 -> end)
 *   IGX_CJ_TAKE   with map2[key2]: emit (this row, the row stored there); either way delete it
 *                 (:314-327)
 *   IGX_CJ_DROP   delete map2[key2]; emit nothing (TCP_CLOSE, :311-312, :327)
 *   IGX_CJ_HELD   map2[key2] := this row, unconditionally: a PASS row that was admitted in an
 *                 earlier batch and is carried in band (below)
 * key1 matters for ENTER / PASS / ABORT rows only, key2 for PASS / HELD / TAKE / DROP rows only
 * (both columns are read for every row, so every entry must be readable).
 * take_row, pass_row (device, nrows entries each): entry j is the j-th emitting TAKE in stream
 * order and the PASS or HELD row it found.  *d_ntake (device u64) is their number; entries at and
 * past it are unspecified.  The rows still in a map at the end of the batch -- the ENTER rows in
 * map 1 and the PASS / HELD rows in map 2 -- go to pend_row together, in stream order: nothing is
 * written past pend_cap entries, and *d_npend (device u64) is their true number, which may exceed
 * pend_cap.
 *
 * State crosses a batch boundary in band: put those rows, every column, in that order, in front
 * of the next batch, and rewrite the kind of each carried PASS row to IGX_CJ_HELD -- its ENTER has
 * been consumed, so as a PASS it would find map 1 empty and be dropped.  Carried ENTER and HELD
 * rows keep their kind.  Any cut of one stream into batches then gives the emissions of the whole
 * stream.  The maps' max_entries are not reproduced.
 *
 * How it reduces: two igx_lw_join pipelines over the same row index space.  Stage 1 on key1 with
 * ENTER = SET_A, PASS / ABORT = TAKE_A; stage 2 on key2 with SET_A = a PASS that emitted in stage 1
 * or a HELD row, TAKE_A = TAKE / DROP, and the emissions of DROP rows discarded (a delete is a take
 * nobody reads).  The hand-over between them and the merge of the two pending lists are plain
 * grids; the counts stay on the device.
 *
 * nrows <= 2^32 - 2 (IGX_EINVAL otherwise, checked before anything else is looked at); 0 is
 * valid.  The keys and the counts are 8-byte aligned, the row outputs 4-byte aligned (IGX_EINVAL
 * otherwise).  The outputs may not overlap the inputs or each other.  Work per row does not
 * depend on how long a key's run is; beside the sort's, about 10 bytes per row of the context's
 * scratch and 5 of its side arena (IGX_ENOMEM if they cannot be had, and nothing stays
 * allocated).  Two host synchronisations (one digit plan per sort).  igx_chain_join_tile: the
 * rows per tile of the device scans. */
enum igx_cj_kind { IGX_CJ_ENTER = 0, IGX_CJ_PASS = 1, IGX_CJ_ABORT = 2,
                   IGX_CJ_TAKE = 3, IGX_CJ_DROP = 4, IGX_CJ_HELD = 5 };
int igx_chain_join(igx_ctx *ctx, const uint64_t *key1, const uint64_t *key2, const uint8_t *kind,
                   const uint8_t *valid /*nullable*/, uint64_t nrows,
                   uint32_t *take_row, uint32_t *pass_row, uint64_t *d_ntake,
                   uint32_t *pend_row, uint64_t pend_cap, uint64_t *d_npend);
int igx_chain_join_tile(void);

/* ---- trace tcp: what each probe decides per row -------------------------------------------- */
/* One row per probe firing of tcptracer.bpf.c, with the fields the probe reads (device columns,
 * nrows entries each): probe (u8, enum igx_tcp_probe), tid, pid, uid (u32), mntns (u64), ret (i32,
 * connect-return), state (u8: the new state for set-state, the socket's skc_state for close),
 * family (u16: skc_family; for connect-return the probe's own constant, :238, :250), netns (u32),
 * saddr, daddr (16 bytes each; AF_INET uses the first 4), dport, sport (u16, as the socket holds
 * them, i.e. network order), num (u16, skc_num, accept only).  filter_pid (0: none), filter_uid
 * ((uint32_t)-1: none) and mntns_set (device, n_mntns <= 1024 ids sorted ascending; null: no
 * mount-namespace filter, while a non-null set of 0 ids passes nothing) are the gadget's filter
 * constants (:14-16, :72-77).
 *
 * Per row: kind[i], an igx_cj_kind or IGX_TCP_NO_KIND; event[i], 0 none, 1 accept, 2 close (the
 * events a probe emits without a map); tuple + 40 * i, the tuple_key_t (:31-43: saddr 16, daddr
 * 16, sport 2, dport 2, netns 4), written for PASS / TAKE / DROP rows and rows with an event and
 * zero for all others; key1[i] = tid (key1 nullable).
 *   fill_tuple (:79-122) reads netns, then saddr, daddr, dport, sport; the first zero among the
 *     last four stops it and every later field stays zero.  AF_INET reads 4 bytes of each address
 *     (the other 12 key bytes are zero whatever the column holds), AF_INET6 tests all 16 bytes,
 *     any other family fails.
 *   filter_event (:147-166) runs at connect-enter, close and accept only: family, then mount
 *     namespace, then pid, then uid.
 *   connect-enter   ENTER if filter_event passes.
 *   connect-return  ABORT with ret != 0 or an incomplete tuple, else PASS.  No filter.
 *   set-state       no filter.  A state other than ESTABLISHED (1) / CLOSE (7): nothing.  An
 *                   incomplete tuple: nothing (its delete uses a key with a zero field, and no
 *                   stored key has one).  CLOSE: DROP.  ESTABLISHED: TAKE.
 *   close           (:253-294) old state SYN_SENT (2), SYN_RECV (3) or NEW_SYN_RECV (12): nothing;
 *                   an incomplete tuple: nothing; else a close event.
 *   accept          (:332-372) fill_tuple's result is ignored, then sport := bswap16(num), then
 *                   nothing if saddr or daddr (as 128 bits), dport or sport is zero; else an
 *                   accept event.  A socket whose inet_sport is zero but whose skc_num is not is
 *                   reported.
 * The return probe's socket fields are carried on the connect-return row (the reference reads
 * them through the pointer its kprobe stored; csrc/k_tcptrace.h says when the two differ).
 *
 * nrows <= 2^32 - 2, n_mntns <= 1024; saddr / daddr 16-byte aligned, mntns, tuple, key1 and
 * mntns_set 8-byte aligned, the other columns aligned to their width (IGX_EINVAL otherwise, and
 * for a null context, before any pointer is read).  One launch, asynchronous, no scratch. */
enum igx_tcp_probe { IGX_TCP_CONNECT_ENTER = 0, IGX_TCP_CONNECT_RETURN = 1, IGX_TCP_CLOSE = 2,
                     IGX_TCP_SET_STATE = 3, IGX_TCP_ACCEPT_RETURN = 4 };
#define IGX_TCP_NO_KIND 255
#define IGX_TCP_TUPLE_BYTES 40
typedef struct {
    const uint8_t *probe;
    const uint32_t *tid;
    const uint32_t *pid;
    const uint32_t *uid;
    const uint64_t *mntns;
    const int32_t *ret;
    const uint8_t *state;
    const uint16_t *family;
    const uint32_t *netns;
    const uint8_t *saddr;   /* n x 16 */
    const uint8_t *daddr;   /* n x 16 */
    const uint16_t *dport;
    const uint16_t *sport;
    const uint16_t *num;
} igx_tcp_rows;
int igx_tcp_classify(igx_ctx *ctx, const igx_tcp_rows *rows, uint64_t nrows,
                     uint32_t filter_pid, uint32_t filter_uid,
                     const uint64_t *mntns_set /*nullable*/, uint32_t n_mntns,
                     uint8_t *tuple, uint8_t *kind, uint8_t *event, uint64_t *key1 /*nullable*/);

/* ---- profile cpu: row interning, symbol lookup -------------------------------------------- */
/* profile cpu (pkg/gadgets/profile/cpu/tracer/bpf/profile.bpf.c:60-114) keys its counts by
 * key_t (profile.h:9-16), whose two stack fields are ids: bpf_get_stackid (:93, :98) turns a
 * stack of up to 127 return addresses (1016 bytes) into a small number through the stack map.
 * igx_intern is that map for any fixed-width row of up to 1 KiB: it reduces a row to a u32 that
 * can be a group-by key column (group-by keys themselves end at IGX_MAX_KEY_BYTES).
 *
 * The object owns a device store of the distinct rows seen so far, over all igx_intern_add
 * calls.  A row's id is its rank by first appearance in the stream: 0 for the first distinct
 * row, 1 for the next new one, and so on.  igx_intern_add takes nrows rows of row_bytes at rows
 * + i * row_stride (device) in stream order and writes out_ids (device, nrows entries): for a
 * row whose content is stored, that content's id; for a new content, D + r, with D the number
 * of rows stored before the call and r the number of new contents whose first valid occurrence
 * in this batch comes before this content's first valid occurrence.  Rows with valid[i] == 0
 * (valid nullable) get IGX_NO_COL and are not stored.  Equality is over all row_bytes bytes;
 * callers zero-pad short stacks, as the kernel's stack map does.  So ids are a function of the
 * stream alone: any split of one stream into batches gives the same ids, whatever the
 * scheduling.
 *
 * Limits (IGX_EINVAL otherwise): row_bytes a multiple of 8 in 8..1024; rows 8-byte aligned;
 * row_stride a multiple of 8 and at least row_bytes; out_ids 4-byte aligned; capacity in
 * 1..2^28; nrows <= 2^31 - 1 (0 is valid).  The table has S slots, S a power of two and at
 * least 2 x capacity (igx_intern_slots).  Memory: capacity x row_bytes for the store, 8 bytes
 * per slot, and per-call scratch of about 5 bytes per row plus 12 per 1024 rows; device memory
 * that cannot be had returns IGX_ENOMEM and nothing stays allocated.
 *
 * Overflow: when a call would take the distinct count past capacity, that call's ids and
 * later calls' ids are unspecified (nothing is written out of bounds) and igx_intern_count
 * returns IGX_ENOSPC from then on.  The reference's max_entries (256 stacks, 10240 keys:
 * profile.bpf.c:17-30) and the stack map's bucket-collision -EEXIST are kernel artifacts and
 * are not reproduced.
 *
 * igx_intern_count (synchronises): the number of distinct rows stored.  igx_intern_rows
 * (asynchronous gather): out (device, 8-byte aligned) receives k rows of row_bytes, row j the
 * content of ids[j] (device, 4-byte aligned); an id of IGX_NO_COL, or one at or above the
 * distinct count, yields a zero row.  igx_intern_slots (host): S.
 *
 * igx_intern_hash_rows (host only, no GPU): out[i] = the 64-bit hash of the row at rows +
 * i * row_stride, the function the kernels use (csrc/k_stack.h compiles for both sides).  A
 * row's home slot is hash & (S - 1), probing is linear from there, and a slot carries the tag
 * hash >> 32: a candidate row is compared only where the tags agree.  Rows equal in both and
 * different in content are the table's worst case, and these two statements let a caller build
 * them.
 *
 * igx_intern_add_first does what igx_intern_add does -- the same store, the same ids -- and
 * writes out_first (device u8, nrows entries): 1 iff row i is valid and is the first valid
 * occurrence, over all calls on the object, of its content; 0 otherwise.  That is the `seen` map
 * of trace capabilities' --unique (capable.bpf.c:128-139: only the first cap_capable of a (cap,
 * mntns) passes).  The mask is a function of the stream alone: any split into batches gives the
 * same mask.  out_ids may be NULL here (the ids are then not written).  After overflow the mask
 * is unspecified, as the ids are. */
typedef struct igx_intern igx_intern;
int igx_intern_create(igx_ctx *ctx, uint32_t row_bytes, uint64_t capacity, igx_intern **out);
int igx_intern_add(igx_intern *t, const void *rows, uint64_t row_stride, const uint8_t *valid /*nullable*/,
                   uint64_t nrows, uint32_t *out_ids);
int igx_intern_add_first(igx_intern *t, const void *rows, uint64_t row_stride, const uint8_t *valid /*nullable*/,
                         uint64_t nrows, uint32_t *out_ids /*nullable*/, uint8_t *out_first);
int igx_intern_count(igx_intern *t, uint64_t *n_distinct);
int igx_intern_rows(igx_intern *t, const uint32_t *ids, uint64_t k, void *out);
int igx_intern_slots(igx_intern *t, uint64_t *n_slots);
int igx_intern_destroy(igx_intern *t);
int igx_intern_hash_rows(const void *rows, uint32_t row_bytes, uint64_t row_stride, uint64_t n, uint64_t *out);

/* findKernelSymbol (pkg/gadgets/profile/cpu/tracer/tracer.go:184-208) for n addresses:
 * out_idx[i] (device u32) is the index into the symbol table of the symbol ips[i] resolves to,
 * or IGX_NO_COL for "[unknown]".  sym_addr (device, nsyms u64) is the table in the order given
 * (readKernelSymbols, :139-177, does not sort /proc/kallsyms and neither does this).  Exactly
 * as written:
 *   start = 0, end = nsyms - 1 (signed), addr = 0
 *   while start < end: mid = start + (end - start + 1) / 2; addr = sym[mid];
 *                      if addr <= ip: start = mid, else end = mid - 1
 *   the result is start if start == end && sym[start] <= addr
 * The last comparison is against addr, the last address probed, not against ip.  So in a sorted
 * table of two or more symbols an ip below every symbol still resolves to symbol 0, and a
 * one-symbol table resolves only if that symbol's address is 0.  nsyms <= 2^32 - 2; sym_addr
 * and ips 8-byte aligned, out_idx 4-byte aligned (IGX_EINVAL otherwise).  Asynchronous. */
int igx_ksym_lookup(igx_ctx *ctx, const uint64_t *sym_addr, uint64_t nsyms,
                    const uint64_t *ips, uint64_t n, uint32_t *out_idx);

/* ---- traceloop: the enter / exit / cont join by timestamp ---------------------------------- */
/* Tracer.Read of traceloop (pkg/gadgets/traceloop/tracer/tracer.go:246-545) joins sys_enter
 * records, sys_exit records and "continued" parameter records by the monotonic timestamp the BPF
 * program stamps on all of them (traceloop.bpf.c:174, :400, :410), then sorts by event time.
 * igx_traceloop_join is that join over two record streams in the order readOverWritable's callback
 * delivers them (reading the overwritable perf ring stays with the caller).
 *
 * Syscall rows (ns, device columns): mntns (u64, the container's; NULL: one container), mono_ts
 * (u64), sort_ts (u64: the boot timestamp, or the monotonic one where the kernel has no
 * bpf_ktime_get_boot_ns, :232-244), typ (u8: 0 enter, 1 exit), id (u16), pid (u32), valid (u8,
 * nullable).  Cont rows (nc): c_mntns (NULL iff mntns is), c_mono_ts, c_index (u8), c_valid.
 * Rows with valid == 0 and syscall rows of any other typ (:304-311) do not exist for the join.
 * Only the order inside each stream matters.
 *
 * A group is all rows with the same (mntns, mono_ts); the reference has one map set per
 * container.  In a group, in row order, E are the enters, X the exits, C the conts;
 *   skip(e)   e.id is nr_exit, nr_exit_group or nr_rt_sigreturn (60 / 231 / 15 on x86_64,
 *             93 / 94 / 139 on arm64; traceloop.bpf.c:12-35, tracer.go:418)
 *   match(e)  the first x in X with x.id == e.id && x.pid == e.pid (:438-441)
 *   m         the first e in E with !skip(e) and a match;   e0: the first row of E.
 * What the loops at :362-530 publish for a group:
 *   1. complete events: every skip enter, with no exit row; m, with exit row match(m).  Once m
 *      matched the exit list is gone (:446) and later non-skip enters are dropped (:431-436);
 *      non-skip enters without a match are dropped too once anything completed (:419, :445).
 *   2. conts belong to e0 only (:415 deletes them after the first enter, whatever becomes of
 *      it): for i in 0..5 the first row of C with index == i (:400-407).  Conts of index >= 6,
 *      of a group without enters, or of a group whose e0 is not a complete event are lost.
 *   3. if nothing completed, every row of E is an incomplete enter (:468-498).
 *   4. if m does not exist, every row of X is an incomplete exit (:500-530), also when skip
 *      enters completed.
 * Events come out ascending by sort_ts of their own row (the enter row; the exit row for an
 * incomplete exit).  The reference's order among equal times is map iteration followed by an
 * unstable sort, i.e. undefined; here ties go ascending by syscall row index -- a choice within
 * the reference's freedom.
 *
 * Outputs (device; ns entries each, ev_cont 6 x ns), event j in output order: ev_row[j] its
 * syscall row; ev_class[j] 0 complete, 1 incomplete enter, 2 incomplete exit; ev_exit[j] the exit
 * row or IGX_NO_COL; ev_cont[6 * j + i] the cont row of parameter i or IGX_NO_COL.  *d_nev (device
 * u64) is the number of events; entries at and past it hold IGX_NO_COL (ev_class: 0xFF).
 *
 * Not reproduced: the maps' max_entries; WallTimeFromBootTime(0) = the wall clock now (a zero
 * timestamp is converted like any other); the one-byte-short copy of a sample that wraps the
 * ring (perf_buffer.go:183), which belongs to the ring reader.
 *
 * ns + nc <= 2^32 - 2 (0 is valid).  The u64 columns and d_nev are 8-byte aligned, pid and the
 * row outputs 4-byte aligned, id 2-byte aligned; the outputs may not overlap the inputs or each
 * other.  IGX_EINVAL otherwise, before any GPU work.  Work per row does not depend on the size
 * of a group or of an (id, pid) run inside it.  Device memory of about 60 bytes per row of either
 * stream beside the sorts' comes from the context's arenas; IGX_ENOMEM if it cannot be had, with
 * nothing of the call's left allocated.  Two sorts, each with one host synchronisation (its digit
 * plan); the count stays on the device.  The result is a function of the input alone.
 * igx_traceloop_tile: the positions per tile of the device scan. */
int igx_traceloop_join(igx_ctx *ctx,
                       const uint64_t *mntns /*nullable*/, const uint64_t *mono_ts, const uint64_t *sort_ts,
                       const uint8_t *typ, const uint16_t *id, const uint32_t *pid,
                       const uint8_t *valid /*nullable*/, uint64_t ns,
                       const uint64_t *c_mntns /*null iff mntns is*/, const uint64_t *c_mono_ts,
                       const uint8_t *c_index, const uint8_t *c_valid /*nullable*/, uint64_t nc,
                       uint16_t nr_exit, uint16_t nr_exit_group, uint16_t nr_rt_sigreturn,
                       uint32_t *ev_row, uint32_t *ev_exit, uint8_t *ev_class, uint32_t *ev_cont,
                       uint64_t *d_nev);
int igx_traceloop_tile(void);

/* ---- advise seccomp-profile: per-mntns syscall sets ---------------------------------------- */
/* ig_seccomp_e (pkg/gadgets/advise/seccomp/tracer/bpf/seccomp.bpf.c:67-139) keeps, per mount
 * namespace, a value of 501 bytes: 500 presence bytes (one per syscall id) and a footer byte that
 * says whether runc's rows are being recorded yet.  igx_seccomp is that map.  Per row, over the
 * device columns mntns (u64), id (u32), arg0 (u64, PT_REGS_PARM1), comm (at comm + i *
 * comm_stride; only its first four bytes are read) and compat (u8, nullable = all 0):
 *   1. compat != 0, id >= 500 or mntns == 0: the row is dropped and makes no entry.
 *   2. otherwise the entry of mntns exists from this row on, even if nothing is recorded in it.
 *   3. a row whose comm starts with "runc", while the entry is not armed: if id == nr_prctl and
 *      arg0 == 2 (PR_GET_PDEATHSIG; all 64 bits compared) it arms the entry; it records nothing.
 *   4. such a row when the entry is armed: (id == nr_prctl and arg0 == 38, PR_SET_NO_NEW_PRIVS) or
 *      id == nr_seccomp records nothing; every other row records, a later prctl(2) included.
 *   5. any other row records: value[id] = 1.
 * Rows with valid[i] == 0 (valid nullable) are skipped.  The object counts the rows of all updates,
 * so the result is a function of the stream alone, however it is cut into updates.  nr_prctl and
 * nr_seccomp are fixed at creation (157 / 317 on x86_64, 167 / 277 on arm64).
 *
 * igx_seccomp_peek (asynchronous): for n namespaces at mntns (device), out (device, n x 501
 * bytes) receives the values and found (device, n bytes) whether the entry exists; an absent
 * entry's value is zero.  Namespace 0 is found and blank: the reference installs a blank value at
 * key 0 (tracer.go:77).  igx_seccomp_delete (asynchronous) removes the entries of n namespaces
 * (device; absent ones are ignored): a later row of that namespace starts from a blank, unarmed
 * value.  igx_seccomp_list (synchronises): *n = the number of entries, the first min(*n, cap) of
 * them written to out (device u64) in no particular order.  igx_seccomp_count (synchronises): the
 * number of entries.
 *
 * Capacity is the number of distinct namespaces the object can ever hold: a deleted namespace
 * keeps its slot (so that the probe chains of others stay whole, and its own rows find it again)
 * and keeps counting against capacity.  The table has S slots, S the smallest power of two that
 * is at least 2 x capacity and at least 2 (igx_seccomp_slots); tables of up to 2048 slots are
 * marked through LDS, larger ones in global memory, with the same result.  When an update takes
 * the distinct namespaces past capacity, the values are unspecified from then on (nothing is
 * written out of bounds), igx_seccomp_count and igx_seccomp_list return IGX_ENOSPC, and once one
 * of them has, igx_seccomp_update does too.  The reference's max_entries of 1024 and its silent
 * drop of new namespaces in a full map are kernel artifacts and are not reproduced.
 *
 * Limits (IGX_EINVAL otherwise, checked before any GPU work): capacity in 1..2^19; comm_stride >=
 * 4; no null column when nrows > 0 (compat and valid may be null); mntns and arg0 8-byte, id
 * 4-byte aligned; nrows <= 2^31 - 1 (0 is valid).  Memory: 81 bytes per slot and per-call scratch
 * of 4 bytes per row; device memory that cannot be had returns IGX_ENOMEM and nothing stays
 * allocated.
 *
 * igx_seccomp_home (host only, no GPU): *home = the slot a namespace's probe starts at in a table
 * of nslots (a power of two; IGX_EINVAL otherwise); probing is linear from there.  With it a
 * caller can build namespaces that share a home slot, the table's worst case. */
typedef struct igx_seccomp igx_seccomp;
int igx_seccomp_create(igx_ctx *ctx, uint64_t capacity, uint32_t nr_prctl, uint32_t nr_seccomp, igx_seccomp **out);
int igx_seccomp_update(igx_seccomp *t, const uint64_t *mntns, const uint32_t *id, const uint64_t *arg0,
                       const void *comm, uint64_t comm_stride, const uint8_t *compat /*nullable*/,
                       const uint8_t *valid /*nullable*/, uint64_t nrows);
int igx_seccomp_peek(igx_seccomp *t, const uint64_t *mntns, uint64_t n, uint8_t *out, uint8_t *found);
int igx_seccomp_delete(igx_seccomp *t, const uint64_t *mntns, uint64_t n);
int igx_seccomp_list(igx_seccomp *t, uint64_t *out, uint64_t cap, uint64_t *n);
int igx_seccomp_count(igx_seccomp *t, uint64_t *n);
int igx_seccomp_slots(igx_seccomp *t, uint64_t *n_slots);
int igx_seccomp_destroy(igx_seccomp *t);
int igx_seccomp_home(uint64_t mntns, uint64_t nslots, uint64_t *home);

/* ---- group:sum of float columns, IP text --------------------------------------------- */
/* GroupEntries' float group:sum (group.go:133-156, flattenValues): perm (device u32, n) is a
 * stable sort of the rows by the group key (key_bytes at row * key_stride of keys); each run
 * of equal keys is one group in input order.  For each run, out[first row of the run] =
 * v[first] + v[second] + ... in that order, in float64, rounded to float32 after every add
 * when val_width is 4 (SetFloat on a float32 field).  Rows with valid[row] == 0 (nullable)
 * are nil entries and belong to no run.  Other out entries are left untouched.  Async. */
int igx_segment_fsum(igx_ctx *ctx, const uint8_t *keys, uint32_t key_stride, uint32_t key_bytes,
                     const uint32_t *perm, uint64_t n, const uint8_t *valid, const void *vals,
                     uint32_t val_width, double *out);

/* IPStringFromBytes (pkg/gadgets/helpers.go:111-120) for n rows: addr (16 bytes at row *
 * addr_stride) rendered as netip.AddrFrom16(...).String() when the u16 family at row *
 * family_stride is AF_INET6 (10), else netip.AddrFrom4(addr[0:4]).String().  out (device,
 * 8-byte aligned) receives n x IGX_IPTEXT_WIDTH bytes, each text zero-padded, so byte order
 * of two rows is Go's string order.  rowmap (device, nullable): row r reads row rowmap[r].
 * Asynchronous. */
#define IGX_IPTEXT_WIDTH 40
int igx_ip_text(igx_ctx *ctx, const uint8_t *addr, uint32_t addr_stride, const uint8_t *family,
                uint32_t family_stride, const uint32_t *rowmap, uint64_t n, uint8_t *out);

/* ---- data movement either side of the path ---------------------------------------------- */
/* Sender side of the group-by all-to-all: rows (device, nrows x
 * row_bytes, 4-byte aligned) are copied to out (device, same size) grouped by owner part,
 * stable within a part; owner = FNV-1a(32) over the first key_bytes/4 u32 words of the row,
 * mod nparts (1..64).  part_counts (device u64[nparts]) receives the rows per part.  Async. */
int igx_partition_rows(igx_ctx *ctx, const uint8_t *rows, uint64_t nrows, uint32_t row_bytes,
                       uint32_t key_bytes, uint32_t nparts, uint8_t *out, uint64_t *part_counts);
/* The same partition straight from a finalized table (igx_groupby_finalize or _async): its
 * groups as igx_groupby_gather rows (key words | aggregates wrapped to out_widths[x] bytes
 * (nullable: 8) | first index) grouped by owner part, stable in slot order within a part.  The
 * group count is read on the device (view->d_n_groups), so an asynchronously finalized table
 * is partitioned without a host round trip; out holds cap_rows rows (>= the table's capacity).
 * Overflow: a table may list more groups than cap_rows (an interval over its capacity whose
 * IGX_ENOSPC has not been collected yet: finalized asynchronously and not waited on).  Then no
 * more than cap_rows rows are written and EVERY part_counts[p] is UINT64_MAX (-1 read as int64):
 * the rows are incomplete and no count is a send count.  Callers test the counts they read back
 * before using them (the Python binding's dist.exchange_partitioned raises IGX_ENOSPC).
 * The sender side of the owner exchange (C4 / C5 at N > 1; replaces the reference's per-node
 * fan-out + client merge, grpc-runtime.go:221-237 -> snapshotcombiner.go:79-106).  Async. */
int igx_partition_groups(igx_ctx *ctx, const igx_table_view *view, const uint32_t *out_widths,
                         uint32_t nparts, uint8_t *out, uint64_t cap_rows, uint64_t *part_counts);
/* ---- multi-GPU merges over RCCL ----------------------------------------
 * One process per GPU.  Replaces the reference's node fan-out + client concatenation
 * (pkg/runtime/grpc/grpc-runtime.go:221-237 -> pkg/snapshotcombiner/snapshotcombiner.go:79-106)
 * with exact merges over xGMI.  Setup: rank 0 calls igx_dist_get_unique_id and hands the
 * IGX_DIST_ID_BYTES bytes to every rank by the caller's own channel (ncclUniqueId); every rank
 * then calls igx_dist_init on its context.  Collectives are enqueued on the context's stream
 * and must be called in the same order on every rank.  The row exchanges all-gather their
 * counts, capacities and an argument-error flag first (they synchronise the stream) and plan
 * with igx_dist_plan_* below, so either every rank proceeds or every rank returns the same
 * error (IGX_ENOSPC, or IGX_EINVAL when some rank's arguments are invalid).  With out == NULL
 * on every rank they are a size query: the counts are exchanged and returned, no rows move.
 * Failure detection: the communicator is non-blocking and every wait inside these calls (a call
 * still being issued, the stream draining after the metadata all-gather, igx_dist_wait) polls
 * ncclCommGetAsyncError under a deadline (IGX_DIST_TIMEOUT_MS, default 120000, or
 * igx_dist_set_timeout).  An RCCL error, an asynchronous error or a missed deadline -- a peer
 * that died mid-collective -- returns IGX_EIO, aborts this rank's communicator (ncclCommAbort:
 * its kernels waiting on the peer exit) and marks it broken: every later call returns IGX_EIO
 * at once.  The reference drops a node that stops answering after its TTL instead of waiting on
 * it (pkg/snapshotcombiner/snapshotcombiner.go:91-100). */
#define IGX_DIST_ID_BYTES 128
typedef struct igx_dist igx_dist;
int igx_dist_get_unique_id(uint8_t *out_id);
int igx_dist_init(igx_ctx *ctx, const uint8_t *id, int nranks, int rank, igx_dist **out);
int igx_dist_destroy(igx_dist *d);
int igx_dist_rank(igx_dist *d, int *rank, int *nranks);
int igx_dist_barrier(igx_dist *d);   /* synchronises (bounded) */
/* The deadline of every wait on this communicator, in ms (> 0). */
int igx_dist_set_timeout(igx_dist *d, int timeout_ms);
/* Bounded hipStreamSynchronize of the context's stream for a caller that must wait on an
 * asynchronous collective (igx_dist_allreduce_u32, the row exchanges' data phase): IGX_EIO, and
 * the communicator aborted, on an RCCL error or when the deadline passes. */
int igx_dist_wait(igx_dist *d);
/* Marks the communicator unusable, as a failed group does: every later call returns IGX_EIO
 * without entering a collective.  For a caller that learned of a peer's failure out of band
 * (e.g. a node's gRPC stream ended, grpc-runtime.go:221-237). */
int igx_dist_mark_broken(igx_dist *d);
/* C3: in-place sum of a u32 buffer (log2 histograms) over all ranks (mod 2^32, exact).  Async. */
int igx_dist_allreduce_u32(igx_dist *d, uint32_t *buf, uint64_t n);
/* Top-K candidate merge (C2, C5): every rank's nrows x row_bytes rows (device) concatenated in
 * rank order into out (device, cap_rows rows); counts (host, nranks, nullable) receives each
 * rank's row count.  Feed the result to igx_topk with the rows' global first index as the
 * position for the exact global top-K. */
int igx_dist_allgather_rows(igx_dist *d, const void *rows, uint64_t nrows, uint32_t row_bytes, void *out,
                            uint64_t cap_rows, uint64_t *counts);
/* Group-by / distinct exchange (C4, C5): rows (device) already grouped by destination rank,
 * send_counts[p] (host) rows for rank p in rank order, go to their rank; out (device,
 * cap_rows rows) receives this rank's rows in source-rank order; recv_counts (host, nranks,
 * nullable) their counts. */
int igx_dist_alltoallv_rows(igx_dist *d, const void *rows, const uint64_t *send_counts, uint32_t row_bytes,
                            void *out, uint64_t cap_rows, uint64_t *recv_counts);
/* igx_partition_rows (owner = FNV-1a of the key words mod nranks) + igx_dist_alltoallv_rows:
 * packed partial-group rows (igx_groupby_gather layout) go to the rank owning their key, which
 * merges them with igx_groupby_update_ex (SUM of partials, MIN of first indices).  *out_nrows =
 * rows received. */
int igx_dist_exchange_groups(igx_dist *d, const void *rows, uint64_t nrows, uint32_t row_bytes,
                             uint32_t key_bytes, void *out, uint64_t cap_rows, uint64_t *out_nrows);
/* The planning step of the row exchanges, as a host function (no GPU, no communicator): every
 * rank calls it on the same all-gathered metadata, so every rank reaches the same decision.
 * meta holds nranks rows, rank r's row written by rank r:
 *   igx_dist_plan_alltoallv: nranks + 2 words = send_counts[0..nranks) | cap_rows | flags
 *   igx_dist_plan_allgather: 3 words          = nrows | cap_rows | flags
 * flags: IGX_DIST_F_BADARG (that rank's own arguments are invalid), IGX_DIST_F_QUERY (a size
 * query: out == NULL).  status: IGX_OK (proceed; for a query on every rank, only the counts are
 * meaningful), IGX_EINVAL (a rank flagged BADARG, or ranks disagree on QUERY), IGX_ENOSPC (a
 * rank's capacity is below the rows it would receive); culprit = that rank (lowest), else -1.
 * Row offsets: send_off[p] = first row this rank sends to rank p (alltoallv; 0 for allgather);
 * recv_off[p] / recv_counts[p] = where rank p's rows land in this rank's output and how many. */
#define IGX_DIST_MAX_RANKS 64
#define IGX_DIST_F_BADARG 1u
#define IGX_DIST_F_QUERY 2u
typedef struct {
    int32_t status;
    int32_t culprit;
    uint64_t total_rows;
    uint64_t recv_counts[IGX_DIST_MAX_RANKS];
    uint64_t send_off[IGX_DIST_MAX_RANKS];
    uint64_t recv_off[IGX_DIST_MAX_RANKS];
} igx_dist_plan;
int igx_dist_plan_alltoallv(int nranks, int rank, const uint64_t *meta, igx_dist_plan *out);
int igx_dist_plan_allgather(int nranks, int rank, const uint64_t *meta, igx_dist_plan *out);

/* The step before the path: array-of-structs records on the device (a BPF
 * map dump of {key, value} structs or perf-ring event structs, e.g. tcptopIpKeyT +
 * tcptopTrafficT, pkg/gadgets/top/tcp/tracer/tcptop_bpfel_x86.go:15-30) are cut into SoA
 * columns: field f (byte offset field_off[f], field_width[f] bytes) of record r goes to
 * out_cols[f] + r * field_width[f].  1..16 fields.  Async. */
/* trace open's perf-ring samples (struct event, pkg/gadgets/trace/open/tracer/bpf/opensnoop.h:14-24,
 * bpf2go opensnoopEvent: ts u64 @0, pid u32 @8, uid u32 @12, mntns u64 @16, ret s32 @24,
 * flags s32 @28, comm[16] @32, fname[255] @48; 304 bytes) -> the Event fields the tracer's
 * run loop fills (trace/open/tracer/tracer.go:182-208):
 *   timestamp = WallTimeFromBootTime(ts) = ts + boot_to_wall_ns;  ret = int(Ret) (sign-
 *   extended); fd = ret >= 0 ? ret : 0;  err = ret < 0 ? -ret : 0;  comm / path =
 *   FromCString (the bytes before the first NUL; the rest of the row zeroed; path rows are
 *   256 bytes, the 255-byte name plus a NUL).
 * samples: device, n x sample_bytes (sample_bytes >= 304, a multiple of 8; 8-byte aligned).
 * Null output columns are skipped.  Asynchronous. */
typedef struct {
    int64_t *timestamp;
    uint32_t *pid;
    uint32_t *uid;
    uint64_t *mntns;
    int64_t *ret;
    int64_t *fd;
    int64_t *err;
    uint8_t *comm;   /* n x 16 */
    uint8_t *path;   /* n x 256 */
} igx_open_cols;
int igx_ingest_open_events(igx_ctx *ctx, const uint8_t *samples, uint64_t n, uint32_t sample_bytes,
                           int64_t boot_to_wall_ns, const igx_open_cols *out);
int igx_ingest_aos(igx_ctx *ctx, const void *records, uint64_t nrec, uint32_t rec_bytes,
                   const uint32_t *field_off, const uint32_t *field_width, uint32_t nfields,
                   void *const *out_cols);

/* ---- test hooks (k_debug.hip; not part of the aggregation path) ----
 * igx_debug_hold_stream: one wave on the context's stream that waits on a host-mapped flag
 * (at most ~max_ms), so a test can make a collective queued behind it miss igx_dist's deadline
 * the way a dead peer would.  igx_debug_release sets the flag, waits for the stream, frees the
 * token; *how = 1 if the wave saw the release, 2 if its own budget ran out. */
int igx_debug_hold_stream(igx_ctx *ctx, uint32_t max_ms, void **token);
int igx_debug_release(igx_ctx *ctx, void *token, uint32_t *how);

/* ---- synthetic event generators (device; bit-identical with oracle/igx_oracle.c) ---- */
int igx_gen_tcp(igx_ctx *ctx, uint64_t seed, uint64_t rank, uint64_t G, uint64_t permA,
                uint64_t permB, const uint64_t *cdf, uint64_t base, uint64_t n, uint8_t *saddr,
                uint8_t *daddr, uint64_t *mntns, uint32_t *pid, uint8_t *comm, uint16_t *lport,
                uint16_t *dport, uint16_t *family, uint32_t *size, uint8_t *dir);
int igx_gen_open(igx_ctx *ctx, uint64_t seed, const uint64_t *comm_cdf, uint64_t base,
                 uint64_t n, uint32_t *pid, uint32_t *uid, uint64_t *mntns, uint8_t *comm,
                 int64_t *ret, int64_t *fd, int64_t *err, uint32_t *path_id);
int igx_gen_bio(igx_ctx *ctx, uint64_t seed, const uint64_t *q, uint64_t nq, uint64_t base,
                uint64_t n, uint32_t *dev, uint32_t *cont, uint64_t *delta);
int igx_gen_np(igx_ctx *ctx, uint64_t seed, uint64_t nsrc, uint64_t npeer, uint64_t base,
               uint64_t n, uint32_t *src, uint32_t *peer, uint16_t *port, uint8_t *pkt,
               uint8_t *typ, uint8_t *proto, uint32_t *hostip, uint32_t *raddr);
int igx_gen_file(igx_ctx *ctx, uint64_t seed, uint64_t rank, uint64_t G, uint64_t permA,
                 uint64_t permB, const uint64_t *cdf, uint64_t base, uint64_t n,
                 uint64_t *inode, uint32_t *dev, uint32_t *pid, uint32_t *tid, uint8_t *op,
                 uint32_t *count);

#ifdef __cplusplus
}
#endif
#endif /* IGX_H */
