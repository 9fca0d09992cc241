"""Wide group-by tables: key records of 4 GiB and more (64-bit record addressing).

A table is wide when n_slots x key_stride >= 2^32 (igx_groupby_create in include/igx.h): its
direct and partitioned forms address key records per lane with 64-bit addresses, AUTO plans every
interval partitioned and the cached form is refused.  The tables here are sized by `capacity`,
not by the stream: 2^18 events over 2^17 keys (Zipf 0.6, more than 50 000 groups) land in 2^25 or
2^26 slots, so uniformly hashed groups sit on both sides of byte offset 2^32.

  create      exactly 4 GiB (ip_key_t, capacity 2^23 + 1) and 8 GiB (2^24 + 1) of key records;
              capacity 2^23 is still narrow
  parity      AUTO (reports the partitioned form), PART and DIRECT on the 8 GiB top-tcp table:
              group count, every row (key | sums | first index) and the top-20 by -sent, -recv
              against the oracle; the slot list crosses byte offset 2^32
  intervals   one interval in 4 chunked updates, a reset and a second interval over the stream's
              next events; partial-group rows merged with an index column in the direct form
  generic     a 128-byte generic key (256-B records, 8 GiB at capacity 2^23 + 1) with an aggregate
              of out_width 4 that wraps
  file        top file's layout at capacity 2^24 + 1: 4 GiB of key records and 4 GiB of value
              records (the claims' plain value-record stores)
  read side   sort after a synchronous and an asynchronous finalize, an IP-text sort key, gather,
              select_ge, lookup and partition, against the oracle and a narrow table of the same
              events
  modes       set_mode(CACHED) is IGX_ENOTSUP on a wide table, which still works afterwards

Tables are created and destroyed one at a time.  A test is skipped only when the device reports
less free memory than its table needs plus 4 GiB (never on an MI355X); on a device with 64 GiB
free such a skip is reported as an xfail instead.
"""
import numpy as np
import pytest

import test_gpu_select_lookup as SL

pytestmark = pytest.mark.gpu

GiB = 1 << 30
N, KEYS, ZIPF = 1 << 18, 1 << 17, 0.6
TCP_W = [16, 16, 8, 4, 16, 2, 2, 2]
FILE_W = [8, 4, 4, 4]
GEN_W = [16] * 8                        # 32 key words: GenericLayout<32>, 256-B records
KSTRIDE = {"tcp": 128, "file": 64, "gen": 256}
VSTRIDE = {"tcp": 32, "file": 64, "gen": 32}
CAP = {"tcp": (1 << 24) + 1, "file": (1 << 24) + 1, "gen": (1 << 23) + 1}   # 8 GiB, 4 + 4 GiB, 8 GiB
_cache = {}


def _nslots(capacity):
    ns = 1024
    while ns * 4 < 8 * capacity:
        ns <<= 1
    return ns


def _table_bytes(name, capacity):
    """device memory of a table: key and value records, the slot list, the occupancy maps"""
    return _nslots(capacity) * (KSTRIDE[name] + VSTRIDE[name] + 4 + 1) + _nslots(capacity) // 8


def _need(torch, nbytes):
    free = torch.cuda.mem_get_info()[0]
    if free >= nbytes + 4 * GiB:
        return
    why = f"{free / GiB:.1f} GiB free, the table needs {nbytes / GiB:.1f} GiB + 4 GiB"
    if free >= 64 * GiB:
        pytest.xfail(why)
    pytest.skip(why)


def _layout(name, igx, oracle, base=0):
    """(host events, device columns, key widths, key column indices, igx aggs, oracle aggs, key names)"""
    if (name, base) in _cache:
        return _cache[name, base]
    E, H, A = igx.engine, igx.columns, igx._abi
    if name == "tcp":
        h = oracle.gen_tcp(0xC2, 0, KEYS, E.zipf_cdf(KEYS, ZIPF), base, N)
        names, knames, widths = SL.TCP_NAMES, SL.TCP_NAMES[:8], TCP_W
        aggs = [A.Agg(A.AGG_SUM, 8, 9, 8, 0), A.Agg(A.AGG_SUM, 8, 9, 8, 1)]
        oaggs = [{"kind": "sum", "val": h["size"], "cond": h["dir"], "cond_val": 0},
                 {"kind": "sum", "val": h["size"], "cond": h["dir"], "cond_val": 1}]
    elif name == "file":
        h = oracle.gen_file(0xC5, 0, KEYS, E.zipf_cdf(KEYS, ZIPF), base, N)
        names, knames, widths = SL.FILE_NAMES, SL.FILE_NAMES[:4], FILE_W
        aggs = [A.Agg(A.AGG_COUNT, 0, 4, 8, 0), A.Agg(A.AGG_SUM, 5, 4, 8, 0),
                A.Agg(A.AGG_COUNT, 0, 4, 8, 1), A.Agg(A.AGG_SUM, 5, 4, 8, 1)]
        oaggs = [{"kind": "count", "cond": h["op"], "cond_val": 0},
                 {"kind": "sum", "val": h["count"], "cond": h["op"], "cond_val": 0},
                 {"kind": "count", "cond": h["op"], "cond_val": 1},
                 {"kind": "sum", "val": h["count"], "cond": h["op"], "cond_val": 1}]
    else:
        # 128 key bytes from a key id: sixteen odd multiples of it, cut into eight 16-byte columns;
        # a u32 value near 2^32, so a 4-byte sum wraps from a key's second event on
        rng = np.random.default_rng(11)
        kid = np.where(rng.random(N) < 0.3, rng.integers(0, 2000, N), rng.integers(0, KEYS, N)).astype(np.uint64)
        mult = (np.arange(16, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0xD1B54A32D192ED03)) | np.uint64(1)
        kb = np.ascontiguousarray((kid[:, None] + np.uint64(1)) * mult[None, :]).view(np.uint8).reshape(N, 8, 16)
        h = {f"k{i}": np.ascontiguousarray(kb[:, i, :]) for i in range(8)}
        h["val"] = rng.integers(1 << 31, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
        knames = tuple(f"k{i}" for i in range(8))
        names, widths = knames + ("val",), GEN_W
        aggs = [A.Agg(A.AGG_COUNT, 0, A.NO_COL, 8, 0), A.Agg(A.AGG_SUM, 8, A.NO_COL, 8, 0),
                A.Agg(A.AGG_SUM, 8, A.NO_COL, 4, 0)]
        oaggs = [{"kind": "count"}, {"kind": "sum", "val": h["val"]},
                 {"kind": "sum", "val": h["val"], "out_width": 4}]
    cols = [H.to_device(h[k]) for k in names]
    _cache[name, base] = (h, cols, widths, list(range(len(knames))), aggs, oaggs, knames)
    return _cache[name, base]


def _ref(name, igx, oracle, base=0):
    """the oracle's rows of the layout's whole stream, computed once"""
    if ("ref", name, base) not in _cache:
        h, _, _, _, _, oaggs, knames = _layout(name, igx, oracle, base)
        _cache["ref", name, base] = SL._ref_rows(oracle, h, knames, oaggs, base=base)
    return _cache["ref", name, base]


def _mode(igx, form):
    A = igx._abi
    return {"auto": A.GB_AUTO, "part": A.GB_PART, "direct": A.GB_DIRECT, "cached": A.GB_CACHED}[form]


def _wide_table(igx, torch, oracle, name, form, capacity=None):
    capacity = capacity or CAP[name]
    widths, aggs = _layout(name, igx, oracle)[2], _layout(name, igx, oracle)[4]
    # the partitioned form's scratch is sized by the rows, the partition buffer by the capacity
    _need(torch, _table_bytes(name, capacity) + 2 * GiB)
    tab = igx.engine.Table(widths, aggs, capacity)
    if form != "auto":
        tab.set_mode(_mode(igx, form))
    return tab


def _rows_and_slots(igx, torch, tab):
    slots = SL._slots(tab, torch)
    return igx.columns.host(tab.gather(slots)), igx.columns.host(slots).astype(np.uint64)


def _assert_crosses(slots, stride, line=1 << 32):
    """the groups' key records lie on both sides of byte offset `line`"""
    off = slots * np.uint64(stride)
    assert (off < np.uint64(line)).any() and (off >= np.uint64(line)).any()
    assert int(off.max()) >= line


def _expect_form(igx, form):
    A = igx._abi
    return A.GB_DIRECT if form == "direct" else A.GB_PART   # AUTO runs partitioned on a wide table


def test_create_at_and_past_4gib(igx, torch, oracle):
    A = igx._abi
    for capacity, want in (((1 << 23) + 1, 4 * GiB), ((1 << 24) + 1, 8 * GiB)):
        tab = _wide_table(igx, torch, oracle, "tcp", "auto", capacity)
        fin = tab.finalize()
        assert fin["n_groups"] == 0
        assert fin["key_stride"] == 128 and fin["n_slots"] * fin["key_stride"] == want
        with pytest.raises(A.IgxError) as e:      # wide: no cached form
            tab.set_mode(A.GB_CACHED)
        assert e.value.code == A.IGX_ENOTSUP
        tab.destroy()
    tab = igx.engine.Table(TCP_W, _layout("tcp", igx, oracle)[4], 1 << 23)
    fin = tab.finalize()
    assert fin["n_slots"] * fin["key_stride"] == 2 * GiB
    tab.set_mode(A.GB_CACHED)                     # narrow: as before
    tab.destroy()


@pytest.mark.parametrize("form", ["auto", "part", "direct"])
def test_parity_8gib_top_tcp(igx, torch, oracle, form):
    A, H = igx._abi, igx.columns
    h, cols, widths, kc, aggs, oaggs, knames = _layout("tcp", igx, oracle)
    ref = _ref("tcp", igx, oracle)
    assert ref.shape[0] > 50_000
    tab = _wide_table(igx, torch, oracle, "tcp", form)
    tab.update(cols, kc, N, 0)
    fin = tab.finalize()
    assert fin["n_slots"] * fin["key_stride"] == 8 * GiB
    assert tab.info()["form"] == _expect_form(igx, form)
    assert fin["n_groups"] == ref.shape[0]
    rows, slots = _rows_and_slots(igx, torch, tab)
    _assert_crosses(slots, fin["key_stride"])
    assert np.array_equal(SL._sorted(rows), SL._sorted(ref))
    # top-20 by -sent, -recv (ties in first-occurrence order)
    top = H.host(tab.gather(tab.sort([(A.TSRC_AGG, 0, True), (A.TSRC_AGG, 1, True)], 20)))
    Gref, okeys, osent, orecv, ofirst = oracle.top_tcp(h, 20)
    assert Gref == fin["n_groups"]
    assert np.array_equal(SL._agg_col(top, 72, 0), osent) and np.array_equal(SL._agg_col(top, 72, 1), orecv)
    assert np.array_equal(SL._agg_col(top, 72, 2), ofirst)
    tab.destroy()


@pytest.mark.parametrize("stress", ["lds_overflow", "region_overflow"])
def test_partitioned_merges_into_the_8gib_table(igx, torch, oracle, monkeypatch, stress):
    """The rows the partitioned form merges into the table with CAS claims (its region-overflow
    and LDS-overflow path, the wide probe) on both sides of byte offset 2^32."""
    A = igx._abi
    if stress == "lds_overflow":
        monkeypatch.setenv("IGX_GBP_ENTRIES", "16")
    else:
        # AUTO runs the region variant; 2^14 final buckets in 2^10 first-level slices: regions of 16
        # records hold 16K of an update's 120K+ rows, the rest spill
        monkeypatch.setenv("IGX_GBP_REGSIZE", "16")
    h, cols, widths, kc, aggs, oaggs, knames = _layout("tcp", igx, oracle)
    tab = _wide_table(igx, torch, oracle, "tcp", "part" if stress == "lds_overflow" else "auto")
    for a, b in ((0, 120_000), (120_000, N)):
        tab.update([c[a:b] for c in cols], kc, b - a, a)
    fin = tab.finalize()
    info = tab.info()
    assert info["form"] == A.GB_PART and info["region"] == (1 if stress == "region_overflow" else 0)
    rows, slots = _rows_and_slots(igx, torch, tab)
    _assert_crosses(slots, fin["key_stride"])
    assert np.array_equal(SL._sorted(rows), SL._sorted(_ref("tcp", igx, oracle)))
    tab.destroy()


@pytest.mark.parametrize("form", ["auto", "part", "direct"])
def test_intervals_chunked_then_shifted(igx, torch, oracle, form):
    H = igx.columns
    h, cols, widths, kc, aggs, oaggs, knames = _layout("tcp", igx, oracle)
    tab = _wide_table(igx, torch, oracle, "tcp", form)
    cuts = [0, 50_004, 131_072, 200_000, N]   # multiples of 4 rows: the u8 / u16 columns stay 4-byte aligned
    for a, b in zip(cuts[:-1], cuts[1:]):
        tab.update([c[a:b] for c in cols], kc, b - a, a)
    fin = tab.finalize()
    assert tab.info()["form"] == _expect_form(igx, form)
    rows, slots = _rows_and_slots(igx, torch, tab)
    _assert_crosses(slots, fin["key_stride"])
    assert np.array_equal(SL._sorted(rows), SL._sorted(_ref("tcp", igx, oracle)))
    # the second interval: the stream's next N events (another, overlapping key window)
    h2, cols2 = _layout("tcp", igx, oracle, base=N)[:2]
    ref2 = _ref("tcp", igx, oracle, base=N)
    assert not np.array_equal(SL._sorted(ref2[:, :72]), SL._sorted(_ref("tcp", igx, oracle)[:, :72]))
    tab.reset()
    tab.update(cols2, kc, N, N)
    tab.finalize()
    assert tab.info()["form"] == _expect_form(igx, form)
    rows2, _ = _rows_and_slots(igx, torch, tab)
    assert np.array_equal(SL._sorted(rows2), SL._sorted(ref2))
    tab.destroy()


def test_direct_merge_of_partial_groups(igx, torch, oracle):
    """Partial-group rows of three shards merged into a wide table with an index column, as
    dist.merge_partials does on an owner."""
    A, E, D = igx._abi, igx.engine, igx.dist
    h, cols, widths, kc, aggs, oaggs, knames = _layout("tcp", igx, oracle)
    parts = []
    for a, b in ((0, 90_000), (90_000, 170_000), (170_000, N)):
        t = E.Table(widths, aggs, KEYS)
        t.update([c[a:b] for c in cols], kc, b - a, a)
        t.finalize()
        parts.append(t.gather(t.sort([(A.TSRC_FIRST, 0, False)], 0)))
        t.destroy()
    # the owner's table (dist.owner_table's aggregates: SUM of each partial), in the direct form
    _need(torch, _table_bytes("tcp", CAP["tcp"]) + 2 * GiB)
    tab = E.Table(widths, [A.Agg(A.AGG_SUM, 8 + x, A.NO_COL, 8, 0) for x in range(2)], CAP["tcp"])
    tab.set_mode(A.GB_DIRECT)
    D.merge_partials(torch.cat(parts), widths, [8, 8], CAP["tcp"], table=tab)
    assert tab.info()["form"] == A.GB_DIRECT
    rows, slots = _rows_and_slots(igx, torch, tab)
    _assert_crosses(slots, 128)
    assert np.array_equal(SL._sorted(rows), SL._sorted(_ref("tcp", igx, oracle)))
    tab.destroy()


@pytest.mark.parametrize("form", ["direct", "part"])
def test_generic_128_byte_key(igx, torch, oracle, form):
    h, cols, widths, kc, aggs, oaggs, knames = _layout("gen", igx, oracle)
    ref = _ref("gen", igx, oracle)
    full = SL._agg_col(SL._ref_rows(oracle, h, knames, [dict(a, out_width=8) for a in oaggs]), 128, 2)
    assert ref.shape[0] > 50_000 and (full >= 1 << 32).any()      # the 4-byte sums do wrap
    tab = _wide_table(igx, torch, oracle, "gen", form)
    tab.update(cols, kc, N, 0)
    fin = tab.finalize()
    assert fin["key_stride"] == 256 and fin["n_slots"] * fin["key_stride"] == 8 * GiB
    assert tab.info()["form"] == _expect_form(igx, form)
    rows, slots = _rows_and_slots(igx, torch, tab)
    _assert_crosses(slots, 256)
    assert int(SL._agg_col(rows, 128, 2).max()) < 1 << 32
    assert np.array_equal(SL._sorted(rows), SL._sorted(ref))
    tab.destroy()


@pytest.mark.parametrize("form", ["auto", "direct", "part"])
def test_file_keys_and_values_past_4gib(igx, torch, oracle, form):
    h, cols, widths, kc, aggs, oaggs, knames = _layout("file", igx, oracle)
    ref = _ref("file", igx, oracle)
    assert ref.shape[0] > 50_000
    tab = _wide_table(igx, torch, oracle, "file", form)
    cuts = [0, 100_000, N]                      # claims and finds of a key span launches
    for a, b in zip(cuts[:-1], cuts[1:]):
        tab.update([c[a:b] for c in cols], kc, b - a, a)
    fin = tab.finalize()
    assert fin["n_slots"] * fin["key_stride"] == 4 * GiB and fin["n_slots"] * fin["val_stride"] == 4 * GiB
    assert tab.info()["form"] == _expect_form(igx, form)
    rows, slots = _rows_and_slots(igx, torch, tab)
    _assert_crosses(slots, 64, 1 << 31)     # exactly 4 GiB: every offset fits 32 bits, the array's size does not
    assert np.array_equal(SL._sorted(rows), SL._sorted(ref))
    tab.destroy()


def _read_side(igx, torch, oracle, tab, sync):
    """what the read-side calls return for the finalized tcp table, as slot-free values"""
    A, H = igx._abi, igx.columns
    out = {}
    # a device top-K straight after the finalize (an asynchronous one keeps the count on the device)
    out["top"] = H.host(tab.gather(tab.sort([(A.TSRC_AGG, 0, True), (A.TSRC_AGG, 1, True)], 20)))
    if not sync:
        tab.wait()
    out["n"] = tab.fin["n_groups"]
    out["full"] = H.host(tab.gather(tab.sort([(A.TSRC_AGG, 1, True), (A.TSRC_KEY, (40, 4, A.KIND_UINT), False)], 0)))
    out["iptext"] = H.host(tab.gather(tab.sort([(A.TSRC_IPTEXT, (0, 68), False), (A.TSRC_AGG, 0, True)], 50)))
    rows = H.host(tab.gather(SL._slots(tab, torch)))
    out["rows"] = SL._sorted(rows)
    v = SL._agg_col(rows, 72, 0)
    med = int(np.sort(v)[len(v) // 2])
    s, n = tab.select_ge(0, med, tab.capacity)
    assert n == int((v >= np.uint64(med)).sum()) == s.numel()
    out["select"] = SL._sorted(H.host(tab.gather(s)))
    assert np.array_equal(out["select"], SL._sorted(rows[v >= np.uint64(med)]))
    SL._check_lookup(igx, torch, tab, 72)
    buf, cnt = tab.partition(8)
    cnt = H.host(cnt)
    assert int(cnt.sum()) == out["n"]
    part = H.host(buf[:int(cnt.sum())])
    ends = np.cumsum(cnt)
    out["parts"] = [SL._sorted(part[e - c:e]) for c, e in zip(cnt, ends)]
    owner = oracle.key_owner(rows[:, :72].copy(), 8)
    for p in range(8):
        assert np.array_equal(out["parts"][p], SL._sorted(rows[owner == p]))
    return out


@pytest.mark.parametrize("sync", [True, False], ids=["sync", "async"])
def test_read_side_against_oracle_and_narrow(igx, torch, oracle, sync):
    A, H = igx._abi, igx.columns
    h, cols, widths, kc, aggs, oaggs, knames = _layout("tcp", igx, oracle)
    ref = _ref("tcp", igx, oracle)
    got = {}
    for which in ("narrow", "wide"):
        if which == "wide":
            tab = _wide_table(igx, torch, oracle, "tcp", "auto")
        else:
            tab = igx.engine.Table(widths, aggs, 2 * KEYS)
            tab.set_mode(A.GB_PART)
        tab.update(cols, kc, N, 0)
        tab.finalize(sync=sync)
        got[which] = _read_side(igx, torch, oracle, tab, sync)
        if which == "wide":
            assert tab.fin["n_slots"] * tab.fin["key_stride"] == 8 * GiB
        tab.destroy()
    w, n = got["wide"], got["narrow"]
    assert w["n"] == n["n"] == ref.shape[0]
    assert np.array_equal(w["rows"], SL._sorted(ref))
    for k in ("top", "full", "iptext", "select"):
        assert np.array_equal(w[k], n[k]), k
    for p in range(8):
        assert np.array_equal(w["parts"][p], n["parts"][p])
    # against the oracle: the top-20, and the IP-text order (ascending text of saddr)
    _, _, osent, orecv, ofirst = oracle.top_tcp(h, 20)
    assert np.array_equal(SL._agg_col(w["top"], 72, 0), osent) and np.array_equal(SL._agg_col(w["top"], 72, 2), ofirst)
    recv = SL._agg_col(w["full"], 72, 1)
    assert len(recv) == ref.shape[0] and (recv[:-1] >= recv[1:]).all()
    fam = w["iptext"][:, 68:70].copy().view(np.uint16).ravel()
    text = [bytes(t) for t in oracle.ip_text_rows(np.ascontiguousarray(w["iptext"][:, :16]), fam)]
    assert text == sorted(text)
    allfam = ref[:, 68:70].copy().view(np.uint16).ravel()
    alltext = sorted(bytes(t) for t in oracle.ip_text_rows(np.ascontiguousarray(ref[:, :16]), allfam))
    assert text[0] == alltext[0] and text[-1] == alltext[49]


def test_mode_handling(igx, torch, oracle):
    A = igx._abi
    h, cols, widths, kc, aggs, oaggs, knames = _layout("tcp", igx, oracle)
    tab = _wide_table(igx, torch, oracle, "tcp", "direct")
    with pytest.raises(A.IgxError) as e:
        tab.set_mode(A.GB_CACHED)
    assert e.value.code == A.IGX_ENOTSUP and "wide" in str(e.value)
    tab.update(cols, kc, N, 0)                    # the refused call left the mode alone
    tab.finalize()
    assert tab.info()["form"] == A.GB_DIRECT
    rows, _ = _rows_and_slots(igx, torch, tab)
    assert np.array_equal(SL._sorted(rows), SL._sorted(_ref("tcp", igx, oracle)))
    tab.set_mode(A.GB_AUTO)
    tab.reset()
    tab.update(cols, kc, N, 0)
    tab.finalize()
    assert tab.info()["form"] == A.GB_PART
    tab.destroy()
    # a narrow table: the cached form as before
    tab = igx.engine.Table(widths, aggs, 2 * KEYS)
    tab.set_mode(A.GB_CACHED)
    tab.update(cols, kc, N, 0)
    tab.finalize()
    assert tab.info()["form"] == A.GB_CACHED
    rows, _ = _rows_and_slots(igx, torch, tab)
    assert np.array_equal(SL._sorted(rows), SL._sorted(_ref("tcp", igx, oracle)))
    tab.destroy()
