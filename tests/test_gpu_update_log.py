"""The cached group-by's update log (k_gb_log.hip; DESIGN.md §4 "The update log").

A cached update of an eligible table streams the sums of the rows that miss the LDS cache to a
per-workgroup log; a partition pass and a per-bucket LDS reduce pass add them to the value
records.  Minima, values of 2^32 or more and whatever finds a region full still go out as atomics.
Every case compares the whole table -- key bytes, every sum, the first index, the group count --
with oracle.groupby, once with the log and once under IGX_GB_LOG=0, and reads
Table.log_stats() (logged records and the value / log-full / bucket-full fallback counts).

The stream: 300 001 top-tcp rows over 20 000 keys at Zipf 1.1 with the bench's two predicates --
more keys than a workgroup's cache has entries, and about a thousand rows per workgroup, so most
rows miss and tens of thousands of records go through both passes.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NMAX = 300_001
GK = 20_000
TCP_NAMES = ("saddr", "daddr", "mntns", "pid", "comm", "lport", "dport", "family", "size", "dir")
TCP_KEY = TCP_NAMES[:8]
TCP_WIDTHS = [16, 16, 8, 4, 16, 2, 2, 2]
FILE_NAMES = ("inode", "dev", "pid", "tid", "op", "count")
C5_CAP = 12_500_000   # the bench's top-file capacity: 2^25 slots x 4 sums do not fit the buckets


@pytest.fixture(scope="module")
def E(igx):
    return igx.engine


@pytest.fixture(scope="module")
def H(igx):
    return igx.columns


@pytest.fixture(scope="module")
def A(igx):
    return igx._abi


def _family_in(A, col):
    p = A.Pred()
    p.col, p.cmp, p.negate, p.ref_len = col, A.CMP_IN, 0, 4
    for i, b in enumerate((2).to_bytes(2, "little") + (10).to_bytes(2, "little")):
        p.ref[i] = b
    return p


def _copied(A, col, dir_col):
    p = A.Pred()
    p.col, p.cmp, p.negate, p.ref_len = col, A.CMP_GT, 0, 4
    p.guard_col, p.guard_len, p.guard_ref[0] = dir_col, 1, 1
    return p


@pytest.fixture(scope="module")
def tcp(oracle, H, torch):
    O = oracle
    ev = O.gen_tcp(0x109, 0, GK, O.zipf_cdf(GK, 1.1), 0, NMAX)
    ev["family"][6::7] = 3
    ev["size"][5::13] = 0
    keep = np.isin(ev["family"], (2, 10)) & ~((ev["dir"] == 1) & (ev["size"].view(np.int32) <= 0))
    dev = {k: H.to_device(v) for k, v in ev.items()}
    return {"h": ev, "d": dev, "keep": keep, "keys": O.pad_keys(ev, TCP_KEY)}


def _cols(torch, d, a, b):
    return [d[k][a:b] for k in TCP_NAMES] + [d["size"][a:b].view(torch.int32)]


def _preds(A):
    return [_family_in(A, 7), _copied(A, 10, 9)]


def _tcp_table(E, A, cap=2 * GK):
    t = E.Table(TCP_WIDTHS, [A.Agg(A.AGG_SUM, 8, 9, 8, 0), A.Agg(A.AGG_SUM, 8, 9, 8, 1)], cap)
    t.set_mode(A.GB_CACHED)
    return t


def _read(E, H, tab, fin):
    keys, aggs, first = E.table_tensors(tab, fin)
    hk, ha, hf = H.host(keys), [H.host(a) for a in aggs], H.host(first)
    got = {hk[i].tobytes(): tuple(int(a[i]) for a in ha) + (int(hf[i]),) for i in range(len(hk))}
    assert len(got) == len(hk), "duplicate groups"
    return got


def _table(E, H, tab):
    fin = tab.finalize()
    return _read(E, H, tab, fin), fin["n_groups"]


def _want(oracle, keys, aggs, keep, base=0):
    if len(keys) == 0:
        return {}
    ok, oa, of = oracle.groupby(keys, aggs, valid=keep, base_idx=base)
    return {ok[i].tobytes(): tuple(int(a[i]) for a in oa[:len(aggs)]) + (int(of[i]),) for i in range(len(ok))}


def _tcp_aggs(h, a, b, val="size"):
    return [{"kind": "sum", "val": h[val][a:b], "cond": h["dir"][a:b], "cond_val": 0},
            {"kind": "sum", "val": h[val][a:b], "cond": h["dir"][a:b], "cond_val": 1}]


def _both(monkeypatch, run):
    """run() with the log and under IGX_GB_LOG=0; returns the logged run's counters."""
    monkeypatch.delenv("IGX_GB_LOG", raising=False)
    on = run()
    monkeypatch.setenv("IGX_GB_LOG", "0")
    off = run()
    assert off == {"logged": 0, "fallback_value": 0, "fallback_log_full": 0, "fallback_bucket_full": 0}
    return on


@pytest.fixture(scope="module")
def want_all(oracle, tcp):
    return _want(oracle, tcp["keys"], _tcp_aggs(tcp["h"], 0, NMAX), tcp["keep"])


def test_stream_goes_through_the_log(E, H, A, torch, monkeypatch, tcp, want_all, oracle):
    n = 300_000
    want = _want(oracle, tcp["keys"][:n], _tcp_aggs(tcp["h"], 0, n), tcp["keep"][:n])
    tab = _tcp_table(E, A)

    def run():
        tab.reset()
        tab.update(_cols(torch, tcp["d"], 0, n), list(range(8)), n, 0, _preds(A))
        got, ng = _table(E, H, tab)
        assert ng == len(want) and got == want
        return tab.log_stats()

    try:
        st = _both(monkeypatch, run)
        assert st["logged"] > 20_000, st
        assert st["fallback_value"] == st["fallback_log_full"] == st["fallback_bucket_full"] == 0, st
    finally:
        tab.destroy()


@pytest.mark.parametrize("n", [0, 1, 63, 1000, NMAX])
def test_row_counts(E, H, A, torch, monkeypatch, tcp, want_all, oracle, n):
    want = want_all if n == NMAX else _want(oracle, tcp["keys"][:n], _tcp_aggs(tcp["h"], 0, n), tcp["keep"][:n])
    tab = _tcp_table(E, A)

    def run():
        tab.reset()
        tab.update(_cols(torch, tcp["d"], 0, n), list(range(8)), n, 0, _preds(A))
        got, ng = _table(E, H, tab)
        assert ng == len(want) and got == want
        return tab.log_stats()

    try:
        st = _both(monkeypatch, run)
        assert st["fallback_log_full"] == st["fallback_bucket_full"] == 0, st
    finally:
        tab.destroy()


def test_three_updates_one_interval(E, H, A, torch, monkeypatch, tcp, want_all):
    tab = _tcp_table(E, A)
    # a large, a sub-wave and a larger update (the scratch grows); cuts at multiples of 4 rows, as
    # the 1- and 2-byte columns must start 4-byte aligned
    cuts = (0, 100_000, 100_060, NMAX)

    def run():
        tab.reset()
        for a, b in zip(cuts, cuts[1:]):
            tab.update(_cols(torch, tcp["d"], a, b), list(range(8)), b - a, a, _preds(A))
        got, ng = _table(E, H, tab)
        assert ng == len(want_all) and got == want_all
        return tab.log_stats()

    try:
        st = _both(monkeypatch, run)
        assert st["logged"] > 20_000 and st["fallback_log_full"] == st["fallback_bucket_full"] == 0, st
    finally:
        tab.destroy()


def test_three_intervals_kept_keys_async(E, H, A, torch, monkeypatch, tcp, oracle):
    """reset / update / finalize(sync=False) / top-K, three times on one table, as bench.py steps."""
    n = 100_000
    wants = [_want(oracle, tcp["keys"][i * n:(i + 1) * n], _tcp_aggs(tcp["h"], i * n, (i + 1) * n),
                   tcp["keep"][i * n:(i + 1) * n], i * n) for i in range(3)]
    tab = _tcp_table(E, A)

    def run():
        logged = 0
        for i in range(3):
            tab.reset()
            tab.update(_cols(torch, tcp["d"], i * n, (i + 1) * n), list(range(8)), n, i * n, _preds(A))
            fin = tab.finalize(sync=False)
            tab.gather(tab.sort([(A.TSRC_AGG, 0, True), (A.TSRC_AGG, 1, True)], 20))
            ng = tab.wait()
            fin = dict(fin, n_groups=ng)
            assert ng == len(wants[i]) and _read(E, H, tab, fin) == wants[i]
            st = tab.log_stats()
            assert st["fallback_log_full"] == st["fallback_bucket_full"] == 0, st
            logged += st["logged"]
        return logged

    try:
        monkeypatch.delenv("IGX_GB_LOG", raising=False)
        assert run() > 20_000
        monkeypatch.setenv("IGX_GB_LOG", "0")
        assert run() == 0
    finally:
        tab.destroy()


def test_large_values_take_the_atomics(E, H, A, torch, monkeypatch, tcp, oracle):
    """An 8-byte value column, a third of its values >= 2^32: both paths in one update."""
    n = 100_000
    h = tcp["h"]
    size64 = h["size"][:n].astype(np.uint64)
    size64[::3] += np.uint64(1) << np.uint64(32)
    cols = _cols(torch, tcp["d"], 0, n)
    cols[8] = H.to_device(size64)
    cols[10] = tcp["d"]["size"][:n].clone().view(torch.int32)   # `copied` stays the 4-byte column
    want = _want(oracle, tcp["keys"][:n], _tcp_aggs({"size": size64, "dir": h["dir"][:n]}, 0, n), tcp["keep"][:n])
    tab = _tcp_table(E, A)

    def run():
        tab.reset()
        tab.update(cols, list(range(8)), n, 0, _preds(A))
        got, ng = _table(E, H, tab)
        assert ng == len(want) and got == want
        return tab.log_stats()

    try:
        st = _both(monkeypatch, run)
        assert st["logged"] > 0 and st["fallback_value"] > 0, st
    finally:
        tab.destroy()


@pytest.mark.parametrize("knob,field", [("IGX_GB_LOG_CAP", "fallback_log_full"),
                                        ("IGX_GB_LOG_BCAP", "fallback_bucket_full")])
def test_full_regions_fall_back(E, H, A, torch, monkeypatch, tcp, want_all, knob, field):
    tab = _tcp_table(E, A)

    def run():
        tab.reset()
        tab.update(_cols(torch, tcp["d"], 0, NMAX), list(range(8)), NMAX, 0, _preds(A))
        got, ng = _table(E, H, tab)
        assert ng == len(want_all) and got == want_all
        return tab.log_stats()

    try:
        monkeypatch.setenv(knob, "64" if knob == "IGX_GB_LOG_CAP" else "16")
        st = _both(monkeypatch, run)
        assert st[field] > 0, st
        if knob == "IGX_GB_LOG_CAP":
            assert st["fallback_log_full"] > st["logged"], st
    finally:
        tab.destroy()


def test_index_column_update(E, H, A, torch, monkeypatch, tcp, oracle):
    """The owner merge's shape: key columns, two u64 partial sums, a u64 first-index column."""
    n = 50_000
    h = tcp["h"]
    rng = np.random.default_rng(0x10C)
    p0 = rng.integers(0, 1 << 20, n, dtype=np.uint64)
    p1 = rng.integers(0, 1 << 31, n, dtype=np.uint64)
    idx = rng.permutation(n).astype(np.uint64) + np.uint64(7)
    ok, oa, _ = oracle.groupby(tcp["keys"][:n], [{"kind": "sum", "val": p0}, {"kind": "sum", "val": p1}])
    _, inv = np.unique(np.ascontiguousarray(tcp["keys"][:n]).view(np.dtype((np.void, tcp["keys"].shape[1]))).ravel(),
                       return_inverse=True)
    fmin = np.full(inv.max() + 1, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(fmin, inv, idx)
    first_of = {tcp["keys"][i].tobytes(): int(fmin[inv[i]]) for i in range(n)}
    want = {ok[i].tobytes(): (int(oa[0][i]), int(oa[1][i]), first_of[ok[i].tobytes()]) for i in range(len(ok))}
    cols = [tcp["d"][k][:n] for k in TCP_KEY] + [H.to_device(p0), H.to_device(p1), H.to_device(idx)]
    tab = E.Table(TCP_WIDTHS, [A.Agg(A.AGG_SUM, 8, A.NO_COL, 8, 0), A.Agg(A.AGG_SUM, 9, A.NO_COL, 8, 0)], 2 * GK)
    tab.set_mode(A.GB_CACHED)

    def run():
        tab.reset()
        tab.update(cols, list(range(8)), n, 0, idx_col=10)
        got, ng = _table(E, H, tab)
        assert ng == len(want) and got == want
        return tab.log_stats()

    try:
        st = _both(monkeypatch, run)
        assert st["logged"] > 0 and st["fallback_log_full"] == st["fallback_bucket_full"] == 0, st
    finally:
        tab.destroy()


def test_top_file_capacity_is_ineligible(E, H, A, monkeypatch, oracle):
    """The top-file layout at the bench's capacity: too many (slot, aggregate) sums for the buckets."""
    n = 200_000
    O = oracle
    ev = O.gen_file(0x10F, 0, GK, O.zipf_cdf(GK, 1.05), 0, n)
    aggs = [{"kind": "count", "cond": ev["op"], "cond_val": 0},
            {"kind": "sum", "val": ev["count"], "cond": ev["op"], "cond_val": 0},
            {"kind": "count", "cond": ev["op"], "cond_val": 1},
            {"kind": "sum", "val": ev["count"], "cond": ev["op"], "cond_val": 1}]
    want = _want(O, O.pad_keys(ev, FILE_NAMES[:4]), aggs, None)
    cols = [H.to_device(ev[k]) for k in FILE_NAMES]
    spec = [A.Agg(A.AGG_COUNT, 0, 4, 8, 0), A.Agg(A.AGG_SUM, 5, 4, 8, 0),
            A.Agg(A.AGG_COUNT, 0, 4, 8, 1), A.Agg(A.AGG_SUM, 5, 4, 8, 1)]
    monkeypatch.delenv("IGX_GB_LOG", raising=False)
    tab = E.Table([8, 4, 4, 4], spec, C5_CAP)
    try:
        tab.set_mode(A.GB_CACHED)
        tab.update(cols, [0, 1, 2, 3], n, 0)
        got, ng = _table(E, H, tab)
        assert ng == len(want) and got == want
        assert tab.log_stats()["logged"] == 0
    finally:
        tab.destroy()
