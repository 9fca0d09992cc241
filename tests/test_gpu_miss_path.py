"""The cached group-by's miss path (k_gb_cached.hip; DESIGN.md §4 "The miss path").

A loader that misses the LDS cache tells the prober whether the key's set is closed -- all 8 tags
set, none the key's -- and a closed miss skips the second cache lookup, the admission filter and
the adoption attempt: it goes straight to the HBM probe and then to the update ring.  Whatever
path a row takes, its sums are added and its index is a candidate minimum, so every case compares
the whole table -- key bytes, every sum, the first index, the group count -- with oracle.groupby.

The stream is tests/test_gpu_update_log.py's: 300 001 top-tcp rows over 20 000 keys at Zipf 1.1
with the bench's two predicates, about a thousand rows per workgroup.  With the second-miss
admission filter so few rows adopt about a hundred keys per workgroup into some 130 sets, and no
set fills.  Every kept-key interval here runs seeded (IGX_GB_SEED_MIN=1, as
tests/test_gpu_persist.py sets it; the default asks for 8M rows), which puts up to a cache's worth
of keys into the sets before the first row -- but seeds that race for one entry of a set lose and
are dropped, and few sets reach eight: the counting debug kernel reports 16-48 closed misses in
some 170 000 on such an interval.  So at these sizes the cases run the changed code -- the lookup
that computes the bit, the cell that carries it, the probers that test it -- almost always with
the bit clear.  test_closed_misses_are_counted feeds four times the rows (7 500-8 400 closed
misses in 425 000 under either prober), asserts that there were some and that the table is exact; the bit set on a large share of
the misses is what tests/test_gpu_fullsize.py's 100M-row intervals run.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NMAX = 300_001
GK = 20_000
TCP_NAMES = ("saddr", "daddr", "mntns", "pid", "comm", "lport", "dport", "family", "size", "dir")
TCP_KEY = TCP_NAMES[:8]
TCP_WIDTHS = [16, 16, 8, 4, 16, 2, 2, 2]
FILE_NAMES = ("inode", "dev", "pid", "tid", "op", "count")
C5_CAP = 12_500_000   # the bench's top-file capacity: not eligible for the update log
NO_FALLBACK = ("fallback_value", "fallback_log_full", "fallback_bucket_full")


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


def _preds(A):
    return [_family_in(A, 7), _copied(A, 10, 9)]


def _keep(ev):
    return np.isin(ev["family"], (2, 10)) & ~((ev["dir"] == 1) & (ev["size"].view(np.int32) <= 0))


def _stream(O, H, ev):
    return {"h": ev, "d": {k: H.to_device(v) for k, v in ev.items()}, "keep": _keep(ev),
            "keys": O.pad_keys(ev, TCP_KEY)}


@pytest.fixture(scope="module")
def tcp(oracle, H):
    O = oracle
    ev = O.gen_tcp(0x109, 0, GK, O.zipf_cdf(GK, 1.1), 0, NMAX)
    ev["family"][6::7] = 3
    ev["size"][5::13] = 0
    return _stream(O, H, ev)


def _cols(torch, d, a, b):
    return [d[k][a:b] for k in TCP_NAMES] + [d["size"][a:b].view(torch.int32)]


def _tcp_table(E, A, cap=2 * GK):
    t = E.Table(TCP_WIDTHS, [A.Agg(A.AGG_SUM, 8, 9, 8, 0), A.Agg(A.AGG_SUM, 8, 9, 8, 1)], cap)
    t.set_mode(A.GB_CACHED)
    return t


def _table(E, H, tab):
    fin = tab.finalize()
    keys, aggs, first = E.table_tensors(tab, fin)
    hk, ha, hf = H.host(keys), [H.host(a) for a in aggs], H.host(first)
    got = {hk[i].tobytes(): tuple(int(a[i]) for a in ha) + (int(hf[i]),) for i in range(len(hk))}
    assert len(got) == len(hk), "duplicate groups"
    return got, fin["n_groups"]


def _want(oracle, keys, aggs, keep, base=0):
    ok, oa, of = oracle.groupby(keys, aggs, valid=keep, base_idx=base)
    return {ok[i].tobytes(): tuple(int(a[i]) for a in oa[:len(aggs)]) + (int(of[i]),) for i in range(len(ok))}


def _tcp_aggs(val, dirs):
    return [{"kind": "sum", "val": val, "cond": dirs, "cond_val": 0},
            {"kind": "sum", "val": val, "cond": dirs, "cond_val": 1}]


def _want_slice(oracle, s, a, b, base=None):
    return _want(oracle, s["keys"][a:b], _tcp_aggs(s["h"]["size"][a:b], s["h"]["dir"][a:b]), s["keep"][a:b],
                 a if base is None else base)


def _interval(E, H, A, torch, tab, s, a, b, want):
    tab.reset()
    tab.update(_cols(torch, s["d"], a, b), list(range(8)), b - a, a, _preds(A))
    got, ng = _table(E, H, tab)
    assert ng == len(want) and got == want
    return tab.log_stats()


@pytest.fixture(scope="module")
def want_all(oracle, tcp):
    return _want_slice(oracle, tcp, 0, NMAX)


@pytest.fixture(scope="module")
def long(oracle, H, tcp):
    """The stream four times over, 1 200 000 rows: about 4 700 rows per workgroup."""
    ev = {k: np.concatenate([v[:300_000]] * 4) for k, v in tcp["h"].items()}
    s = _stream(oracle, H, ev)
    s["want"] = _want_slice(oracle, s, 0, 1_200_000)
    return s


@pytest.fixture
def seeded(monkeypatch):
    monkeypatch.delenv("IGX_GB_LOG", raising=False)
    monkeypatch.delenv("IGX_GB_DEBUG", raising=False)
    monkeypatch.setenv("IGX_GB_SEED_MIN", "1")
    return monkeypatch


def _debug_counts(tab):
    cnt = (ctypes.c_uint64 * 32)()
    tab.ctx.check(tab.ctx.L.igx_groupby_debug_counts(tab.h, cnt))
    return {"hits": cnt[0], "misses": cnt[1], "closed": cnt[2]}


@pytest.mark.parametrize("log", ["1", "0"])
def test_three_intervals_on_kept_keys(E, H, A, torch, seeded, tcp, want_all, log):
    """Interval 1 claims its keys with a cold, unseeded cache (there is nothing to look seeds up
    in); 2 and 3 find kept keys and run seeded.  The server wave logs the sums, or with IGX_GB_LOG=0
    issues them."""
    if log == "0":
        seeded.setenv("IGX_GB_LOG", "0")
    tab = _tcp_table(E, A)
    try:
        for i in range(3):
            st = _interval(E, H, A, torch, tab, tcp, 0, NMAX, want_all)
            print("interval", i, st)
            assert all(st[f] == 0 for f in NO_FALLBACK), st
            assert (st["logged"] > 0) == (log == "1"), st
    finally:
        tab.destroy()


@pytest.mark.parametrize("sm", ["0", "1"])
def test_closed_misses_are_counted(E, H, A, torch, seeded, long, sm):
    """Closure made visible, under the batch prober and under the state-machine prober
    (IGX_GB_PROBER sets GbArgs::sm directly), on 1 200 000 rows.  Interval 1 claims the keys.
    Interval 2 runs the debug kernel, which with IGX_GB_DEBUG=8 only counts and is seeded like the
    production kernel: it is exact, and igx_groupby_debug_counts reports the misses whose cell
    carried the bit.  Interval 3 is the production kernel on the same seeds.

    Only `closed > 0` is asserted.  How many sets fill depends on which seeds win their entry and
    on the order of adoptions, and nothing bounds it from below but the count itself; each figure is
    printed."""
    n = 1_200_000
    seeded.setenv("IGX_GB_PROBER", sm)
    tab = _tcp_table(E, A)
    try:
        _interval(E, H, A, torch, tab, long, 0, n, long["want"])
        seeded.setenv("IGX_GB_DEBUG", "8")
        _debug_counts(tab)   # clears the counters
        _interval(E, H, A, torch, tab, long, 0, n, long["want"])
        cnt = _debug_counts(tab)
        print("sm", sm, cnt)
        assert cnt["hits"] + cnt["misses"] == int(long["keep"].sum()), cnt
        assert 0 < cnt["closed"] <= cnt["misses"], cnt
        seeded.delenv("IGX_GB_DEBUG")
        st = _interval(E, H, A, torch, tab, long, 0, n, long["want"])
        assert st["logged"] > 0 and all(st[f] == 0 for f in NO_FALLBACK), st
    finally:
        tab.destroy()


def test_state_machine_prober(E, H, A, torch, seeded, oracle, tcp, want_all):
    """200 000 rows of all-distinct keys, two intervals (the first claims every key, the second
    finds every key kept; nothing is ever adopted, so no set closes), then two intervals of the
    Zipf stream on the same table: its keys are new in the first and kept, with seeds, in the
    second.  All through prober_sm: the table picks that prober by itself only after an
    interval of a million rows or more with over 70 % misses, so at this size the test picks it,
    with the library's own IGX_GB_PROBER=1, which sets GbArgs::sm whatever the table prefers."""
    O = oracle
    n = 200_000
    seeded.setenv("IGX_GB_PROBER", "1")
    ev = {k: v[:n].copy() for k, v in tcp["h"].items()}
    ev["pid"][:] = np.arange(n, dtype=ev["pid"].dtype)
    ev["mntns"][:] = np.arange(n, dtype=ev["mntns"].dtype) * 7 + 1
    s = _stream(O, H, ev)
    want = _want_slice(O, s, 0, n)
    assert len(want) == int(s["keep"].sum())
    tab = _tcp_table(E, A, cap=2 * n + 2 * GK)
    try:
        _interval(E, H, A, torch, tab, s, 0, n, want)
        st = _interval(E, H, A, torch, tab, s, 0, n, want)
        assert st["logged"] > 0, st
        _interval(E, H, A, torch, tab, tcp, 0, NMAX, want_all)
        _interval(E, H, A, torch, tab, tcp, 0, NMAX, want_all)
    finally:
        tab.destroy()


def test_table_the_log_does_not_take(E, H, A, seeded, oracle):
    """Top-file keys at the bench's capacity, two intervals, the second seeded: the ring carries
    every update as an atomic."""
    n = 300_000
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
    tab = E.Table([8, 4, 4, 4], spec, C5_CAP)
    try:
        tab.set_mode(A.GB_CACHED)
        for _ in range(2):
            tab.reset()
            tab.update(cols, [0, 1, 2, 3], n, 0)
            got, ng = _table(E, H, tab)
            assert ng == len(want) and got == want
            assert tab.log_stats()["logged"] == 0
    finally:
        tab.destroy()


def test_large_values_and_minima(E, H, A, torch, seeded, oracle, tcp):
    """Every 13th size 2^32 - 1 (the largest value a record holds), every 17th zero (nothing to
    add: only its minimum travels); then the value as an 8-byte column with 2^33 on every 11th
    row, which no record holds.  Interval 1 claims the keys; the two checked intervals run on kept
    keys with seeds.  Keys of the tail have only missing rows: their first index
    is whatever the ring's minima made it."""
    O = oracle
    n = 300_000
    ev = {k: v[:n].copy() for k, v in tcp["h"].items()}
    ev["size"][::13] = 0xFFFFFFFF
    ev["size"][::17] = 0
    s = _stream(O, H, ev)
    want = _want_slice(O, s, 0, n)
    val64 = ev["size"].astype(np.uint64)
    val64[::11] = np.uint64(1) << np.uint64(33)
    want64 = _want(O, s["keys"], _tcp_aggs(val64, ev["dir"]), s["keep"])
    cols64 = _cols(torch, s["d"], 0, n)
    cols64[8] = H.to_device(val64)
    cols64[10] = s["d"]["size"].clone().view(torch.int32)   # `copied` stays the 4-byte column
    tab = _tcp_table(E, A)
    try:
        _interval(E, H, A, torch, tab, s, 0, n, want)
        st = _interval(E, H, A, torch, tab, s, 0, n, want)
        assert st["logged"] > 0 and all(st[f] == 0 for f in NO_FALLBACK), st
        tab.reset()
        tab.update(cols64, list(range(8)), n, 0, _preds(A))
        got, ng = _table(E, H, tab)
        assert ng == len(want64) and got == want64
        st = tab.log_stats()
        assert st["logged"] > 0 and st["fallback_value"] > 0, st
    finally:
        tab.destroy()
