"""IGX_GB_WIDE=1: the wide (64-bit record addressing) instances on narrow-sized tables.

The knob is read by igx_groupby_create and gives a table of any size the kernel instances a table
past 4 GiB of key records runs (tests/test_gpu_wide_table.py), so the same code is checked here on
the three layouts and the shapes of tests/test_gpu_select_lookup.py -- 200 000 events over 20 000
keys, and a capacity equal to the number of keys (long probe chains, region wrap) -- with little
memory.  Every table must equal the oracle in the direct and the partitioned form; AUTO runs
partitioned and the cached form is refused, as on any wide table.
"""
import numpy as np
import pytest

import test_gpu_select_lookup as SL

pytestmark = pytest.mark.gpu

_ref = {}


def _ref_rows(oracle, igx, name):
    if name not in _ref:
        h, _, _, _, _, oaggs, knames = SL._layout(name, igx, oracle)
        _ref[name] = SL._ref_rows(oracle, h, knames, oaggs)
    return _ref[name]


def _modes(igx):
    A = igx._abi
    return {"direct": A.GB_DIRECT, "part": A.GB_PART, "auto": A.GB_AUTO}


def _is_wide(igx, tab):
    """a wide table refuses the cached form (and keeps its mode)"""
    A = igx._abi
    try:
        tab.set_mode(A.GB_CACHED)
    except A.IgxError as e:
        assert e.code == A.IGX_ENOTSUP
        return True
    return False


@pytest.mark.parametrize("fit", ["roomy", "tight"])
@pytest.mark.parametrize("form", ["direct", "part"])
@pytest.mark.parametrize("name", ["file", "tcp", "generic"])
def test_wide_instances_equal_oracle(igx, torch, oracle, monkeypatch, name, form, fit):
    H = igx.columns
    monkeypatch.setenv("IGX_GB_WIDE", "1")
    ref = _ref_rows(oracle, igx, name)
    widths = SL._layout(name, igx, oracle)[2]
    kb = sum((w + 3) // 4 * 4 for w in widths)
    tab = igx.engine.Table(widths, SL._layout(name, igx, oracle)[4], ref.shape[0] if fit == "tight" else 25_000)
    assert _is_wide(igx, tab)
    tab.set_mode(_modes(igx)[form])
    SL._table(igx, oracle, name, tab=tab)              # reset, one update of all rows, finalize
    assert tab.info()["form"] == _modes(igx)[form]
    assert tab.fin["n_groups"] == ref.shape[0]
    rows = H.host(SL._check_lookup(igx, torch, tab, kb))
    assert np.array_equal(SL._sorted(rows), SL._sorted(ref))
    tab.destroy()


@pytest.mark.parametrize("stress", ["lds_overflow", "region_overflow"])
@pytest.mark.parametrize("name", ["file", "tcp", "generic"])
def test_partitioned_merges_into_the_table(igx, torch, oracle, monkeypatch, name, stress):
    """The partitioned form's rows that leave its LDS path are merged into the table with CAS
    claims (the wide probe): a pass-C table of 16 entries overflows on nearly every group, and
    regions of 600 records overflow in passes A and B of the region variant."""
    A, H = igx._abi, igx.columns
    monkeypatch.setenv("IGX_GB_WIDE", "1")
    if stress == "lds_overflow":
        monkeypatch.setenv("IGX_GBP_ENTRIES", "16")
    else:
        monkeypatch.setenv("IGX_GBP_REGION", "1")
        monkeypatch.setenv("IGX_GBP_REGSIZE", "600")
    ref = _ref_rows(oracle, igx, name)
    h, cols, widths, kc, aggs, oaggs, knames = SL._layout(name, igx, oracle)
    tab = igx.engine.Table(widths, aggs, 25_000)
    assert _is_wide(igx, tab)
    tab.set_mode(A.GB_PART)
    for a, b in ((0, 120_000), (120_000, SL.N)):
        tab.update([c[a:b] for c in cols], kc, b - a, a)
    tab.finalize()
    info = tab.info()
    assert info["form"] == A.GB_PART and info["region"] == (1 if stress == "region_overflow" else 0)
    got = H.host(tab.gather(SL._slots(tab, torch)))
    assert np.array_equal(SL._sorted(got), SL._sorted(ref))
    tab.destroy()


@pytest.mark.parametrize("form", ["direct", "part", "auto"])
def test_wide_instances_over_intervals(igx, torch, oracle, monkeypatch, form):
    """claims and finds of the same keys across launches, then a reset and another interval"""
    A, H = igx._abi, igx.columns
    monkeypatch.setenv("IGX_GB_WIDE", "1")
    monkeypatch.setenv("IGX_GB_MODE", "1")             # must not force the cached form on a wide table
    h, cols, widths, kc, aggs, oaggs, knames = SL._layout("file", igx, oracle)
    tab = igx.engine.Table(widths, aggs, 25_000)
    monkeypatch.delenv("IGX_GB_MODE")
    assert _is_wide(igx, tab)
    tab.set_mode(_modes(igx)[form])
    cuts = [0, 40_000, 100_000, 160_000, SL.N]
    for a, b in zip(cuts[:-1], cuts[1:]):
        tab.update([c[a:b] for c in cols], kc, b - a, a)
    tab.finalize()
    assert tab.info()["form"] == (A.GB_DIRECT if form == "direct" else A.GB_PART)
    got = H.host(tab.gather(SL._slots(tab, torch)))
    assert np.array_equal(SL._sorted(got), SL._sorted(_ref_rows(oracle, igx, "file")))
    half = np.arange(0, SL.N, 2)
    SL._table(igx, oracle, "file", rows=half, tab=tab)
    got = H.host(tab.gather(SL._slots(tab, torch)))
    assert np.array_equal(SL._sorted(got), SL._sorted(SL._ref_rows(oracle, h, knames, oaggs, rows=half)))
    tab.destroy()


def test_knob_off_is_narrow(igx, torch, oracle, monkeypatch):
    A = igx._abi
    monkeypatch.setenv("IGX_GB_WIDE", "0")
    h, cols, widths, kc, aggs, oaggs, knames = SL._layout("file", igx, oracle)
    tab = igx.engine.Table(widths, aggs, 25_000)
    assert not _is_wide(igx, tab)                      # the cached form was accepted
    SL._table(igx, oracle, "file", tab=tab)
    assert tab.info()["form"] == A.GB_CACHED
    tab.destroy()


def test_owner_table_falls_back_to_auto(igx, torch, oracle, monkeypatch):
    """dist.owner_table prefers the cached form; on a wide table it stays in AUTO (partitioned)
    and dist.merge_partials merges partial groups into it all the same."""
    A, D, H = igx._abi, igx.dist, igx.columns
    h, cols, widths, kc, aggs, oaggs, knames = SL._layout("file", igx, oracle)
    src = SL._table(igx, oracle, "file")                # a narrow table: the partial groups
    rows = src.gather(SL._slots(src, torch))
    src.destroy()
    monkeypatch.setenv("IGX_GB_WIDE", "1")
    own = D.owner_table(widths, [8, 8, 8, 8], 25_000)
    assert _is_wide(igx, own)
    D.merge_partials(rows, widths, [8, 8, 8, 8], 25_000, table=own)
    assert own.info()["form"] == A.GB_PART
    got = H.host(own.gather(SL._slots(own, torch)))
    assert np.array_equal(SL._sorted(got), SL._sorted(_ref_rows(oracle, igx, "file")))
    own.destroy()

