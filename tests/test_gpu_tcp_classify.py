"""igx_tcp_classify on the device against the restatement in tests/tcptracer_ref.py, over the
exhaustive small field table that tests/sanitize/tcptrace_main.cpp walks on the CPU (4608 rows:
every probe with its ret / state cases, three families, every tuple field zero or not in each
position): tuple bytes, kind and event of every row, without a filter, with each filter alone, with
all of them, and with a mount-namespace set of 1, 2 and 1024 ids."""
import numpy as np
import pytest

import tcptracer_ref as R

pytestmark = pytest.mark.gpu

BIG = np.arange(1024, dtype=np.uint64) * np.uint64(2) + np.uint64(4026532000)      # the even ids
FILTERS = {
    "none": {},
    "pid": {"filter_pid": 12},
    "uid0": {"filter_uid": 0},
    "mntns1": {"mntns": np.array([4026532003], np.uint64)},
    "mntns2": {"mntns": np.array([4026532001, 4026532010], np.uint64)},
    "mntns1024": {"mntns": BIG},
    "all": {"filter_pid": 14, "filter_uid": 2, "mntns": BIG},
}


@pytest.fixture(scope="module")
def table():
    return R.field_table()


@pytest.fixture(scope="module")
def device_table(igx, table):
    return {f: igx.columns.to_device(table[f]) for f in R.FIELDS}


@pytest.mark.parametrize("name", list(FILTERS))
def test_field_table(igx, table, device_table, name):
    H = igx.columns
    flt = FILTERS[name]
    want = R.classify(table, **flt)
    n = len(table["probe"])
    assert n == 4608
    # the case is not vacuous: the filter passes some filtered probes' rows and drops others
    base = R.classify(table)
    assert 0 < int((want["kind"] == R.ENTER).sum()) and 0 < int((want["event"] != 0).sum())
    if flt:
        assert int((want["kind"] == R.ENTER).sum()) < int((base["kind"] == R.ENTER).sum())
        assert int((want["event"] != 0).sum()) < int((base["event"] != 0).sum())
    # the unfiltered probes are the same under every filter
    for k in (R.PASS, R.ABORT, R.TAKE, R.DROP):
        assert int((want["kind"] == k).sum()) == int((base["kind"] == k).sum()) > 0
    dev = dict(flt)
    if "mntns" in dev:
        dev["mntns_set"] = H.to_device(dev.pop("mntns"))
    got = igx.engine.tcp_classify(device_table, **dev)
    assert np.array_equal(H.host(got["kind"]), want["kind"])
    assert np.array_equal(H.host(got["event"]), want["event"])
    assert np.array_equal(H.host(got["tuple"]), want["tuple"])
    assert np.array_equal(H.host(got["key1"]).view(np.uint64), want["key1"])


def test_zero_rows_and_argument_checks(igx, torch, device_table):
    ctx = igx.runtime.context()
    empty = {f: device_table[f][:0] for f in R.FIELDS}
    got = igx.engine.tcp_classify(empty)
    assert got["kind"].numel() == 0 and tuple(got["tuple"].shape) == (0, 40)
    with pytest.raises(igx._abi.IgxError) as e:
        igx.engine.tcp_classify(device_table, mntns_set=torch.zeros(1025, dtype=torch.int64, device="cuda"))
    assert e.value.code == igx._abi.IGX_EINVAL and "1024" in str(e.value)
    shifted = dict(device_table, saddr=device_table["saddr"].flatten()[8:-8].view(-1, 16))
    with pytest.raises(igx._abi.IgxError) as e:
        igx.engine.tcp_classify(dict({f: device_table[f][:-1] for f in R.FIELDS}, saddr=shifted["saddr"]))
    assert e.value.code == igx._abi.IGX_EINVAL and "16-byte aligned" in str(e.value)
    assert ctx.L.igx_tcp_classify(ctx.h, None, 4, 0, 0, None, 0, None, None, None, None) == igx._abi.IGX_EINVAL
    assert b"null argument" in ctx.L.igx_last_error(ctx.h)
