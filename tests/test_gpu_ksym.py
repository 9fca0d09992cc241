"""igx_ksym_lookup on the device against findKernelSymbol restated line by line
(tests/stack_ref.py), bit for bit: the hand cases, a 50 000-symbol sorted table, and the same
table with a shuffled tail (kallsyms lists modules after the core symbols)."""
import numpy as np
import pytest

from stack_ref import KSYM_HAND_CASES, find_kernel_symbol

pytestmark = pytest.mark.gpu


def _lookup(igx, addrs, ips):
    out = igx.engine.ksym_lookup(igx.columns.to_device(np.asarray(addrs, np.uint64)),
                                 igx.columns.to_device(np.asarray(ips, np.uint64)))
    return igx.columns.host(out).view(np.uint32)


def test_hand_cases(igx):
    for addrs, ip, want in KSYM_HAND_CASES:
        assert _lookup(igx, addrs, [ip]).tolist() == [want], (addrs, ip)
    # no addresses at all is valid
    assert _lookup(igx, [1, 2, 3], []).tolist() == []


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(11)
    base = 0xffffffff81000000
    addrs = base + np.cumsum(rng.integers(0, 4096, 50000)).astype(np.uint64)   # duplicates included
    ips = np.concatenate([rng.integers(int(addrs[0]) - 5000, int(addrs[-1]) + 5000, 99000, dtype=np.uint64),
                          addrs[rng.integers(0, 50000, 900)],                 # ip equal to an address
                          rng.integers(0, 1 << 63, 98, dtype=np.uint64), np.array([0, 2 ** 64 - 1], np.uint64)])
    return addrs, ips


def test_sorted_table(igx, table):
    addrs, ips = table
    got = _lookup(igx, addrs, ips)
    al = addrs.tolist()
    assert got.tolist() == [find_kernel_symbol(al, ip) for ip in ips.tolist()]
    # a 2-D batch of addresses keeps its shape
    out = igx.engine.ksym_lookup(igx.columns.to_device(addrs), igx.columns.to_device(ips[:1000].reshape(10, 100)))
    assert tuple(out.shape) == (10, 100)
    assert np.array_equal(igx.columns.host(out).view(np.uint32).ravel(), got[:1000])


def test_shuffled_tail(igx, table):
    addrs, ips = table
    rng = np.random.default_rng(12)
    mixed = addrs.copy()
    mixed[40000:] = rng.permutation(mixed[40000:])
    got = _lookup(igx, mixed, ips)
    ml = mixed.tolist()
    want = [find_kernel_symbol(ml, ip) for ip in ips.tolist()]
    assert got.tolist() == want
    al = addrs.tolist()
    assert len(set(want)) > 30000 and want != [find_kernel_symbol(al, ip) for ip in ips.tolist()]


def test_shuffled_table(igx, table):
    """No order at all: the final comparison fails for the addresses whose search never leaves
    symbol 0 (tracer.go:203 compares with the last address probed)."""
    addrs, ips = table
    mixed = np.random.default_rng(13).permutation(addrs)
    ml = mixed.tolist()
    want = [find_kernel_symbol(ml, ip) for ip in ips.tolist()]
    assert _lookup(igx, mixed, ips).tolist() == want
    assert 0xFFFFFFFF in want and any(w != 0xFFFFFFFF for w in want)
