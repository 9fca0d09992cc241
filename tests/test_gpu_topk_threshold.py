"""dist.topk_threshold: the exact global top-K from three small all-gathers instead of the full
group exchange.

Every case compares the rows -- keys, all four aggregates, the global first index -- with the
oracle's group-by + Go sort (go_sort_entries) of the union of all ranks' events.

Single process (dist.topk_threshold_ranks: the protocol's round functions, the all-gathers
played by concatenation):
  zipf      8 and 3 ranks on the C5 test stream (gen_file(0xC5), 200 000 keys, Zipf 1.05,
            200 000 events per rank, K = 20) under ["-wbytes"] and ["-reads", "-wbytes"]: the
            threshold path, with the union far inside cand_cap
  planted   hand-built streams: a group in no rank's local top-K that is the global top-1; ties
            at the K-th value split unevenly, one group absent on some ranks; a group whose
            earliest event lies on a rank where it is below T
  fallbacks fewer than K groups, tau == 0, cand_cap = 1, an ASC first key, a first key of
            out_width 4, a key column first, local values near 2^63 on two ranks: the oracle's
            rows by the full exchange, with the reason
Two processes (torch.distributed.run, both ranks on cuda:0 over gloo): tests/dist_worker_topk.py
runs the real dist.topk_threshold on the Zipf stream (400 000 events per rank) and the planted
streams.
"""
import importlib
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_zipf = {}


def _w():
    if os.path.join(ROOT, "tests") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
    return importlib.import_module("dist_worker_topk")


def _zipf_ranks(igx, oracle):
    """eight ranks' slices of the C5 test stream: host events and partial tables, built once"""
    if not _zipf:
        W = _w()
        E, H = igx.engine, igx.columns
        n, G = 200_000, W.G_ZIPF
        cdf = E.zipf_cdf(G, 1.05)
        cdf_d = H.to_device(cdf)
        _zipf["hosts"] = [oracle.gen_file(0xC5, 0, G, cdf, r * n, n) for r in range(8)]
        _zipf["tables"] = [W.rank_table(igx, E.gen_file(0xC5, 0, G, cdf_d, r * n, n), n, r * n, G + G // 4)
                           for r in range(8)]
    return _zipf["hosts"], _zipf["tables"]


def _play(igx, oracle, hosts, k, sort, tables=None, out_widths=(8, 8, 8, 8), cand_cap=None, capacity=4096):
    """(rows, info, the oracle's rows) for the ranks' events under the named sort spec"""
    W = _w()
    D, H, A = igx.dist, igx.columns, igx._abi
    skeys, okeys = W.sort_spec(A, sort)
    own = tables is None
    if own:
        tables = [W.rank_table(igx, W.to_device(igx, e), len(e["op"]), b, capacity, out_widths)
                  for e, b in zip(hosts, W.bases(hosts))]
    try:
        rows, info = D.topk_threshold_ranks(tables, skeys, k, W.WIDTHS, list(out_widths), capacity, cand_cap=cand_cap)
    finally:
        if own:
            for t in tables:
                t.destroy()
    ref, groups = W.oracle_topk(oracle, hosts, okeys, k, out_widths)
    print(f"{len(hosts)} ranks [{sort}] k={k}: {info} of {groups} groups")
    return H.host(rows), info, ref


@pytest.mark.parametrize("sort", ["-wbytes", "-reads,-wbytes"])
@pytest.mark.parametrize("ws", [8, 3])
def test_zipf_stream_takes_the_threshold_path(igx, torch, oracle, ws, sort):
    W = _w()
    hosts, tables = _zipf_ranks(igx, oracle)
    cap = W.G_ZIPF + W.G_ZIPF // 4
    rows, info, ref = _play(igx, oracle, hosts[:ws], W.K_ZIPF, sort, tables=tables[:ws], capacity=cap)
    assert info["path"] == "threshold" and info["tau"] > 0
    assert info["cand_cap"] == max(4096, 64 * W.K_ZIPF) and info["union"] <= info["cand_cap"]
    assert len(info["sent"]) == ws and max(info["sent"]) <= info["cand_cap"]
    assert info["union"] >= W.K_ZIPF
    assert W.rows_equal(rows, ref)


@pytest.mark.parametrize("sort", ["-wbytes", "-reads,-wbytes"])
@pytest.mark.parametrize("what", ["hidden", "ties", "late_first"])
def test_planted_streams(igx, torch, oracle, what, sort):
    W = _w()
    hosts, k = W.PLANTED[what](3)
    rows, info, ref = _play(igx, oracle, hosts, k, sort)
    assert info["path"] == "threshold", info
    assert W.rows_equal(rows, ref)
    if sort != "-wbytes":
        return
    wb = rows[:, W.KB + 24:W.KB + 32].copy().view(np.uint64).ravel()
    inode = rows[:, :8].copy().view(np.uint64).ravel()
    if what == "hidden":
        # the global top-1 is the group no rank had among its candidates
        assert inode[0] == 1001 and wb[0] == 270
        for e in hosts:
            loc, _ = W.oracle_topk(oracle, [e], W.sort_spec(igx._abi, sort)[1], k)
            assert 1001 not in loc[:, :8].copy().view(np.uint64).ravel()
    elif what == "ties":
        assert list(wb) == [200, 120, 50]     # four groups tie at 50; the oracle's rows say which
    else:
        first = rows[:, W.KB + 32:W.KB + 40].copy().view(np.uint64).ravel()
        assert inode[0] == 1001 and wb[0] == 301 and first[0] == 0   # rank 0's 1-byte event leads


def _stream(per_rank, seed=5):
    W = _w()
    return W._build(len(per_rank), per_rank, seed)


FALLBACKS = {
    # name: (events per rank, k, sort, out_widths, cand_cap, word expected in the reason)
    "fewer_than_k_groups": (lambda: [_w()._events([(1, 1, 5), (2, 1, 7), (1, 0, 1)]),
                                     _w()._events([(2, 1, 1), (3, 1, 9)]),
                                     _w()._events([(4, 0, 2), (1, 1, 1)])], 20, "-wbytes", (8, 8, 8, 8), None, "fewer"),
    # only two groups are ever written: the k-th wbytes is 0
    "tau_zero": (lambda: [_w()._events([(1, 1, 5), (2, 1, 6)] + [(10 + j, 0, 3) for j in range(12)]),
                          _w()._events([(1, 1, 2)] + [(10 + j, 0, 4) for j in range(3, 15)])], 5, "-wbytes",
                 (8, 8, 8, 8), None, "tau == 0"),
    "cand_cap_1": (lambda: _w().planted_hidden(3)[0], 4, "-wbytes", (8, 8, 8, 8), 1, "cand_cap"),
    "asc_first_key": (lambda: _w().planted_ties(3)[0], 3, "wbytes", (8, 8, 8, 8), None, "ascending"),
    "out_width_4": (lambda: _w().planted_ties(3)[0], 3, "-wbytes", (8, 8, 8, 4), None, "wraps"),
    "key_column_first": (lambda: _w().planted_hidden(3)[0], 4, "-dev,-wbytes", (8, 8, 8, 8), None, "not an aggregate"),
    # 2^63 and 2^63 + 5 on two ranks: the global sum wraps to 5
    "wrap_guard": (lambda: _stream([[(1, 1, 1 << 63), (2, 1, 40)], [(1, 1, (1 << 63) + 5), (3, 1, 50)]]), 2,
                   "-wbytes", (8, 8, 8, 8), None, "wrap"),
}


@pytest.mark.parametrize("name", list(FALLBACKS))
def test_fallbacks_take_the_full_exchange(igx, torch, oracle, name):
    W = _w()
    make, k, sort, ow, cand_cap, word = FALLBACKS[name]
    hosts = make()
    rows, info, ref = _play(igx, oracle, hosts, k, sort, out_widths=ow, cand_cap=cand_cap)
    assert info["path"] == "full" and word in info["reason"], info
    assert W.rows_equal(rows, ref)
    if name == "wrap_guard":
        wb = rows[:, W.KB + 24:W.KB + 32].copy().view(np.uint64).ravel()
        assert list(wb) == [50, 40]           # group 1's sum wrapped to 5: it is not in the top 2


def test_one_rank_is_local(igx, torch, oracle):
    W = _w()
    hosts, k = W.planted_ties(3)
    rows, info, ref = _play(igx, oracle, hosts[:1], k, "-wbytes")
    assert info["path"] == "local" and W.rows_equal(rows, ref)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_world2_topk_threshold():
    env = dict(os.environ, OMP_NUM_THREADS="4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "dist_worker_topk.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "TOPK_THRESHOLD_OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
