"""Streams, tables and the oracle's answer for the threshold top-K tests, and the world_size-2
worker of tests/test_gpu_topk_threshold.py.

As a worker (torch.distributed.run, both ranks on cuda:0 over gloo, as dist_worker_gpu.py):
every rank aggregates its own events, calls the real dist.topk_threshold, and rank 0 compares
the rows -- keys, all four aggregates, the global first index -- with the oracle's group-by +
Go sort of the union of both ranks' events: the C5 test stream (400 000 events per rank) and
the planted streams, under ["-wbytes"] and ["-reads", "-wbytes"]; then two fallbacks through the
real full exchange (cand_cap = 1, a key column first).  Prints TOPK_THRESHOLD_OK.

Top file's layout throughout: key (inode, dev, pid, tid), aggregates reads, rbytes, writes,
wbytes.  The planted streams carry `count` as a u64 column so that a partial sum can sit near
2^63 (the wrap guard's case).
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAMES = ("inode", "dev", "pid", "tid", "op", "count")
KNAMES = NAMES[:4]
WIDTHS = [8, 4, 4, 4]
KB = 20
G_ZIPF, K_ZIPF = 200_000, 20


def file_aggs(A, out_widths=(8, 8, 8, 8)):
    return [A.Agg(A.AGG_COUNT, 0, 4, out_widths[0], 0), A.Agg(A.AGG_SUM, 5, 4, out_widths[1], 0),
            A.Agg(A.AGG_COUNT, 0, 4, out_widths[2], 1), A.Agg(A.AGG_SUM, 5, 4, out_widths[3], 1)]


def sort_spec(A, name):
    """(Table.sort keys, oracle keys from (group keys, aggs)) for a sortBy list given by name"""
    agg = lambda x, desc: ((A.TSRC_AGG, x, desc), lambda k, a: (a[x], "uint64", desc))   # noqa: E731
    dev = ((A.TSRC_KEY, (8, 4, A.KIND_UINT), True),
           lambda k, a: (np.ascontiguousarray(k[:, 8:12]).view(np.uint32).ravel(), "uint32", True))
    spec = {"-wbytes": [agg(3, True)], "-reads,-wbytes": [agg(0, True), agg(3, True)],
            "wbytes": [agg(3, False)], "-dev,-wbytes": [dev, agg(3, True)]}[name]
    return [s for s, _ in spec], [o for _, o in spec]


def oracle_topk(O, hosts, okeys, k, out_widths=(8, 8, 8, 8)):
    """The expected rows: the oracle's group-by of the union of the ranks' events (rank r's
    events follow rank r-1's: its base index is the events before it), then Go's sort, first k."""
    h = {f: np.concatenate([e[f] for e in hosts]) for f in NAMES}
    op, cnt = h["op"], h["count"]
    k_, a_, f_ = O.groupby(O.pad_keys(h, KNAMES),
                           [{"kind": "count", "cond": op, "cond_val": 0, "out_width": out_widths[0]},
                            {"kind": "sum", "val": cnt, "cond": op, "cond_val": 0, "out_width": out_widths[1]},
                            {"kind": "count", "cond": op, "cond_val": 1, "out_width": out_widths[2]},
                            {"kind": "sum", "val": cnt, "cond": op, "cond_val": 1, "out_width": out_widths[3]}])
    perm = O.go_sort_entries([f(k_, a_) for f in okeys], len(f_))[:k].astype(np.int64)
    parts = [k_[perm]] + [a_[x][perm].copy().view(np.uint8).reshape(-1, 8) for x in range(4)]
    return np.concatenate(parts + [f_[perm].copy().view(np.uint8).reshape(-1, 8)], axis=1), len(f_)


def bases(hosts):
    out, b = [], 0
    for e in hosts:
        out.append(b)
        b += len(e["op"])
    return out


def rank_table(igx, ev, n, base, capacity, out_widths=(8, 8, 8, 8)):
    """a rank's partial table over its events (device columns), synchronously finalized"""
    E, A = igx.engine, igx._abi
    tab = E.Table(WIDTHS, file_aggs(A, out_widths), capacity)
    tab.update([ev[f] for f in NAMES], [0, 1, 2, 3], n, base)
    tab.finalize()
    return tab


def to_device(igx, e):
    return {f: igx.columns.to_device(e[f]) for f in NAMES}


# ---- planted streams (numpy): per rank a list of (key id, op, count) events -----------------
def _events(triples):
    kid = np.array([t[0] for t in triples], dtype=np.uint64)
    return {"inode": kid + np.uint64(1000), "dev": (kid % np.uint64(3) + np.uint64(7)).astype(np.uint32),
            "pid": (kid * np.uint64(3)).astype(np.uint32), "tid": (kid * np.uint64(5) + np.uint64(1)).astype(np.uint32),
            "op": np.array([t[1] for t in triples], dtype=np.uint8),
            "count": np.array([t[2] for t in triples], dtype=np.uint64)}


def _noise(r, seed):
    """small groups under every planted one: 50 keys of rank r alone (write 1..3 bytes, a read),
    30 keys on every rank (write 2 bytes)"""
    rng = np.random.default_rng(seed + r)
    ev = []
    for j in range(50):
        ev += [(10_000 + 100 * r + j, 1, int(rng.integers(1, 4))), (10_000 + 100 * r + j, 0, 9)]
    ev += [(20_000 + j, 1, 2) for j in range(30)]
    return ev


def _build(ws, per_rank, seed, first=None):
    """per_rank[r]: planted (key id, op, count) events; shuffled with the noise (first[r], if
    given, stays the rank's first event)"""
    out = []
    for r in range(ws):
        ev = per_rank[r] + _noise(r, seed)
        order = np.random.default_rng(seed * 31 + r).permutation(len(ev))
        ev = [ev[i] for i in order]
        if first and first.get(r):
            ev = [first[r]] + ev
        out.append(_events(ev))
    return out


def planted_hidden(ws, k=4):
    """A group that is in no rank's local top-k but is the global top-1: 90 bytes on every rank
    under k groups of 100..100+k-1 bytes that each rank holds alone (their top values tie across
    the ranks, too)."""
    per = [[(1, 1, 45), (1, 0, 7), (1, 1, 45)] + [(100 + 10 * r + j, 1, 100 + j) for j in range(k)] +
           [(100 + 10 * r + j, 0, 1) for j in range(k) for _ in range(r + j)] for r in range(ws)]
    return _build(ws, per, 11), k


def planted_ties(ws):
    """Ties at the k-th wbytes (50), split unevenly over the ranks, one group on one rank only;
    k = 3: P (200) and Q, then one of the four 50s -- ["-wbytes"] orders ties by position DESC."""
    split = {2: {"X": (50, 0), "Y": (20, 30), "Z": (10, 40), "W": (0, 50), "P": (0, 200), "Q": (60, 60)},
             3: {"X": (50, 0, 0), "Y": (20, 20, 10), "Z": (10, 15, 25), "W": (0, 25, 25), "P": (0, 200, 0),
                 "Q": (40, 40, 40)}}[ws]
    ids = {"X": 1, "Y": 2, "Z": 3, "W": 4, "P": 5, "Q": 6}
    per = [[] for _ in range(ws)]
    for g, vals in split.items():
        for r, v in enumerate(vals):
            if v:
                per[r] += [(ids[g], 1, v - v // 2), (ids[g], 1, v // 2)] if v > 1 else [(ids[g], 1, v)]
                per[r] += [(ids[g], 0, 3)] * (ids[g] % 3)
    return _build(ws, per, 23), 3


def planted_late_first(ws):
    """A group whose earliest event lies on rank 0, where it holds 1 byte (below T): only round
    3 can supply its global first index.  k = 2: F (1 + 300 on the last rank) over G (100 each)."""
    per = [[(2, 1, 100)] for _ in range(ws)]
    per[ws - 1] += [(1, 1, 300)]
    return _build(ws, per, 37, first={0: (1, 1, 1)}), 2


PLANTED = {"hidden": planted_hidden, "ties": planted_ties, "late_first": planted_late_first}


def rows_equal(got, ref):
    return got.shape == ref.shape and np.array_equal(got, ref)


# ---- the worker ---------------------------------------------------------------------------------
def main():
    import torch
    import torch.distributed as dist
    from oracle import oracle as O
    igx = importlib.import_module("inspektor-gadget_amd")
    D, E, H, A = igx.dist, igx.engine, igx.columns, igx._abi

    def check(ok, what):
        if not ok:
            print(f"MISMATCH: {what}", flush=True)
            sys.exit(3)

    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank, ws = dist.get_rank(), dist.get_world_size()

    def run(what, hosts, mine_dev, k, capacity, sorts=("-wbytes", "-reads,-wbytes"), cand_cap=None, path="threshold"):
        n = len(hosts[rank]["op"])
        tab = rank_table(igx, mine_dev, n, bases(hosts)[rank], capacity)
        for name in sorts:
            skeys, okeys = sort_spec(A, name)
            rows, info = D.topk_threshold(tab, skeys, k, WIDTHS, [8, 8, 8, 8], capacity, cand_cap=cand_cap)
            every = H.host(D.allgather_rows(rows))
            if rank == 0:
                ref, groups = oracle_topk(O, hosts, okeys, k)
                print(f"{what} [{name}]: {info} of {groups} groups", flush=True)
                check(info["path"] == path, f"{what} [{name}] took {info}")
                check(rows_equal(H.host(rows), ref), f"{what} [{name}] rows vs oracle")
                check(all(rows_equal(every[i * len(ref):(i + 1) * len(ref)], ref) for i in range(ws)),
                      f"{what} [{name}] rows differ between the ranks")
        tab.destroy()

    # the C5 test stream: one global key universe, rank r's slice of one global stream
    n = 400_000
    cdf = E.zipf_cdf(G_ZIPF, 1.05)
    ev = E.gen_file(0xC5, 0, G_ZIPF, H.to_device(cdf), rank * n, n)
    hosts = [O.gen_file(0xC5, 0, G_ZIPF, cdf, r * n, n) for r in range(ws)] if rank == 0 else \
        [{"op": np.empty(n, np.uint8)} for _ in range(ws)]
    run("zipf", hosts, ev, K_ZIPF, G_ZIPF + G_ZIPF // 4)
    for what, make in PLANTED.items():
        hosts, k = make(ws)
        run(what, hosts, to_device(igx, hosts[rank]), k, 4096)
    # the fallback's own exchange (partition by owner, all-to-all, owner merge, all-gather)
    hosts, k = planted_hidden(ws)
    run("hidden, cand_cap=1", hosts, to_device(igx, hosts[rank]), k, 4096, cand_cap=1, path="full")
    run("hidden, a key column first", hosts, to_device(igx, hosts[rank]), k, 4096, sorts=("-dev,-wbytes",), path="full")
    dist.barrier()
    if rank == 0:
        print("TOPK_THRESHOLD_OK", flush=True)
    D.shutdown()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
