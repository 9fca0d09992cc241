"""The group-by table's lifetime protocol -- generations, seeds, the epoch counter's wrap, the
event-index limit -- under the asynchronous pipeline the benchmark runs (reset, update,
finalize(sync=False), top-K, gather, no wait before the next reset), where the host learns an
interval's outcome one or two intervals late.

(a) test_async_pipeline_*: the seeded stream of test_gpu_persist.test_seeded_cache_exact with
    asynchronous finalizes.  Two of every three intervals are fetched (the rows first, wait()
    after them); every third is *blind* -- nothing of it is read on the host before the next
    reset, its rows are snapshot on the device (partition(1) and the top-20, both sized by the
    device's group count) and compared at the end -- so the next reset finds its read-back in
    flight.  A small table ages its generation out and takes an over-capacity interval, whose
    IGX_ENOSPC must come back exactly once from a later call.
(b) test_wrap_inside_seeded_generation: a live, seeded generation is walked to epoch 65535; the
    reset after it wraps (the table is cleared, epochs restart at 1, as does the start epoch that
    identifies a generation) and the interval after the wrapped one starts before the wrapped
    one's read-back is collected.
(c) test_index_limit_*: index column values and row indices at the contract's limit
    (include/igx.h, igx_groupby_update: indices stay below 2^48 - 2), on keys the interval
    inserts and on keys it finds kept, in every form.

References: oracle.groupby per interval (test_gpu_persist._ref_rows); for the index-column
cases, which the oracle does not have, numpy: per distinct key the u64 sum mod 2^64 and the
minimum of the index column.
"""
import importlib
import time

import numpy as np
import pytest

import test_gpu_persist as P
from test_gpu_persist import NAMES, Run, _batch, _ref_rows, _universe

pytestmark = pytest.mark.gpu

KB = 20           # top file's packed key: inode 8 | dev 4 | pid 4 | tid 4
TOPK = 20


def _sorted(rows):
    rows = np.ascontiguousarray(rows)
    return np.sort(rows.view(np.dtype((np.void, rows.shape[1]))).ravel())


def _ref_top(oracle, bench, h, base):
    """(first, wbytes) of the interval's top-20 by -wbytes: Go's SliceStable over the groups in
    first-occurrence order, as test_gpu_owner_exchange builds it"""
    keys = oracle.pad_keys(h, ("inode", "dev", "pid", "tid"))
    _, aggs, first = oracle.groupby(keys, bench.c5_oracle_aggs(h), base_idx=base)
    order = np.argsort(first, kind="stable")
    perm = oracle.go_sort_entries([(aggs[3][order], "uint64", True)], len(first))
    sel = order[perm[:TOPK].astype(np.int64)]
    return first[sel], aggs[3][sel]


def _u64(a, o):
    return a[:, o:o + 8].copy().view(np.uint64).ravel()


class AsyncRun(Run):
    """Run (test_gpu_persist) with the benchmark's interval: nothing in issue() reads the device"""

    def upload(self, h):
        return [self.H.to_device(np.ascontiguousarray(h[k])) for k in NAMES]

    def issue(self, cols, n, base, snapshot=True):
        """reset, update, finalize(sync=False), top-20, and the whole table as partition(1)'s rows
        (sized by the device's group count).  Returns (errors raised by the calls that may report
        an earlier interval, top rows, table rows, their count), all on the device."""
        A, tab = self.A, self.tab
        raised = 0
        try:
            tab.reset()
        except A.IgxError as e:
            assert e.code == A.IGX_ENOSPC, e
            raised += 1
        tab.update(cols, [0, 1, 2, 3], n, base)
        try:
            tab.finalize(sync=False)
        except A.IgxError as e:
            assert e.code == A.IGX_ENOSPC and "previous interval" in str(e), e
            raised += 1
            tab.finalize(sync=False)        # a non-zero return means "not finalized": now it is
        top = rows = cnt = None
        if snapshot:
            top = tab.gather(tab.sort([(A.TSRC_AGG, 3, True)], TOPK)).clone()
            rows, cnt = tab.partition(1)
            rows = rows.clone()             # partition() reuses its buffer
        return raised, top, rows, cnt

    def check(self, h, base, top, rows, cnt):
        """the fetched snapshot against the oracle; returns the group count"""
        G = int(cnt.cpu()[0])
        want = _ref_rows(self.oracle, self.bench, h, base)
        got = _sorted(self.H.host(rows[:max(G, 0)]))
        assert G == want.shape[0], (G, want.shape[0])
        assert np.array_equal(got, want)
        first, wbytes = _ref_top(self.oracle, self.bench, h, base)
        t = self.H.host(top)
        assert np.array_equal(_u64(t, KB + 32), first) and np.array_equal(_u64(t, KB + 24), wbytes)
        return G

    def model(self, ids, fresh=False):
        """claims the generation model expects of an interval with these key ids (Run.interval's)"""
        if fresh or len(self.gen) > self.limit():
            self.gen = set()
        keys = set(ids.tolist())
        expect = len(keys - self.gen)
        self.gen |= keys
        return expect


def _pipeline(r, batches, blind_every=3):
    """batches: [(h, ids, base)].  Fetched intervals are checked at once (rows, then wait() and
    the claims); blind ones at the end.  Returns the claims checked, as (k, got, want)."""
    up = [r.upload(h) for h, _, _ in batches]
    later, claims = [], []
    last = len(batches) - 1
    for k, (h, ids, base) in enumerate(batches):
        raised, top, rows, cnt = r.issue(up[k], len(h["op"]), base)
        assert raised == 0, k
        want = r.model(ids, fresh=(k == 0))
        if k % blind_every == blind_every - 1 or k == last:
            later.append((k, h, base, top, rows, cnt, want))      # nothing of it is read yet
            continue
        G = r.check(h, base, top, rows, cnt)
        assert r.tab.wait() == G, k
        claims.append((k, r.tab.info()["claims"], want))
    G = r.tab.wait()                                              # the last interval, waited once
    claims.append((last, r.tab.info()["claims"], later[-1][-1]))
    for k, h, base, top, rows, cnt, _ in later:
        Gk = r.check(h, base, top, rows, cnt)
        assert k != last or Gk == G
    return claims


@pytest.mark.parametrize("prober,rowplan", [("0", None), ("1", None), ("0", "0")])
def test_async_pipeline_seeded_generation(igx, torch, oracle, monkeypatch, prober, rowplan):
    """test_seeded_cache_exact's stream (every interval seeded, seeds recomputed every 4) with a
    60 000-key window, so the generation's keys load the 262 144 slots past 30 % from the
    seventh interval on (60.5k + 3k per interval; the limit is 109 715) and probe chains exist.
    The registered top-file shape runs its row plan (2); IGX_GB_ROWPLAN=0 the general kernel."""
    monkeypatch.setenv("IGX_GB_SEED_MIN", "1")
    monkeypatch.setenv("IGX_GB_SEED_EVERY", "4")
    monkeypatch.setenv("IGX_GB_PROBER", prober)
    if rowplan is not None:
        monkeypatch.setenv("IGX_GB_ROWPLAN", rowplan)
    rng = np.random.default_rng(0xA5F + int(prober))
    U = _universe(150_000)
    r = AsyncRun(igx, torch, oracle, 100_000, igx._abi.GB_CACHED)
    batches = []
    for k in range(12):
        h, ids = _batch(rng, U, 3_000 * k, 60_000, 800_000)
        batches.append((h, ids, 0 if k % 3 else k * 800_000))
    claims = _pipeline(r, batches)
    assert all(g == w for _, g, w in claims), claims
    assert len(r.gen) >= 0.3 * 262_144 and len(r.gen) <= r.limit()
    assert r.tab.rowplan() == (0 if rowplan == "0" else 2)
    r.tab.destroy()


def test_async_pipeline_age_out_and_overflow(igx, torch, oracle, monkeypatch):
    """test_age_out_rebuild_and_recovery's small table under the same pipeline: the generation
    passes its limit (22 428 keys) every few intervals and the next interval starts an empty
    table -- decided on the device, so it must not depend on when the host collects anything.
    Then an interval over capacity, never waited on: its IGX_ENOSPC comes back exactly once, from
    the next reset or the next finalize(sync=False), and the interval after it is exact and
    starts a generation."""
    monkeypatch.setenv("IGX_GB_SEED_MIN", "1")
    monkeypatch.setenv("IGX_GB_SEED_EVERY", "4")
    A = igx._abi
    rng = np.random.default_rng(0xA6E)
    U = _universe(300_000)
    r = AsyncRun(igx, torch, oracle, 30_000, A.GB_CACHED)
    batches, sizes, rebuilt = [], [], 0
    for k in range(12):
        h, ids = _batch(rng, U, 3_000 * k, 12_000, 300_000)
        batches.append((h, ids, k * 300_000))
    claims = _pipeline(r, batches)
    assert all(g == w for _, g, w in claims), claims
    # the model's generation was emptied at least twice (the claims above follow it)
    m = AsyncRun.__new__(AsyncRun)
    m.gen, m.cap = set(), r.cap
    for k, (_, ids, _) in enumerate(batches):
        before = len(m.gen)
        m.model(ids, fresh=(k == 0))
        rebuilt += bool(k and before > m.limit())
        sizes.append(before)
    assert rebuilt >= 2, sizes
    # over capacity (more distinct keys than 30 000, within the 65 536 slots): issued blind
    h, ids = _batch(rng, U, 100_000, 35_500, 1_500_000)
    assert len(ids) > 30_000
    raised, _, _, _ = r.issue(r.upload(h), len(h["op"]), 0, snapshot=False)
    assert raised == 0
    # ... and the next interval, issued at once, reports it exactly once and is itself exact
    h, ids = _batch(rng, U, 50_000, 12_000, 300_000)
    raised, top, rows, cnt = r.issue(r.upload(h), len(h["op"]), 7)
    assert raised == 1
    G = r.check(h, 7, top, rows, cnt)
    assert r.tab.wait() == G == len(ids)
    assert r.tab.info()["claims"] == r.model(ids, fresh=True) == G
    r.tab.destroy()


# ---- (b) the wrap inside a live, seeded generation ------------------------------------------
# The premise of the asynchronous variant is that the reset after the wrapped interval W does
# NOT collect W's read-back (that read-back is what drops stale seeds on the host).  The stream
# is therefore kept busy ahead of W: DELAY_SORTS sorts of 2^26 int32 keys on the table's stream.
# Measured on an MI355X (the test prints both figures, -s): 4 such sorts keep the stream busy for
# 11.2 ms and the 16 used here for 46.5 ms, while the host needs 0.35 ms from W's reset to the
# reset after it (reset, update, finalize(sync=False), top-20, partition(1), reset; 1.25 ms when
# these are the process's first launches).  That is a margin of 37x to 130x, enough for a host
# thread that loses its CPU for a few scheduler ticks.  If the premise fails all the same, the
# test fails (it does not skip): lengthen the delay.
DELAY_ELEMS = 1 << 26
DELAY_SORTS = 16


WRAP_ROWS = 500_000


def _wrap_run(igx, torch, oracle, monkeypatch, prober, sync):
    monkeypatch.setenv("IGX_GB_SEED_MIN", "1")
    monkeypatch.setenv("IGX_GB_SEED_EVERY", "4")
    monkeypatch.setenv("IGX_GB_PROBER", prober)
    A = igx._abi
    rng = np.random.default_rng(0xE9 + int(prober))
    U = _universe(150_000)
    r = AsyncRun(igx, torch, oracle, 100_000, A.GB_CACHED)
    tab = r.tab
    # 84 000-key windows sliding by 3 000, 500k rows: ~80k groups an interval, and the generation
    # holds a third of the 262 144 slots at the wrap (its limit is 109 715: no age-out on the way)
    hA, idsA = _batch(rng, U, 0, 84_000, WRAP_ROWS)
    hB, idsB = _batch(rng, U, 3_000, 84_000, WRAP_ROWS)
    hC, idsC = _batch(rng, U, 6_000, 84_000, WRAP_ROWS)
    perm = rng.permutation(WRAP_ROWS)                     # W: C's rows (so C's key set) in another order
    hW, idsW = {k: v[perm] for k, v in hC.items()}, idsC
    hX, idsX = _batch(rng, U, 9_000, 84_000, WRAP_ROWS)
    cW, cX = r.upload(hW), r.upload(hX)
    noise = torch.randint(0, 1 << 30, (DELAY_ELEMS,), dtype=torch.int32, device="cuda")
    torch.sort(noise)                                   # warm the allocator: later sorts only launch
    torch.cuda.synchronize()

    def sync_interval(h, ids, base, reset, fresh=False):
        cols = r.upload(h)
        if reset:
            tab.reset()
        tab.update(cols, [0, 1, 2, 3], len(h["op"]), base)
        fin = tab.finalize()
        got = P._dev_rows(r.bench, r.E, r.H, torch, tab, fin)
        assert np.array_equal(got, _ref_rows(oracle, r.bench, h, base))
        want = r.model(ids, fresh=fresh)
        assert tab.info()["claims"] == want
        return want

    # A: the table's first interval, no reset before it: its generation starts at epoch 1
    assert sync_interval(hA, idsA, 0, reset=False, fresh=True) == len(idsA)
    # B: epoch 2, seeded, computes the seeds (A's read-back started a generation: no seeds yet)
    sync_interval(hB, idsB, 5, reset=True)
    # bare resets continue the generation (the last finalize still follows the last update):
    # epochs 3 .. 65534
    for _ in range(65_532):
        tab.reset()
    # C at epoch 65535 adopts B's seeds; its claims and the generation's key count show that the
    # generation lived through the walk (an ended one would claim every key of C)
    claims_c = sync_interval(hC, idsC, 0, reset=True)
    info = tab.info()
    assert info["gen_keys"] == len(r.gen) and claims_c < len(idsC) // 5
    assert 0.3 * 262_144 <= len(r.gen) <= r.limit()
    GW = _ref_rows(oracle, r.bench, hW, 11).shape[0]
    assert claims_c != GW                               # what tells the two read-backs apart below

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    if sync:
        tab.reset()                                     # wraps
        tab.update(cW, [0, 1, 2, 3], WRAP_ROWS, 11)
        fin = tab.finalize()
        got = P._dev_rows(r.bench, r.E, r.H, torch, tab, fin)
        assert np.array_equal(got, _ref_rows(oracle, r.bench, hW, 11))
        assert tab.info()["claims"] == r.model(idsW, fresh=True) == GW
        tab.reset()
        tab.update(cX, [0, 1, 2, 3], WRAP_ROWS, 3)
    else:
        ev[0].record()
        for _ in range(DELAY_SORTS):
            torch.sort(noise)
        ev[1].record()
        t0 = time.perf_counter()
        tab.reset()                                     # wraps: the table is cleared, epoch 1 again
        tab.update(cW, [0, 1, 2, 3], WRAP_ROWS, 11)
        tab.finalize(sync=False)
        top = tab.gather(tab.sort([(A.TSRC_AGG, 3, True)], TOPK)).clone()
        rows, cnt = tab.partition(1)
        rows = rows.clone()
        tab.reset()                                     # at once: W's read-back is still in flight
        host_s = time.perf_counter() - t0
        # the premise: that reset did not collect W (the claims are still C's, not W's)
        assert tab.info()["claims"] == claims_c, "the reset after W collected W's read-back"
        tab.update(cX, [0, 1, 2, 3], WRAP_ROWS, 3)
        assert tab.wait() == GW                         # now W is collected ...
        assert tab.info()["claims"] == r.model(idsW, fresh=True) == GW   # ... a table of its own
        assert r.check(hW, 11, top, rows, cnt) == GW
        print(f"wrap premise: delay {ev[0].elapsed_time(ev[1]):.1f} ms on the stream ahead of W, "
              f"host calls reset..reset {host_s * 1e3:.2f} ms")
    # X: the interval after the wrapped one, whole table and claims
    fin = tab.finalize()
    got = P._dev_rows(r.bench, r.E, r.H, torch, tab, fin)
    want = _ref_rows(oracle, r.bench, hX, 3)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    assert tab.info()["claims"] == r.model(idsX)
    tab.destroy()


@pytest.mark.parametrize("prober", ["0", "1"])
def test_wrap_inside_seeded_generation_async(igx, torch, oracle, monkeypatch, prober):
    """W finalized asynchronously, the next reset at once, X seeded: seeds looked up before the
    wrap carry slots of the table that was cleared, and the generation they name (start epoch 1)
    exists again.  X must not adopt them."""
    _wrap_run(igx, torch, oracle, monkeypatch, prober, sync=False)


@pytest.mark.parametrize("prober", ["0", "1"])
def test_wrap_inside_seeded_generation_sync(igx, torch, oracle, monkeypatch, prober):
    """the same with synchronous finalizes (the gadgets' path): W's read-back is applied before
    X starts, which has always dropped the seeds"""
    _wrap_run(igx, torch, oracle, monkeypatch, prober, sync=True)


# ---- (c) index limits -------------------------------------------------------------------------
L = (1 << 48) - 3                        # the largest index the contract allows
EDGES = [0, 1, (1 << 32) - 1, 1 << 32, L - 1, L]
PAST = [L + 1, 1 << 48, (1 << 64) - 1]
NKEYS = 300


class IdxRun:
    """top file's key, one u64 SUM, an index column; results against numpy"""

    def __init__(self, igx, torch, mode):
        self.E, self.H, self.A, self.torch = igx.engine, igx.columns, igx._abi, torch
        self.bench = importlib.import_module("bench")
        A = self.A
        self.tab = self.E.Table(P.WIDTHS, [A.Agg(A.AGG_SUM, 4, A.NO_COL, 8, 0)], 2048)
        self.tab.set_mode(mode)
        self.U = _universe(4096)

    def feed(self, ids, val, idx=None, base=0, reset=True):
        U, H = self.U, self.H
        cols = [H.to_device(np.ascontiguousarray(U[k][ids])) for k in ("inode", "dev", "pid", "tid")]
        cols.append(H.to_device(val))
        if idx is not None:
            cols.append(H.to_device(idx))
        if reset:
            self.tab.reset()
        self.tab.update(cols, [0, 1, 2, 3], len(ids), base, idx_col=None if idx is None else 5)

    def rows(self):
        fin = self.tab.finalize()
        return _sorted(self.H.host(self.bench.table_rows(self.E, self.torch, self.tab, fin)))

    def ref(self, ids, val, idx):
        """numpy: per distinct key the u64 sum mod 2^64 and the smallest index"""
        U = self.U
        uk, inv = np.unique(ids, return_inverse=True)
        s = np.zeros(len(uk), np.uint64)
        np.add.at(s, inv, val)                          # u64 arithmetic wraps
        f = np.full(len(uk), np.iinfo(np.uint64).max, np.uint64)
        np.minimum.at(f, inv, idx)
        key = np.concatenate([U["inode"][uk].copy().view(np.uint8).reshape(-1, 8)] +
                             [U[k][uk].copy().view(np.uint8).reshape(-1, 4) for k in ("dev", "pid", "tid")], axis=1)
        return _sorted(np.concatenate([key, s.view(np.uint8).reshape(-1, 8), f.view(np.uint8).reshape(-1, 8)], axis=1))

    def exact(self, ids, val, idx, **kw):
        self.feed(ids, val, idx, **kw)
        got, want = self.rows(), self.ref(ids, val, idx)
        assert got.shape == want.shape and np.array_equal(got, want)

    def fails(self, ids, val, idx):
        self.feed(ids, val, idx)
        with pytest.raises(self.A.IgxError) as ei:
            self.tab.finalize()
        assert ei.value.code == self.A.IGX_ENOSPC


def _edge_stream(rng):
    """4 000 rows over NKEYS keys with small random indices, a dozen of them carrying an edge
    value as one row among a key's several; plus, per edge value e, three more keys: one whose
    only row carries e, and two with e and a smaller index, in both row orders.  Sums wrap 2^64."""
    n = 4_000
    ids_r = rng.integers(0, NKEYS, n)
    idx_r = rng.integers(2, 1_000_000, n).astype(np.uint64)
    idx_r[rng.choice(n, 2 * len(EDGES), replace=False)] = np.array(EDGES * 2, dtype=np.uint64)
    xi, xx = [], []
    for j, e in enumerate(EDGES):
        lo = int(rng.integers(0, min(e, 1 << 40))) if e else 0
        k0, k1, k2 = NKEYS + 3 * j, NKEYS + 3 * j + 1, NKEYS + 3 * j + 2
        xi += [k0, k1, k1, k2, k2]
        xx += [e, e, lo, lo, e]
    special = np.zeros(n + len(xi), dtype=bool)                   # where the planted rows go: in
    special[rng.choice(n + len(xi), len(xi), replace=False)] = True   # their order, anywhere
    ids = np.empty(n + len(xi), dtype=np.int64)
    idx = np.empty(n + len(xi), dtype=np.uint64)
    ids[special], ids[~special] = xi, ids_r
    idx[special], idx[~special] = np.array(xx, dtype=np.uint64), idx_r
    val = rng.integers(0, 1 << 63, len(ids), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    return ids, val, idx


def _one_bad(rng, key, bad):
    """the random stream plus one key whose only row carries an index past the limit"""
    ids = rng.integers(0, NKEYS, 3_000)
    idx = rng.integers(2, 1_000_000, len(ids)).astype(np.uint64)
    at = int(rng.integers(0, len(ids)))
    ids = np.insert(ids, at, key)
    idx = np.insert(idx, at, np.uint64(bad))
    val = rng.integers(0, 1 << 63, len(ids), dtype=np.uint64)
    return ids.astype(np.int64), val, idx


@pytest.mark.parametrize("prober", ["0", "1"])
@pytest.mark.parametrize("seeded", [False, True])
def test_index_limit_cached_fresh_and_kept(igx, torch, monkeypatch, prober, seeded):
    """The cached form.  Unseeded, a kept key's first row of an interval re-stamps `ready`
    (index + 2 in 48 bits: the path that used to reject L + 1 = 2^48 - 2 while a claim accepted
    it); seeded (IGX_GB_SEED_MIN=1), the kept keys sit in the LDS cache from the start and their
    rows are hits that reach neither a claim nor a re-stamp.  Either way a key accepts every
    index up to L and the interval fails on one past it, whether the key is new or kept."""
    monkeypatch.setenv("IGX_GB_PROBER", prober)
    monkeypatch.setenv("IGX_GB_SEED_MIN", "1" if seeded else str(1 << 40))
    monkeypatch.setenv("IGX_GB_SEED_EVERY", "2")
    A = igx._abi
    rng = np.random.default_rng(0x1D + 2 * int(prober) + int(seeded))
    r = IdxRun(igx, torch, A.GB_CACHED)
    a = _edge_stream(rng)
    r.exact(*a)                                                   # every key fresh
    assert r.tab.info()["claims"] == len(np.unique(a[0]))
    b = _edge_stream(rng)                                         # the same keys, now kept
    r.exact(*b)
    assert r.tab.info()["claims"] == 0
    # the same rows once more in reverse row order (the kept keys' pairs the other way round)
    r.exact(*(x[::-1].copy() for x in b))
    assert r.tab.info()["claims"] == 0
    fresh_key = 2_000
    for bad in PAST:
        # on a key the generation has never held ...
        r.fails(*_one_bad(rng, fresh_key, bad))
        fresh_key += 1
        c = _edge_stream(rng)
        r.exact(*c)                                               # the next interval is exact
        assert r.tab.info()["claims"] == len(np.unique(c[0]))     # (a failure ends the generation)
        # ... and on a kept key (of the interval just before), its only row of the interval
        kept = int(c[0][0])
        ids, val, idx = _one_bad(rng, kept, bad)
        keep = ids != kept
        keep[np.flatnonzero(idx == np.uint64(bad))[0]] = True
        r.fails(ids[keep], val[keep], idx[keep])
        r.exact(*_edge_stream(rng))
    r.tab.destroy()


@pytest.mark.parametrize("mode", ["direct", "part"])
def test_index_limit_direct_and_partitioned(igx, torch, mode):
    """fresh keys (these forms start a generation every interval) take the same edge values, and
    an index past the limit as a key's only row fails the interval"""
    A = igx._abi
    rng = np.random.default_rng(0x1D7 + len(mode))
    r = IdxRun(igx, torch, A.GB_DIRECT if mode == "direct" else A.GB_PART)
    r.exact(*_edge_stream(rng))
    for bad in PAST:
        r.fails(*_one_bad(rng, 2_000, bad))
        r.exact(*_edge_stream(rng))
    r.tab.destroy()


@pytest.mark.parametrize("mode", ["cached", "direct", "part"])
def test_row_index_limit(igx, torch, mode):
    """base_idx + nrows: the last row's index may be L.  IGX_EINVAL at the first value past that
    (and for a base_idx that would wrap 64 bits), success one below -- on fresh keys and, in the
    cached form, on keys kept from the interval before (their re-stamp carries L + 2)."""
    A = igx._abi
    rng = np.random.default_rng(0x1D9)
    r = IdxRun(igx, torch, {"cached": A.GB_CACHED, "direct": A.GB_DIRECT, "part": A.GB_PART}[mode])
    n = 3_000
    ids = rng.integers(0, NKEYS, n).astype(np.int64)
    ids[-1] = NKEYS + 1                                           # the last row's key: its only row
    val = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    for _ in range(2):                                            # fresh, then kept (cached form)
        for base in (L + 2 - n, 1 << 48, (1 << 64) - 1, (1 << 64) - n):
            with pytest.raises(A.IgxError) as ei:
                r.feed(ids, val, base=base)
            assert ei.value.code == A.IGX_EINVAL, base
        base = L + 1 - n                                          # rows base .. L
        r.feed(ids, val, base=base)
        want = r.ref(ids, val, np.uint64(base) + np.arange(n, dtype=np.uint64))
        got = r.rows()
        assert got.shape == want.shape and np.array_equal(got, want)
    r.tab.destroy()
