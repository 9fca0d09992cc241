"""igx_groupby_select_ge and igx_groupby_lookup: the two table steps of the cross-rank threshold
top-K, checked against engine.table_tensors, numpy and the oracle group-by.

Three key layouts over 200 000 events and about 20 000 keys: top file's [8, 4, 4, 4] with its
four aggregates (a static layout), top tcp's 72-byte key (static, 18 words) and a generic layout
with odd widths [3, 8, 1] whose third aggregate has out_width 4 and wraps.

select_ge  the slots whose aggregate, masked to its out_width, is >= T, as a set, for T in
           {0 (every group), 1, a median value, the maximum, the maximum + 1 (none), 2^64 - 1},
           after a synchronous and an asynchronous finalize; with cap below the count the count
           is still the total, exactly cap distinct qualifying slots are written and the words
           past cap are untouched.
lookup     every group's key (shuffled, with duplicates) gives gather()'s row of its slot; keys
           never inserted give a zero row and found 0; so do keys the table keeps from an
           earlier interval of the generation (interval 1 feeds A u B, interval 2 only A: B's key
           records are still there); in the cached, direct and partitioned forms; with the
           capacity equal to the number of keys (long probe chains, region wrap); n == 0.
Both are read-only: the top-K counters do not move, and a reset plus another interval still
equals the oracle.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, KEYS = 200_000, 20_000
U64 = (1 << 64) - 1
FILE_NAMES = ("inode", "dev", "pid", "tid", "op", "count")
TCP_NAMES = ("saddr", "daddr", "mntns", "pid", "comm", "lport", "dport", "family", "size", "dir")
_cache = {}


def _generic_events(seed=7, n=N):
    """numpy events for the generic layout [3, 8, 1]: key columns derived from a key id, a u32
    value near 2^32 so that a 4-byte sum wraps from the second event on."""
    rng = np.random.default_rng(seed)
    kid = np.where(rng.random(n) < 0.5, rng.integers(0, 200, n), rng.integers(0, KEYS, n)).astype(np.uint64)
    h = kid * np.uint64(0x9E3779B97F4A7C15)
    a = np.stack([(h >> np.uint64(s)).astype(np.uint8) for s in (40, 48, 56)], axis=1)
    return {"a": np.ascontiguousarray(a), "b": h ^ (kid << np.uint64(7)), "c": (kid % np.uint64(251)).astype(np.uint8),
            "val": rng.integers(1 << 31, 1 << 32, n, dtype=np.uint64).astype(np.uint32)}


def _layout(name, igx, oracle):
    """(host events, device columns, key widths, key column indices, igx aggs, oracle aggs, key names)"""
    if name in _cache:
        return _cache[name]
    E, H, A = igx.engine, igx.columns, igx._abi
    if name == "file":
        cdf = E.zipf_cdf(KEYS, 1.05)
        h = oracle.gen_file(0xC5, 0, KEYS, cdf, 0, N)
        names, knames, widths = FILE_NAMES, FILE_NAMES[:4], [8, 4, 4, 4]
        aggs = [A.Agg(A.AGG_COUNT, 0, 4, 8, 0), A.Agg(A.AGG_SUM, 5, 4, 8, 0),
                A.Agg(A.AGG_COUNT, 0, 4, 8, 1), A.Agg(A.AGG_SUM, 5, 4, 8, 1)]
        oaggs = [{"kind": "count", "cond": h["op"], "cond_val": 0},
                 {"kind": "sum", "val": h["count"], "cond": h["op"], "cond_val": 0},
                 {"kind": "count", "cond": h["op"], "cond_val": 1},
                 {"kind": "sum", "val": h["count"], "cond": h["op"], "cond_val": 1}]
    elif name == "tcp":
        cdf = E.zipf_cdf(KEYS, 1.1)
        h = oracle.gen_tcp(0xC2, 0, KEYS, cdf, 0, N)
        names, knames, widths = TCP_NAMES, TCP_NAMES[:8], [16, 16, 8, 4, 16, 2, 2, 2]
        aggs = [A.Agg(A.AGG_SUM, 8, 9, 8, 0), A.Agg(A.AGG_SUM, 8, 9, 8, 1)]
        oaggs = [{"kind": "sum", "val": h["size"], "cond": h["dir"], "cond_val": 0},
                 {"kind": "sum", "val": h["size"], "cond": h["dir"], "cond_val": 1}]
    else:
        h = _generic_events()
        names, knames, widths = ("a", "b", "c", "val"), ("a", "b", "c"), [3, 8, 1]
        aggs = [A.Agg(A.AGG_COUNT, 0, A.NO_COL, 8, 0), A.Agg(A.AGG_SUM, 3, A.NO_COL, 8, 0),
                A.Agg(A.AGG_SUM, 3, A.NO_COL, 4, 0)]
        oaggs = [{"kind": "count"}, {"kind": "sum", "val": h["val"]},
                 {"kind": "sum", "val": h["val"], "out_width": 4}]
    cols = [H.to_device(h[k]) for k in names]
    _cache[name] = (h, cols, widths, list(range(len(knames))), aggs, oaggs, knames)
    return _cache[name]


def _ref_rows(oracle, h, knames, oaggs, rows=None, base=0):
    """the oracle's group-by of events `rows` (default all) as packed rows key | aggs | first"""
    if rows is not None:
        h = {k: v[rows] for k, v in h.items()}
        oaggs = [dict(a, **{f: a[f][rows] for f in ("val", "cond") if a.get(f) is not None}) for a in oaggs]
    k, aggs, first = oracle.groupby(oracle.pad_keys(h, knames), oaggs, base_idx=base)
    parts = [k] + [aggs[x].copy().view(np.uint8).reshape(-1, 8) for x in range(len(oaggs))]
    return np.concatenate(parts + [first.copy().view(np.uint8).reshape(-1, 8)], axis=1)


def _sorted(rows):
    rows = np.ascontiguousarray(rows)
    return np.sort(rows.view(np.dtype((np.void, rows.shape[1]))).ravel())


def _slots(tab, torch):
    G = tab.fin["n_groups"]
    s = torch.empty(max(1, G), dtype=torch.int32, device="cuda")[:G]
    if G:
        tab.ctx.check(tab.ctx.L.igx_memcpy_d2d(tab.ctx.h, C.c_void_p(s.data_ptr()), C.c_void_p(tab.fin["groups_ptr"]), G * 4))
    return s


def _table(igx, oracle, name, sync=True, mode=None, capacity=None, rows=None, tab=None):
    """a finalized table of the layout's events (rows: a subset, in order)"""
    E = igx.engine
    h, cols, widths, kc, aggs, oaggs, knames = _layout(name, igx, oracle)
    if tab is None:
        tab = E.Table(widths, aggs, capacity or KEYS + KEYS // 4)
        if mode is not None:
            tab.set_mode(mode)
    else:
        tab.reset()
    if rows is None:
        tab.update(cols, kc, N, 0)
    else:
        sub = E.take(cols, igx.columns.to_device(rows.astype(np.int32)))   # igx_take: any column dtype
        tab.update(sub, kc, len(rows), 0)
    tab.finalize(sync=sync)
    return tab


def _agg_col(rows, kb, x):
    return rows[:, kb + 8 * x:kb + 8 * x + 8].copy().view(np.uint64).ravel()


@pytest.mark.parametrize("sync", [True, False], ids=["sync", "async"])
@pytest.mark.parametrize("name", ["file", "tcp", "generic"])
def test_select_ge_matches_numpy(igx, torch, oracle, name, sync):
    H = igx.columns
    h, cols, widths, kc, aggs, oaggs, knames = _layout(name, igx, oracle)
    tab = _table(igx, oracle, name, sync=sync)
    kb = sum((w + 3) // 4 * 4 for w in widths)
    cap = tab.capacity
    got = {}
    x_list = range(len(aggs)) if name == "generic" else [len(aggs) - 1]
    # before the count is collected (an asynchronous finalize keeps it on the device)
    for x in x_list:
        got[x, 0] = tab.select_ge(x, 0, cap)
    if not sync:
        tab.wait()
    slots = H.host(_slots(tab, torch))
    rows = H.host(tab.gather(_slots(tab, torch)))
    assert np.array_equal(_sorted(rows), _sorted(_ref_rows(oracle, h, knames, oaggs)))   # the table itself
    _, tt_aggs, _ = igx.engine.table_tensors(tab, tab.fin)   # the groups in the slot list's order
    for x in x_list:
        v = H.host(tt_aggs[x])              # masked to the out_width, as gather gives it
        assert np.array_equal(v, _agg_col(rows, kb, x))
        if aggs[x].out_width == 4:
            assert v.max() < 1 << 32 and int(v.max()) > 1 << 31
            full = _agg_col(_ref_rows(oracle, h, knames, [dict(a, out_width=8) for a in oaggs]), kb, x)
            assert (full >= 1 << 32).any()  # the sums did wrap: the comparison below is on the masked value
        vmax, med = int(v.max()), int(np.sort(v)[len(v) // 2])
        for T in (0, 1, med, vmax, vmax + 1, U64):
            s, n = got.get((x, T)) or tab.select_ge(x, T, cap)
            s = H.host(s)
            want = slots[v >= np.uint64(T)]
            print(f"{name} agg {x} T={T}: {n} of {len(slots)} groups")
            assert n == len(want) == len(s)
            assert np.array_equal(np.sort(s), np.sort(want))
        assert got[x, 0][1] == len(slots) and int((v >= np.uint64(vmax + 1)).sum()) == 0
    tab.destroy()


def test_select_ge_cap_below_count(igx, torch, oracle):
    H = igx.columns
    tab = _table(igx, oracle, "file", sync=False)
    ctx = tab.ctx
    cap, CANARY = 100, 0x5A5A5A5A
    buf = torch.full((cap + 64,), CANARY, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.check(ctx.L.igx_groupby_select_ge(tab.h, 3, 1, C.c_void_p(buf.data_ptr()), cap, C.c_void_p(cnt.data_ptr())))
    G = tab.wait()
    slots = H.host(_slots(tab, torch))
    v = _agg_col(H.host(tab.gather(_slots(tab, torch))), 20, 3)
    qual = set(slots[v >= 1].tolist())
    b = H.host(buf)
    assert cap < len(qual) < G and int(cnt.item()) == len(qual)          # the true total, past cap
    assert len(set(b[:cap].tolist())) == cap and set(b[:cap].tolist()) <= qual
    assert (b[cap:] == CANARY).all()
    # cap == 0 counts only (no output buffer at all)
    ctx.check(ctx.L.igx_groupby_select_ge(tab.h, 3, 1, None, 0, C.c_void_p(cnt.data_ptr())))
    assert int(cnt.item()) == len(qual)
    s, n = tab.select_ge(3, 1, cap)
    assert n == len(qual) and s.numel() == cap
    # not after a later update or reset, and not for an aggregate the table does not have
    A = igx._abi
    assert ctx.L.igx_groupby_select_ge(tab.h, 4, 1, C.c_void_p(buf.data_ptr()), cap, C.c_void_p(cnt.data_ptr())) == A.IGX_EINVAL
    tab.reset()
    assert ctx.L.igx_groupby_select_ge(tab.h, 3, 1, C.c_void_p(buf.data_ptr()), cap, C.c_void_p(cnt.data_ptr())) == A.IGX_EINVAL
    tab.destroy()


def _check_lookup(igx, torch, tab, kb, seed=1):
    """every group's key, shuffled and with duplicates, and keys never inserted"""
    H = igx.columns
    slots = _slots(tab, torch)
    rows = tab.gather(slots)
    G = rows.shape[0]
    rng = np.random.default_rng(seed)
    pick = H.to_device(np.concatenate([rng.permutation(G), rng.integers(0, G, G // 2)]).astype(np.int64))
    q = rows[pick].contiguous()
    got, found = tab.lookup(q)                       # gather()'s rows passed as they are
    assert bool(found.bool().all()) and torch.equal(got, q)
    got, found = tab.lookup(q[:, :kb].contiguous())  # packed keys alone
    assert bool(found.bool().all()) and torch.equal(got, q)
    # keys never inserted: existing keys with one byte changed, those that hit another key dropped
    hk = H.host(rows[:, :kb])
    have = set(map(bytes, hk))
    alien = hk[rng.integers(0, G, 3000)].copy()
    alien[:, 0] ^= 0x80
    alien[:, kb - 4] ^= 0x01
    alien = np.array([r for r in alien if bytes(r) not in have], dtype=np.uint8).reshape(-1, kb)
    assert len(alien) > 1000
    mixed = np.concatenate([alien, hk[:500]])
    got, found = tab.lookup(H.to_device(mixed))
    f = H.host(found)
    assert not f[:len(alien)].any() and f[len(alien):].all()
    assert not H.host(got)[:len(alien)].any()
    assert torch.equal(got[len(alien):], rows[:500])
    return rows


@pytest.mark.parametrize("sync", [True, False], ids=["sync", "async"])
@pytest.mark.parametrize("name", ["file", "tcp", "generic"])
def test_lookup_matches_gather(igx, torch, oracle, name, sync):
    widths = _layout(name, igx, oracle)[2]
    kb = sum((w + 3) // 4 * 4 for w in widths)
    tab = _table(igx, oracle, name, sync=sync)
    if not sync:
        # the probe needs no count: look a few keys up before it is collected
        h, cols, _, kc, _, oaggs, knames = _layout(name, igx, oracle)
        k0 = oracle.pad_keys({k: v[:64] for k, v in h.items()}, knames)
        rows0, found0 = tab.lookup(igx.columns.to_device(k0))
        tab.wait()
        assert bool(found0.bool().all())
        assert np.array_equal(igx.columns.host(rows0)[:, :kb], k0)
    _check_lookup(igx, torch, tab, kb)
    # n == 0
    rows, found = tab.lookup(torch.empty((0, kb), dtype=torch.uint8, device="cuda"))
    assert tuple(rows.shape) == (0, kb + 8 * tab.naggs + 8) and tuple(found.shape) == (0,)
    tab.destroy()


@pytest.mark.parametrize("mode", ["cached", "direct", "part"])
@pytest.mark.parametrize("name", ["file", "generic"])
def test_lookup_and_select_in_every_form(igx, torch, oracle, name, mode):
    A, H = igx._abi, igx.columns
    h, cols, widths, kc, aggs, oaggs, knames = _layout(name, igx, oracle)
    kb = sum((w + 3) // 4 * 4 for w in widths)
    tab = _table(igx, oracle, name, mode={"cached": A.GB_CACHED, "direct": A.GB_DIRECT, "part": A.GB_PART}[mode])
    assert tab.info()["form"] == {"cached": A.GB_CACHED, "direct": A.GB_DIRECT, "part": A.GB_PART}[mode]
    rows = H.host(_check_lookup(igx, torch, tab, kb))
    assert np.array_equal(_sorted(rows), _sorted(_ref_rows(oracle, h, knames, oaggs)))
    v = _agg_col(rows, kb, 1)
    med = int(np.sort(v)[len(v) // 2])
    s, n = tab.select_ge(1, med, tab.capacity)
    assert n == int((v >= med).sum())
    assert np.array_equal(np.sort(H.host(s)), np.sort(H.host(_slots(tab, torch))[v >= med]))
    # a second interval in the same form (the direct and partitioned forms start a generation
    # each interval: the first interval's records are stale, not kept)
    half = np.arange(0, N, 2)
    _table(igx, oracle, name, rows=half, tab=tab)
    rows2 = H.host(_check_lookup(igx, torch, tab, kb, seed=2))
    assert np.array_equal(_sorted(rows2), _sorted(_ref_rows(oracle, h, knames, oaggs, rows=half)))
    gone = sorted(set(map(bytes, rows[:, :kb])) - set(map(bytes, rows2[:, :kb])))
    assert len(gone) > 100
    gk = np.frombuffer(b"".join(gone), dtype=np.uint8).reshape(-1, kb).copy()
    got, found = tab.lookup(H.to_device(gk))
    assert not H.host(found).any() and not H.host(got).any()
    tab.destroy()


@pytest.mark.parametrize("name", ["file", "tcp"])
def test_lookup_capacity_equals_keys(igx, torch, oracle, name):
    """capacity == the number of distinct keys: the fullest table the contract allows"""
    h, cols, widths, kc, aggs, oaggs, knames = _layout(name, igx, oracle)
    kb = sum((w + 3) // 4 * 4 for w in widths)
    G = _ref_rows(oracle, h, knames, oaggs).shape[0]
    tab = _table(igx, oracle, name, capacity=G)
    assert tab.fin["n_groups"] == G
    _check_lookup(igx, torch, tab, kb)
    tab.destroy()


@pytest.mark.parametrize("sync", [True, False], ids=["sync", "async"])
def test_lookup_kept_keys_are_not_groups(igx, torch, oracle, sync):
    """Interval 1 feeds the keys A u B, interval 2 only A, in the cached form with the keys
    kept: B's key records stay in the table, but B is no group of interval 2."""
    A_, H = igx._abi, igx.columns
    h, cols, widths, kc, aggs, oaggs, knames = _layout("file", igx, oracle)
    kb = 20
    keys = oracle.pad_keys(h, knames)
    inA = (h["inode"] % np.uint64(2)) == 0          # A: even inodes; B: the others
    rowsA = np.flatnonzero(inA)
    tab = _table(igx, oracle, "file", mode=A_.GB_CACHED)
    G1 = tab.fin["n_groups"]
    _table(igx, oracle, "file", sync=sync, rows=rowsA, tab=tab)
    keysB = np.unique(keys[~inA], axis=0)
    keysA = np.unique(keys[inA], axis=0)
    gotB, foundB = tab.lookup(H.to_device(keysB))
    gotA, foundA = tab.lookup(H.to_device(keysA))
    G2 = tab.wait() if not sync else tab.fin["n_groups"]
    info = tab.info()
    # the keys were kept: interval 2 inserted none, and the generation still holds A u B
    assert info["persist"] == 1 and info["claims"] == 0 and info["gen_keys"] == G1 == len(keysA) + len(keysB)
    assert G2 == len(keysA)
    assert not H.host(foundB).any() and not H.host(gotB).any()
    assert H.host(foundA).all()
    ref = _ref_rows(oracle, h, knames, oaggs, rows=rowsA)     # interval 2's values only
    assert np.array_equal(_sorted(H.host(gotA)), _sorted(ref))
    # select_ge sees interval 2's groups only, too
    s, n = tab.select_ge(0, 0, tab.capacity)
    assert n == len(keysA)
    tab.destroy()


def test_select_and_lookup_are_read_only(igx, torch, oracle):
    A_, H = igx._abi, igx.columns
    h, cols, widths, kc, aggs, oaggs, knames = _layout("file", igx, oracle)
    tab = _table(igx, oracle, "file")
    top = tab.gather(tab.sort([(A_.TSRC_AGG, 3, True)], 20))
    before_counts = tab.topk_counts()
    before = tab.gather(_slots(tab, torch)).clone()
    tab.select_ge(3, 1, tab.capacity)
    tab.select_ge(3, 0, 10)
    tab.lookup(before)
    tab.lookup(top)
    assert tab.topk_counts() == before_counts
    assert torch.equal(tab.gather(_slots(tab, torch)), before)
    assert torch.equal(tab.gather(tab.sort([(A_.TSRC_AGG, 3, True)], 20)), top)
    # the table goes on as if they had not been called: another interval equals the oracle
    rows = np.arange(N // 3, N)
    _table(igx, oracle, "file", rows=rows, tab=tab)
    got = H.host(tab.gather(_slots(tab, torch)))
    assert np.array_equal(_sorted(got), _sorted(_ref_rows(oracle, h, knames, oaggs, rows=rows)))
    tab.destroy()
