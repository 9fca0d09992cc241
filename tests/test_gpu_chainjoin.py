"""igx_chain_join (the join through two chained maps on the device) against the sequential
restatement in tests/tcptracer_ref.py: both row arrays, both counts and the pending list, bit for
bit.

T is igx_chain_join_tile().  Sizes 0, 1, 2, T - 1, T, T + 1, 3T + 17; one key1 run and one key2 run
spanning three tiles; ENTER, PASS and TAKE of one connection in three different tiles; every kind
after every kind on one key, for both maps; the contract's hand cases; valid masks; pend_cap below
the true count; the argument checks on a live context; random streams cut into batches with the
in-band carry (PASS -> HELD).

Every random case first asserts on the CPU that the restatement emits and leaves an ENTER and a
PASS pending: a join that emits nothing cannot pass."""
import ctypes as C
import itertools

import numpy as np
import pytest

import tcptracer_ref as R

pytestmark = pytest.mark.gpu

E, P, A, T, D, H = R.ENTER, R.PASS, R.ABORT, R.TAKE, R.DROP, R.HELD
KINDS = (E, P, A, T, D, H)


def _u64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64))


def _device_join(igx, key1, key2, kind, valid=None, pend_cap=None):
    Hc = igx.columns
    j = igx.engine.chain_join(Hc.to_device(_u64(key1)), Hc.to_device(_u64(key2)),
                              Hc.to_device(np.asarray(kind, np.uint8)),
                              None if valid is None else Hc.to_device(np.asarray(valid, np.uint8)), pend_cap=pend_cap)
    got = {k: Hc.host(j[k]).view(np.uint32) for k in ("take", "pass", "pend")}
    return got, j["n_take"], j["n_pend"]


def _check(igx, key1, key2, kind, valid=None):
    take, pas, live = R.chain_join_arrays(key1, key2, kind, valid)
    got, nt, npend = _device_join(igx, key1, key2, kind, valid)
    assert nt == len(take) and npend == len(live)
    assert np.array_equal(got["take"], take)
    assert np.array_equal(got["pass"], pas)
    assert np.array_equal(got["pend"], live)
    return take, pas, live


def _pending_kinds(kind, live):
    return {int(kind[i]) for i in live}


def test_hand_cases(igx):
    x = [7] * 8
    cases = [([E, P, T], None, None), ([P, T], None, None), ([T], None, None), ([E, A, T], None, None),
             ([E, P, D, T], None, None), ([E, P, T, T], None, None), ([H, T], None, None),
             ([E, P, E, P, T], None, None), ([E, E, P], None, None), ([E, P, E], None, None),
             ([E, E, P, T], [1, 2, 1, 9], [5, 5, 5, 5]), ([H, H, D, H, T], None, None)]
    expect = [([(2, 1)], []), ([], []), ([], []), ([], []), ([], []), ([(2, 1)], []), ([(1, 0)], []),
              ([(4, 3)], []), ([], [2]), ([], [1, 2]), ([(3, 2)], [1]), ([(4, 3)], [])]
    for (kinds, k1, k2), (em, live) in zip(cases, expect):
        n = len(kinds)
        assert R.chain_join(k1 or x[:n], k2 or x[:n], kinds) == (em, live), kinds
        got, nt, npend = _device_join(igx, k1 or x[:n], k2 or x[:n], kinds)
        assert list(zip(got["take"], got["pass"])) == em and list(got["pend"]) == live, kinds
        assert nt == len(em) and npend == len(live)


def test_tile_edges(igx):
    t = igx.engine.chain_join_tile()
    for n in (0, 1, 2, t - 1, t, t + 1, 3 * t + 17):
        key1, key2, kind = R.random_chain_stream(n, 16, 8, seed=100 + n % 7)
        take, _, live = _check(igx, key1, key2, kind)
        if n >= t - 1:
            assert len(take) > 50 and _pending_kinds(kind, live) >= {E, P}


def test_one_key_runs_span_three_tiles(igx):
    """All rows of one thread and one tuple: both sorts leave one run over 3T + 17 rows, so every
    tile boundary hands both maps' state over."""
    t = igx.engine.chain_join_tile()
    n = 3 * t + 17
    _, _, kind = R.random_chain_stream(n, 1, 1, seed=5, p_other=0.0)
    take, _, live = _check(igx, np.full(n, 0x1234567, np.uint64), np.full(n, 0xABCDEF, np.uint64), kind)
    assert len(take) > 100 and len(live) >= 1


def test_enter_pass_take_in_three_tiles(igx):
    """One connection: ENTER in tile 0, PASS in tile 1, TAKE in tile 2; everything between belongs
    to other threads and tuples, or is an attempt on the same keys that must not disturb it."""
    t = igx.engine.chain_join_tile()
    n = 3 * t
    key1, key2, kind = R.random_chain_stream(n, 32, 16, seed=6)
    me1, me2 = np.uint64(0xFFFF0001), np.uint64(0xFFFF0002)
    for r, k in ((5, E), (t + 9, P), (2 * t + 11, T)):
        key1[r], key2[r], kind[r] = me1, me2, k
    take, pas, _ = _check(igx, key1, key2, kind)
    assert (2 * t + 11, t + 9) in set(zip(take.tolist(), pas.tolist()))


@pytest.mark.parametrize("which", ["map1", "map2", "both"])
def test_every_kind_after_every_kind(igx, which):
    """All 36 ordered pairs of kinds on one key, each pair on empty maps, after an ENTER and after
    a HELD, and closed by a TAKE that shows what map 2 ended with: <= 4 rows per key, a key per
    case, all cases and many copies of them in one call, ordered so that a key's rows are far
    apart.  map1: the rows of a case share key1 and every row has a key2 of its own (what map 1
    ends with shows in the pending list); map2: the other way round; both: they share both."""
    cases = []
    for a, b in itertools.product(KINDS, KINDS):
        for prefix in ((), (E,), (H,)):
            cases.append(list(prefix) + [a, b, T])
    assert len(cases) == 108
    copies = 24
    key1, key2, kind, pos = [], [], [], []
    uniq = itertools.count(1 << 40)
    for c, kinds in enumerate(cases * copies):
        for j, k in enumerate(kinds):
            key1.append((1 << 20) + c if which != "map2" else next(uniq))
            key2.append((1 << 30) + c if which != "map1" else next(uniq))
            kind.append(k)
            pos.append((j, c))
    order = sorted(range(len(pos)), key=lambda i: pos[i])      # row j of every case before row j + 1
    key1, key2, kind = (np.array(x)[order] for x in (key1, key2, kind))
    take, _, live = _check(igx, key1, key2, kind.astype(np.uint8))
    if which == "both":
        assert len(take) > 20 * copies
    if which != "map2":
        assert E in _pending_kinds(kind, live)
    assert len(kind) > 8000 and len(cases) * copies > 2000


def test_pass_without_enter_and_take_without_pass(igx):
    n = 5000
    key1, key2, kind = R.random_chain_stream(n, 40, 20, seed=9, p_kind=(0.0, 0.5, 0.1, 0.3, 0.1, 0.0))
    take, _, live = _check(igx, key1, key2, kind)
    assert len(take) == 0 and len(live) == 0
    key1, key2, kind = R.random_chain_stream(n, 40, 20, seed=10, p_kind=(0.5, 0.0, 0.1, 0.3, 0.1, 0.0))
    take, _, live = _check(igx, key1, key2, kind)
    assert len(take) == 0 and _pending_kinds(kind, live) == {E}


def test_valid_mask(igx):
    n = 20_000
    key1, key2, kind = R.random_chain_stream(n, 64, 32, seed=31)
    valid = (np.random.default_rng(32).random(n) >= 0.3).astype(np.uint8)
    take, pas, live = _check(igx, key1, key2, kind, valid)
    assert len(take) > 300 and _pending_kinds(kind, live) >= {E, P}
    keep = np.flatnonzero(valid)
    t2, p2, l2 = R.chain_join_arrays(key1[keep], key2[keep], kind[keep])
    assert np.array_equal(keep[t2], take) and np.array_equal(keep[p2], pas) and np.array_equal(keep[l2], live)
    _check(igx, key1, key2, kind, np.zeros(n, np.uint8))


def test_pend_cap_below_live_count(igx, torch):
    Hc = igx.columns
    n, cap = 10_000, 37
    key1, key2, kind = R.random_chain_stream(n, 4000, 4000, seed=61, p_kind=(0.5, 0.3, 0.02, 0.05, 0.03, 0.1))
    _, _, live = R.chain_join_arrays(key1, key2, kind)
    assert len(live) > 10 * cap
    ctx = igx.runtime.context()
    d = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2)]
    pend = torch.full((cap + 3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    p = igx.runtime.ptr
    t = [Hc.to_device(x) for x in (key1, key2, kind)]
    ctx.check(ctx.L.igx_chain_join(ctx.h, p(t[0]), p(t[1]), p(t[2]), None, n, p(d[0]), p(d[1]),
                                   C.c_void_p(cnt.data_ptr()), p(pend), cap, C.c_void_p(cnt.data_ptr() + 8)))
    got = pend.cpu().numpy().view(np.uint32)
    assert int(cnt[1]) == len(live)
    assert np.array_equal(got[:cap], live[:cap])
    assert np.all(got[cap:] == 0x5A5A5A5A)


def test_argument_checks_on_a_live_context(igx, torch):
    """In the documented order: the row limit before any argument is looked at (the pointers are
    null); then the null counts, their alignment, null arguments, the keys' and the row outputs'
    alignment."""
    ctx = igx.runtime.context()
    L, EINVAL = ctx.L, igx._abi.IGX_EINVAL
    assert L.igx_chain_join(ctx.h, None, None, None, None, (1 << 32) - 1, None, None, None, None, 0, None) == EINVAL
    assert b"rows" in L.igx_last_error(ctx.h)
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    p, odd, odd4 = C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + 4), C.c_void_p(buf.data_ptr() + 2)
    q = C.c_void_p(buf.data_ptr() + 256)
    assert L.igx_chain_join(ctx.h, p, p, p, None, 4, p, p, None, p, 4, q) == EINVAL
    assert b"null count" in L.igx_last_error(ctx.h)
    assert L.igx_chain_join(ctx.h, p, p, p, None, 4, p, p, odd, p, 4, q) == EINVAL
    assert b"counts not 8-byte aligned" in L.igx_last_error(ctx.h)
    assert L.igx_chain_join(ctx.h, p, None, p, None, 4, p, p, q, p, 4, q) == EINVAL
    assert b"null argument" in L.igx_last_error(ctx.h)
    assert L.igx_chain_join(ctx.h, p, p, p, None, 4, p, p, q, None, 4, q) == EINVAL
    assert b"null argument" in L.igx_last_error(ctx.h)
    assert L.igx_chain_join(ctx.h, p, odd, p, None, 4, p, p, q, p, 4, q) == EINVAL
    assert b"keys must be 8-byte aligned" in L.igx_last_error(ctx.h)
    assert L.igx_chain_join(ctx.h, p, p, p, None, 4, p, odd4, q, p, 4, q) == EINVAL
    assert b"4-byte aligned" in L.igx_last_error(ctx.h)
    # 0 rows are valid and clear the counts, whatever the other pointers are
    cnt = torch.full((2,), 77, dtype=torch.int64, device="cuda")
    assert L.igx_chain_join(ctx.h, None, None, None, None, 0, None, None, C.c_void_p(cnt.data_ptr()), None, 0,
                            C.c_void_p(cnt.data_ptr() + 8)) == 0
    assert cnt.tolist() == [0, 0]


@pytest.mark.parametrize("seed,nthreads,ntuples", [(71, 8, 4), (72, 24, 12), (73, 64, 32)])
def test_random_streams_cut_into_batches(igx, seed, nthreads, ntuples):
    t = igx.engine.chain_join_tile()
    n = 5 * t + seed
    key1, key2, kind = R.random_chain_stream(n, nthreads, ntuples, seed=seed)
    whole, live = R.chain_join(key1, key2, kind)
    assert len(whole) >= 1 and _pending_kinds(kind, live) >= {E, P}
    take, _, _ = _check(igx, key1, key2, kind)
    assert len(take) == len(whole)
    cuts = sorted(int(x) for x in np.random.default_rng(seed + 1000).choice(np.arange(1, n), 3, replace=False))
    # the restatement itself is invariant under the cut, and at least one cut carries both kinds
    assert R.chain_join_batches(key1, key2, kind, cuts) == (whole, live)

    def device(k1, k2, kd, v):
        got, nt, npend = _device_join(igx, k1, k2, kd, v)
        assert nt == len(got["take"]) and npend == len(got["pend"])
        return list(zip(got["take"].tolist(), got["pass"].tolist())), got["pend"].tolist()

    em, lv = R.chain_join_batches(key1, key2, kind, cuts, join_fn=device)
    assert em == whole and lv == live
