"""igx_lw_join (the two-register last-writer join on the device) against the sequential restatement
in tests/lwjoin_ref.py: all three output arrays, both counts and the live rows, bit for bit.

Sizes: the contract's hand cases; 0, 1 and the scan tile - 1 / tile / tile + 1 / 3 tiles + 5 rows
(the tile comes from the library) and 1024 tiles + 1 row (more tiles than the carry and the count
scan have threads); one key for 70 000 rows (a run across many tiles and workgroups)
and 70 000 distinct keys; 200 000 rows over 64 keys that differ in byte 7 only, and in byte 0 only
(the sort's digit plan at both ends); SET_A-heavy, TAKE-only and T T A T T streams; one key whose B
has to cross every tile boundary between a SET_A at row 0 and a TAKE_A at the last row; a nil mask;
kinds 4 and 255; pend_cap below the live count; the row limit and misalignment; batch invariance.

Every random case states a floor on its emissions and pending rows; the seeds were chosen so that
lwjoin_ref alone meets the floor (a case that emits nothing proves nothing)."""
import ctypes as C

import numpy as np
import pytest

import lwjoin_ref as R

pytestmark = pytest.mark.gpu


def _device_join(igx, key, kind, valid=None, pend_cap=None):
    H = igx.columns
    j = igx.engine.lw_join(H.to_device(key), H.to_device(kind), None if valid is None else H.to_device(valid),
                           pend_cap=pend_cap)
    got = {k: H.host(j[k]).view(np.uint32) for k in ("take", "a", "b", "pend")}
    return got, j["n_take"], j["n_pend"]


def _check(igx, key, kind, valid=None):
    take, a, b, live = R.join_arrays(key, kind, valid)
    got, nt, npend = _device_join(igx, key, kind, valid)
    assert nt == len(take) and npend == len(live)
    assert np.array_equal(got["take"], take)
    assert np.array_equal(got["a"], a)
    assert np.array_equal(got["b"], b)
    assert np.array_equal(got["pend"], live)
    return take, b, live


@pytest.mark.parametrize("case", R.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(igx, case):
    _, key, kind, emitted, live = case
    got, nt, npend = _device_join(igx, key, kind)
    assert [tuple(int(x) for x in t) for t in zip(got["take"], got["a"], got["b"])] == emitted
    assert list(got["pend"]) == live and nt == len(emitted) and npend == len(live)


def test_tile_edges(igx):
    tile = igx.engine.lw_join_tile()
    for n in (0, 1, tile - 1, tile, tile + 1, 3 * tile + 5):
        key, kind = R.random_stream(n, 5, seed=100 + n % 7) if n else (np.zeros(0, np.uint64), np.zeros(0, np.uint8))
        take, b, live = _check(igx, key, kind)
        # floor: 100 emissions, 50 of them with a B row, and 3 pending rows from one tile on
        assert n < tile - 1 or (len(take) > 100 and int((b != R.NONE).sum()) > 50 and len(live) >= 3)


def test_more_tiles_than_scan_threads(igx):
    """1025 scan tiles and 2049 compaction tiles: threads of the one-workgroup carry (1024) and of
    the count scan (1024) each fold more than one tile, which no smaller case makes them do."""
    n = 1024 * igx.engine.lw_join_tile() + 1
    key, kind = R.random_stream(n, 5, seed=1)
    take, b, live = _check(igx, key, kind)
    assert len(take) > 100_000 and int((b != R.NONE).sum()) > 50_000 and len(live) >= 3


def test_one_key_many_tiles(igx):
    n = 70_000
    _, kind = R.random_stream(n, 1, seed=3)
    key = np.full(n, 0x00001234000056C0, np.uint64)
    take, b, live = _check(igx, key, kind)
    assert len(take) > 3000 and 1000 < int((b != R.NONE).sum()) < len(take) - 1000
    assert len(live) == 2                              # one key: both registers end full


def test_all_distinct_keys(igx):
    n = 70_000
    _, kind = R.random_stream(n, 1, seed=4)
    key = np.uint64(1 << 32) + np.random.default_rng(4).permutation(n).astype(np.uint64) * np.uint64(64)
    take, _, live = _check(igx, key, kind)
    assert len(take) == 0 and len(live) == int((kind <= R.SET_B).sum()) and len(live) > 30_000


@pytest.mark.parametrize("shift", [56, 0], ids=["byte7", "byte0"])
def test_keys_differ_in_one_byte(igx, shift):
    n = 200_000
    rng = np.random.default_rng(shift + 1)
    _, kind = R.random_stream(n, 1, seed=5 + shift)
    ids = rng.permutation(256)[:64].astype(np.uint64)
    base = np.uint64(0x0000123412345600) if shift == 56 else np.uint64(0x1234123412345600)
    key = base + (ids[rng.integers(0, 64, n)] << np.uint64(shift))
    take, b, live = _check(igx, key, kind)
    assert len(take) > 10_000 and int((b != R.NONE).sum()) > 3000 and len(live) > 20


@pytest.mark.parametrize("mix", ["seta-heavy", "take-only", "ttatt"])
def test_adversarial_mixes(igx, mix):
    n = 30_000
    key, kind = R.random_stream(n, 7, seed=21, p_kind=(0.85, 0.05, 0.05, 0.05))
    if mix == "take-only":
        kind[:] = R.TAKE_A
    elif mix == "ttatt":
        kind = np.tile(np.array([R.TAKE_A, R.TAKE_A, R.SET_A, R.TAKE_A, R.TAKE_A], np.uint8), n // 5)
        key = np.repeat(key[: n // 5], 5)          # each T T A T T on one key, keys interleaved in blocks
    take, _, live = _check(igx, key, kind)
    if mix == "take-only":
        assert len(take) == 0 and len(live) == 0
    elif mix == "ttatt":
        assert len(take) == n // 5                 # exactly the T after each A
    else:
        assert len(take) > 1000 and len(live) >= 7


@pytest.mark.parametrize("end", ["set", "clear"])
def test_b_crosses_every_tile(igx, end):
    """One key: SET_A at row 0, TAKE_A at the last row, 70 000 SET_B / CLEAR_B rows between.  The
    A row and the last B writer are handed over every tile boundary in between."""
    m = 70_000
    mid = np.random.default_rng(9).choice(np.array([R.SET_B, R.CLEAR_B], np.uint8), m)
    mid[-1] = R.SET_B if end == "set" else R.CLEAR_B
    kind = np.concatenate([[R.SET_A], mid, [R.TAKE_A]]).astype(np.uint8)
    key = np.full(m + 2, 0x0000ABCD0000ABCE, np.uint64)
    take, b, live = _check(igx, key, kind)
    assert list(take) == [m + 1]
    assert list(b) == ([m] if end == "set" else [R.NONE])
    assert list(live) == ([m] if end == "set" else [])


def test_valid_mask(igx):
    n = 50_000
    key, kind = R.random_stream(n, 300, seed=31)
    valid = (np.random.default_rng(32).random(n) >= 0.3).astype(np.uint8)
    take, b, live = _check(igx, key, kind, valid)
    assert len(take) > 1500 and len(live) > 200
    # the same as joining the surviving rows alone, with their ids mapped back
    keep = np.flatnonzero(valid)
    t2, a2, b2, l2 = R.join_arrays(key[keep], kind[keep])
    assert np.array_equal(keep[t2], take) and np.array_equal(keep[l2], live)
    assert np.array_equal(np.where(b2 == R.NONE, R.NONE, keep[np.where(b2 == R.NONE, 0, b2)]), b)


def test_other_kinds_are_ignored(igx):
    n = 20_000
    key, kind = R.random_stream(n, 50, seed=41)
    rng = np.random.default_rng(42)
    kind[rng.random(n) < 0.15] = 4
    kind[rng.random(n) < 0.15] = 255
    take, _, live = _check(igx, key, kind)
    assert len(take) > 500 and len(live) > 30


def test_pend_cap_below_live_count(igx, torch):
    H = igx.columns
    n, cap = 10_000, 37
    key, kind = R.random_stream(n, 4000, seed=61, p_kind=(0.4, 0.4, 0.1, 0.1))
    _, _, _, live = R.join_arrays(key, kind)
    assert len(live) > 10 * cap
    ctx = igx.runtime.context()
    d = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3)]
    pend = torch.full((cap + 3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    p = igx.runtime.ptr
    t = [H.to_device(x) for x in (key, kind)]
    ctx.check(ctx.L.igx_lw_join(ctx.h, p(t[0]), p(t[1]), None, n, p(d[0]), p(d[1]), p(d[2]),
                                C.c_void_p(cnt.data_ptr()), p(pend), cap, C.c_void_p(cnt.data_ptr() + 8)))
    got = pend.cpu().numpy().view(np.uint32)
    assert int(cnt[1]) == len(live)
    assert np.array_equal(got[:cap], live[:cap])
    assert np.all(got[cap:] == 0x5A5A5A5A)


def test_argument_checks_on_a_live_context(igx, torch):
    """nrows = 2^32 - 1 is refused before any argument is looked at (the pointers are null); then
    the null counts, a misaligned key and a misaligned row output."""
    ctx = igx.runtime.context()
    L, EINVAL = ctx.L, igx._abi.IGX_EINVAL
    assert L.igx_lw_join(ctx.h, None, None, None, (1 << 32) - 1, None, None, None, None, None, 0, None) == EINVAL
    assert b"rows" in L.igx_last_error(ctx.h)
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    p, odd, odd4 = C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + 4), C.c_void_p(buf.data_ptr() + 2)
    q = C.c_void_p(buf.data_ptr() + 256)
    assert L.igx_lw_join(ctx.h, p, p, None, 4, p, p, p, None, p, 4, q) == EINVAL
    assert b"null count" in L.igx_last_error(ctx.h)
    assert L.igx_lw_join(ctx.h, odd, p, None, 4, p, p, p, q, p, 4, q) == EINVAL
    assert b"8-byte aligned" in L.igx_last_error(ctx.h)
    assert L.igx_lw_join(ctx.h, p, p, None, 4, p, odd4, p, q, p, 4, q) == EINVAL
    assert b"4-byte aligned" in L.igx_last_error(ctx.h)
    assert L.igx_lw_join(ctx.h, p, None, None, 4, p, p, p, q, p, 4, q) == EINVAL
    assert b"null argument" in L.igx_last_error(ctx.h)


@pytest.mark.parametrize("ncuts", [1, 2, 7])
def test_batch_invariance(igx, ncuts):
    """One stream cut at random points and fed batch by batch with the carry in front gives the
    emissions of the whole stream, row ids mapped back."""
    n = 40_000
    key, kind = R.random_stream(n, 500, seed=71)
    cuts = sorted(int(x) for x in np.random.default_rng(72 + ncuts).choice(np.arange(1, n), ncuts, replace=False))
    whole, live = R.join(key, kind)
    assert len(whole) > 2000 and len(live) > 400

    def device(k, kd, v):
        got, nt, npend = _device_join(igx, k, kd, v)
        assert nt == len(got["take"]) and npend == len(got["pend"])
        return list(zip(got["take"], got["a"], got["b"])), got["pend"]

    em, lv = R.join_batches(key, kind, cuts, join_fn=device)
    assert em == whole and lv == live
