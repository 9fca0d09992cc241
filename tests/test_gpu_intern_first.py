"""igx_intern_add_first on the device: the first-appearance mask against a Python set walk, with
and without a nil mask; rows built to collide in hash tag and home slot; splits into two and five
calls equal to one call; and igx_intern_add's ids unchanged when both entry points run on equal
streams (the 16-byte rows are trace capabilities' unique key: cap, four zero bytes, mntns)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _dev(igx, a):
    return igx.columns.to_device(np.ascontiguousarray(a))


def _walk(rows, valid=None, seen=None):
    """1 where a valid row's content was not seen before, over all calls sharing `seen`."""
    seen = set() if seen is None else seen
    out = np.zeros(len(rows), np.uint8)
    for i, r in enumerate(rows):
        if valid is not None and not valid[i]:
            continue
        b = r.tobytes()
        if b not in seen:
            seen.add(b)
            out[i] = 1
    return out


def _first(igx, t, rows, valid=None):
    ids, first = t.add(_dev(igx, rows), None if valid is None else _dev(igx, np.asarray(valid, np.uint8)), first=True)
    return igx.columns.host(ids).view(np.uint32), igx.columns.host(first)


def _cap_rows(rng, n, ncap=41, nns=8):
    """n unique keys of --unique: cap u32, four zero bytes, mntns u64."""
    rows = np.zeros((n, 16), np.uint8)
    rows[:, 0:4] = rng.integers(0, ncap, n).astype(np.uint32).view(np.uint8).reshape(n, 4)
    rows[:, 8:16] = (np.uint64(4026531840) + rng.integers(0, nns, n).astype(np.uint64)).view(np.uint8).reshape(n, 8)
    return rows


@pytest.mark.parametrize("masked", [False, True], ids=["all-valid", "nil-mask"])
def test_mask_against_set_walk(igx, masked):
    rng = np.random.default_rng(5)
    n = 5003                                   # five scan tiles, the last one partial
    rows = _cap_rows(rng, n)
    valid = (rng.random(n) >= 0.4).astype(np.uint8) if masked else None
    if masked:                                 # an invalid first occurrence followed by two valid ones
        rows[0] = rows[7] = rows[11] = np.frombuffer(np.array([77, 0, 99, 0], np.uint32).tobytes(), np.uint8)
        valid[0], valid[7], valid[11] = 0, 1, 1
    t = igx.engine.Interner(16, 1024)
    try:
        ids, first = _first(igx, t, rows, valid)
        want = _walk(rows, valid)
        assert np.array_equal(first, want) and 200 < int(want.sum()) < 400
        if masked:
            assert first[0] == 0 and first[7] == 1 and first[11] == 0 and ids[0] == 0xFFFFFFFF
        assert t.count() == int(want.sum())
        # a first row's id is its rank among the first rows
        assert np.array_equal(ids[want == 1], np.arange(int(want.sum()), dtype=np.uint32))
    finally:
        t.destroy()


def test_rows_equal_in_tag_and_home_slot(igx):
    t = igx.engine.Interner(8, 8)
    try:
        S = t.slots()
        cand = np.arange(1 << 22, dtype=np.uint64).reshape(-1, 1)
        h = igx.engine.intern_hash_rows(cand)
        key = ((h >> np.uint64(32)) << np.uint64(8)) | (h & np.uint64(S - 1))
        order = np.argsort(key, kind="stable")
        same = np.flatnonzero(key[order][1:] == key[order][:-1])
        assert len(same) > 0, "no colliding pair among the candidates"
        a, b = int(order[same[0]]), int(order[same[0] + 1])
        rows = np.array([a, b, a, b, b, a, a + (1 << 40)], np.uint64).reshape(-1, 1).view(np.uint8)
        ids, first = _first(igx, t, rows)
        assert first.tolist() == [1, 1, 0, 0, 0, 0, 1] and ids.tolist() == [0, 1, 0, 1, 1, 0, 2]
        ids, first = _first(igx, t, rows[::-1].copy())
        assert not first.any() and ids.tolist() == [2, 0, 1, 1, 0, 1, 0]
    finally:
        t.destroy()


@pytest.mark.parametrize("ncalls", [2, 5])
def test_splits_equal_one_call(igx, ncalls):
    rng = np.random.default_rng(6 + ncalls)
    n = 9001
    rows = _cap_rows(rng, n, ncap=60, nns=40)
    valid = (rng.random(n) >= 0.2).astype(np.uint8)
    want = _walk(rows, valid)
    assert int(want.sum()) > 1500
    cuts = [0] + sorted(int(x) for x in rng.choice(np.arange(1, n), ncalls - 1, replace=False)) + [n]
    t1, tk = igx.engine.Interner(16, 4096), igx.engine.Interner(16, 4096)
    try:
        ids1, first1 = _first(igx, t1, rows, valid)
        parts = [_first(igx, tk, rows[lo:hi], valid[lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:])]
        assert all(int(p[1].sum()) > 0 for p in parts)          # every call admits something new
        assert np.array_equal(first1, want)
        assert np.array_equal(np.concatenate([p[1] for p in parts]), want)
        assert np.array_equal(np.concatenate([p[0] for p in parts]), ids1)
    finally:
        t1.destroy()
        tk.destroy()


def test_add_ids_unchanged(igx):
    """igx_intern_add and igx_intern_add_first on equal streams give equal ids, also when the calls
    alternate on one object, and the mask can be had without the ids."""
    rng = np.random.default_rng(8)
    rows = _cap_rows(rng, 6000, ncap=50, nns=30)
    valid = (rng.random(6000) >= 0.1).astype(np.uint8)
    ta, tf, tm = (igx.engine.Interner(16, 2048) for _ in range(3))
    try:
        H = igx.columns
        plain = [H.host(ta.add(_dev(igx, rows[lo:lo + 2000]), _dev(igx, valid[lo:lo + 2000]))).view(np.uint32)
                 for lo in (0, 2000, 4000)]
        mixed = [_first(igx, tf, rows[:2000], valid[:2000])[0],
                 H.host(tf.add(_dev(igx, rows[2000:4000]), _dev(igx, valid[2000:4000]))).view(np.uint32),
                 _first(igx, tf, rows[4000:], valid[4000:])[0]]
        assert all(np.array_equal(p, m) for p, m in zip(plain, mixed))
        assert ta.count() == tf.count() > 1000
        # out_ids NULL: the mask alone
        torch = igx.runtime.torch_mod()
        d, v = _dev(igx, rows), _dev(igx, valid)
        mask = torch.empty(6000, dtype=torch.uint8, device=d.device)
        p = igx.runtime.ptr
        tm.ctx.check(tm.ctx.L.igx_intern_add_first(tm.h, p(d), 16, p(v), 6000, None, p(mask)))
        assert np.array_equal(H.host(mask), _walk(rows, valid)) and tm.count() == ta.count()
    finally:
        for t in (ta, tf, tm):
            t.destroy()
