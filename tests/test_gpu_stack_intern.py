"""igx_intern_* on the device against the dict restatement (tests/stack_ref.py), bit for bit:
row shapes and counts around the kernels' edges, duplicates, strides, masks, split invariance,
rows built to collide in home slot and tag, overflow, the argument rules, and a store and a
batch past 4 GiB."""
import ctypes as C

import numpy as np
import pytest

from stack_ref import NO_COL, DictInterner

pytestmark = pytest.mark.gpu

WG_ROWS = 4       # rows per workgroup pass of the wave-per-row kernels (k_stack.hip WPB)
SCAN_TILE = 1024  # rows per tile of the rank scan (k_stack.hip CTILE)


def _dev(igx, a):
    return igx.columns.to_device(np.ascontiguousarray(a))


def _ids(igx, t, rows, valid=None):
    """Device ids of numpy rows (n, row_bytes) uint8 as a list of u32."""
    out = t.add(_dev(igx, rows), None if valid is None else _dev(igx, np.asarray(valid, np.uint8)))
    return igx.columns.host(out).view(np.uint32).tolist()


def _ref_ids(ref, rows, valid=None):
    return ref.add([r.tobytes() for r in rows], valid)


def _rand_rows(rng, n, rb, distinct):
    """n rows of rb bytes drawn from `distinct` random contents."""
    pool = rng.integers(0, 256, (distinct, rb), dtype=np.uint8)
    return pool[rng.integers(0, distinct, n)]


@pytest.mark.parametrize("rb", [8, 16, 1016, 1024])
def test_row_shapes_and_counts(igx, rb):
    rng = np.random.default_rng(rb)
    t, ref = igx.engine.Interner(rb, 4096), DictInterner()
    try:
        for n in (0, 1, 63, 64, 65, WG_ROWS - 1, WG_ROWS, WG_ROWS + 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1):
            rows = _rand_rows(rng, n, rb, max(1, n // 3))
            assert _ids(igx, t, rows) == _ref_ids(ref, rows), (rb, n)
        assert t.count() == len(ref.rows)
        back = igx.columns.host(t.rows(_dev(igx, np.arange(len(ref.rows), dtype=np.int32))))
        assert [r.tobytes() for r in back] == ref.rows
    finally:
        t.destroy()


def test_duplicates(igx):
    rng = np.random.default_rng(1)
    # all rows distinct
    t, ref = igx.engine.Interner(1016, 5000), DictInterner()
    try:
        rows = rng.integers(0, 256, (3001, 1016), dtype=np.uint8)
        assert _ids(igx, t, rows) == list(range(3001)) == _ref_ids(ref, rows)
        # rows that differ only in the last word, and only in the first
        base = rng.integers(0, 256, 1016, dtype=np.uint8)
        rows = np.tile(base, (400, 1))
        rows[:200, 1008:] = rng.integers(0, 256, (200, 8), dtype=np.uint8)
        rows[200:, :8] = rng.integers(0, 256, (200, 8), dtype=np.uint8)
        rows = rows[rng.integers(0, 400, 1500)]
        assert _ids(igx, t, rows) == _ref_ids(ref, rows)
    finally:
        t.destroy()
    # 70 000 identical rows: every row meets the same slot
    t = igx.engine.Interner(1016, 8)
    try:
        one = np.tile(rng.integers(0, 256, 1016, dtype=np.uint8), (70000, 1))
        assert _ids(igx, t, one) == [0] * 70000
        one[69999, 500] ^= 1
        assert _ids(igx, t, one[-3:]) == [0, 0, 1]
        assert t.count() == 2
    finally:
        t.destroy()


def test_stride_and_mask(igx, torch):
    rng = np.random.default_rng(2)
    rb, stride, n = 24, 64, 700
    wide = rng.integers(0, 256, (n, stride), dtype=np.uint8)      # garbage in the gap
    wide[:, :rb] = _rand_rows(rng, n, rb, 90)
    t, ref = igx.engine.Interner(rb, 256), DictInterner()
    try:
        d = _dev(igx, wide)
        got = igx.columns.host(t.add(d[:, :rb])).view(np.uint32).tolist()   # a view: row stride 64
        assert got == _ref_ids(ref, wide[:, :rb])
        # a mask, with an invalid first occurrence followed by a valid one
        rows = _rand_rows(rng, 900, rb, 120)
        rows[0] = rows[5] = rows[9] = rng.integers(0, 256, rb, dtype=np.uint8)
        valid = (rng.integers(0, 3, 900) > 0).astype(np.uint8)
        valid[0], valid[5], valid[9] = 0, 1, 1
        got, want = _ids(igx, t, rows, valid), _ref_ids(ref, rows, valid)
        assert got == want and got[0] == NO_COL and got[5] == got[9] != NO_COL
        assert t.count() == len(ref.rows)
    finally:
        t.destroy()


def test_split_invariance(igx):
    rng = np.random.default_rng(3)
    n, rb = 20011, 1016
    pool = rng.integers(0, 256, (3000, rb), dtype=np.uint8)
    pick = np.minimum(rng.zipf(1.3, n) - 1, 2999)
    stream = pool[pick]
    ref = DictInterner()
    want = _ref_ids(ref, stream)
    cut = int(rng.integers(4098, n - 1))
    results = []
    for cuts in ([], [1, 64, 4097, cut]):
        t = igx.engine.Interner(rb, 4096)
        try:
            got, lo = [], 0
            for hi in cuts + [n]:
                got += _ids(igx, t, stream[lo:hi])
                lo = hi
            results.append(got)
            assert t.count() == len(ref.rows)
            back = igx.columns.host(t.rows(_dev(igx, np.array(got, np.uint32).view(np.int32))))
            assert np.array_equal(back, stream)
            # ids past the count, and IGX_NO_COL, give zero rows
            odd = igx.columns.host(t.rows(_dev(igx, np.array([len(ref.rows), -1, 0], np.int32))))
            assert not odd[:2].any() and odd[2].tobytes() == ref.rows[0]
        finally:
            t.destroy()
    assert results[0] == want and results[1] == want


N_CANDIDATES = 1 << 22   # 4M 8-byte candidates: ~128 pairs expected over 32 + 4 bits


def test_collisions(igx):
    """Rows equal in hash >> 32 and in home slot but different in content, and more than four
    rows on one home slot (include/igx.h states both parts of the hash's use), interleaved."""
    t = igx.engine.Interner(8, 8)
    try:
        S = t.slots()
        assert S >= 16 and S & (S - 1) == 0
        cand = np.arange(N_CANDIDATES, dtype=np.uint64).reshape(-1, 1)
        h = igx.engine.intern_hash_rows(cand)
        key = ((h >> np.uint64(32)) << np.uint64(8)) | (h & np.uint64(S - 1))
        order = np.argsort(key, kind="stable")
        same = np.flatnonzero(key[order][1:] == key[order][:-1])
        assert len(same) > 0, f"no colliding pair among {N_CANDIDATES} candidates"
        pairs = [(int(order[i]), int(order[i + 1])) for i in same[:3]]
        a, b = pairs[0]
        home = int(h[a] & np.uint64(S - 1))
        crowd = [int(x) for x in np.flatnonzero((h & np.uint64(S - 1)) == np.uint64(home))
                 if int(x) not in (a, b)][:5]
        assert len(crowd) == 5
        rng = np.random.default_rng(4)
        for members in ([a, b] + crowd + [12345], [x for p in pairs for x in p] + crowd[:2]):
            members = list(dict.fromkeys(members))[:8]
            t2, ref = igx.engine.Interner(8, 8), DictInterner()
            try:
                seq = np.array(members, np.uint64)[rng.integers(0, len(members), 600)]
                seq[:4] = [members[1], members[0], members[1], members[2]]
                rows = seq.reshape(-1, 1).view(np.uint8)
                # two batches: the second meets the colliding rows in the store
                assert _ids(igx, t2, rows[:300]) == _ref_ids(ref, rows[:300])
                assert _ids(igx, t2, rows[300:]) == _ref_ids(ref, rows[300:])
                assert t2.count() == len(ref.rows) == len(members)
            finally:
                t2.destroy()
    finally:
        t.destroy()


def test_overflow(igx):
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 256, (1000, 16), dtype=np.uint8)
    t = igx.engine.Interner(16, 16)
    try:
        assert len(_ids(igx, t, rows)) == 1000          # the call returns
        with pytest.raises(igx._abi.IgxError) as e:
            t.count()
        assert e.value.code == igx._abi.IGX_ENOSPC
        _ids(igx, t, rows[:10])
        with pytest.raises(igx._abi.IgxError):
            t.count()
    finally:
        t.destroy()
    # more distinct rows than slots: some row finds no slot
    t = igx.engine.Interner(8, 1)
    try:
        _ids(igx, t, rows[:, :8])
        with pytest.raises(igx._abi.IgxError):
            t.count()
    finally:
        t.destroy()
    t, ref = igx.engine.Interner(16, 1000), DictInterner()
    try:
        assert _ids(igx, t, rows) == _ref_ids(ref, rows)
        assert t.count() == 1000
    finally:
        t.destroy()


def test_argument_rules(igx, torch):
    ctx = igx.runtime.context()
    L, EINVAL = ctx.L, igx._abi.IGX_EINVAL
    h = C.c_void_p()
    for rb, cap in ((0, 8), (4, 8), (12, 8), (1032, 8), (16, 0), (16, (1 << 28) + 1)):
        assert L.igx_intern_create(ctx.h, rb, cap, C.byref(h)) == EINVAL and not h.value, (rb, cap)
    assert L.igx_intern_create(ctx.h, 16, 1 << 10, C.byref(h)) == 0
    try:
        n = C.c_uint64()
        assert L.igx_intern_slots(h, C.byref(n)) == 0 and n.value >= 2048 and n.value & (n.value - 1) == 0
        buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        out = torch.zeros(64, dtype=torch.int32, device="cuda")
        p, o = buf.data_ptr(), out.data_ptr()
        add = lambda rows, stride, nrows, ids: L.igx_intern_add(h, C.c_void_p(rows), stride, None, nrows,  # noqa: E731
                                                                C.c_void_p(ids))
        assert add(p + 4, 16, 4, o) == EINVAL          # rows not 8-byte aligned
        assert add(p, 20, 4, o) == EINVAL              # stride not a multiple of 8
        assert add(p, 8, 4, o) == EINVAL               # stride below row_bytes
        assert add(p, 16, 4, o + 2) == EINVAL          # out_ids not 4-byte aligned
        assert add(p, 16, 1 << 31, o) == EINVAL        # more than 2^31 - 1 rows
        assert add(p, 16, 0, o) == 0                   # zero rows are valid
        assert add(p, 24, 4, o) == 0
        assert L.igx_intern_count(h, C.byref(n)) == 0 and n.value == 1
    finally:
        L.igx_intern_destroy(h)


def test_store_and_batch_past_4gib(igx, torch):
    """Byte offsets of the batch and of the store beyond 2^32: all rows distinct (word 0 is the
    row number), so the ids are the row numbers; then rows from the far end are found again."""
    n = (1 << 22) + 5
    rows = torch.zeros((n, 128), dtype=torch.int64, device="cuda")
    rows[:, 0] = torch.arange(n, device="cuda")
    rows[:, 127] = ~torch.arange(n, device="cuda")
    t = igx.engine.Interner(1024, n)
    try:
        ids = t.add(rows.view(torch.uint8))
        assert bool((ids.to(torch.int64) == torch.arange(n, device="cuda")).all())
        tail = rows[n - 7:].view(torch.uint8)
        assert igx.columns.host(t.add(tail)).tolist() == list(range(n - 7, n))
        back = t.rows(ids[n - 7:])
        assert bool((back == tail).all())
        assert t.count() == n
    finally:
        t.destroy()
        del rows
