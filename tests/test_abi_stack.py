"""CPU checks of profile cpu's part of the C ABI: the new symbols are exported and mirrored in
_abi, and igx_intern_hash_rows -- the host entry to the hash the kernels use -- behaves as
include/igx.h says.  No GPU."""
import re
import subprocess

import numpy as np
import pytest

NEW = ["igx_intern_create", "igx_intern_add", "igx_intern_count", "igx_intern_rows", "igx_intern_slots",
       "igx_intern_destroy", "igx_intern_hash_rows", "igx_ksym_lookup"]


def test_new_symbols_exported_and_mirrored(igx):
    out = subprocess.check_output(["nm", "-D", "--defined-only", igx._abi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (igx_[a-z0-9_]+)", out))
    assert set(NEW) <= exported, set(NEW) - exported
    assert set(NEW) <= {s[0] for s in igx._abi.SIGNATURES}
    for name in NEW:
        assert getattr(igx.lib(), name).argtypes is not None


def test_hash_agrees_across_strides(igx):
    rng = np.random.default_rng(5)
    for rb in (8, 16, 24, 1016, 1024):
        rows = rng.integers(0, 256, (37, rb), dtype=np.uint8)
        h = igx.engine.intern_hash_rows(rows)
        assert len(set(h.tolist())) == 37
        for stride in (rb + 8, rb + 64, 2048):
            wide = rng.integers(0, 256, (37, stride), dtype=np.uint8)   # garbage in the gap
            wide[:, :rb] = rows
            assert np.array_equal(igx.engine.intern_hash_rows(wide, row_bytes=rb), h), (rb, stride)
        # one row at a time, from a buffer of its own
        assert [int(igx.engine.intern_hash_rows(rows[i:i + 1].copy())[0]) for i in range(37)] == h.tolist()
    # the row length is part of the hash: a zero row of 8 bytes and one of 16 differ
    assert igx.engine.intern_hash_rows(np.zeros((1, 8), np.uint8))[0] != \
        igx.engine.intern_hash_rows(np.zeros((1, 16), np.uint8))[0]


def test_hash_depends_on_word_order(igx):
    rng = np.random.default_rng(6)
    for nw in (2, 3, 127, 128):
        row = rng.integers(1, 1 << 62, nw, dtype=np.uint64)
        h = igx.engine.intern_hash_rows(row.reshape(1, nw))[0]
        seen = {int(h)}
        for _ in range(20):
            p = rng.permutation(nw)
            if np.array_equal(row[p], row):
                continue
            seen.add(int(igx.engine.intern_hash_rows(row[p].reshape(1, nw))[0]))
        assert len(seen) > 1 and (nw > 3 or len(seen) >= 2)
        sw = row.copy()
        sw[0], sw[-1] = row[-1], row[0]
        assert igx.engine.intern_hash_rows(sw.reshape(1, nw))[0] != h
    # differing in the first word only, and in the last only
    a = np.zeros((3, 127), np.uint64)
    a[1, 0] = 1
    a[2, 126] = 1
    assert len(set(igx.engine.intern_hash_rows(a).tolist())) == 3


def test_hash_rejects_bad_shapes(igx):
    import ctypes as C
    L = igx.lib()
    buf = np.zeros(4096, np.uint8)
    out = np.zeros(4, np.uint64)
    p, o = buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for rb, stride in ((0, 8), (4, 8), (12, 16), (1032, 1032), (16, 8)):
        assert L.igx_intern_hash_rows(p, rb, stride, 1, o) == igx._abi.IGX_EINVAL, (rb, stride)
    assert L.igx_intern_hash_rows(p, 16, 16, 0, None) == 0
    with pytest.raises(igx._abi.IgxError):
        igx.engine.intern_hash_rows(np.zeros((1, 12), np.uint8))
