"""CPU checks of the last-writer join's and the first-appearance mask's part of the C ABI: the
symbols are declared in include/igx.h, exported by the library and mirrored in _abi, the tile query
needs no GPU, and the argument errors come back without one (without a GPU there is no context, so
the row limit, a misaligned key and null arguments all meet the null-context check first and must
return IGX_EINVAL without touching a pointer; tests/test_gpu_lwjoin.py repeats them on a live
context, where the order of the checks shows)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

NEW = ["igx_lw_join", "igx_lw_join_tile", "igx_intern_add_first"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_declared_exported_and_mirrored(igx):
    header = open(os.path.join(ROOT, "include", "igx.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", igx._abi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (igx_[a-z0-9_]+)", out))
    assert set(NEW) <= exported, set(NEW) - exported
    sig = dict((s[0], s[2]) for s in igx._abi.SIGNATURES)
    assert set(NEW) <= set(sig)
    assert len(sig["igx_lw_join"]) == 12 and sig["igx_lw_join_tile"] == [] and len(sig["igx_intern_add_first"]) == 7
    for name in NEW:
        assert getattr(igx.lib(), name).argtypes is not None


def test_kinds_match_the_header(igx):
    header = open(os.path.join(ROOT, "include", "igx.h")).read()
    m = re.search(r"enum igx_lw_kind \{([^}]*)\}", header)
    vals = dict((k, int(v)) for k, v in re.findall(r"IGX_(LW_[A-Z_]+) = (\d+)", m.group(1)))
    assert vals == {"LW_SET_A": 0, "LW_SET_B": 1, "LW_CLEAR_B": 2, "LW_TAKE_A": 3}
    for k, v in vals.items():
        assert getattr(igx._abi, k) == v


def test_tile_needs_no_gpu(igx):
    t = igx.engine.lw_join_tile()
    assert t == igx.lib().igx_lw_join_tile() and t >= 64 and t % 64 == 0


def test_null_context_is_einval(igx):
    L, EINVAL = igx.lib(), igx._abi.IGX_EINVAL
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data_as(C.c_void_p)
    odd = C.c_void_p(buf.ctypes.data + 1)
    assert L.igx_lw_join(None, p, p, None, 4, p, p, p, p, p, 4, p) == EINVAL
    assert L.igx_lw_join(None, None, None, None, 0, None, None, None, None, None, 0, None) == EINVAL
    # the row limit and a misaligned key with no context: still IGX_EINVAL, and no pointer is read
    assert L.igx_lw_join(None, None, None, None, (1 << 32) - 1, None, None, None, None, None, 0, None) == EINVAL
    assert L.igx_lw_join(None, odd, p, None, 4, p, p, p, p, p, 4, p) == EINVAL
    assert L.igx_intern_add_first(None, p, 16, None, 4, p, p) == EINVAL
    assert L.igx_intern_add_first(None, None, 0, None, 0, None, None) == EINVAL
