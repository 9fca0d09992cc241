"""CPU checks of traceloop's part of the C ABI: the two symbols are declared in include/igx.h,
exported by the library and mirrored in _abi, and the argument errors that igx_traceloop_join
reports before any GPU work come back without a GPU (without one there is no context, so these
are the errors of a null context; tests/test_gpu_traceloop.py repeats the rest on a live one)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

NEW = ["igx_traceloop_join", "igx_traceloop_tile"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_declared_exported_and_mirrored(igx):
    header = open(os.path.join(ROOT, "include", "igx.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", igx._abi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (igx_[a-z0-9_]+)", out))
    assert set(NEW) <= exported, set(NEW) - exported
    assert set(NEW) <= {s[0] for s in igx._abi.SIGNATURES}
    sig = dict((s[0], s[2]) for s in igx._abi.SIGNATURES)
    assert len(sig["igx_traceloop_join"]) == 22 and sig["igx_traceloop_tile"] == []
    for name in NEW:
        assert getattr(igx.lib(), name).argtypes is not None


def test_tile_needs_no_gpu(igx):
    t = igx.engine.traceloop_tile()
    assert t == igx.lib().igx_traceloop_tile() and t >= 64 and t % 64 == 0


def test_null_context_is_einval(igx):
    L, EINVAL = igx.lib(), igx._abi.IGX_EINVAL
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.igx_traceloop_join(None, None, p, p, p, p, p, None, 4, None, p, p, None, 2, 60, 231, 15,
                                p, p, p, p, p) == EINVAL
    assert L.igx_traceloop_join(None, None, None, None, None, None, None, None, 0, None, None, None, None, 0,
                                60, 231, 15, None, None, None, None, None) == EINVAL
