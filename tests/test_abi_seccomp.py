"""CPU checks of advise seccomp-profile's part of the C ABI: the new symbols are exported and
mirrored in _abi, the argument errors come back before any GPU work, and igx_seccomp_home -- the
host entry to the hash the kernels place namespaces with -- behaves as include/igx.h says.
No GPU: without one no object can be made, so the argument errors here are those a call reports
for a null object or context; tests/test_gpu_seccomp.py repeats them on a live object."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

NEW = ["igx_seccomp_create", "igx_seccomp_update", "igx_seccomp_peek", "igx_seccomp_delete", "igx_seccomp_list",
       "igx_seccomp_count", "igx_seccomp_slots", "igx_seccomp_destroy", "igx_seccomp_home"]


def test_new_symbols_exported_and_mirrored(igx):
    out = subprocess.check_output(["nm", "-D", "--defined-only", igx._abi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (igx_[a-z0-9_]+)", out))
    assert set(NEW) <= exported, set(NEW) - exported
    assert set(NEW) <= {s[0] for s in igx._abi.SIGNATURES}
    for name in NEW:
        assert getattr(igx.lib(), name).argtypes is not None
    assert igx._abi.SECCOMP_VALUE_BYTES == 501 and igx._abi.SECCOMP_SYSCALLS == 500


def test_argument_errors_need_no_gpu(igx):
    L, EINVAL = igx.lib(), igx._abi.IGX_EINVAL
    h = C.c_void_p()
    assert L.igx_seccomp_create(None, 0, 157, 317, C.byref(h)) == EINVAL and not h.value      # capacity 0
    assert L.igx_seccomp_create(None, 1024, 157, 317, C.byref(h)) == EINVAL and not h.value   # no context
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.igx_seccomp_update(None, None, None, None, None, 16, None, None, 4) == EINVAL    # null columns
    assert L.igx_seccomp_update(None, p, p, p, p, 3, None, None, 4) == EINVAL                 # comm_stride < 4
    n = C.c_uint64()
    assert L.igx_seccomp_peek(None, p, 1, p, p) == EINVAL
    assert L.igx_seccomp_delete(None, p, 1) == EINVAL
    assert L.igx_seccomp_list(None, p, 1, C.byref(n)) == EINVAL
    assert L.igx_seccomp_count(None, C.byref(n)) == EINVAL
    assert L.igx_seccomp_slots(None, C.byref(n)) == EINVAL
    assert L.igx_seccomp_destroy(None) == 0


def test_home_is_deterministic_and_below_nslots(igx):
    rng = np.random.default_rng(11)
    keys = [0, 1, 2, 4026531840, 4026532000, (1 << 64) - 1] + [int(k) for k in rng.integers(1, 1 << 63, 200)]
    for nslots in (1, 2, 2048, 4096, 1 << 20):
        homes = [igx.engine.seccomp_home(k, nslots) for k in keys]
        assert all(0 <= h < nslots for h in homes)
        assert homes == [igx.engine.seccomp_home(k, nslots) for k in keys]
    # the home among 2 S slots extends the home among S by one bit: the hash does not depend on S
    for k in keys:
        assert igx.engine.seccomp_home(k, 4096) & 2047 == igx.engine.seccomp_home(k, 2048)
    # it spreads: 200 random keys do not all land in a few of 2048 slots
    assert len({igx.engine.seccomp_home(k, 2048) for k in keys}) > 150
    h = C.c_uint64()
    for bad in (0, 3, 6, 1000):
        assert igx.lib().igx_seccomp_home(5, bad, C.byref(h)) == igx._abi.IGX_EINVAL
        with pytest.raises(igx._abi.IgxError):
            igx.engine.seccomp_home(5, bad)
    assert igx.lib().igx_seccomp_home(5, 8, None) == igx._abi.IGX_EINVAL
