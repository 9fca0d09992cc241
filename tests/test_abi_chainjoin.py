"""CPU checks of the chained join's and trace tcp's part of the C ABI: the symbols are declared in
include/igx.h, exported by the library and mirrored in _abi, the enum values match the header, the
tile query needs no GPU, and the argument errors come back without one (without a GPU there is no
context, so the row limit, a misaligned key and null arguments all meet the null-context check
first and must return IGX_EINVAL without touching a pointer; tests/test_gpu_chainjoin.py repeats
them on a live context, where the order of the checks shows)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

NEW = ["igx_chain_join", "igx_chain_join_tile", "igx_tcp_classify"]
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
    assert len(sig["igx_chain_join"]) == 12 and sig["igx_chain_join_tile"] == [] and len(sig["igx_tcp_classify"]) == 11
    for name in NEW:
        assert getattr(igx.lib(), name).argtypes is not None


def test_enums_match_the_header(igx):
    header = open(os.path.join(ROOT, "include", "igx.h")).read()
    m = re.search(r"enum igx_cj_kind \{([^}]*)\}", header)
    vals = dict((k, int(v)) for k, v in re.findall(r"IGX_(CJ_[A-Z_]+) = (\d+)", m.group(1)))
    assert vals == {"CJ_ENTER": 0, "CJ_PASS": 1, "CJ_ABORT": 2, "CJ_TAKE": 3, "CJ_DROP": 4, "CJ_HELD": 5}
    for k, v in vals.items():
        assert getattr(igx._abi, k) == v
    m = re.search(r"enum igx_tcp_probe \{([^}]*)\}", header)
    vals = dict((k, int(v)) for k, v in re.findall(r"IGX_(TCP_[A-Z_]+) = (\d+)", m.group(1)))
    assert vals == {"TCP_CONNECT_ENTER": 0, "TCP_CONNECT_RETURN": 1, "TCP_CLOSE": 2, "TCP_SET_STATE": 3,
                    "TCP_ACCEPT_RETURN": 4}
    for k, v in vals.items():
        assert getattr(igx._abi, k) == v
    assert re.search(r"#define IGX_TCP_NO_KIND 255\b", header) and igx._abi.TCP_NO_KIND == 255
    assert re.search(r"#define IGX_TCP_TUPLE_BYTES 40\b", header) and igx._abi.TCP_TUPLE_BYTES == 40
    # the row struct of the mirror has the header's fields in the header's order
    m = re.search(r"typedef struct \{([^}]*)\} igx_tcp_rows;", header)
    fields = re.findall(r"\*(\w+);", m.group(1))
    assert fields == [f[0] for f in igx._abi.TcpRows._fields_] == list(igx.engine.TCP_ROW_FIELDS)


def test_tile_needs_no_gpu(igx):
    t = igx.engine.chain_join_tile()
    assert t == igx.lib().igx_chain_join_tile() and t >= 64 and t % 64 == 0


def test_null_context_is_einval(igx):
    L, EINVAL = igx.lib(), igx._abi.IGX_EINVAL
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data_as(C.c_void_p)
    odd = C.c_void_p(buf.ctypes.data + 1)
    assert L.igx_chain_join(None, p, p, p, None, 4, p, p, p, p, 4, p) == EINVAL
    assert L.igx_chain_join(None, None, None, None, None, 0, None, None, None, None, 0, None) == EINVAL
    # the row limit and a misaligned key with no context: still IGX_EINVAL, and no pointer is read
    assert L.igx_chain_join(None, None, None, None, None, (1 << 32) - 1, None, None, None, None, 0, None) == EINVAL
    assert L.igx_chain_join(None, odd, p, p, None, 4, p, p, p, p, 4, p) == EINVAL
    assert L.igx_chain_join(None, p, odd, p, None, 4, p, p, p, p, 4, p) == EINVAL
    rows = igx._abi.TcpRows(*([p] * 14))
    assert L.igx_tcp_classify(None, C.byref(rows), 4, 0, 0xFFFFFFFF, None, 0, p, p, p, p) == EINVAL
    assert L.igx_tcp_classify(None, None, 0, 0, 0xFFFFFFFF, None, 0, None, None, None, None) == EINVAL
    assert L.igx_tcp_classify(None, None, (1 << 32) - 1, 0, 0, None, 0, None, None, None, None) == EINVAL
