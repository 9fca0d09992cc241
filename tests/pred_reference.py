"""A plain reference evaluator of FilterSpec semantics, `(field OP ref) != negate`, for the
differential predicate tests (test_gpu_filter_matrix.py, test_gpu_groupby_preds.py).

Pure Python over Python ints, floats and bytes: it shares no code with the library or with
oracle.match_rows.  tests/test_filter_parse_host.py checks it on hand-written rows.

  int / uint  the row value and the reference are Python ints in the column's type; the
              reference wraps to the column width (reflect Convert); the compare is exact.
  float       a float32 column rounds the reference to float32 first; both sides compare as
              float64; a NaN on either side makes every operator false, EQ included; the
              result is then XORed with negate.
  bytes       the value is the row's bytes before the first NUL, the reference its raw bytes,
              compared as Python bytes (unsigned, lexicographic, a proper prefix is smaller).
  IN          the value is one of the set, XOR negate.
  guard       rows whose guard value differs from guard_ref pass.
"""
import math

import numpy as np

EQ, REGEX, LT, LE, GT, GE, IN = range(7)
OPS = (EQ, LT, LE, GT, GE)
F_ANY, F_NIL_MATCH = 1, 2
MAX_REF = 256


class Column:
    """kind: 'int' | 'uint' | 'float' | 'bytes'; width in bytes; values: one Python int / float /
    bytes (the raw row, `width` long) per row."""

    def __init__(self, kind, width, values):
        self.kind, self.width, self.values = kind, width, list(values)

    def numpy(self):
        if self.kind == "bytes":
            rows = [v + bytes(self.width - len(v)) for v in self.values]
            return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), self.width).copy()
        dt = {"int": "i", "uint": "u", "float": "f"}[self.kind] + str(self.width)
        return np.array(self.values, dtype=dt)


class Pred:
    """ref: int (int / uint), float, bytes, or a list of ints (IN).  guard: (column index,
    value) or None."""

    def __init__(self, col, op, ref, negate=False, guard=None):
        self.col, self.op, self.ref, self.negate, self.guard = col, op, ref, bool(negate), guard


def wrap_int(v, kind, width):
    """reflect Convert to an integer type of `width` bytes: truncate, reinterpret."""
    bits = 8 * width
    v &= (1 << bits) - 1
    if kind == "int" and v >> (bits - 1):
        v -= 1 << bits
    return v


def int_range(kind, width):
    bits = 8 * width
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if kind == "int" else (0, (1 << bits) - 1)


def _three_way(a, b):
    return (a > b) - (a < b)


def _op(op, c):
    return {EQ: c == 0, LT: c < 0, LE: c <= 0, GT: c > 0, GE: c >= 0}[op]


def match_value(col, v, p):
    """One non-nil row's value against one predicate, the guard aside."""
    if p.op == IN:
        return (v in {wrap_int(x, col.kind, col.width) for x in p.ref}) != p.negate
    if col.kind in ("int", "uint"):
        r = _op(p.op, _three_way(v, wrap_int(p.ref, col.kind, col.width)))
    elif col.kind == "float":
        ref = float(np.float32(p.ref)) if col.width == 4 else float(p.ref)
        v = float(v)
        r = False if (math.isnan(v) or math.isnan(ref)) else _op(p.op, _three_way(v, ref))
    else:
        r = _op(p.op, _three_way(v.split(b"\0")[0], p.ref))
    return r != p.negate


def match_row(cols, row, p):
    if p.guard is not None:
        gcol, gval = p.guard
        if cols[gcol].values[row] != wrap_int(gval, cols[gcol].kind, cols[gcol].width):
            return True
    return match_value(cols[p.col], cols[p.col].values[row], p)


def select(cols, preds, n, valid=None, flags=0):
    """igx_filter_ex as include/igx.h states it: AND of preds, or OR with F_ANY (zero preds then
    select nothing); a nil row (valid == 0) is skipped, or with F_NIL_MATCH yields negate for
    every predicate, combined like the other rows.  Returns the selected row ids in order."""
    out = []
    for row in range(n):
        nil = valid is not None and not valid[row]
        if nil and not flags & F_NIL_MATCH:
            continue
        bits = [p.negate if nil else match_row(cols, row, p) for p in preds]
        if any(bits) if flags & F_ANY else all(bits):
            out.append(row)
    return out


def keep_mask(cols, preds, n, valid=None):
    """The rows a group-by update aggregates: valid and every predicate (uint8 mask)."""
    sel = select(cols, preds, n, valid, 0)
    m = np.zeros(n, np.uint8)
    m[sel] = 1
    return m


def ref_bytes(col, p):
    """The reference as igx_pred.ref holds it: already converted to the column type."""
    if p.op == IN:
        return b"".join(wrap_int(x, "uint", col.width).to_bytes(col.width, "little") for x in p.ref)
    if col.kind in ("int", "uint"):
        return wrap_int(p.ref, "uint", col.width).to_bytes(col.width, "little")
    if col.kind == "float":
        return (np.float32(p.ref) if col.width == 4 else np.float64(p.ref)).tobytes()
    return bytes(p.ref)


def abi_pred(A, cols, p):
    """The igx_pred of a Pred (A: the package's _abi module)."""
    import ctypes as C
    col = cols[p.col]
    rb = ref_bytes(col, p)
    assert len(rb) <= MAX_REF
    q = A.Pred(p.col, p.op, int(p.negate), len(rb), (C.c_uint8 * A.MAX_REF)(*rb))
    if p.guard is not None:
        g = cols[p.guard[0]]
        q.guard_col, q.guard_len = p.guard[0], g.width
        q.guard_ref = (C.c_uint8 * 8)(*wrap_int(p.guard[1], "uint", g.width).to_bytes(g.width, "little").ljust(8, b"\0"))
    return q


# ---- value pools ---------------------------------------------------------------------------
def int_pool(kind, width):
    """{min, min+1, -1, 0, 1, max-1, max} of the type (wrapped into it)."""
    lo, hi = int_range(kind, width)
    return sorted({wrap_int(v, kind, width) for v in (lo, lo + 1, -1, 0, 1, hi - 1, hi)})


def int_values(kind, width, refs):
    """The pool plus ref-1, ref, ref+1 of every reference, wrapped into the type."""
    vals = set(int_pool(kind, width))
    for r in refs:
        vals |= {wrap_int(r + d, kind, width) for d in (-1, 0, 1)}
    return sorted(vals)


FLOAT_REFS = (0.0, -0.0, float("nan"), float("inf"), float("-inf"), 0.1, 16777217.0)


def float_values(width):
    """{+0, -0, +-Inf, NaN, +-smallest subnormal, +-largest finite, 1/3} and the two neighbours
    (nextafter) of every reference as the column holds it."""
    ft = np.float32 if width == 4 else np.float64
    fi = np.finfo(ft)
    sub = float(np.nextafter(ft(0), ft(1)))
    vals = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), sub, -sub, float(fi.max), -float(fi.max),
            float(ft(1) / ft(3))]
    for r in FLOAT_REFS:
        r = ft(r)
        if not np.isnan(r):
            vals += [float(r), float(np.nextafter(r, ft(np.inf))), float(np.nextafter(r, ft(-np.inf)))]
    return vals
