"""Host checks (no GPU): the number forms igx_filter_parse takes, against Go's strconv
(ParseInt / ParseUint base 10, ParseFloat) as filter.go:53-87 calls it, and the plain reference
evaluator of the predicate tests (tests/pred_reference.py) on hand-written rows."""
import numpy as np
import pytest

import pred_reference as R


@pytest.fixture(scope="module")
def cols(igx):
    return igx.columns.Columns([(k, k) for k in ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32",
                                                 "uint64", "float32", "float64")])


def _parse(igx, cols, text):
    """The compiled reference bytes, or None when the parser rejects the filter."""
    try:
        s = igx.filter.GetFilterFromString(cols, text)
    except igx.filter.FilterError:
        return None
    return bytes(s.pred.ref[: s.pred.ref_len])


def _int(b, signed):
    return int.from_bytes(b, "little", signed=signed)


def test_parse_integer_forms(igx, cols):
    """strconv.ParseInt(s, 10, 64) / ParseUint(s, 10, 64): signs, the 64-bit limits, no
    exponent / base prefix / underscore / empty value; then Convert truncation."""
    P = lambda t: _parse(igx, cols, t)   # noqa: E731
    assert _int(P("int64:+5"), True) == 5
    assert _int(P("int64:-0"), True) == 0
    assert _int(P("int64:9223372036854775807"), True) == 2**63 - 1
    assert _int(P("int64:-9223372036854775808"), True) == -2**63
    assert P("int64:9223372036854775808") is None
    assert P("int64:-9223372036854775809") is None
    assert _int(P("uint64:18446744073709551615"), False) == 2**64 - 1
    assert P("uint64:18446744073709551616") is None
    assert P("uint32:+1") is None and P("uint64:+1") is None and P("uint8:-1") is None
    for bad in ("1e3", "0x10", "1_000", "", "+", "-", " 1", "1 "):
        assert P("int32:" + bad) is None, bad
        assert P("uint32:" + bad) is None, bad
    assert _int(P("int8:300"), True) == 44
    assert _int(P("uint16:65537"), False) == 1
    assert _int(P("int32:-4294967295"), True) == 1
    assert len(P("int8:300")) == 1 and len(P("uint16:65537")) == 2 and len(P("int32:-4294967295")) == 4


def test_parse_float_forms(igx, cols):
    """strconv.ParseFloat(s, 64): decimal forms, underflow to 0, hex floats with a 'p' exponent,
    inf / infinity (signed) and nan (unsigned) in any letter case; range and syntax errors."""
    P = lambda t: _parse(igx, cols, t)   # noqa: E731
    f64 = lambda t: np.frombuffer(P("float64:" + t), np.float64)[0]   # noqa: E731
    assert f64(".5") == 0.5 and f64("5.") == 5.0 and f64("+.5") == 0.5 and f64("-5.") == -5.0
    assert f64("1e-400") == 0.0
    assert f64("0x1p-2") == 0.25 and f64("0X1P-2") == 0.25 and f64("-0x1.8p1") == -3.0
    for t in ("inf", "Inf", "INF", "+inf", "infinity", "+Infinity", "INFINITY"):
        assert f64(t) == np.inf, t
    for t in ("-inf", "-Infinity", "-INF"):
        assert f64(t) == -np.inf, t
    for t in ("NaN", "nan", "NAN"):
        assert np.isnan(f64(t)), t
    assert np.signbit(f64("-0")) and f64("-0") == 0.0
    # rejected: a range error, a truncated special, a hex mantissa without its exponent, a sign on nan
    for bad in ("1e400", "-1e400", "infin", "0x1", "0x1.8", "-0x10", "+nan", "-nan", "+NaN", "", "+", "e5", "1e",
                "1 ", "0x", "nanx", "in"):
        assert P("float64:" + bad) is None, bad
        assert P("float32:" + bad) is None, bad
    # a float32 column stores the reference rounded to float32
    for t, v in (("0.1", 0.1), ("16777217", 16777217.0), ("1e-400", 0.0), ("0x1p-2", 0.25), ("-inf", -np.inf),
                 ("-0", -0.0)):
        assert P("float32:" + t) == np.float32(v).tobytes(), t
        assert P("float64:" + t) == np.float64(v).tobytes(), t
    assert np.isnan(np.frombuffer(P("float32:nan"), np.float32)[0])


# ---- the reference evaluator, on rows small enough to check by eye ---------------------------
def _sel(col, op, ref, negate=False):
    return R.select([col], [R.Pred(0, op, ref, negate)], len(col.values))


def test_reference_ints():
    c = R.Column("int", 1, [-128, -1, 0, 1, 127])
    assert _sel(c, R.LT, 0) == [0, 1]
    assert _sel(c, R.GE, -1) == [1, 2, 3, 4]
    assert _sel(c, R.EQ, -1) == [1]
    assert _sel(c, R.EQ, 255) == [1]                        # Convert truncation: 255 -> int8 -1
    assert _sel(c, R.LE, 128) == [0]                        # 128 -> int8 -128
    assert _sel(c, R.EQ, 0, negate=True) == [0, 1, 3, 4]
    u = R.Column("uint", 2, [0, 1, 65535])
    assert _sel(u, R.GT, 1) == [2]
    assert _sel(u, R.EQ, -1) == [2] and _sel(u, R.EQ, 65537) == [1]
    assert _sel(u, R.IN, [0, 65535]) == [0, 2] and _sel(u, R.IN, [0, 65535], negate=True) == [1]
    assert R.ref_bytes(c, R.Pred(0, R.EQ, -2)) == b"\xfe" and R.ref_bytes(u, R.Pred(0, R.IN, [1, 258])) == b"\1\0\2\1"


def test_reference_floats():
    nan, inf = float("nan"), float("inf")
    c = R.Column("float", 8, [nan, -0.0, 0.0, 0.1, inf])
    assert _sel(c, R.EQ, nan) == []                          # NaN EQ NaN is false
    assert _sel(c, R.EQ, nan, negate=True) == [0, 1, 2, 3, 4]
    assert _sel(c, R.LE, inf) == [1, 2, 3, 4]                # the NaN row fails every operator
    assert _sel(c, R.LE, inf, negate=True) == [0]            # ... and passes every negated one
    assert _sel(c, R.EQ, 0.0) == [1, 2] and _sel(c, R.EQ, -0.0) == [1, 2]   # -0 == +0
    assert _sel(c, R.LT, 0.0) == [] and _sel(c, R.GE, -0.0) == [1, 2, 3, 4]
    assert _sel(c, R.EQ, 0.1) == [3]
    f = R.Column("float", 4, [float(np.float32(0.1)), 16777216.0, 16777218.0])
    assert _sel(f, R.EQ, 0.1) == [0]                         # the reference rounds to float32 first
    assert _sel(f, R.EQ, 16777217.0) == [1] and _sel(f, R.GT, 16777217.0) == [2]
    assert R.ref_bytes(f, R.Pred(0, R.EQ, 16777217.0)) == np.float32(16777216.0).tobytes()


def test_reference_bytes():
    rows = [b"", b"ab", b"abc", b"ab\x7f", b"ab\x80", b"b"]
    c = R.Column("bytes", 4, [r.ljust(4, b"\0") for r in rows])
    assert _sel(c, R.LT, b"abc") == [0, 1]                   # "ab" < "abc": a proper prefix is smaller
    assert _sel(c, R.GT, b"ab\x7f") == [4, 5]                # 0x80 > 0x7F: bytes are unsigned
    assert _sel(c, R.EQ, b"") == [0] and _sel(c, R.EQ, b"", negate=True) == [1, 2, 3, 4, 5]
    assert _sel(c, R.LE, b"abcde") == [0, 1, 2]              # a reference longer than the column
    assert _sel(c, R.GE, b"abcd") == [3, 4, 5]
    full = R.Column("bytes", 3, [b"abc", b"abd"])            # full width, no NUL
    assert _sel(full, R.LT, b"abcd") == [0] and _sel(full, R.EQ, b"abc") == [0]
    assert c.numpy().shape == (6, 4) and bytes(c.numpy()[1]) == b"ab\0\0"


def test_reference_guard_flags_and_nil():
    v = R.Column("int", 4, [5, -5, 5, -5])
    g = R.Column("uint", 1, [1, 1, 0, 0])
    cols = [v, g]
    p = R.Pred(0, R.GT, 0, guard=(1, 1))                     # v > 0 where g == 1; other rows pass
    assert R.select(cols, [p], 4) == [0, 2, 3]
    assert R.keep_mask(cols, [p], 4, valid=[1, 1, 0, 1]).tolist() == [1, 0, 0, 1]
    pos, neg = R.Pred(0, R.GT, 0), R.Pred(0, R.GT, 0, negate=True)
    valid = [1, 1, 0, 0]
    assert R.select(cols, [pos], 4, valid, 0) == [0]
    assert R.select(cols, [pos], 4, valid, R.F_NIL_MATCH) == [0]          # Match(nil) == negate
    assert R.select(cols, [neg], 4, valid, R.F_NIL_MATCH) == [1, 2, 3]
    assert R.select(cols, [pos, neg], 4, valid, R.F_NIL_MATCH) == []      # MatchAll: every pred negated
    assert R.select(cols, [pos, neg], 4, valid, R.F_ANY | R.F_NIL_MATCH) == [0, 1, 2, 3]
    assert R.select(cols, [pos, neg], 4, valid, R.F_ANY) == [0, 1]
    # zero predicates: nothing under ANY; every row under AND, the non-nil ones without NIL_MATCH
    assert R.select(cols, [], 4, valid, R.F_ANY) == [] and R.select(cols, [], 4, valid, R.F_ANY | R.F_NIL_MATCH) == []
    assert R.select(cols, [], 4, valid, 0) == [0, 1] and R.select(cols, [], 4, valid, R.F_NIL_MATCH) == [0, 1, 2, 3]
