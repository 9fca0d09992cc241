"""igx_filter_ex against the plain reference evaluator (tests/pred_reference.py): the two
filter evaluators at the values, widths and row counts where they can differ.

  k_filter_mark_int / pred_eval_int   a chunk (up to four predicates) that holds only integer
                                      comparisons: values loaded zero-extended, then sign-fixed
  k_filter_mark / pred_match/pred_cmp every other chunk -- here one with a string or a float
                                      predicate in it: ints again, float32/64, byte strings on
                                      the 4-byte-word path (aligned base, width % 4 == 0) and
                                      the byte-wise path

Every comparison is an exact equality of the selected row ids, in order.  The shapes are a few
thousand rows at most: ballot-word (64), workgroup (256) and tile (1024) edges.
"""
import numpy as np
import pytest

import pred_reference as R

pytestmark = pytest.mark.gpu

NS = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 5000)


@pytest.fixture(scope="module")
def E(igx):
    return igx.engine


@pytest.fixture(scope="module")
def H(igx):
    return igx.columns


@pytest.fixture(params=["fused-compaction", "split-compaction"])
def compaction(request, monkeypatch):
    """As is: k_filter_compact_sf.  IGX_FILTER_SF_MAX=0 (the A/B knob): k_scan_counts +
    k_filter_compact, which otherwise needs more than 4M rows."""
    if request.param == "split-compaction":
        monkeypatch.setenv("IGX_FILTER_SF_MAX", "0")
    return request.param


def _odd_base(H, a):
    """The (n, w) byte column as a view at storage offset 1 of a flat byte tensor: an odd base
    address (device allocations are at least 256-byte aligned)."""
    n, w = a.shape
    flat = np.zeros(n * w + 1, np.uint8)
    flat[1:] = a.reshape(-1)
    return H.to_device(flat)[1:].view(n, w)


class Dev:
    """Reference columns and their device tensors."""

    def __init__(self, H, cols, odd=()):
        self.cols = cols
        self.n = len(cols[0].values) if cols else 0
        self.t = [_odd_base(H, c.numpy()) if i in odd else H.to_device(c.numpy()) for i, c in enumerate(cols)]


def _run(E, H, igx, d, preds, flags=0, valid=None, dvalid=None):
    got = E.filter_rows(d.t, [R.abi_pred(igx._abi, d.cols, p) for p in preds], d.n,
                        valid=dvalid if dvalid is not None else (None if valid is None else H.to_device(valid)),
                        any=bool(flags & R.F_ANY), nil_match=bool(flags & R.F_NIL_MATCH))
    return H.host(got).astype(np.int64).tolist()


def _tile(vals, n):
    return [vals[i % len(vals)] for i in range(n)]


# ---- row counts, both compactions, survivor patterns --------------------------------------------
def _patterns(n):
    rows = np.arange(n)
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "first": rows == 0, "last": rows == n - 1,
            "alternating": rows % 2 == 1, "lane63": rows % 64 == 63}


def test_row_counts_and_survivor_patterns(E, H, igx, compaction):
    """Every row count of NS (0 included) x survivor pattern (all, none, only row 0, only row
    n-1, alternating, only lane 63 of every 64), through an int-only chunk (k_filter_mark_int)
    and through a chunk with a string predicate (k_filter_mark), in the fused compaction and --
    IGX_FILTER_SF_MAX=0 -- the split scan + compact.  Then the same positions as nil rows: dropped
    without IGX_FILTER_NIL_MATCH, and the only survivors of a negated predicate with it."""
    for n in NS:
        for name, pat in _patterns(n).items():
            want = np.flatnonzero(pat).tolist()
            flag = R.Column("uint", 4, pat.astype(int).tolist())
            text = R.Column("bytes", 4, [b"yes\0" if x else b"no\0\0" for x in pat])
            ones = R.Column("uint", 4, [1] * n)
            d = Dev(H, [flag, text, ones])
            valid = (~pat).astype(np.uint8)
            dv = H.to_device(valid)
            for col, ref in ((0, 1), (1, b"yes")):
                p = R.Pred(col, R.EQ, ref)
                assert R.select(d.cols, [p], n) == want
                assert _run(E, H, igx, d, [p]) == want, (n, name, col)
            # the same positions as nil rows under a predicate that holds on every row
            for p in (R.Pred(2, R.EQ, 1), R.Pred(1, R.GE, b"")):
                w0 = R.select(d.cols, [p], n, valid, 0)
                assert w0 == np.flatnonzero(~pat).tolist()
                assert _run(E, H, igx, d, [p], 0, dvalid=dv) == w0, (n, name, p.col)
                assert _run(E, H, igx, d, [p], R.F_NIL_MATCH, dvalid=dv) == w0, (n, name, p.col)
                # negated it fails on every row but the nil ones: Match(nil) == negate
                q = R.Pred(p.col, p.op, p.ref, negate=True)
                assert R.select(d.cols, [q], n, valid, R.F_NIL_MATCH) == want
                assert _run(E, H, igx, d, [q], R.F_NIL_MATCH, dvalid=dv) == want, (n, name, p.col)
                assert _run(E, H, igx, d, [q], 0, dvalid=dv) == [], (n, name, p.col)


# ---- integers ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,width", [(k, w) for k in ("int", "uint") for w in (1, 2, 4, 8)])
def test_integer_predicates_both_kernels(E, H, igx, kind, width):
    """All five operators x negate on one integer type, values and references from {min, min+1,
    -1, 0, 1, max-1, max} plus ref-1, ref, ref+1.  Each predicate runs alone -- an int-only chunk:
    k_filter_mark_int / pred_eval_int -- and again in a chunk with a neutral string predicate
    (always true under AND, always false under ANY) -- k_filter_mark / pred_cmp's integer path.
    Both agree with the reference, hence with each other."""
    refs = R.int_pool(kind, width)
    vals = R.int_values(kind, width, refs)
    n = 257
    d = Dev(H, [R.Column(kind, width, _tile(vals, n)), R.Column("bytes", 4, [b"x\0\0\0"] * n)])
    true_s, false_s = R.Pred(1, R.EQ, b"x"), R.Pred(1, R.EQ, b"y")
    for ref in refs:
        for op in R.OPS:
            for neg in (False, True):
                p = R.Pred(0, op, ref, neg)
                want = R.select(d.cols, [p], n)
                assert R.select(d.cols, [p, true_s], n) == want == R.select(d.cols, [false_s, p], n, None, R.F_ANY)
                assert _run(E, H, igx, d, [p]) == want, ("int-only", ref, op, neg)
                assert _run(E, H, igx, d, [p, true_s]) == want, ("generic AND", ref, op, neg)
                assert _run(E, H, igx, d, [false_s, p], R.F_ANY) == want, ("generic ANY", ref, op, neg)


# ---- floats -----------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 8])
def test_float_predicates(E, H, igx, width):
    """float32 / float64 through k_filter_mark / pred_cmp: values {+-0, +-Inf, NaN, +-smallest
    subnormal, +-largest finite, 1/3, the neighbours of each reference}, references {0, -0, NaN,
    +-Inf, 0.1, 16777217} (the last two round in a float32 column), five operators x negate.
    A NaN on either side fails every operator and passes every negated one."""
    vals = R.float_values(width)
    n = 2 * len(vals) + 1
    d = Dev(H, [R.Column("float", width, _tile(vals, n))])
    for ref in R.FLOAT_REFS:
        for op in R.OPS:
            for neg in (False, True):
                p = R.Pred(0, op, ref, neg)
                assert _run(E, H, igx, d, [p]) == R.select(d.cols, [p], n), (ref, op, neg)
    # the parser's reference bytes are the ones the matrix used (float32 rounds)
    cols = igx.columns.Columns([("f", "float%d" % (8 * width))])
    for text, ref in (("0.1", 0.1), ("16777217", 16777217.0), ("-0", -0.0), ("-inf", float("-inf"))):
        s = igx.filter.GetFilterFromString(cols, "f:>=" + text)
        assert bytes(s.pred.ref[: s.pred.ref_len]) == R.ref_bytes(d.cols[0], R.Pred(0, R.GE, ref))


# ---- byte strings -----------------------------------------------------------------------------
def _string_cases(w):
    a = b"a" * w
    vals = [b"", b"a", b"\x7f", b"\x80", b"\xff", a, a[:-1] + b"b", a[:-1] + b"`", a[:-1] + b"\x7f",
            a[:-1] + b"\x80", a[:-1] + b"\xff", a[: w // 2], a[: w - 1], a[: w // 2] + b"\x80"[: w - w // 2]]
    refs = [b"", b"a" * 256, a[: max(1, w // 2)], a[:-1] + b"\x80", b"\x80"]
    if w <= R.MAX_REF:
        refs.append(a)                  # equal to the width
    if w < R.MAX_REF:
        refs += [a + b"a", a + b"\x01"]  # longer: the full-width value is the reference's first w bytes
    if w > R.MAX_REF:
        # a column wider than IGX_MAX_REF: the reference reads as zeros past byte 256, so a value
        # with a byte there is greater than any reference it otherwise equals
        m = b"a" * R.MAX_REF
        vals += [m, m + b"\x01", m + b"a", m[:-1] + b"b", m[:-1] + b"`" + b"z" * (w - R.MAX_REF)]
        refs += [m, m[:-1] + b"b"]
    vals = [v for v in dict.fromkeys(vals) if len(v) <= w and b"\0" not in v.rstrip(b"\0")]
    return [v.ljust(w, b"\0") for v in vals], [r for r in dict.fromkeys(refs) if len(r) <= R.MAX_REF]


@pytest.mark.parametrize("base", ["aligned", "odd"])
@pytest.mark.parametrize("w", [1, 3, 4, 6, 16, 17, 64, 255, 256, 300])
def test_string_predicates(E, H, igx, w, base):
    """Byte-string ordering through pred_cmp: the word path (aligned base and width % 4 == 0)
    and the byte-wise path (any other width, or an odd base address).  Values: empty, one byte,
    full width without a NUL, pairs that differ only in the last byte, 0x7F / 0x80 / 0xFF at the
    deciding position, proper prefixes of one another; references: empty, shorter than, equal
    to and longer than the width (the value being the reference's first `width` bytes), and 256
    bytes.  Width 300 is wider than IGX_MAX_REF: reference bytes at or past 256 count as zero."""
    vals, refs = _string_cases(w)
    n = len(vals) + 3
    d = Dev(H, [R.Column("bytes", w, _tile(vals, n))], odd=(0,) if base == "odd" else ())
    assert d.t[0].data_ptr() % 4 == (1 if base == "odd" else 0)
    # any value is >= "": a neutral predicate whose compiled form follows or precedes p's in the
    # kernel arguments, where a read past p's 256 reference bytes would land
    t = R.Pred(0, R.GE, b"")
    for ref in refs:
        for op in R.OPS:
            for neg in (False, True):
                p = R.Pred(0, op, ref, neg)
                want = R.select(d.cols, [p], n)
                assert _run(E, H, igx, d, [p]) == want, (ref[:8], len(ref), op, neg)
                assert _run(E, H, igx, d, [p, t]) == want, ("first of two", ref[:8], len(ref), op, neg)
                assert _run(E, H, igx, d, [t, t, t, p]) == want, ("last of four", ref[:8], len(ref), op, neg)


# ---- chunking and flags -----------------------------------------------------------------------
def _chunk_preds(rng, kinds, negs, q):
    """One predicate per entry of kinds ('i': integer, 'g': float or string), each true -- after
    its negation -- on about q of the rows of _chunk_cols."""
    preds = []
    for j, (k, neg) in enumerate(zip(kinds, negs)):
        t = int(round(1000 * (1 - q if neg else q)))   # v < t holds for t / 1000 of the rows
        t = min(999, max(1, t + int(rng.integers(-30, 30))))
        if k == "i":
            col = int(rng.integers(0, 4))
            ref = t - 500 if col == 0 else t
        else:
            col = 4 + j % 2
            ref = float(t) if col == 4 else b"%03d" % t
        preds.append(R.Pred(col, R.LT, ref, neg))
    return preds


def _chunk_cols(rng, n):
    u = lambda: rng.integers(0, 1000, n)   # noqa: E731
    return [R.Column("int", 2, (u() - 500).tolist()), R.Column("uint", 2, u().tolist()),
            R.Column("int", 4, u().tolist()), R.Column("uint", 8, u().tolist()),
            R.Column("float", 4, [float(x) for x in u()]), R.Column("bytes", 8, [b"%03d" % x for x in u()])]


@pytest.mark.parametrize("npreds", [1, 4, 5, 8, 9])
def test_chunks_flags_and_nil_rows(E, H, igx, compaction, npreds):
    """1, 4, 5, 8 and 9 predicates: one to three mark launches, the later ones combining with
    the mask of the earlier ones (`acc`) in both mark kernels.  Chunks of four are int-only
    (k_filter_mark_int) or hold a float / string predicate (k_filter_mark), in both orders and
    unmixed; all-negated, none-negated and mixed sets; the four flag combinations of
    igx_filter_ex (0, ANY, NIL_MATCH, ANY | NIL_MATCH) over about 10 % nil rows."""
    rng = np.random.default_rng(100 + npreds)
    n = 2049
    d = Dev(H, _chunk_cols(rng, n))
    valid = (rng.random(n) > 0.1).astype(np.uint8)
    dv = H.to_device(valid)
    nchunks = (npreds + 3) // 4
    layouts = {"int-first": "ig", "generic-first": "gi", "all-int": "ii", "all-generic": "gg"}
    for lname, pair in layouts.items():
        kinds = "".join(pair[c % 2] * 4 for c in range(nchunks))[:npreds]
        for nname, negs in (("none", [False] * npreds), ("all", [True] * npreds),
                            ("mixed", [bool((j + j // 4) % 2) for j in range(npreds)])):
            for flags in (0, R.F_ANY, R.F_NIL_MATCH, R.F_ANY | R.F_NIL_MATCH):
                q = 0.12 if flags & R.F_ANY else 0.85
                preds = _chunk_preds(rng, kinds, negs, q)
                want = R.select(d.cols, preds, n, valid, flags)
                assert _run(E, H, igx, d, preds, flags, dvalid=dv) == want, (lname, nname, flags)
                assert 0 < len(want) < n


def test_zero_predicates(E, H, igx, compaction):
    """No predicates: ANY selects nothing; AND selects every row, or only the non-nil rows
    when IGX_FILTER_NIL_MATCH is not set."""
    n = 1025
    d = Dev(H, [R.Column("uint", 4, list(range(n)))])
    valid = (np.arange(n) % 7 != 3).astype(np.uint8)
    alive = np.flatnonzero(valid).tolist()
    for flags, want in ((0, alive), (R.F_NIL_MATCH, list(range(n))), (R.F_ANY, []), (R.F_ANY | R.F_NIL_MATCH, [])):
        assert R.select(d.cols, [], n, valid, flags) == want
        assert _run(E, H, igx, d, [], flags, valid=valid) == want, flags
    assert _run(E, H, igx, d, [], 0) == list(range(n))
