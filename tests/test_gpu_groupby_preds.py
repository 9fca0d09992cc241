"""Group-by predicates against the plain reference evaluator (tests/pred_reference.py).

igx_groupby_update evaluates its predicates in three places:
  fused in the cached / direct forms   row_raw -> assemble -> pred_scalar (k_gb_table.h): up to
                                       two scalar comparisons or IN sets on 1/2/4/8-byte columns;
                                       the value is cut out of a loaded dword by (row * width) & 3,
                                       or taken from the SUM's own loaded value (pshare); a guard is
                                       read from an aggregate's condition value (pguard)
  fused in the partitioned form        k_gbp_mask (k_gb_part.hip): ld_val, the guard from gptr
  spilled to the row mask              k_pred_mask -> pred_match (k_common.h): string rules, a third
                                       scalar comparison, a guard on a column that is no aggregate's
                                       condition column (pred_match's gwidth branch)

A tiny table (key: one u8 column with 8 distinct values, capacity 64; COUNT and one SUM) makes
every kept row visible in the result: the expected groups are oracle.groupby(..., valid=keep)
with keep from the reference evaluator, compared exactly (keys, both aggregates, first index).
Up to eight predicate sets share one interval: set j feeds its rows under the keys 8j..8j+7.
Every set runs in IGX_GB_CACHED, IGX_GB_DIRECT and IGX_GB_PART, at n in NS, as one update and
as two updates; the second update's columns are interior slices of larger tensors, cut at a
multiple of four rows: a 1- or 2-byte non-key column that starts off a 4-byte boundary is
outside igx.h's alignment contract and rejected (test_misaligned_columns_are_rejected).
"""
import ctypes as C

import numpy as np
import pytest

import pred_reference as R

pytestmark = pytest.mark.gpu

NS = (1, 3, 64, 257, 1000, 4099)
NMAX = max(NS)
PAD = 9        # rows that stay behind every slice
MODES = ("GB_CACHED", "GB_DIRECT", "GB_PART")


@pytest.fixture(scope="module")
def E(igx):
    return igx.engine


@pytest.fixture(scope="module")
def H(igx):
    return igx.columns


def _padded(a):
    """a with PAD more rows of 0xA5 bytes."""
    tail = np.frombuffer(bytes([0xA5]) * (PAD * a[:1].nbytes), dtype=a.dtype).reshape((PAD,) + a.shape[1:])
    return np.concatenate([a, tail])


def _cut(n):
    """Where the two-update feed cuts: a multiple of four rows, so that every column of the second
    update starts on a 4-byte boundary (igx.h: a 1- or 2-byte column off one is rejected)."""
    return (n // 2) & ~3


class Data:
    """Columns of NMAX rows: 0 = the key (row % 8), 1 = the SUM's value column, the others as the
    test needs them.  Smaller row counts read a prefix."""

    def __init__(self, H, cols, valid=None):
        key = R.Column("uint", 1, [i % 8 for i in range(NMAX)])
        self.cols = [key] + list(cols)
        assert all(len(c.values) == NMAX for c in self.cols)
        self.np = [c.numpy() for c in self.cols]
        self.t = [H.to_device(_padded(a)) for a in self.np]
        self.keyt = [H.to_device(_padded((self.np[0] + 8 * j).astype(np.uint8))) for j in range(8)]
        self.valid = valid
        self.dvalid = None if valid is None else H.to_device(_padded(valid))
        self._keep = {}

    def keep(self, preds):
        """The reference's kept rows over all NMAX rows (a prefix serves a smaller n)."""
        k = id(preds)
        if k not in self._keep:
            self._keep[k] = (preds, R.keep_mask(self.cols, preds, NMAX, self.valid))
        return self._keep[k][1]


class Tables:
    """One table per (mode, aggregate variant): key u8, capacity 64, COUNT (optionally where
    column cond_col == cond_val) and SUM of column 1 (optionally divided)."""

    def __init__(self, E, A):
        self.E, self.A, self.tabs = E, A, {}

    def get(self, mode, cond=None, div=0):
        k = (mode, cond, div)
        if k not in self.tabs:
            A = self.A
            aggs = [A.Agg(A.AGG_COUNT, 0, A.NO_COL if cond is None else cond[0], 8, 0 if cond is None else cond[1]),
                    A.Agg(A.AGG_SUM, 1, A.NO_COL, 8, 0, div)]
            t = self.E.Table([1], aggs, 64)
            t.set_mode(getattr(A, mode))
            self.tabs[k] = t
        return self.tabs[k]

    def destroy(self):
        for t in self.tabs.values():
            t.destroy()


def _groups(E, H, tab):
    fin = tab.finalize()
    keys, aggs, first = E.table_tensors(tab, fin)
    gk = H.host(keys)[:, 0]
    assert len(set(gk.tolist())) == len(gk) == fin["n_groups"], "duplicate groups"
    ga, gf = [H.host(a) for a in aggs], H.host(first)
    return {int(k): (int(ga[0][i]), int(ga[1][i]), int(gf[i])) for i, k in enumerate(gk)}


def _run_batch(E, H, A, oracle, tab, data, sets, n, feed, cond=None, div=0):
    """Up to 8 predicate sets in one interval; returns the indices of the sets that differ."""
    assert len(sets) <= 8
    tab.reset()
    cuts = [0, n] if feed == "one" else [0, _cut(n), n]
    for j, preds in enumerate(sets):
        ap = [R.abi_pred(A, data.cols, p) for p in preds]
        for a, b in zip(cuts, cuts[1:]):
            cols = [data.keyt[j][a:b]] + [t[a:b] for t in data.t[1:]]
            tab.update(cols, [0], b - a, j * n + a, preds=ap,
                       valid=None if data.dvalid is None else data.dvalid[a:b])
    m = len(sets)
    keys = np.concatenate([data.np[0][:n] + 8 * j for j in range(m)]).astype(np.uint8).reshape(-1, 1)
    keep = np.concatenate([data.keep(p)[:n] for p in sets])
    count = {"kind": "count"}
    if cond is not None:
        count.update(cond=np.tile(data.np[cond[0]][:n], m), cond_val=cond[1])
    okeys, oaggs, ofirst = oracle.groupby(keys, [count, {"kind": "sum", "val": np.tile(data.np[1][:n], m), "div": div}],
                                          valid=keep)
    want = {int(k[0]): (int(oaggs[0][i]), int(oaggs[1][i]), int(ofirst[i])) for i, k in enumerate(okeys)}
    got = _groups(E, H, tab)
    bad = sorted({k // 8 for k in set(want) | set(got) if want.get(k) != got.get(k)})
    return bad, want, got


def _describe(p):
    return (p.col, p.op, p.ref if not isinstance(p.ref, bytes) else p.ref[:12], p.negate, p.guard)


def _matrix(E, H, igx, oracle, data, sets, cond=None, div=0, ns=NS):
    """Every predicate set x mode x row count x feed."""
    A = igx._abi
    tabs = Tables(E, A)
    try:
        for mode in MODES:
            tab = tabs.get(mode, cond, div)
            for n in ns:
                for feed in ("one", "two"):
                    if feed == "two" and _cut(n) == 0:
                        continue
                    for b in range(0, len(sets), 8):
                        bad, want, got = _run_batch(E, H, A, oracle, tab, data, sets[b:b + 8], n, feed, cond, div)
                        assert not bad, (mode, n, feed, [[_describe(p) for p in sets[b + j]] for j in bad],
                                         {k: (want.get(k), got.get(k)) for k in set(want) | set(got)
                                          if want.get(k) != got.get(k)})
    finally:
        tabs.destroy()


def _tile(vals, n=NMAX):
    return [vals[i % len(vals)] for i in range(n)]


def _value_col():
    return R.Column("uint", 4, [(3 * i + 1) & 0xFFFFFFFF for i in range(NMAX)])


def _singles_and_pairs(col, refs):
    singles = [[R.Pred(col, op, ref, neg)] for ref in refs for op in R.OPS for neg in (False, True)]
    pairs = [[singles[i][0], singles[(i * 7 + 3) % len(singles)][0]] for i in range(0, len(singles), 2)]
    return singles + pairs


# ---- fused scalar predicates --------------------------------------------------------------------
@pytest.mark.parametrize("kind,width", [(k, w) for k in ("int", "uint") for w in (1, 2, 4, 8)])
def test_fused_integer_predicates(E, H, igx, oracle, kind, width):
    """One and two scalar comparisons per update on every integer type, fused in cached/direct
    (row_raw -> assemble -> pred_scalar) and fused in partitioned (k_gbp_mask / ld_val): all five
    operators x negate, values and references from the type's extremes.  The 1- and 2-byte
    columns are read at every (row * width) & 3, and each row's verdict shows in its group."""
    refs = R.int_pool(kind, width)
    data = Data(H, [_value_col(), R.Column(kind, width, _tile(R.int_values(kind, width, refs)))])
    _matrix(E, H, igx, oracle, data, _singles_and_pairs(2, refs))


@pytest.mark.parametrize("width", [4, 8])
def test_fused_float_predicates(E, H, igx, oracle, width):
    """float32 / float64 comparisons fused into the aggregation kernels (no float is fused
    anywhere else in the suite): the float pool, NaN in the values and as a reference."""
    data = Data(H, [_value_col(), R.Column("float", width, _tile(R.float_values(width)))])
    _matrix(E, H, igx, oracle, data, _singles_and_pairs(2, list(R.FLOAT_REFS)))


# ---- IN sets ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,width", [(k, w) for k in ("int", "uint") for w in (1, 2, 4, 8)])
def test_in_sets(E, H, igx, oracle, kind, width):
    """IGX_CMP_IN of 1 .. 8 / width members, plain and negated, with sets that hold 0 and the
    type's maximum; one and two sets per update (pred_scalar unpacks them from a u64)."""
    lo, hi = R.int_range(kind, width)
    pool = R.int_pool(kind, width)
    data = Data(H, [_value_col(), R.Column(kind, width, _tile(R.int_values(kind, width, pool) + [2, 3, 5]))])
    members = [0, hi, 1, lo, hi - 1, 2, -1 if kind == "int" else 3, 5]
    sets = []
    for cnt in range(1, 8 // width + 1):
        for start in (0, 1, 2):
            ms = [members[(start + i) % len(members)] for i in range(cnt)]
            sets += [[R.Pred(2, R.IN, ms, neg)] for neg in (False, True)]
    sets += [[a[0], b[0]] for a, b in zip(sets[::3], sets[1::3])]
    _matrix(E, H, igx, oracle, data, sets)


# ---- a predicate on the SUM's own value column ----------------------------------------------------
@pytest.mark.parametrize("kind,width,div", [("int", 4, 0), ("uint", 4, 1000), ("int", 8, 0)])
def test_predicate_shares_the_sum_column(E, H, igx, oracle, kind, width, div):
    """The predicate column is the SUM's value column, so the fused kernels reuse the aggregate's
    loaded value (pshare): an int32 column (sign-extended sum, signed compare), a uint32 column
    with divisor 1000 (the predicate sees the undivided value), an int64 column."""
    refs = R.int_pool(kind, width) + [1000, 999]
    data = Data(H, [R.Column(kind, width, _tile(R.int_values(kind, width, refs)))])
    sets = [[R.Pred(1, op, ref, neg)] for ref in refs for op in R.OPS for neg in (False, True)]
    _matrix(E, H, igx, oracle, data, sets, div=div)


# ---- guards -------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["cond-column", "other-column"])
@pytest.mark.parametrize("gw", [1, 2, 4, 8])
def test_guards(E, H, igx, oracle, gw, route):
    """Guarded comparisons with guards of 1, 2, 4 and 8 bytes.  'cond-column': the guard column
    is the COUNT's cond_col, so the guard fuses (pguard: the aggregate's condition value).
    'other-column': no aggregate reads it, so the predicate is spilled to the mask (k_pred_mask,
    pred_match's gwidth branch).  Guard values match some rows, no rows, and -- on a constant
    column -- all rows; guarded rows are tested, the others pass."""
    top = 1 << (8 * gw - 1)                       # values with the top bit set: no sign extension
    for gvals in ([top + 1, top + 2, top + 3, top + 1, 1], [top + 1]):
        data = Data(H, [_value_col(), R.Column("uint", gw, _tile(gvals)),
                        R.Column("int", 4, _tile([5, -5, 0, 7, -1, 2**31 - 1, -2**31])),
                        R.Column("uint", 2, _tile([0, 1, 65535, 300, 2]))])
        sets = []
        for g in (top + 1, top + 9, 1):
            sets += [[R.Pred(3, R.GT, 0, guard=(2, g))], [R.Pred(3, R.LE, 0, True, guard=(2, g))],
                     [R.Pred(4, R.IN, [1, 65535], guard=(2, g))] if route == "cond-column" else
                     [R.Pred(4, R.GE, 300, guard=(2, g))],
                     [R.Pred(3, R.LT, 6, guard=(2, g)), R.Pred(4, R.EQ, 0, True)]]
        cond = (2, top + 1) if route == "cond-column" else None
        _matrix(E, H, igx, oracle, data, sets, cond=cond)


# ---- spill to the mask ----------------------------------------------------------------------------
def test_spill_to_the_mask(E, H, igx, oracle):
    """More predicates than the kernels fuse, with a nil mask: three and five scalar
    comparisons (the extra ones are spilled to the mask: k_pred_mask -> pred_match / pred_cmp);
    two IN sets plus two scalars (the scalars spill, the sets stay fused); a string rule next to
    fused ones."""
    rng = np.random.default_rng(5)
    names = [b"bash", b"sshd", b"kworker/0:1", b"", b"\x80x", b"zsh-5.9-abcdefgh"]
    cols = [_value_col(),
            R.Column("int", 4, rng.integers(-50, 50, NMAX).tolist()),
            R.Column("uint", 2, rng.integers(0, 100, NMAX).tolist()),
            R.Column("int", 1, rng.integers(-128, 128, NMAX).tolist()),
            R.Column("float", 4, [float(x) / 4 for x in rng.integers(-40, 40, NMAX)]),
            R.Column("bytes", 16, [names[i].ljust(16, b"\0") for i in rng.integers(0, len(names), NMAX)]),
            R.Column("uint", 1, rng.integers(0, 6, NMAX).tolist())]
    valid = (rng.random(NMAX) > 0.1).astype(np.uint8)
    data = Data(H, cols, valid=valid)
    a, b, c, f, s, m = 2, 3, 4, 5, 6, 7
    sets = [
        [R.Pred(a, R.GE, -40), R.Pred(b, R.LT, 90), R.Pred(c, R.GT, -100)],
        [R.Pred(a, R.GE, -40), R.Pred(b, R.LT, 90), R.Pred(c, R.GT, -100), R.Pred(f, R.LE, 8.0),
         R.Pred(a, R.EQ, 0, True)],
        [R.Pred(b, R.IN, [1, 2, 3, 50], True), R.Pred(m, R.IN, [0, 1, 2, 3]), R.Pred(a, R.LT, 40), R.Pred(c, R.GE, -120)],
        [R.Pred(s, R.GE, b"kworker"), R.Pred(a, R.GT, -45), R.Pred(b, R.LE, 95)],
        [R.Pred(s, R.EQ, b"", True), R.Pred(m, R.IN, [5], True)],
        [R.Pred(f, R.GT, -9.75), R.Pred(s, R.LT, b"\x80"), R.Pred(c, R.LT, 120), R.Pred(b, R.GT, 1, False)],
    ]
    _matrix(E, H, igx, oracle, data, sets)


# ---- pinned argument errors -----------------------------------------------------------------------
def _update_error(E, H, igx, cols, preds, n, valid=None, aggs=None):
    """The IgxError of one update on a fresh table (None when the update is accepted)."""
    A = igx._abi
    tab = E.Table([1], aggs or [A.Agg(A.AGG_COUNT, 0, A.NO_COL, 8, 0), A.Agg(A.AGG_SUM, 1, A.NO_COL, 8, 0)], 64)
    try:
        tab.update(cols, [0], n, 0, preds=preds, valid=valid)
        tab.finalize()
        return None
    except A.IgxError as e:
        return e
    finally:
        tab.destroy()


def _raw_pred(A, col, cmp, ref, negate=False):
    return A.Pred(col, cmp, int(negate), len(ref), (C.c_uint8 * A.MAX_REF)(*ref))


def test_in_set_argument_errors(E, H, igx):
    """Three IN sets in one update: IGX_ENOTSUP.  IN on a float column, or with ref_len not a
    multiple of the column width: IGX_EINVAL.  A guarded IN whose guard column is not an
    aggregate's condition column is not supported (igx.h): IGX_ENOTSUP, with a message that names
    groupby_update and the limitation -- not the filter scan's 'is not a FilterSpec'."""
    A = igx._abi
    n = 64
    key = H.to_device((np.arange(n) % 8).astype(np.uint8))
    val = H.to_device(np.arange(n, dtype=np.uint32))
    u16 = H.to_device(np.arange(n, dtype=np.uint16))
    f32 = H.to_device(np.arange(n, dtype=np.float32))
    g8 = H.to_device((np.arange(n) % 2).astype(np.uint8))
    cols = [key, val, u16, f32, g8]
    one = _raw_pred(A, 2, A.CMP_IN, b"\1\0\2\0")
    assert _update_error(E, H, igx, cols, [one, one], n) is None
    e = _update_error(E, H, igx, cols, [one, one, one], n)
    assert e is not None and e.code == A.IGX_ENOTSUP and "groupby_update" in str(e)
    e = _update_error(E, H, igx, cols, [_raw_pred(A, 3, A.CMP_IN, b"\0\0\x80\x3f")], n)
    assert e is not None and e.code == A.IGX_EINVAL and "IN predicate" in str(e)
    for ref in (b"\1", b"\1\0\2", b"", b"\1\0\2\0\3\0\4\0\5\0"):
        e = _update_error(E, H, igx, cols, [_raw_pred(A, 2, A.CMP_IN, ref)], n)
        assert e is not None and e.code == A.IGX_EINVAL and "IN predicate" in str(e), ref
    guarded = _raw_pred(A, 2, A.CMP_IN, b"\1\0\2\0")
    guarded.guard_col, guarded.guard_len, guarded.guard_ref = 4, 1, (C.c_uint8 * 8)(1)
    e = _update_error(E, H, igx, cols, [guarded], n)
    assert e is not None and e.code == A.IGX_ENOTSUP
    assert "groupby_update" in str(e) and "condition column" in str(e) and "FilterSpec" not in str(e)
    # the same guard fuses when an aggregate's cond_col is the guard column
    aggs = [A.Agg(A.AGG_COUNT, 0, 4, 8, 1), A.Agg(A.AGG_SUM, 1, A.NO_COL, 8, 0)]
    assert _update_error(E, H, igx, cols, [guarded], n, aggs=aggs) is None


def test_misaligned_columns_are_rejected(E, H, igx):
    """igx.h's alignment contract: the fused kernels read every non-key scalar column and the nil
    mask as the 4-byte words that hold each row, counted from the column's base, so a 1- or
    2-byte column that starts at an odd row of a larger tensor -- a base off a 4-byte boundary
    -- returns IGX_EINVAL as a misaligned key column does; a slice at a multiple of four bytes is
    accepted.  (Every slice here ends before its tensor's last row.)"""
    A = igx._abi
    n = 64
    big = n + 8
    key = H.to_device((np.arange(big) % 8).astype(np.uint8))
    val = H.to_device(np.arange(big, dtype=np.uint32))
    u8 = H.to_device((np.arange(big) % 3).astype(np.uint8))
    u16 = H.to_device(np.arange(big, dtype=np.uint16))
    valid = H.to_device(np.ones(big, np.uint8))
    p8, p16 = _raw_pred(A, 2, A.CMP_GE, b"\1"), _raw_pred(A, 3, A.CMP_GE, b"\1\0")
    cond8 = [A.Agg(A.AGG_COUNT, 0, 2, 8, 1), A.Agg(A.AGG_SUM, 1, A.NO_COL, 8, 0)]
    sum8 = [A.Agg(A.AGG_COUNT, 0, A.NO_COL, 8, 0), A.Agg(A.AGG_SUM, 2, A.NO_COL, 8, 0)]
    guard = _raw_pred(A, 3, A.CMP_GE, b"\1\0")
    guard.guard_col, guard.guard_len, guard.guard_ref = 2, 1, (C.c_uint8 * 8)(1)

    def err(o8, o16, preds, ov=None, aggs=None):
        cols = [key[:n], val[:n], u8[o8:o8 + n], u16[o16:o16 + n]]
        return _update_error(E, H, igx, cols, preds, n, valid=None if ov is None else valid[ov:ov + n], aggs=aggs)

    for o8, o16, preds, ov, aggs in ((1, 0, [p8], None, None), (3, 0, [p8], None, None), (0, 1, [p16], None, None),
                                     (0, 0, [p8], 1, None), (0, 0, [], 2, None), (1, 0, [], None, cond8),
                                     (2, 0, [], None, sum8), (1, 0, [guard], None, None), (1, 0, [guard], None, cond8)):
        e = err(o8, o16, preds, ov, aggs)
        assert e is not None and e.code == A.IGX_EINVAL and "misaligned" in str(e), (o8, o16, ov)
    for o8, o16, preds, ov, aggs in ((4, 2, [p8, p16], 4, None), (0, 0, [p8, p16], 0, cond8), (4, 4, [guard], None, cond8),
                                     (4, 0, [], None, sum8), (1, 1, [], None, None)):   # unread columns take any base
        assert err(o8, o16, preds, ov, aggs) is None, (o8, o16, ov)
