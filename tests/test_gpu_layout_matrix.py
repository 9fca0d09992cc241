"""Every key layout of the group-by's layout table (k_gb_table.h, gb_with_layout) in every form.

The record width chosen at create, each form's launch, and the lookup kernel's key words all come
from that one table, so a layout missing from it, or mapped to the wrong width, shows as an error
or a wrong table in some form of some layout.  Layouts: the four named ones (top tcp, top file,
the network-policy tuple, top block-io), single columns of 1, 2, 4, 8 and 16 bytes, and one key
description per generic width (2, 4, 6, 8, 12, 18, 24 and 32 words, made of 4- and 8-byte columns
that match no static layout).  Forms: cached, direct and partitioned through set_mode, then direct
and partitioned again on a table created under IGX_GB_WIDE=1 (64-bit record addressing).

Each case: 4 096 rows over 300 key ids into a table of capacity 1 024, a COUNT and a u64 SUM (its
values span the whole u64 range, so the sums wrap), one update, finalize.  Group count and every
group's key, sums and first index must equal oracle.groupby (or_groupby) bit for bit; a lookup of
the 300 keys plus 50 never inserted must report `found` for exactly the oracle's keys and return
the gathered row of each (a zero row for the others).  The first key column is an injective image
of the key id, so the 300 ids are 300 distinct keys -- except in the 1-byte column, which can only
hold 256 values: there the oracle sees 256 groups and every queried key is present, and the
expectation is derived from the oracle's groups in the same way.
"""
import numpy as np
import pytest

import test_gpu_select_lookup as SL

pytestmark = pytest.mark.gpu

N, KEYS, ABSENT, CAP = 4096, 300, 50, 1024
LAYOUTS = {
    "tcp": [16, 16, 8, 4, 16, 2, 2, 2], "file": [8, 4, 4, 4], "netpolicy": [4, 1, 4, 2], "bio": [8, 4, 4, 4, 4, 16],
    "u8": [1], "u16": [2], "u32": [4], "u64": [8], "u128": [16],
    "generic2": [4, 4], "generic4": [8, 8], "generic6": [8, 8, 8], "generic8": [8] * 4, "generic12": [8] * 6,
    "generic18": [8] * 9, "generic24": [8] * 12, "generic32": [8] * 16,
}
FORMS = {"cached": ("GB_CACHED", False), "direct": ("GB_DIRECT", False), "part": ("GB_PART", False),
         "direct-wide": ("GB_DIRECT", True), "part-wide": ("GB_PART", True)}
_cache = {}


def _mix(x, c):
    """a u64 hash of the key ids x for column c"""
    with np.errstate(over="ignore"):
        h = (x + np.uint64(c + 1)) * np.uint64(0x9E3779B97F4A7C15)
        h ^= h >> np.uint64(29)
        return h * np.uint64(0xBF58476D1CE4E5B9)


def _key_cols(widths, kid):
    """key columns of the ids: column 0 is (id + 1) x an odd constant, injective in any width that
    holds the ids; the others are hashes of the id"""
    cols = {}
    for c, w in enumerate(widths):
        with np.errstate(over="ignore"):
            lo = (kid + np.uint64(1)) * np.uint64(0x9E3779B1) if c == 0 else _mix(kid, c)
        if w == 16:
            cols[f"k{c}"] = np.ascontiguousarray(np.stack([lo, _mix(kid, 100 + c)], axis=1)).view(np.uint8)
        else:
            cols[f"k{c}"] = lo.astype({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[w])
    return cols


def _case(name, igx, oracle):
    """(device columns, reference rows key | count | sum | first, query keys, expected lookup rows, found)"""
    if name in _cache:
        return _cache[name]
    H = igx.columns
    widths = LAYOUTS[name]
    rng = np.random.default_rng(1000 + list(LAYOUTS).index(name))
    kid = rng.integers(0, KEYS, N).astype(np.uint64)
    kid[:KEYS] = np.arange(KEYS, dtype=np.uint64)         # every id occurs
    h = _key_cols(widths, kid)
    h["val"] = rng.integers(0, 1 << 64, N, dtype=np.uint64)
    knames = [f"k{c}" for c in range(len(widths))]
    ref = SL._ref_rows(oracle, h, knames, [{"kind": "count"}, {"kind": "sum", "val": h["val"]}])
    kb = sum((w + 3) // 4 * 4 for w in widths)
    q = oracle.pad_keys(_key_cols(widths, np.arange(KEYS + ABSENT, dtype=np.uint64)), knames)
    by_key = {r[:kb].tobytes(): r for r in ref}
    want = np.stack([by_key.get(k.tobytes(), np.zeros(ref.shape[1], np.uint8)) for k in q])
    found = np.array([k.tobytes() in by_key for k in q], dtype=np.uint8)
    if name != "u8":                                      # the generator's own promise
        assert ref.shape[0] == KEYS and found.sum() == KEYS and not found[KEYS:].any()
    else:
        assert ref.shape[0] == 256 and found.all()
    cols = [H.to_device(h[k]) for k in knames + ["val"]]
    _cache[name] = (cols, ref, H.to_device(q), want, found)
    return _cache[name]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layout_in_form_equals_oracle(igx, torch, oracle, monkeypatch, name, form):
    A, H = igx._abi, igx.columns
    mode, wide = getattr(A, FORMS[form][0]), FORMS[form][1]
    widths = LAYOUTS[name]
    cols, ref, q, want, found = _case(name, igx, oracle)
    if wide:
        monkeypatch.setenv("IGX_GB_WIDE", "1")
    nk = len(widths)
    tab = igx.engine.Table(widths, [A.Agg(A.AGG_COUNT, 0, A.NO_COL, 8, 0), A.Agg(A.AGG_SUM, nk, A.NO_COL, 8, 0)], CAP)
    if wide:                                              # a wide table refuses the cached form
        with pytest.raises(A.IgxError) as e:
            tab.set_mode(A.GB_CACHED)
        assert e.value.code == A.IGX_ENOTSUP
    tab.set_mode(mode)
    tab.update(cols, list(range(nk)), N, 0)
    tab.finalize()
    assert tab.info()["form"] == mode
    assert tab.fin["n_groups"] == ref.shape[0]
    got = H.host(tab.gather(SL._slots(tab, torch)))
    assert np.array_equal(SL._sorted(got), SL._sorted(ref))
    rows, fnd = tab.lookup(q)
    assert np.array_equal(H.host(fnd), found)
    assert np.array_equal(H.host(rows), want)
    tab.destroy()
