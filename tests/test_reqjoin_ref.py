"""CPU checks of the request-pairing restatement (tests/reqjoin_ref.py) that the device join is
compared with: the contract's hand cases, and that cutting a stream into batches with the live
rows carried in band changes nothing.  No GPU."""
import numpy as np
import pytest

import reqjoin_ref as R


@pytest.mark.parametrize("case", R.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    _, req, kind, ts, emitted, live = case
    em, lv = R.join(req, kind, ts)
    assert [e[:3] for e in em] == emitted
    assert lv == live
    for d, i, _, delta in em:
        assert delta == (int(ts[d]) - int(ts[i])) % (1 << 64)


def test_hand_case_wrapping_delta():
    _, req, kind, ts, _, _ = R.hand_cases()[9]
    em, _ = R.join(req, kind, ts)
    assert len(em) == 1 and em[0][3] >= 1 << 63          # 4000 - 5000 mod 2^64; the second D emits nothing


def test_valid_mask_and_other_kinds_do_not_exist():
    a = 0xFFFF888800001000
    req = np.array([a] * 6, np.uint64)
    ts = np.arange(6, dtype=np.uint64) * np.uint64(10)
    kind = np.array([R.START, R.ISSUE, 3, R.ISSUE, 255, R.DONE], np.uint8)
    valid = np.array([1, 1, 1, 0, 1, 1], np.uint8)
    em, live = R.join(req, kind, ts, valid)
    assert em == [(5, 1, 0, 40)] and live == []


@pytest.mark.parametrize("cuts", [(1700, 3400), (1, 4999), (2500,), (10, 20, 30, 4000)])
def test_split_invariance(cuts):
    req, kind, ts = R.random_stream(5000, 97, seed=11)
    whole, live = R.join(req, kind, ts)
    em, lv = R.join_batches(req, kind, ts, cuts)
    assert len(whole) > 500 and live
    assert em == whole
    assert lv == live


def test_split_invariance_with_mask():
    req, kind, ts = R.random_stream(5000, 40, seed=12, wrap_ts=True)
    valid = (np.random.default_rng(5).random(5000) < 0.7).astype(np.uint8)
    whole, live = R.join(req, kind, ts, valid)
    em, lv = R.join_batches(req, kind, ts, (1234, 3210), valid)
    assert em == whole and lv == live
    assert any(e[3] >= 1 << 63 for e in whole)


def test_library_exports_the_join(igx):
    """The scan tile the GPU tests size their edge cases by comes from the library itself."""
    L = igx.lib()
    tile = L.igx_req_join_tile()
    assert tile >= 64 and tile % 64 == 0
    assert igx.engine.req_join_tile() == tile
    assert L.igx_req_join(None, None, None, None, None, 0, None, None, None, None, None, None, 0, None) == \
        igx._abi.IGX_EINVAL
