"""CPU checks of the last-writer join's restatement (tests/lwjoin_ref.py) that the device join is
compared with: the contract's hand cases, the rows that do not exist, and that cutting a stream
into batches with the live rows carried in band changes nothing.  No GPU."""
import numpy as np
import pytest

import lwjoin_ref as R


@pytest.mark.parametrize("case", R.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    _, key, kind, emitted, live = case
    em, lv = R.join(key, kind)
    assert em == emitted
    assert lv == live


def test_b_survives_any_number_of_reads():
    n = 50
    kind = np.array([R.SET_B] + [R.SET_A, R.TAKE_A] * n, np.uint8)
    em, live = R.join(np.full(len(kind), 7, np.uint64), kind)
    assert len(em) == n and all(b == 0 for _, _, b in em) and live == [0]


def test_valid_mask_and_other_kinds_do_not_exist():
    key = np.full(7, 0x1234, np.uint64)
    kind = np.array([R.SET_B, R.SET_A, 4, R.CLEAR_B, 255, R.SET_A, R.TAKE_A], np.uint8)
    valid = np.array([1, 1, 1, 0, 1, 0, 1], np.uint8)
    em, live = R.join(key, kind, valid)
    assert em == [(6, 1, 0)] and live == [0]


@pytest.mark.parametrize("cuts", [(1700, 3400), (1, 4999), (2500,), (10, 20, 30, 4000)])
def test_split_invariance(cuts):
    key, kind = R.random_stream(5000, 97, seed=11)
    whole, live = R.join(key, kind)
    em, lv = R.join_batches(key, kind, cuts)
    assert len(whole) > 200 and len(live) > 50
    assert em == whole and lv == live
