"""tests/rolling_reference.py (the restatement the GPU tests compare olap_store_rolling_multi with) is pinned to the
oracle here: for every position k of a small cube, OracleStore.dice(members of k's window).drill_up(-> one item) equals
row k of the restatement — all four cell types x both defaults x the seven rules, the groupings of
test_cumulate_reference.py, windows that trail, are centred, lead, exclude their own item and cover everything; a
window without members is unset and the oracle is not asked."""
import numpy as np
import pytest

from cumulate_reference import METHODS, NP
from golden_util import expected_typed, same_typed
from rolling_reference import rolling_reference, window_members
from test_cumulate_reference import AXIS, GROUPINGS, LENS, TYPES, cells, oracle_of

WINDOWS = [(2, 0), (1, 1), (0, 2), (1, -1), (-2, 2), (7, 7)]


@pytest.mark.parametrize("grouping", sorted(GROUPINGS))
@pytest.mark.parametrize("default_is_nan", [False, True])
@pytest.mark.parametrize("type_name", TYPES)
def test_every_position_is_the_dice_drillup_chain_of_the_oracle(type_name, default_is_nan, grouping):
    groups = GROUPINGS[grouping]
    g = np.zeros(LENS[AXIS], dtype=np.int64) if groups is None else np.asarray(groups)
    typed, status = cells(type_name, default_is_nan, seed=len(grouping) * 8 + TYPES.index(type_name) * 2 + default_is_nan)
    o = oracle_of(typed, status, type_name, default_is_nan)
    outer, K, inner = LENS
    for before, after in WINDOWS:
        for method in METHODS:
            ref_v, ref_s = rolling_reference(typed, status, LENS, AXIS, method, type_name, default_is_nan, before, after, groups)
            ref_v, ref_s = ref_v.reshape(outer, K, inner), ref_s.reshape(outer, K, inner)
            for k in range(K):
                where = (type_name, default_is_nan, grouping, (before, after), method, k)
                members = window_members(k, K, before, after, g)
                if not members:
                    assert not ref_s[:, k, :].any(), where
                    continue
                mid = [outer, len(members), inner]
                diced = o.dice(LENS, mid, [list(range(outer)), members, list(range(inner))])
                rolled = diced.drill_up(mid, [outer, 1, inner], [list(range(outer)), [0] * len(members), list(range(inner))], method)
                want_v, want_s = expected_typed(rolled)
                assert np.array_equal(ref_s[:, k, :].ravel(), want_s), where
                assert same_typed(ref_v[:, k, :].ravel().astype(NP[type_name]), want_v.astype(NP[type_name])), where


def test_hand_worked_series():
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    # [5, -5, 3, 1] under a 0 default, the item and the one before it: 5 | 5 - 5 = 0, unset | -5 + 3 | 3 + 1
    v, s = rolling_reference(f32([5, -5, 3, 1]), None, [4], 0, "sum", "float32", False, 1)
    assert v.tolist() == [5.0, 0.0, -2.0, 4.0] and s.tolist() == [2, 0, 2, 2]
    # two before: at item 2 the fold restarts inside the window (5 - 5 drops, then 3); at item 3 it is -5 + 3 + 1
    v, s = rolling_reference(f32([5, -5, 3, 1]), None, [4], 0, "sum", "float32", False, 2)
    assert v.tolist() == [5.0, 0.0, 3.0, -1.0] and s.tolist() == [2, 0, 2, 2]
    # rounded once per cell, never in between: 2^24 + 1 - 2^24 = 1
    v, s = rolling_reference(f32([2 ** 24, 1, -(2 ** 24)]), None, [3], 0, "sum", "float32", False, 2)
    assert v.tolist() == [16777216.0, 16777216.0, 1.0] and s.tolist() == [2, 2, 2]
    # average: contributions only
    v, s = rolling_reference(f32([2, 0, 4]), None, [3], 0, "average", "float32", False, 1)
    assert v.tolist() == [2.0, 2.0, 4.0] and s.tolist() == [2, 2, 2]
    # shift by 1 = rolling(1, -1): the item before, when it lies in the same group
    for method in METHODS:
        v, s = rolling_reference(f32([1, 2, 3]), None, [3], 0, method, "float32", False, 1, -1, groups=[0, 0, 1])
        assert v.tolist() == [0.0, 1.0, 0.0] and s.tolist() == [0, 2, 0], method
    # a lead that runs off the end
    v, s = rolling_reference(f32([1, 2, 3]), None, [3], 0, "sum", "float32", False, -2, 2)
    assert v.tolist() == [3.0, 0.0, 0.0] and s.tolist() == [2, 0, 0]


def test_the_window_is_folded_afresh_not_updated():
    """5 + 1e-16-sized terms: a subtract-the-leaving-row update would keep rounding residue; every window is its own fold"""
    x = np.asarray([1e16, 1.0, -1e16, 1.0, 1.0], dtype=np.float64)
    v, s = rolling_reference(x, None, [5], 0, "sum", "float64", False, 1)
    assert v.tolist() == [1e16, 1e16 + 1.0, 1.0 - 1e16, 1.0 - 1e16, 2.0]
