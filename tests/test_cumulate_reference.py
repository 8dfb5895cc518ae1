"""tests/cumulate_reference.py (the restatement the GPU tests compare olap_store_cumulate_multi with) is pinned to the
oracle here: for every position k of small cubes, OracleStore.dice(members of k's group at positions <= k).drill_up(->
one item) equals row k of the restatement — all four cell types x both defaults x the seven rules, contiguous,
interleaved and single-member groups, sparse masks."""
import numpy as np
import pytest

from cumulate_reference import METHODS, NP, cumulate_reference, input_set
from golden_util import expected_typed, same_typed
from oracle.oracle import OracleStore, to_typed

TYPES = ("int32", "uint32", "float32", "float64")
GROUPINGS = {
    "all": None,
    "contiguous 1,4,2": [0, 1, 1, 1, 1, 2, 2],
    "interleaved": [0, 1, 0, 2, 1, 0, 1],
    "single members": [0, 1, 2, 3, 4, 5, 6],
}
LENS, AXIS = [2, 7, 3], 1


def cells(type_name, default_is_nan, seed):
    """typed cells where sums return to 0, products hit 0 and NaN / inf / -0 occur; ~1/3 unset through the mask or the default"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(LENS))
    v = rng.integers(-3, 4, size=n).astype(np.float64)
    if type_name.startswith("float"):
        special = rng.random(n)
        v[special < 0.08] = np.nan
        v[(special >= 0.08) & (special < 0.14)] = np.inf
        v[(special >= 0.14) & (special < 0.20)] = -np.inf
        v[(special >= 0.20) & (special < 0.24)] = -0.0
        v[(special >= 0.24) & (special < 0.30)] = 0.5
    typed = to_typed(v, type_name).astype(NP[type_name])
    status = None
    if not type_name.startswith("float") and default_is_nan:  # the mask is what says "unset"
        status = np.where(rng.random(n) < 0.65, 2, 0).astype(np.int32)
    return typed, status


def oracle_of(typed, status, type_name, default_is_nan):
    o = OracleStore(typed.size, type_name, float("nan") if default_is_nan else 0.0)
    for i in np.nonzero(input_set(typed, status, type_name, default_is_nan))[0]:
        o.set(int(i), float(typed[i]))
    return o


@pytest.mark.parametrize("grouping", sorted(GROUPINGS))
@pytest.mark.parametrize("default_is_nan", [False, True])
@pytest.mark.parametrize("type_name", TYPES)
def test_every_position_is_the_dice_drillup_chain_of_the_oracle(type_name, default_is_nan, grouping):
    groups = GROUPINGS[grouping]
    g = np.zeros(LENS[AXIS], dtype=np.int64) if groups is None else np.asarray(groups)
    typed, status = cells(type_name, default_is_nan, seed=len(grouping) * 8 + TYPES.index(type_name) * 2 + default_is_nan)
    o = oracle_of(typed, status, type_name, default_is_nan)
    outer, K, inner = LENS
    for method in METHODS:
        ref_v, ref_s = cumulate_reference(typed, status, LENS, AXIS, method, type_name, default_is_nan, groups)
        ref_v, ref_s = ref_v.reshape(outer, K, inner), ref_s.reshape(outer, K, inner)
        for k in range(K):
            members = [j for j in range(k + 1) if g[j] == g[k]]
            mid = [outer, len(members), inner]
            diced = o.dice(LENS, mid, [list(range(outer)), members, list(range(inner))])
            rolled = diced.drill_up(mid, [outer, 1, inner], [list(range(outer)), [0] * len(members), list(range(inner))], method)
            want_v, want_s = expected_typed(rolled)
            where = (type_name, default_is_nan, grouping, method, k)
            assert np.array_equal(ref_s[:, k, :].ravel(), want_s), where
            assert same_typed(ref_v[:, k, :].ravel().astype(NP[type_name]), want_v.astype(NP[type_name])), where


def test_hand_worked_series():
    """the cases the issue spells out, by hand"""
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    # [5, -5, 3] under a 0 default: unset in the middle, then the aggregate restarts
    v, s = cumulate_reference(f32([5, -5, 3]), None, [3], 0, "sum", "float32", False)
    assert v.tolist() == [5.0, 0.0, 3.0] and s.tolist() == [2, 0, 2]
    # rounded once per cell, never in between: 2^24 + 1 - 2^24 = 1
    v, s = cumulate_reference(f32([2 ** 24, 1, -(2 ** 24)]), None, [3], 0, "sum", "float32", False)
    assert v.tolist() == [16777216.0, 16777216.0, 1.0] and s.tolist() == [2, 2, 2]
    # inf + -inf under a NaN default: unset, restart
    v, s = cumulate_reference(f32([np.inf, -np.inf, 2]), None, [3], 0, "sum", "float32", True)
    assert np.isnan(v[1]) and v[0] == np.inf and v[2] == 2.0 and s.tolist() == [2, 0, 2]
    # an unset cell receives the carried value; leading unset cells stay unset; `last` is forward-fill
    v, s = cumulate_reference(f32([0, 0, 4, 0, 7, 0]), None, [6], 0, "last", "float32", False)
    assert v.tolist() == [0.0, 0.0, 4.0, 4.0, 7.0, 7.0] and s.tolist() == [0, 0, 2, 2, 2, 2]
    # Int32 sums wrap (ToInt32), negative values wrap into Uint32
    v, s = cumulate_reference(np.asarray([2 ** 31 - 1, 1, 1], dtype=np.int32), None, [3], 0, "sum", "int32", False)
    assert v.tolist() == [2 ** 31 - 1, -(2 ** 31), -(2 ** 31) + 1]
    v, s = cumulate_reference(np.asarray([1, 2 ** 32 - 3], dtype=np.uint32), None, [2], 0, "lowest", "uint32", False)
    assert v.tolist() == [1, 1]
    # average: contributions only, per group
    v, s = cumulate_reference(f32([2, 0, 4, 10, 20]), None, [5], 0, "average", "float32", False, groups=[0, 0, 0, 1, 1])
    assert v.tolist() == [2.0, 2.0, 3.0, 10.0, 15.0]


def test_average_counter_wraps_at_65536():
    ones = np.ones(65537, dtype=np.float32)
    v, s = cumulate_reference(ones, None, [65537], 0, "average", "float32", False)
    assert v[65534] == 1.0 and v[65535] == 65536.0 and v[65536] == 65537.0  # counter 0: the sum is left; then sum / 1
