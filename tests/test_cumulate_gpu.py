"""olap_store_cumulate_multi (running aggregates along a dimension, olap_cumulate.hip) against tests/cumulate_reference.py,
which tests/test_cumulate_reference.py pins to the oracle: typed cells as raw bytes and the mask.  Every case also checks
that the inputs are unchanged and that a second run gives identical bytes.

Shapes are the smallest at which each form can go wrong: the column form (a lane owns a 16-byte slot of `inner`) with
whole and ragged rows, more slots than one workgroup and groups of 300 members; the row form (series staged in LDS) with
more series than one tile holds (several tiles, a partial last one), an odd pitch, `inner` below one slot and between one
and four, series one cell under and over the tile capacity (the chunk carry, over several tiles too), an interleaved map
over a series beyond one tile (one-cell column slots), and both forms with fewer workgroups than tiles."""
import os

import numpy as np
import pytest

from conftest import load_package
from cumulate_reference import METHODS, NP, cumulate_reference

pytestmark = pytest.mark.gpu

pkg = load_package()
TILE = 4096  # kCumulateTileCells (csrc/olap_internal.hpp)
TYPES = ("int32", "uint32", "float32", "float64")


def raw(a):
    return np.ascontiguousarray(a).tobytes()


def make_store(typed, status, type_name, default_is_nan):
    default = float("nan") if default_is_nan else 0.0
    if status is None:
        s = pkg.HipStore(typed.size, type_name, default)
        s.set_data(typed)
        return s
    idx = np.nonzero(status & 2)[0]
    return pkg.HipStore.from_sparse(typed.size, type_name, default, idx, typed[idx])


def random_cells(lens, type_name, default_is_nan, seed, unset=0.0, lead=0):
    """small integers (sums return to 0, products hit 0); `unset`: fraction of unset cells; `lead`: leading cells unset"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(lens))
    v = rng.integers(-3, 4, size=n).astype(np.float64)
    if type_name.startswith("float"):
        v = np.where(rng.random(n) < 0.1, 0.25, v)
    if type_name == "uint32":
        v = np.mod(v, 4294967296.0)
    typed = v.astype(NP[type_name])
    gone = rng.random(n) < unset
    gone[:lead] = True
    status = None
    if not type_name.startswith("float") and default_is_nan:
        status = np.where(gone, 0, 2).astype(np.int32)
    else:
        typed[gone] = np.nan if default_is_nan else 0
    return typed, status


def check(lens, axis, type_name, default_is_nan, method, typed, status=None, groups=None, n_groups=None):
    typed = np.asarray(typed, dtype=NP[type_name])
    s = make_store(typed, status, type_name, default_is_nan)
    before = (raw(s.get_data()), raw(s.get_status()))
    out = s.cumulate(lens, axis, method, groups, n_groups)
    want_v, want_s = cumulate_reference(typed, status, lens, axis, method, type_name, default_is_nan, groups)
    got_v, got_s = out.get_data(), out.get_status()
    where = (lens, axis, type_name, default_is_nan, method)
    assert np.array_equal(got_s, want_s), (where, np.nonzero(got_s != want_s)[0][:8])
    if raw(got_v) != raw(want_v):
        bad = np.nonzero(got_v.view(np.uint8).reshape(typed.size, -1) != want_v.view(np.uint8).reshape(typed.size, -1))[0][:8]
        raise AssertionError((where, bad, got_v[bad], want_v[bad]))
    assert (raw(s.get_data()), raw(s.get_status())) == before, where  # the input is only read
    again = s.cumulate(lens, axis, method, groups, n_groups)
    assert raw(again.get_data()) == raw(got_v) and raw(again.get_status()) == raw(got_s), where
    return out


# ---- forms ------------------------------------------------------------------------------------------------------------
# Rows of fewer than four 16-byte slots take the row form: [3, 5, 8], [2, 6, 9] and [2, 5, 13] are column shapes for 8-byte cells
# only, [2, 7, 5] and [1, 300, 4] row shapes for both.  Column shapes for 4-byte cells too: [2, 3, 1030] and [2, 5, 17] (ragged),
# [2, 300, 16] and [2, 300, 18] (16-byte slots over groups of 300 members, whole and ragged rows).
COLUMN_SHAPES = [([3, 5, 8], 1), ([2, 7, 5], 1), ([2, 3, 1030], 1), ([1, 300, 4], 1), ([2, 6, 9], 1), ([2, 5, 13], 1), ([2, 5, 17], 1),
                 ([2, 300, 16], 1), ([2, 300, 18], 1)]
# A tile holds min(4096 / (K * inner), 256) whole series: [600, 7] is tiles of 256, 256 and 88 series, [300, 33] of 124, 124 and 52;
# the others fit one tile.
ROW_SHAPES = [([5, 7], 1), ([70, 33], 1), ([4, 6, 3], 1), ([3, 6, 7], 1), ([600, 7], 1), ([300, 33], 1)]


@pytest.mark.parametrize("lens,axis", COLUMN_SHAPES + ROW_SHAPES)
def test_every_rule_type_and_default_on_every_form(lens, axis):
    """(one case per shape: the failure message names the cell type, default and rule)"""
    for type_name in TYPES:
        for default_is_nan in (False, True):
            typed, status = random_cells(lens, type_name, default_is_nan, seed=sum(lens) + len(type_name), unset=0.3)
            for method in METHODS:
                check(lens, axis, type_name, default_is_nan, method, typed, status)


@pytest.mark.parametrize("type_name", ["float32", "float64", "int32"])
def test_series_around_the_tile_capacity(type_name):
    """one cell under and over the tile: the owning lane carries its state from chunk to chunk, across group borders"""
    for K in (TILE - 1, TILE, TILE + 1, 2 * TILE + 5):
        series_of(3, K, type_name)
    series_of(19, TILE + 1, type_name)  # the chunked form deals 8 series to a tile: tiles of 8, 8 and 3 series


def series_of(outer, K, type_name):
    lens = [outer, K]
    typed, status = random_cells(lens, type_name, type_name == "int32", seed=K, unset=0.2)
    check(lens, 1, type_name, type_name == "int32", "sum", typed, status)
    borders = np.zeros(K, dtype=np.uint32)
    borders[1:] = 1  # groups of 1, K - 12, 0 (a group id nobody maps to) and 11 members
    borders[K - 11:] = 3
    check(lens, 1, type_name, type_name == "int32", "average", typed, status, borders, 4)
    check(lens, 1, type_name, type_name == "int32", "product", typed, status, borders, 4)


@pytest.mark.parametrize("type_name", ["float32", "float64"])
def test_interleaved_groups_over_a_series_beyond_one_tile(type_name):
    lens = [2, TILE + 3]
    typed, status = random_cells(lens, type_name, False, seed=5, unset=0.2)
    check(lens, 1, type_name, False, "sum", typed, status, np.arange(TILE + 3) % 3, 3)
    lens = [2, TILE + 3, 2]  # inner 2 is below a slot of four 4-byte cells, and a whole slot of 8-byte cells
    typed, status = random_cells(lens, type_name, False, seed=6, unset=0.2)
    check(lens, 1, type_name, False, "highest", typed, status, np.arange(TILE + 3) % 3, 3)


def test_workgroups_that_walk_several_tiles():
    """OLAP_CUMULATE_GRID (a developer knob) caps the workgroups of a launch: with 2 of them every workgroup takes several
    tiles (row forms: a fresh carry per tile) or several strides of lanes (column form), as launches beyond the grid limit do"""
    os.environ["OLAP_CUMULATE_GRID"] = "2"
    try:
        for lens in ([1300, 7], [700, 33], [2, 30, 1030]):  # six tiles, six tiles, 21 workgroups' worth of lanes
            for type_name, default_is_nan in (("float32", False), ("int32", True)):
                typed, status = random_cells(lens, type_name, default_is_nan, seed=sum(lens), unset=0.3)
                for method in ("sum", "average"):
                    check(lens, 1, type_name, default_is_nan, method, typed, status, np.arange(lens[1]) // 3, (lens[1] + 2) // 3)
        series_of(43, TILE + 1, "float32")  # chunked: six tiles for two workgroups
    finally:
        del os.environ["OLAP_CUMULATE_GRID"]


# ---- groups -----------------------------------------------------------------------------------------------------------
GROUPS = {
    "uneven contiguous 1,4,2": ([0, 1, 1, 1, 1, 2, 2], 3),
    "interleaved": ([0, 1, 0, 2, 1, 0], 3),
    "a group id nobody maps to": ([0, 0, 2, 2, 3, 3], 5),
    "NULL map": (None, None),
}


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_groups(name):
    groups, n_groups = GROUPS[name]
    K = len(groups) if groups else 6
    for type_name in TYPES:
        for lens, axis in (([3, K, 8], 1), ([3, K, 5], 1), ([9, K], 1), ([K, 6], 0), ([4, K, 3], 1), ([2, K, 17], 1)):
            typed, status = random_cells(lens, type_name, True, seed=K + len(lens), unset=0.25)
            for method in ("sum", "average", "lowest", "last"):
                check(lens, axis, type_name, True, method, typed, status, groups, n_groups)


# ---- values where a wrong implementation shows ----------------------------------------------------------------------
def series(type_name, default_is_nan, method, values, lens=None, axis=0, status=None):
    values = np.asarray(values, dtype=NP[type_name])
    out = check(lens or [values.size], axis, type_name, default_is_nan, method, values, status)
    return out.get_data(), out.get_status()


def test_float32_is_rounded_once_per_cell_never_in_between():
    v, s = series("float32", False, "sum", [2 ** 24, 1, -(2 ** 24)])
    assert v.tolist() == [16777216.0, 16777216.0, 1.0] and s.tolist() == [2, 2, 2]
    # the same series as a column (inner = 4) and inside a wider row tile
    series("float32", False, "sum", np.repeat([2 ** 24, 1, -(2 ** 24)], 4), lens=[3, 4])
    series("float32", False, "sum", np.tile([2 ** 24, 1, -(2 ** 24)], 5), lens=[5, 3], axis=1)


def test_integer_sums_wrap():
    v, s = series("int32", False, "sum", [2 ** 31 - 1, 1, 1])
    assert v.tolist() == [2 ** 31 - 1, -(2 ** 31), -(2 ** 31) + 1]
    v, s = series("uint32", False, "sum", [2 ** 32 - 1, 2, 2 ** 32 - 2])
    assert v.tolist() == [2 ** 32 - 1, 1, 2 ** 32 - 1]
    v, s = series("int32", True, "product", [65536, 65536, 3])  # 2^32 wraps to a SET 0 under the NaN default
    assert v.tolist() == [65536, 0, 0] and s.tolist() == [2, 2, 2]


def test_restarts():
    v, s = series("float32", False, "sum", [5, -5, 3])
    assert v.tolist() == [5.0, 0.0, 3.0] and s.tolist() == [2, 0, 2]
    v, s = series("float32", True, "sum", [np.inf, -np.inf, 2])
    assert s.tolist() == [2, 0, 2] and v[2] == 2.0
    v, s = series("float64", True, "sum", [np.inf, -np.inf, 2, 5])
    assert s.tolist() == [2, 0, 2, 2] and v[3] == 7.0
    v, s = series("float64", False, "product", [4, 1e-200, 1e-200, 3, 2])  # underflows to 0: unset, then 3, 6
    assert v.tolist()[2:] == [0.0, 3.0, 6.0] and s.tolist() == [2, 2, 0, 2, 2]
    v, s = series("int32", False, "average", [4, -4, 6, 0, 2])  # the count survives the restart
    assert s.tolist() == [2, 0, 2, 2, 2] and v.tolist() == [4, 0, 2, 2, 2]


def test_special_floats():
    for type_name in ("float32", "float64"):
        nan_set = [1, np.nan, 2, 0, 3]  # a set NaN under a 0 default poisons sums and extremes from there on
        for method in METHODS:
            series(type_name, False, method, nan_set)
        minus_zero = [-0.0, 0.0, -1, -0.0, 1, -0.0]  # -0 equals the 0 default: unset; under NaN it is a value
        for method in METHODS:
            series(type_name, False, method, minus_zero)
            series(type_name, True, method, minus_zero)
        v, s = series(type_name, True, "highest", [-0.0, 0.0, -0.0])
        assert np.signbit(v).tolist() == [True, False, False]
        v, s = series(type_name, True, "lowest", [0.0, -0.0, 0.0])
        assert np.signbit(v).tolist() == [False, True, True]


def test_average_counter_wraps_at_65536():
    ones = np.ones(65537, dtype=np.float32)
    v, s = series("float32", False, "average", ones)
    assert v[65534] == 1.0 and v[65535] == 65536.0 and v[65536] == 65537.0
    series("float32", False, "average", np.repeat(ones, 4), lens=[65537, 4])  # rows of 4 cells: the chunked row form, 17 chunks
    series("float64", False, "average", np.ones(65537 * 8), lens=[65537, 8])  # rows of four slots: the column form counts the same way


def test_masks():
    for type_name in TYPES:
        masks_of(type_name)


def masks_of(type_name):
    for lens, axis in (([3, 40, 8], 1), ([6, 40], 1)):
        for default_is_nan in (False, True):
            typed, status = random_cells(lens, type_name, default_is_nan, seed=17, unset=0.5)
            check(lens, axis, type_name, default_is_nan, "sum", typed, status)
            typed, status = random_cells(lens, type_name, default_is_nan, seed=18, unset=0.1, lead=int(np.prod(lens)) // 3)
            for method in ("sum", "last", "average"):
                check(lens, axis, type_name, default_is_nan, method, typed, status)


# ---- batches ----------------------------------------------------------------------------------------------------------
def test_nine_measures_of_one_type_leave_in_two_launches():
    lens = [4, 9, 6]
    inputs = [random_cells(lens, "float32", False, seed=100 + i, unset=0.3)[0] for i in range(9)]
    stores = [make_store(t, None, "float32", False) for t in inputs]
    rules = [METHODS[i % 7] for i in range(9)]
    outs, launches = pkg.HipStore.cumulate_multi(stores, rules, lens, 1, [0, 0, 0, 1, 1, 2, 2, 2, 2])
    assert launches == 2
    for t, rule, out in zip(inputs, rules, outs):
        want_v, want_s = cumulate_reference(t, None, lens, 1, rule, "float32", False, [0, 0, 0, 1, 1, 2, 2, 2, 2])
        assert raw(out.get_data()) == raw(want_v) and np.array_equal(out.get_status(), want_s), rule


def test_mixed_types_defaults_and_rules_in_one_call():
    lens = [5, 11]
    kinds = [("float32", False, "sum"), ("int32", True, "average"), ("float32", False, "highest"), ("float64", True, "product"),
             ("uint32", False, "lowest"), ("int32", True, "sum"), ("float32", True, "last")]
    inputs = [random_cells(lens, t, d, seed=200 + i, unset=0.3) for i, (t, d, _) in enumerate(kinds)]
    stores = [make_store(v, st, t, d) for (v, st), (t, d, _) in zip(inputs, kinds)]
    outs, launches = pkg.HipStore.cumulate_multi(stores, [m for _, _, m in kinds], lens, 1)
    assert launches == len({(t, d) for t, d, _ in kinds}) == 5
    for (v, st), (t, d, m), out in zip(inputs, kinds, outs):
        want_v, want_s = cumulate_reference(v, st, lens, 1, m, t, d)
        assert out.type == t and out.default_is_nan == d
        assert raw(out.get_data()) == raw(want_v) and np.array_equal(out.get_status(), want_s), (t, d, m)
    outs, launches = pkg.HipStore.cumulate_multi([], [], lens, 1)
    assert outs == [] and launches == 0


def test_an_empty_cube_launches_nothing():
    s = pkg.HipStore(0, "float32", 0.0)
    outs, launches = pkg.HipStore.cumulate_multi([s], ["sum"], [3, 0, 2], 1)
    assert launches == 0 and outs[0].size == 0


# ---- the defining chain on the device -------------------------------------------------------------------------------
@pytest.mark.parametrize("type_name,default_is_nan", [("float32", False), ("int32", True)])
def test_bit_for_bit_with_the_device_dice_drillup_chain(type_name, default_is_nan):
    """K < 256: the chain's roll-ups never re-associate, so cumulate equals it bit for bit at every position"""
    lens, groups = [3, 12, 5], [0, 0, 0, 0, 0, 1, 1, 1, 2, 1, 2, 2]
    outer, K, inner = lens
    rng = np.random.default_rng(3)
    typed, status = random_cells(lens, type_name, default_is_nan, seed=3, unset=0.3)
    if type_name == "float32":
        typed = np.where(typed != 0, (rng.random(typed.size) * 8 - 4).astype(np.float32), typed)  # sums that do round
    s = make_store(typed, status, type_name, default_is_nan)
    for method in ("sum", "average", "product", "highest"):
        out = s.cumulate(lens, 1, method, groups)
        got_v, got_s = out.get_data().reshape(lens), out.get_status().reshape(lens)
        for k in range(K):
            members = [j for j in range(k + 1) if groups[j] == groups[k]]
            mid = [outer, len(members), inner]
            chain = s.dice(lens, mid, [range(outer), members, range(inner)]).drill_up(
                mid, [outer, 1, inner], [range(outer), [0] * len(members), range(inner)], method)
            assert raw(chain.get_data()) == raw(got_v[:, k, :]), (method, k)
            assert np.array_equal(chain.get_status(), got_s[:, k, :].ravel()), (method, k)
