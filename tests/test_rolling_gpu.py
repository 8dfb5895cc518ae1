"""olap_store_rolling_multi (rolling windows along a dimension, olap_rolling.hip) against tests/rolling_reference.py, which
tests/test_rolling_reference.py pins to the oracle: typed cells as raw bytes and the mask.  Every case also checks that
the inputs are unchanged and that a second run gives identical bytes.

Shapes are the smallest at which each form can go wrong: tiles of whole-width series (inner below four 16-byte slots)
with several series per tile, several tiles and a partial last one, and series cut into chunks of rows; tiles of columns
with whole and ragged rows, several tiles along inner and along K; windows that straddle tile borders along K; the direct
form just past the window that still fits a tile.  olap_diag_rolling_choice says what the planner does with each shape,
and tests/test_rolling_host.py checks there, without a GPU, that these lists reach every form and every tile border."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import load_package
from cumulate_reference import METHODS, NP
from rolling_reference import rolling_reference
from test_cumulate_gpu import GROUPS, make_store, random_cells, raw

pytestmark = pytest.mark.gpu

pkg = load_package()
TYPES = ("int32", "uint32", "float32", "float64")
SERIES, COLUMNS, DIRECT = 0, 1, 2  # the forms olap_diag_rolling_choice reports

WINDOWS = [(2, 0), (1, 1), (0, 3), (1, -1)]
FORM_SHAPES = [[3, 5, 8], [2, 7, 5], [2, 5, 17], [2, 3, 1030], [5, 7], [70, 33], [600, 7]]  # the dimension is axis 1
# windows of 12 and 41 rows over tiles of fewer rows than K: [3, 300] fits one tile whole, the others are cut along K
STRADDLE_SHAPES = [[2, 300, 16], [3, 300], [3, 2500], [2, 700, 5]]
STRADDLE_BEFORE = (11, 40)
GRID_SHAPES = [[1800, 7], [2, 30, 1030], [6, 2500]]  # six or more tiles each
# (cell type, shape): rows of four slots (columns) and of 15 cells (series); the largest window that fits a tile comes from the planner
EDGE_SHAPES = [("float64", [1, 260, 8]), ("float32", [1, 260, 16]), ("int32", [1, 300, 15])]


def view(lens, axis=1):
    return (int(np.prod(lens[:axis], dtype=np.int64)), lens[axis], int(np.prod(lens[axis + 1:], dtype=np.int64)))


def choice(type_name, lens, before, after=0, axis=1):
    """(form, series per tile, output rows per tile, cells per tile row) the planner chooses"""
    c = (C.c_uint32 * 4)()
    outer, K, inner = view(lens, axis)
    pkg.capi.check(pkg.capi.lib().olap_diag_rolling_choice(NP[type_name]().itemsize, outer, K, inner, before, after, 0, c))
    return tuple(c)


def tiles(type_name, lens, before, after=0, axis=1):
    """tiles along (outer, K, inner) of the tiled forms"""
    form, series, rows, cols = choice(type_name, lens, before, after, axis)
    outer, K, inner = view(lens, axis)
    return (-(-outer // series), -(-K // rows), -(-inner // cols))


def first_direct(type_name, lens):
    """the smallest `before` (after = 0) the planner sends to the direct form"""
    return next(b for b in range(lens[1] + 1) if choice(type_name, lens, b)[0] == DIRECT)


def check(lens, axis, type_name, default_is_nan, method, typed, before, after=0, status=None, groups=None, n_groups=None):
    typed = np.asarray(typed, dtype=NP[type_name])
    s = make_store(typed, status, type_name, default_is_nan)
    held = (raw(s.get_data()), raw(s.get_status()))
    out = s.rolling(lens, axis, method, before, after, groups, n_groups)
    want_v, want_s = rolling_reference(typed, status, lens, axis, method, type_name, default_is_nan, before, after, groups)
    got_v, got_s = out.get_data(), out.get_status()
    where = (lens, axis, type_name, default_is_nan, method, before, after)
    assert np.array_equal(got_s, want_s), (where, np.nonzero(got_s != want_s)[0][:8])
    if raw(got_v) != raw(want_v):
        bad = np.nonzero(got_v.view(np.uint8).reshape(typed.size, -1) != want_v.view(np.uint8).reshape(typed.size, -1))[0][:8]
        raise AssertionError((where, bad, got_v[bad], want_v[bad]))
    assert (raw(s.get_data()), raw(s.get_status())) == held, where  # the input is only read
    again = s.rolling(lens, axis, method, before, after, groups, n_groups)
    assert raw(again.get_data()) == raw(got_v) and raw(again.get_status()) == raw(got_s), where
    return out


# ---- forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type_name", TYPES)
@pytest.mark.parametrize("lens", FORM_SHAPES)
def test_every_rule_default_and_window_on_every_form(lens, type_name):
    for default_is_nan in (False, True):
        typed, status = random_cells(lens, type_name, default_is_nan, seed=sum(lens) + len(type_name), unset=0.3)
        for method in METHODS:
            for before, after in WINDOWS:
                check(lens, 1, type_name, default_is_nan, method, typed, before, after, status)


@pytest.mark.parametrize("lens", STRADDLE_SHAPES)
def test_windows_that_straddle_tile_borders_along_k(lens):
    for type_name in TYPES:
        default_is_nan = type_name == "int32"
        typed, status = random_cells(lens, type_name, default_is_nan, seed=sum(lens), unset=0.3)
        for before in STRADDLE_BEFORE:
            check(lens, 1, type_name, default_is_nan, "sum" if before == 11 else "highest", typed, before, 0, status)
        check(lens, 1, type_name, default_is_nan, "average", typed, 5, 6, status)


@pytest.mark.parametrize("type_name,lens", EDGE_SHAPES)
def test_the_largest_window_that_fits_a_tile_and_the_first_that_does_not(type_name, lens):
    over = first_direct(type_name, lens)
    assert choice(type_name, lens, over - 1)[0] != DIRECT and choice(type_name, lens, over)[0] == DIRECT
    default_is_nan = type_name == "int32"
    typed, status = random_cells(lens, type_name, default_is_nan, seed=over, unset=0.3)
    for before in (over - 1, over):
        check(lens, 1, type_name, default_is_nan, "sum", typed, before, 0, status)
    check(lens, 1, type_name, default_is_nan, "lowest", typed, over // 2, over - over // 2, status)  # the same width, centred: direct
    check(lens, 1, type_name, default_is_nan, "average", typed, over + 3, -3, status)


def test_workgroups_that_walk_several_tiles():
    """OLAP_ROLLING_GRID (a developer knob) caps the workgroups of a launch: with 2 of them every workgroup takes several
    tiles (tiled forms) or several strides of lanes (direct form), as launches beyond the grid limit do"""
    os.environ["OLAP_ROLLING_GRID"] = "2"
    try:
        for lens in GRID_SHAPES:
            for type_name, default_is_nan in (("float32", False), ("int32", True)):
                typed, status = random_cells(lens, type_name, default_is_nan, seed=sum(lens), unset=0.3)
                for method, (before, after) in (("sum", (2, 0)), ("average", (1, 1))):
                    check(lens, 1, type_name, default_is_nan, method, typed, before, after, status, np.arange(lens[1]) // 5, (lens[1] + 4) // 5)
        type_name, lens = EDGE_SHAPES[1]
        typed, status = random_cells(lens, type_name, False, seed=9, unset=0.3)
        check(lens, 1, type_name, False, "sum", typed, first_direct(type_name, lens), 0, status)
    finally:
        del os.environ["OLAP_ROLLING_GRID"]


# ---- groups -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GROUPS))
def test_groups(name):
    groups, n_groups = GROUPS[name]
    K = len(groups) if groups else 6
    for type_name in TYPES:
        for lens, axis in (([3, K, 8], 1), ([3, K, 5], 1), ([9, K], 1), ([K, 6], 0), ([2, K, 17], 1)):
            typed, status = random_cells(lens, type_name, True, seed=K + len(lens), unset=0.25)
            for method, (before, after) in (("sum", (2, 0)), ("average", (1, 1)), ("lowest", (0, 3)), ("last", (1, -1))):
                check(lens, axis, type_name, True, method, typed, before, after, status, groups, n_groups)


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_groups_on_the_direct_form(name):
    """the same four kinds of map over 260 items: uneven runs, interleaved, an id nobody maps to, none"""
    type_name, lens = EDGE_SHAPES[1]
    K = lens[1]
    groups, n_groups = {
        "uneven contiguous 1,4,2": (np.repeat([0, 1, 2], [1, K - 100, 99]), 3),
        "interleaved": (np.arange(K) % 3, 3),
        "a group id nobody maps to": (np.repeat([0, 2, 3], [100, 100, K - 200]), 5),
        "NULL map": (None, None),
    }[name]
    before = first_direct(type_name, lens)
    typed, status = random_cells(lens, type_name, False, seed=K, unset=0.25)
    for method in ("sum", "average"):
        check(lens, 1, type_name, False, method, typed, before, 0, status, groups, n_groups)
        check(lens, 1, type_name, False, method, typed, before - 1, 0, status, groups, n_groups)  # and the widest tiled window


# ---- windows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [[3, 9, 8], [4, 9, 3], [9, 9]])
def test_windows_that_cover_everything_copy_and_run_off_the_end(lens):
    groups = [0, 0, 0, 1, 1, 2, 2, 2, 2]
    outer, K, inner = view(lens)
    for type_name in TYPES:
        default_is_nan = type_name in ("int32", "float64")
        typed, status = random_cells(lens, type_name, default_is_nan, seed=K + len(type_name), unset=0.3)
        s = make_store(typed, status, type_name, default_is_nan)
        for method in ("sum", "average", "product"):
            # before and after beyond K: every cell holds its group's roll-up
            out = check(lens, 1, type_name, default_is_nan, method, typed, K + 5, 2 ** 31 - 1, status, groups)
            got_v, got_s = out.get_data().reshape(outer, K, inner), out.get_status().reshape(outer, K, inner)
            rolled = s.drill_up(lens, [outer, 3, inner], [range(outer), groups, range(inner)], method)
            up_v, up_s = rolled.get_data().reshape(outer, 3, inner), rolled.get_status().reshape(outer, 3, inner)
            assert raw(got_v) == raw(up_v[:, groups, :]) and np.array_equal(got_s, up_s[:, groups, :]), (type_name, method)
            # before = after = 0: a copy, bit for bit
            out = check(lens, 1, type_name, default_is_nan, method, typed, 0, 0, status, groups)
            assert raw(out.get_data()) == raw(s.get_data()) and raw(out.get_status()) == raw(s.get_status()), (type_name, method)
        # a lead of two runs off the end: the last two items are unset; a window wholly off the dimension: everything is
        out = check(lens, 1, type_name, default_is_nan, "sum", typed, -2, 2, status)
        assert not out.get_status().reshape(outer, K, inner)[:, K - 2:, :].any()
        out = check(lens, 1, type_name, default_is_nan, "sum", typed, -(2 ** 31 - 1), 2 ** 31 - 1, status)
        assert not out.get_status().any()


# ---- values where a wrong implementation shows ----------------------------------------------------------------------
def series(type_name, default_is_nan, method, values, before, after=0, lens=None, axis=0, status=None):
    values = np.asarray(values, dtype=NP[type_name])
    out = check(lens or [values.size], axis, type_name, default_is_nan, method, values, before, after, status)
    return out.get_data(), out.get_status()


def test_float32_is_rounded_once_per_cell_never_in_between():
    v, s = series("float32", False, "sum", [2 ** 24, 1, -(2 ** 24)], 2)
    assert v.tolist() == [16777216.0, 16777216.0, 1.0] and s.tolist() == [2, 2, 2]
    # the same series as columns (inner = 16) and among other series of a tile
    series("float32", False, "sum", np.repeat([2 ** 24, 1, -(2 ** 24)], 16), 2, lens=[3, 16])
    series("float32", False, "sum", np.tile([2 ** 24, 1, -(2 ** 24)], 5), 2, lens=[5, 3], axis=1)
    # every window is its own fold: nothing is left over from a value that has left the window
    v, s = series("float64", False, "sum", [1e16, 1.0, -1e16, 1.0, 1.0], 1)
    assert v.tolist() == [1e16, 1e16 + 1.0, 1.0 - 1e16, 1.0 - 1e16, 2.0]


def test_integer_sums_wrap():
    v, s = series("int32", False, "sum", [2 ** 31 - 1, 1, 1], 1)
    assert v.tolist() == [2 ** 31 - 1, -(2 ** 31), 2]
    v, s = series("uint32", False, "sum", [2 ** 32 - 1, 2, 2 ** 32 - 2], 2)
    assert v.tolist() == [2 ** 32 - 1, 1, 2 ** 32 - 1]
    v, s = series("int32", True, "product", [65536, 65536, 3], 1)  # 2^32 wraps to a SET 0 under the NaN default
    assert v.tolist() == [65536, 0, 196608] and s.tolist() == [2, 2, 2]


def test_restarts():
    v, s = series("float32", False, "sum", [5, -5, 3, 1], 1)
    assert v.tolist() == [5.0, 0.0, -2.0, 4.0] and s.tolist() == [2, 0, 2, 2]
    v, s = series("float32", False, "sum", [5, -5, 3, 1], 2)  # the restart falls inside the window of item 2
    assert v.tolist() == [5.0, 0.0, 3.0, -1.0] and s.tolist() == [2, 0, 2, 2]
    v, s = series("float32", True, "sum", [np.inf, -np.inf, 2], 2)
    assert s.tolist() == [2, 0, 2] and v[2] == 2.0
    v, s = series("float64", True, "sum", [np.inf, -np.inf, 2, 5], 3)
    assert s.tolist() == [2, 0, 2, 2] and v[3] == 7.0
    v, s = series("float64", False, "product", [4, 1e-200, 1e-200, 3, 2], 4)  # underflows to 0: unset, then 3, 6
    assert v.tolist()[2:] == [0.0, 3.0, 6.0] and s.tolist() == [2, 2, 0, 2, 2]
    v, s = series("int32", False, "average", [4, -4, 6, 0, 2], 4)  # the count survives the restart
    assert s.tolist() == [2, 0, 2, 2, 2] and v.tolist() == [4, 0, 2, 2, 2]
    v, s = series("float32", False, "average", [2, 0, 4], 1)
    assert v.tolist() == [2.0, 2.0, 4.0]


def test_special_floats():
    for type_name in ("float32", "float64"):
        nan_set = [1, np.nan, 2, 0, 3, 4]  # a set NaN under a 0 default poisons sums and extremes while it is in the window
        minus_zero = [-0.0, 0.0, -1, -0.0, 1, -0.0]  # -0 equals the 0 default: unset; under NaN it is a value
        for method in METHODS:
            for before, after in ((2, 0), (1, 1)):
                series(type_name, False, method, nan_set, before, after)
                series(type_name, False, method, minus_zero, before, after)
                series(type_name, True, method, minus_zero, before, after)
        v, s = series(type_name, True, "highest", [-0.0, 0.0, -0.0], 1)
        assert np.signbit(v).tolist() == [True, False, False]
        v, s = series(type_name, True, "lowest", [0.0, -0.0, 0.0], 1)
        assert np.signbit(v).tolist() == [False, True, True]


def test_average_counter_wraps_at_65536():
    """65 536 contributions: the Uint16 counter reads 0 and the sum is left as it is (by hand: the restatement is not run at this size)"""
    s = make_store(np.ones(65537, dtype=np.float32), None, "float32", False)
    out = s.rolling([65537], 0, "average", 65535)
    v = out.get_data()
    assert (v[:65535] == 1.0).all() and v[65535] == 65536.0 and v[65536] == 65536.0
    assert (out.get_status() == 2).all()


def test_masks():
    for type_name in TYPES:
        for lens in ([3, 40, 8], [6, 40], [2, 40, 20]):
            for default_is_nan in (False, True):
                typed, status = random_cells(lens, type_name, default_is_nan, seed=17, unset=0.5)
                check(lens, 1, type_name, default_is_nan, "sum", typed, 3, 0, status)
                typed, status = random_cells(lens, type_name, default_is_nan, seed=18, unset=0.1, lead=int(np.prod(lens)) // 3)
                for method in ("last", "average"):
                    check(lens, 1, type_name, default_is_nan, method, typed, 1, 2, status)


# ---- batches ----------------------------------------------------------------------------------------------------------
def test_nine_measures_of_one_type_leave_in_two_launches():
    lens, groups = [4, 9, 6], [0, 0, 0, 1, 1, 2, 2, 2, 2]
    inputs = [random_cells(lens, "float32", False, seed=100 + i, unset=0.3)[0] for i in range(9)]
    stores = [make_store(t, None, "float32", False) for t in inputs]
    rules = [METHODS[i % 7] for i in range(9)]
    outs, launches = pkg.HipStore.rolling_multi(stores, rules, lens, 1, 2, 1, groups)
    assert launches == 2
    for t, rule, out in zip(inputs, rules, outs):
        want_v, want_s = rolling_reference(t, None, lens, 1, rule, "float32", False, 2, 1, groups)
        assert raw(out.get_data()) == raw(want_v) and np.array_equal(out.get_status(), want_s), rule


def test_mixed_types_defaults_and_rules_in_one_call():
    lens = [5, 11]
    kinds = [("float32", False, "sum"), ("int32", True, "average"), ("float32", False, "highest"), ("float64", True, "product"),
             ("uint32", False, "lowest"), ("int32", True, "sum"), ("float32", True, "last")]
    inputs = [random_cells(lens, t, d, seed=200 + i, unset=0.3) for i, (t, d, _) in enumerate(kinds)]
    stores = [make_store(v, st, t, d) for (v, st), (t, d, _) in zip(inputs, kinds)]
    outs, launches = pkg.HipStore.rolling_multi(stores, [m for _, _, m in kinds], lens, 1, 1, 1)
    assert launches == len({(t, d) for t, d, _ in kinds}) == 5
    for (v, st), (t, d, m), out in zip(inputs, kinds, outs):
        want_v, want_s = rolling_reference(v, st, lens, 1, m, t, d, 1, 1)
        assert out.type == t and out.default_is_nan == d
        assert raw(out.get_data()) == raw(want_v) and np.array_equal(out.get_status(), want_s), (t, d, m)
    outs, launches = pkg.HipStore.rolling_multi([], [], lens, 1, 1)
    assert outs == [] and launches == 0


def test_an_empty_cube_launches_nothing():
    s = pkg.HipStore(0, "float32", 0.0)
    outs, launches = pkg.HipStore.rolling_multi([s], ["sum"], [3, 0, 2], 1, 2)
    assert launches == 0 and outs[0].size == 0


def test_an_empty_window_is_refused():
    s = pkg.HipStore(6, "float32", 0.0)
    with pytest.raises(pkg.OlapError) as e:
        s.rolling([2, 3], 1, "sum", 1, -2)
    assert e.value.code == pkg.capi.ERR_INVALID_ARGUMENT and "rolling: empty window (before 1, after -2)" in str(e.value)


# ---- the defining chain on the device -------------------------------------------------------------------------------
@pytest.mark.parametrize("type_name,default_is_nan", [("float32", False), ("int32", True)])
def test_bit_for_bit_with_the_device_dice_drillup_chain(type_name, default_is_nan):
    lens, groups = [3, 12, 5], [0, 1, 0, 2, 1, 0, 1, 2, 0, 1, 2, 2]
    outer, K, inner = lens
    rng = np.random.default_rng(3)
    typed, status = random_cells(lens, type_name, default_is_nan, seed=3, unset=0.3)
    if type_name == "float32":
        typed = np.where(typed != 0, (rng.random(typed.size) * 8 - 4).astype(np.float32), typed)  # sums that do round
    s = make_store(typed, status, type_name, default_is_nan)
    for before, after in ((3, 0), (1, 2)):
        for method in ("sum", "average", "product", "highest"):
            out = s.rolling(lens, 1, method, before, after, groups)
            got_v, got_s = out.get_data().reshape(lens), out.get_status().reshape(lens)
            for k in range(K):
                members = [j for j in range(max(k - before, 0), min(k + after, K - 1) + 1) if groups[j] == groups[k]]
                mid = [outer, len(members), inner]
                chain = s.dice(lens, mid, [range(outer), members, range(inner)]).drill_up(
                    mid, [outer, 1, inner], [range(outer), [0] * len(members), range(inner)], method)
                assert raw(chain.get_data()) == raw(got_v[:, k, :]), (method, before, after, k)
                assert np.array_equal(chain.get_status(), got_s[:, k, :].ravel()), (method, before, after, k)
