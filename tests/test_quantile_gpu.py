"""olap_store_quantile_multi (order statistics along a dimension, olap_quantile.hip) against tests/quantile_reference.py,
which tests/test_quantile_reference.py pins by hand-worked literals and numpy.quantile: typed cells as raw bytes and the
mask, no tolerance.  Every case also checks that the inputs are unchanged and that a second run gives identical bytes.

NaN: the library writes ONE NaN — the kernel replaces a NaN result by the quiet NaN 0x7FF8000000000000 before the
conversion to the cell type (Float32: 0x7FC00000), which is also the NaN default — and the restatement emits np.nan, the
same bits, so NaN cells are compared as bytes like every other cell.

Shapes are the smallest at which each form can go wrong; olap_diag_quantile_choice (host only) says which form the
planner takes for each, and tests/test_quantile_host.py asserts the same lists without a device.  OLAP_QUANTILE_TILE
(cells a tile may hold) puts the direct forms within reach of small cubes; the series around the REAL tile are run too."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import load_package
from quantile_reference import NP, quantile_reference

pytestmark = pytest.mark.gpu

pkg = load_package()
TYPES = ("int32", "uint32", "float32", "float64")
QS = (0, 0.25, 0.3, 0.5, 0.9, 1)
COLUMN, ROW, DIRECT_LANES, DIRECT_BLOCK = 0, 1, 2, 3  # the forms olap_diag_quantile_choice reports
SMALL_TILE = 64  # OLAP_QUANTILE_TILE of the direct-form cases

# Rows of fewer than four 16-byte slots take the row form: [3, 5, 8] is a column shape for 8-byte cells only.
COLUMN_SHAPES = [[3, 5, 8], [2, 5, 17], [2, 3, 1030], [2, 300, 16], [2, 300, 18]]
# A tile holds min(tile / (K * inner), 256) whole series: [600, 7] is tiles of 256, 256 and 88 series
ROW_SHAPES = [[5, 7], [70, 33], [4, 6, 3], [600, 7]]
GROUP_SIZES = (1, 2, 3, 31, 64, 65)  # contiguous groups of these many members (rank counting up to 16, bisection above)
SIZED_GROUPS = np.repeat(np.arange(len(GROUP_SIZES)), GROUP_SIZES)
GROUP_SHAPES = [[2, len(SIZED_GROUPS), 16], [3, len(SIZED_GROUPS)]]
# under OLAP_QUANTILE_TILE=64: series one cell under, at, over and twice over the tile; a wide inner with groups beyond a tile
DIRECT_BLOCK_SHAPES = [[3, SMALL_TILE - 1], [3, SMALL_TILE], [3, SMALL_TILE + 1], [3, 2 * SMALL_TILE + 5]]
DIRECT_LANES_SHAPE = [1, 40, 4096]


def raw(a):
    return np.ascontiguousarray(a).tobytes()


def has_mask(type_name, default_is_nan):
    return default_is_nan and not type_name.startswith("float")


def choice(type_name, default_is_nan, lens, axis=1, groups=None, n_groups=None):
    """(form, tile cells, series, pitch, cols, rows) the planner picks"""
    outer, K, inner = int(np.prod(lens[:axis], dtype=np.int64)), lens[axis], int(np.prod(lens[axis + 1:], dtype=np.int64))
    if groups is None:
        G, longest, contiguous = 1, K, 1
    else:
        g = np.asarray(groups)
        G = int(n_groups) if n_groups is not None else int(g.max()) + 1
        longest = int(np.bincount(g, minlength=G).max())
        contiguous = int(np.all(np.diff(g) >= 0))
    c = (C.c_uint32 * 6)()
    pkg.capi.check(pkg.capi.lib().olap_diag_quantile_choice(NP[type_name]().itemsize, int(has_mask(type_name, default_is_nan)), outer, K, inner, G,
                                                            longest, contiguous, c))
    return tuple(c)


def make_store(typed, status, type_name, default_is_nan):
    default = float("nan") if default_is_nan else 0.0
    if status is None:
        s = pkg.HipStore(typed.size, type_name, default)
        s.set_data(typed)
        return s
    idx = np.nonzero(status & 2)[0]
    return pkg.HipStore.from_sparse(typed.size, type_name, default, idx, typed[idx])


def random_cells(lens, type_name, default_is_nan, seed, unset=0.3):
    """values where shortcuts fail: small integers (mostly duplicates) with `unset` of the cells unset; Float64 members
    equal in their upper 32 bits; uint32 above 2^31; negative int32"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(lens))
    v = rng.integers(-3, 4, size=n).astype(np.float64)
    if type_name == "float64":
        v = np.where(rng.random(n) < 0.5, 1.0 + rng.integers(0, 1000, size=n) * 2.0 ** -52, v)  # 1 + a few ulps: one upper word
    if type_name == "float32":
        v = np.where(rng.random(n) < 0.2, rng.integers(-8, 8, size=n) * 0.375, v)
    if type_name == "uint32":
        v = np.where(v < 0, 4294967296.0 + v * 1000, v)  # 2^32 - 1000 .. 2^32 - 3000: above 2^31
    if type_name == "int32":
        v = np.where(rng.random(n) < 0.2, -(2.0 ** 31) + rng.integers(0, 3, size=n), v)
    typed = v.astype(NP[type_name])
    gone = rng.random(n) < unset
    status = None
    if has_mask(type_name, default_is_nan):
        status = np.where(gone, 0, 2).astype(np.int32)
    else:
        typed[gone] = np.nan if default_is_nan else 0
    return typed, status


def check(lens, axis, type_name, default_is_nan, qs, typed, status=None, groups=None, n_groups=None):
    typed = np.asarray(typed, dtype=NP[type_name])
    s = make_store(typed, status, type_name, default_is_nan)
    before = (raw(s.get_data()), raw(s.get_status()))
    wants = quantile_reference(typed, status, lens, axis, list(qs), type_name, default_is_nan, groups, n_groups)
    out = None
    for q, (want_v, want_s) in zip(qs, wants):
        out = s.quantile(lens, axis, q, groups, n_groups)
        got_v, got_s = out.get_data(), out.get_status()
        where = (lens, axis, type_name, default_is_nan, q)
        assert out.size == want_v.size and out.type == type_name and out.default_is_nan == default_is_nan, where
        assert np.array_equal(got_s, want_s), (where, np.nonzero(got_s != want_s)[0][:8])
        if raw(got_v) != raw(want_v):
            bad = np.nonzero(got_v.view(np.uint8).reshape(want_v.size, -1) != want_v.view(np.uint8).reshape(want_v.size, -1))[0][:8]
            raise AssertionError((where, bad, got_v[bad], want_v[bad]))
    assert (raw(s.get_data()), raw(s.get_status())) == before  # the input is only read
    again = s.quantile(lens, axis, qs[-1], groups, n_groups)
    assert raw(again.get_data()) == raw(out.get_data()) and raw(again.get_status()) == raw(out.get_status())
    return out


def every_type_and_default(lens, axis=1, groups=None, n_groups=None, qs=QS, want_form=None, types=TYPES):
    for type_name in types:
        for default_is_nan in (False, True):
            if want_form is not None:
                assert choice(type_name, default_is_nan, lens, axis, groups, n_groups)[0] in want_form, (lens, type_name)
            typed, status = random_cells(lens, type_name, default_is_nan, seed=sum(lens) + len(type_name))
            check(lens, axis, type_name, default_is_nan, qs, typed, status, groups, n_groups)


def expected_form(lens, type_name):
    """COLUMN_SHAPES / ROW_SHAPES / GROUP_SHAPES under the real tile"""
    inner = int(np.prod(lens[2:], dtype=np.int64))
    return COLUMN if inner >= 4 * (16 // NP[type_name]().itemsize) else ROW


# ---- forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", COLUMN_SHAPES + ROW_SHAPES)
def test_every_type_default_and_q_on_the_tiled_forms(lens):
    for type_name in TYPES:
        assert choice(type_name, False, lens)[0] == expected_form(lens, type_name)
    every_type_and_default(lens)


@pytest.mark.parametrize("lens", GROUP_SHAPES)
def test_groups_of_1_2_3_31_64_and_65_members(lens):
    every_type_and_default(lens, groups=SIZED_GROUPS, want_form=(expected_form(lens, "float32"),))


@pytest.mark.parametrize("lens", [[2, 12, 16], [3, 12, 5], [7, 12]])
def test_interleaved_groups_and_group_ids_nobody_maps_to(lens):
    every_type_and_default(lens, groups=np.arange(12) % 5, qs=(0.3, 0.5))
    every_type_and_default(lens, groups=[0, 0, 2, 2, 3, 3, 0, 5, 5, 5, 2, 0], n_groups=8, qs=(0.25, 1))
    every_type_and_default([12] + lens[2:] + [3], axis=0, groups=np.arange(12) % 5, qs=(0.5,))  # along the first dimension


def test_rank_counting_and_bisection_agree_with_the_reference_on_the_same_groups():
    """OLAP_QUANTILE_RANK (a developer knob): groups of at most that many members count ranks; 0: every group bisects"""
    for knob in ("0", "1000"):
        os.environ["OLAP_QUANTILE_RANK"] = knob
        try:
            for lens in GROUP_SHAPES:
                every_type_and_default(lens, groups=SIZED_GROUPS, qs=(0.25, 0.3, 1))
        finally:
            del os.environ["OLAP_QUANTILE_RANK"]


def small_tile(fn):
    os.environ["OLAP_QUANTILE_TILE"] = str(SMALL_TILE)
    try:
        fn()
    finally:
        del os.environ["OLAP_QUANTILE_TILE"]


def direct_cases():
    for lens in DIRECT_BLOCK_SHAPES:
        want = ROW if lens[1] <= SMALL_TILE else DIRECT_BLOCK
        every_type_and_default(lens, want_form=(want,), qs=(0, 0.3, 0.5, 1))
    K = SMALL_TILE + 1
    # interleaved groups over a series beyond the tile: groups that fit a tile are staged member by member (the column form
    # with the whole row a slice), groups beyond it are read in place
    every_type_and_default([2, K], groups=np.arange(K) % 3, want_form=(COLUMN,), qs=(0.3, 0.9))
    every_type_and_default([2, K, 3], groups=np.arange(K) // 9, want_form=(COLUMN,), qs=(0.3, 0.9))
    every_type_and_default([2, 2 * K + 3], groups=np.arange(2 * K + 3) % 2, want_form=(DIRECT_BLOCK,), qs=(0.3, 0.9))
    every_type_and_default([2, K, 16], groups=np.arange(K) % 2, want_form=(DIRECT_BLOCK,), qs=(0.5,))  # groups of 33 rows of 16: beyond 64 cells
    every_type_and_default(DIRECT_LANES_SHAPE, want_form=(DIRECT_LANES,), qs=(0.3, 0.5), types=("float32", "float64", "int32"))
    # the tiled forms with tiles this small: several group tiles per slice, several series tiles
    every_type_and_default([2, 30, 16], groups=np.arange(30) // 3, want_form=(COLUMN,), qs=(0.3, 0.5))
    every_type_and_default([40, 7], want_form=(ROW,), qs=(0.3, 0.5))


def test_the_direct_forms_around_a_small_tile():
    small_tile(direct_cases)


@pytest.mark.parametrize("type_name,default_is_nan", [("float32", False), ("int32", True), ("float64", True)])
def test_series_around_the_real_tile(type_name, default_is_nan):
    tile = choice(type_name, default_is_nan, [3, 5])[1]
    assert tile == 32768 // (NP[type_name]().itemsize + (4 if has_mask(type_name, default_is_nan) else 0))
    for K in (tile - 1, tile, tile + 1, 2 * tile + 5):
        lens = [3, K]
        assert choice(type_name, default_is_nan, lens)[0] == (ROW if K <= tile else DIRECT_BLOCK)
        typed, status = random_cells(lens, type_name, default_is_nan, seed=K)
        check(lens, 1, type_name, default_is_nan, (0.3, 0.5), typed, status)
    for K, G, form in ((tile + 1, 3, COLUMN), (2 * tile + 5, 2, DIRECT_BLOCK)):  # interleaved groups that fit a tile, and that do not
        lens, groups = [2, K], np.arange(K) % G
        assert choice(type_name, default_is_nan, lens, 1, groups)[0] == form
        typed, status = random_cells(lens, type_name, default_is_nan, seed=5)
        check(lens, 1, type_name, default_is_nan, (0.9,), typed, status, groups)


def test_every_form_again_with_one_workgroup():
    """OLAP_QUANTILE_GRID (a developer knob) caps the workgroups of a launch: with one, a workgroup takes every tile and a
    lane every stride, as launches beyond the grid limit do"""
    os.environ["OLAP_QUANTILE_GRID"] = "1"
    try:
        for lens in ([2, 5, 17], [2, 3, 1030], [600, 7], [4, 6, 3]):
            every_type_and_default(lens, qs=(0.3,))
        every_type_and_default(GROUP_SHAPES[0], groups=SIZED_GROUPS, qs=(0.5,))
        small_tile(direct_cases)
    finally:
        del os.environ["OLAP_QUANTILE_GRID"]


# ---- values where a wrong implementation shows ----------------------------------------------------------------------
def series(type_name, default_is_nan, q, values, lens=None, axis=0, status=None):
    values = np.asarray(values, dtype=NP[type_name])
    out = check(lens or [values.size], axis, type_name, default_is_nan, (q,), values, status)
    return out.get_data(), out.get_status()


def test_the_interpolation_is_not_fused():
    v, s = series("float64", False, 0.3, [0.1, 0.7])
    assert v.tolist() == [0.28] and s.tolist() == [2]  # fused: 0.27999999999999997
    v, s = series("float64", True, 0.3, np.repeat([0.7, 0.1], 8), lens=[2, 8])  # the same in the column form
    assert v.tolist() == [0.28] * 8
    v, s = series("float64", False, 0.3, np.tile([0.7, 0.1], 5), lens=[5, 2], axis=1)
    assert v.tolist() == [0.28] * 5


def test_special_floats():
    inf = np.inf
    for type_name in ("float32", "float64"):
        v, s = series(type_name, True, 0.5, [inf, -inf, 1, 2])
        assert v.tolist() == [1.5]
        v, s = series(type_name, True, 0.5, [inf, -inf])  # -inf + 0.5 * (inf - -inf) = NaN: the default, so unset
        assert s.tolist() == [0] and np.isnan(v[0])
        v, s = series(type_name, False, 0.5, [inf, -inf])  # a set NaN under a 0 default
        assert s.tolist() == [2] and np.isnan(v[0])
        v, s = series(type_name, False, 1, [1, np.nan, 2, 0, 3])  # a NaN member sorts last
        assert s.tolist() == [2] and np.isnan(v[0])
        v, s = series(type_name, False, 0.5, [1, -np.nan, 2, 0, 3])  # ... whatever its sign; members 1 2 3 NaN: 2.5
        assert v.tolist() == [2.5]
        v, s = series(type_name, False, 0.75, [1, np.nan, 2, 0, 3])  # h = 2.25 between 3 and NaN
        assert s.tolist() == [2] and np.isnan(v[0])
        v, s = series(type_name, True, 0, [0.0, -0.0, 0.0])  # -0 sorts before +0 under a NaN default
        assert np.signbit(v).tolist() == [True] and s.tolist() == [2]
        v, s = series(type_name, True, 1, [-0.0, 0.0, -0.0])
        assert np.signbit(v).tolist() == [False]
        v, s = series(type_name, False, 0.5, [-0.0, 0.0, -0.0])  # all equal to the 0 default: no member
        assert s.tolist() == [0]


def test_integer_cells_truncate_once():
    assert series("int32", False, 0.5, [1, 2])[0].tolist() == [1]  # 1.5
    assert series("int32", False, 0.5, [-1, -2])[0].tolist() == [-1]  # -1.5
    assert series("int32", True, 0.5, [-1, 1], status=np.array([2, 2], np.int32))[1].tolist() == [2]  # a SET 0 under the NaN default
    assert series("int32", False, 0.5, [-1, 1])[1].tolist() == [0]  # 0 is the default: unset
    assert series("uint32", False, 0.5, [2 ** 32 - 1, 2 ** 32 - 2])[0].tolist() == [2 ** 32 - 2]
    assert series("int32", False, 0.5, [-(2 ** 31), 2 ** 31 - 1])[0].tolist() == [0]  # -0.5 truncates to 0: unset
    assert series("float64", False, 0.5, [1, 2])[0].tolist() == [1.5]  # an integer measure held in Float64 cells keeps 1.5


def test_all_unset_and_single_members():
    for type_name in TYPES:
        for default_is_nan in (False, True):
            lens = [3, 6, 4]
            typed, status = random_cells(lens, type_name, default_is_nan, seed=1, unset=1.0)
            out = check(lens, 1, type_name, default_is_nan, (0.5,), typed, status)
            assert not out.get_status().any()
            typed, status = random_cells(lens, type_name, default_is_nan, seed=2, unset=0.85)
            check(lens, 1, type_name, default_is_nan, (0, 0.5, 1), typed, status, [0, 1, 0, 1, 2, 2])


# ---- batches, tracked stores --------------------------------------------------------------------------------------------
def test_nine_measures_of_mixed_types_and_defaults():
    lens = [4, 9, 6]
    kinds = [("float32", False)] * 9
    inputs = [random_cells(lens, t, d, seed=100 + i) for i, (t, d) in enumerate(kinds)]
    stores = [make_store(v, st, t, d) for (v, st), (t, d) in zip(inputs, kinds)]
    groups = [0, 0, 0, 1, 1, 2, 2, 2, 2]
    outs, launches = pkg.HipStore.quantile_multi(stores, lens, 1, 0.3, groups)
    assert launches == 2  # nine of one kind: 8 + 1
    kinds = [("float32", False), ("int32", True), ("float32", False), ("float64", True), ("uint32", False), ("int32", True), ("float32", True),
             ("float64", True), ("int32", False)]
    inputs = [random_cells(lens, t, d, seed=200 + i) for i, (t, d) in enumerate(kinds)]
    stores = [make_store(v, st, t, d) for (v, st), (t, d) in zip(inputs, kinds)]
    outs, launches = pkg.HipStore.quantile_multi(stores, lens, 1, 0.3, groups)
    assert launches == len(set(kinds)) == 6
    for (v, st), (t, d), out in zip(inputs, kinds, outs):
        want_v, want_s = quantile_reference(v, st, lens, 1, 0.3, t, d, groups)
        assert out.type == t and out.default_is_nan == d and out.size == 4 * 3 * 6
        assert raw(out.get_data()) == raw(want_v) and np.array_equal(out.get_status(), want_s), (t, d)
    outs, launches = pkg.HipStore.quantile_multi([], lens, 1, 0.5)
    assert outs == [] and launches == 0


def test_a_dimension_without_items_gives_unset_cells():
    s = pkg.HipStore(0, "float32", 0.0)
    outs, launches = pkg.HipStore.quantile_multi([s], [3, 0, 2], 1, 0.5)
    assert outs[0].size == 6 and not outs[0].get_status().any() and not outs[0].get_data().any()
    outs, launches = pkg.HipStore.quantile_multi([s], [3, 0, 2], 0, 0.5)  # no output cell: nothing to launch
    assert launches == 0 and outs[0].size == 0


@pytest.mark.parametrize("type_name,default_is_nan", [("float32", False), ("int32", True)])
def test_a_tracked_store_filled_out_of_order_gives_the_untracked_bytes(type_name, default_is_nan):
    lens = [5, 8, 4]
    typed, status = random_cells(lens, type_name, default_is_nan, seed=9)
    plain = make_store(typed, status, type_name, default_is_nan)
    idx = np.nonzero(plain.get_status() & 2)[0][::-1].copy()  # descending indices
    tracked = pkg.HipStore(typed.size, type_name, float("nan") if default_is_nan else 0.0).track_order()
    tracked.set_values(idx, typed[idx].astype(np.float64))  # the order is now explicit: the last cell is the oldest
    assert tracked.keys()[0] == idx[0] and raw(tracked.get_data()) == raw(plain.get_data())
    groups = [0, 1, 0, 1, 2, 2, 2, 0]
    a, b = plain.quantile(lens, 1, 0.3, groups), tracked.quantile(lens, 1, 0.3, groups)
    assert tracked.order_tracked and not b.order_tracked
    assert raw(a.get_data()) == raw(b.get_data()) and raw(a.get_status()) == raw(b.get_status())
    outs, launches = pkg.HipStore.quantile_multi([plain, tracked], lens, 1, 0.3, groups)
    assert launches == 1 and raw(outs[1].get_data()) == raw(a.get_data())


def test_q_outside_0_1_is_refused():
    s = pkg.HipStore(6, "float32", 0.0)
    for q in (-0.1, 1.5, float("nan")):
        with pytest.raises(pkg.capi.OlapError) as e:
            s.quantile([2, 3], 1, q)
        assert e.value.code == pkg.capi.ERR_INVALID_ARGUMENT and "quantile: q must lie in [0, 1] (got " in str(e.value)
