"""olap_store_variance_multi (variance and standard deviation along a dimension, olap_variance.hip) against
tests/variance_reference.py, which tests/test_variance_reference.py pins by hand-worked literals, statistics over
Fractions and numpy.var: typed cells as raw bytes and the mask, no tolerance, for kind in {0, 1} x ddof in {0, 1}.  Every
case also checks that the inputs are unchanged and that a second run gives identical bytes.

NaN: the library writes ONE NaN — the kernel replaces a NaN result by the quiet NaN 0x7FF8000000000000 before the
conversion to the cell type (Float32: 0x7FC00000), which is also the NaN default — and the restatement emits np.nan, the
same bits, so NaN cells are compared as bytes like every other cell.

Shapes are the smallest at which each form can go wrong; olap_diag_variance_choice (host only) says which form the
planner takes for each, and tests/test_variance_host.py asserts the same lists without a device.  OLAP_VARIANCE_TILE
(cells a tile may hold) puts the lane-per-cell direct form within reach of small cubes, OLAP_VARIANCE_BLOCK (members of
the largest group from which few output cells take a workgroup each) the workgroup form; the series around the REAL tile
are run too, with OLAP_VARIANCE_BLOCK out of reach so that they stay in the one-lane forms.

The workgroup-per-output-cell form is RE-ASSOCIATED: it is compared byte for byte only on data whose every sum is exact
in float64 in any order (integers in [-8, 8) with a power-of-two count of set members: the mean, the deviations, their
squares and the sum of those are all exact), and on Float64 uniform [1, 2) data within 4 (N u + N^2 k^2 u^2) — twice the
sum of the two sides' Chan-Golub-LeVeque two-pass bounds, which hold for any summation order; about 2.2e-12 at N = 5000,
where the summation orders tried on the CPU differ by a few 1e-15 and a dropped member moves the result by 4e-4."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import load_package
from variance_reference import COMBOS, NP, moments_of, variance_reference, variance_reference_all

pytestmark = pytest.mark.gpu

pkg = load_package()
TYPES = ("int32", "uint32", "float32", "float64")
COLUMN, ROW, DIRECT_LANES, DIRECT_BLOCK = 0, 1, 2, 3  # the forms olap_diag_variance_choice reports
SMALL_TILE = 64  # OLAP_VARIANCE_TILE of the direct-form cases
NEVER = str(2 ** 32 - 1)  # OLAP_VARIANCE_BLOCK that no group reaches
BLOCK_CELLS, BLOCK_MEMBERS = 65536, 1024  # the planner's cut for the workgroup form: at most / at least

# Rows of fewer than four 16-byte slots take the row form: [3, 5, 8] is a column shape for 8-byte cells only.
COLUMN_SHAPES = [[3, 5, 8], [2, 5, 17], [2, 3, 1030], [2, 300, 16], [2, 300, 18]]
# A tile holds min(tile / (K * inner), 256) whole series: [600, 7] is tiles of 256, 256 and 88 series
ROW_SHAPES = [[5, 7], [70, 33], [4, 6, 3], [600, 7]]
GROUP_SIZES = (1, 2, 3, 31, 64, 65)  # contiguous groups of these many members
SIZED_GROUPS = np.repeat(np.arange(len(GROUP_SIZES)), GROUP_SIZES)
GROUP_SHAPES = [[2, len(SIZED_GROUPS), 16], [3, len(SIZED_GROUPS)]]
# under OLAP_VARIANCE_TILE=64: series one cell under, at, over and twice over the tile; a wide inner with groups beyond a tile
AROUND_SMALL_TILE = [[3, SMALL_TILE - 1], [3, SMALL_TILE], [3, SMALL_TILE + 1], [3, 2 * SMALL_TILE + 5]]
DIRECT_LANES_SHAPE = [1, 40, 4096]
BLOCK_SHAPE = [2, 5000]  # the real cut: 2 output cells of 5000 members


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
    pkg.capi.check(pkg.capi.lib().olap_diag_variance_choice(NP[type_name]().itemsize, int(has_mask(type_name, default_is_nan)), outer, K, inner, G,
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
    """values where shortcuts fail: small integers (mostly duplicates) with `unset` of the cells unset; Float64 with a
    large common offset (1e9 + {0..7}: E[x^2] - mean^2 cancels); Float32 around 2^24, whose float32 sum would round;
    uint32 above 2^31; negative int32"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(lens))
    v = rng.integers(-3, 4, size=n).astype(np.float64)
    if type_name == "float64":
        v = np.where(rng.random(n) < 0.5, 1e9 + rng.integers(0, 8, size=n), v + 0.1)
    if type_name == "float32":
        v = np.where(rng.random(n) < 0.3, 16777216.0 + 2 * rng.integers(0, 4, size=n), np.where(rng.random(n) < 0.3, v * 0.375, v))
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


def exact_cells(lens, axis, type_name, default_is_nan, seed, members, groups=None):
    """integers in [-8, 8) ([0, 16) for uint32) with exactly `members` (a power of two) set cells per output cell: every
    sum of both passes is exact in float64, whatever the order"""
    rng = np.random.default_rng(seed)
    outer, K, inner = int(np.prod(lens[:axis], dtype=np.int64)), lens[axis], int(np.prod(lens[axis + 1:], dtype=np.int64))
    low = 0 if type_name == "uint32" else -8
    masked = has_mask(type_name, default_is_nan)
    zero_is_unset = not default_is_nan
    v = rng.integers(low, low + 16, size=(outer, K, inner)).astype(np.float64)
    if zero_is_unset:
        v[v == 0] = 5
    keep = np.zeros((outer, K, inner), dtype=bool)
    g = np.zeros(K, dtype=np.int64) if groups is None else np.asarray(groups)
    for gid in range(int(g.max()) + 1):
        items = np.nonzero(g == gid)[0]
        for o in range(outer):
            for i in range(inner):
                keep[o, rng.choice(items, size=members, replace=False), i] = True
    typed = v.astype(NP[type_name]).ravel()
    status = None
    if masked:
        status = np.where(keep.ravel(), 2, 0).astype(np.int32)
    else:
        typed[~keep.ravel()] = np.nan if default_is_nan else 0
    return typed, status


def run_all(s, lens, axis, groups, n_groups):
    return {c: s.variance(lens, axis, c[0], c[1], groups, n_groups) for c in COMBOS}


def check(lens, axis, type_name, default_is_nan, typed, status=None, groups=None, n_groups=None):
    """kind x ddof against the restatement, bytes and mask; the input unchanged; a second run the same bytes"""
    typed = np.asarray(typed, dtype=NP[type_name])
    s = make_store(typed, status, type_name, default_is_nan)
    before = (raw(s.get_data()), raw(s.get_status()))
    wants = variance_reference_all(typed, status, lens, axis, type_name, default_is_nan, groups, n_groups)
    outs = run_all(s, lens, axis, groups, n_groups)
    for c in COMBOS:
        out, (want_v, want_s) = outs[c], wants[c]
        got_v, got_s = out.get_data(), out.get_status()
        where = (lens, axis, type_name, default_is_nan, c)
        assert out.size == want_v.size and out.type == type_name and out.default_is_nan == default_is_nan, where
        assert np.array_equal(got_s, want_s), (where, np.nonzero(got_s != want_s)[0][:8])
        if raw(got_v) != raw(want_v):
            bad = np.nonzero(got_v.view(np.uint8).reshape(want_v.size, -1) != want_v.view(np.uint8).reshape(want_v.size, -1))[0][:8]
            raise AssertionError((where, bad, got_v[bad], want_v[bad]))
    assert (raw(s.get_data()), raw(s.get_status())) == before  # the input is only read
    for c, again in run_all(s, lens, axis, groups, n_groups).items():
        assert raw(again.get_data()) == raw(outs[c].get_data()) and raw(again.get_status()) == raw(outs[c].get_status())
    return outs


def every_type_and_default(lens, axis=1, groups=None, n_groups=None, want_form=None, types=TYPES):
    for type_name in types:
        for default_is_nan in (False, True):
            if want_form is not None:
                assert choice(type_name, default_is_nan, lens, axis, groups, n_groups)[0] in want_form, (lens, type_name)
            typed, status = random_cells(lens, type_name, default_is_nan, seed=sum(lens) + len(type_name))
            check(lens, axis, type_name, default_is_nan, typed, status, groups, n_groups)


def expected_form(lens, type_name):
    """COLUMN_SHAPES / ROW_SHAPES / GROUP_SHAPES under the real tile"""
    inner = int(np.prod(lens[2:], dtype=np.int64))
    return COLUMN if inner >= 4 * (16 // NP[type_name]().itemsize) else ROW


def with_env(fn, **env):
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        fn()
    finally:
        for k in env:
            del os.environ[k]


# ---- forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", COLUMN_SHAPES + ROW_SHAPES)
def test_every_type_default_kind_and_ddof_on_the_tiled_forms(lens):
    for type_name in TYPES:
        assert choice(type_name, False, lens)[0] == expected_form(lens, type_name)
    every_type_and_default(lens)


@pytest.mark.parametrize("lens", GROUP_SHAPES)
def test_groups_of_1_2_3_31_64_and_65_members(lens):
    every_type_and_default(lens, groups=SIZED_GROUPS, want_form=(expected_form(lens, "float32"),))


@pytest.mark.parametrize("lens", [[2, 12, 16], [3, 12, 5], [7, 12]])
def test_interleaved_groups_group_ids_nobody_maps_to_and_as_many_groups_as_items(lens):
    every_type_and_default(lens, groups=np.arange(12) % 5)
    every_type_and_default(lens, groups=[0, 0, 2, 2, 3, 3, 0, 5, 5, 5, 2, 0], n_groups=8)
    every_type_and_default(lens, groups=np.arange(12)[::-1].copy())  # n_groups == K: one member each, 0 or unset
    every_type_and_default([12] + lens[2:] + [3], axis=0, groups=np.arange(12) % 5)  # along the first dimension


def test_each_axis_of_a_three_dimensional_cube():
    lens = [6, 5, 18]
    for axis in range(3):
        g = np.arange(lens[axis]) % 2
        every_type_and_default(lens, axis=axis, groups=g, types=("float64", "int32"))
        every_type_and_default(lens, axis=axis, types=("float32", "uint32"))


def direct_cases():
    for lens in AROUND_SMALL_TILE:
        every_type_and_default(lens, want_form=(ROW if lens[1] <= SMALL_TILE else DIRECT_LANES,))
    K = SMALL_TILE + 1
    # interleaved groups over a series beyond the tile: groups that fit a tile are staged member by member (the column form
    # with the whole row a slice), groups beyond it are read in place
    every_type_and_default([2, K], groups=np.arange(K) % 3, want_form=(COLUMN,))
    every_type_and_default([2, K, 3], groups=np.arange(K) // 9, want_form=(COLUMN,))
    every_type_and_default([2, 2 * K + 3], groups=np.arange(2 * K + 3) % 2, want_form=(DIRECT_LANES,))
    every_type_and_default([2, K, 16], groups=np.arange(K) % 2, want_form=(DIRECT_LANES,))  # groups of 33 rows of 16: beyond 64 cells
    every_type_and_default(DIRECT_LANES_SHAPE, want_form=(DIRECT_LANES,), types=("float32", "float64", "int32"))
    # the tiled forms with tiles this small: several group tiles per slice, several series tiles
    every_type_and_default([2, 30, 16], groups=np.arange(30) // 3, want_form=(COLUMN,))
    every_type_and_default([40, 7], want_form=(ROW,))


def test_the_direct_form_around_a_small_tile():
    with_env(direct_cases, OLAP_VARIANCE_TILE=SMALL_TILE)


@pytest.mark.parametrize("type_name,default_is_nan", [("float32", False), ("int32", True), ("float64", True)])
def test_series_around_the_real_tile_in_the_one_lane_forms(type_name, default_is_nan):
    def cases():
        tile = choice(type_name, default_is_nan, [3, 5])[1]
        assert tile == 32768 // (NP[type_name]().itemsize + (4 if has_mask(type_name, default_is_nan) else 0))
        for K in (tile - 1, tile, tile + 1, 2 * tile + 5):
            lens = [3, K]
            assert choice(type_name, default_is_nan, lens)[0] == (ROW if K <= tile else DIRECT_LANES)
            typed, status = random_cells(lens, type_name, default_is_nan, seed=K)
            check(lens, 1, type_name, default_is_nan, typed, status)
        for K, G, form in ((tile + 1, 3, COLUMN), (2 * tile + 5, 2, DIRECT_LANES)):  # interleaved groups that fit a tile, and that do not
            lens, groups = [2, K], np.arange(K) % G
            assert choice(type_name, default_is_nan, lens, 1, groups)[0] == form
            typed, status = random_cells(lens, type_name, default_is_nan, seed=5)
            check(lens, 1, type_name, default_is_nan, typed, status, groups)

    with_env(cases, OLAP_VARIANCE_BLOCK=NEVER)


def test_every_form_again_with_one_workgroup():
    """OLAP_VARIANCE_GRID (a developer knob) caps the workgroups of a launch: with one, a workgroup takes every tile and a
    lane every stride, as launches beyond the grid limit do"""
    def cases():
        for lens in ([2, 5, 17], [2, 3, 1030], [600, 7], [4, 6, 3]):
            every_type_and_default(lens)
        every_type_and_default(GROUP_SHAPES[0], groups=SIZED_GROUPS)
        with_env(direct_cases, OLAP_VARIANCE_TILE=SMALL_TILE)
        with_env(small_block_cases, OLAP_VARIANCE_BLOCK=100)

    with_env(cases, OLAP_VARIANCE_GRID=1)


# ---- the re-associated form: a workgroup per output cell --------------------------------------------------------------
def exact_everywhere(lens, axis, members, groups=None, types=TYPES):
    for type_name in types:
        for default_is_nan in (False, True):
            assert choice(type_name, default_is_nan, lens, axis, groups)[0] == DIRECT_BLOCK, (lens, type_name)
            typed, status = exact_cells(lens, axis, type_name, default_is_nan, len(type_name) + members, members, groups)
            outs = check(lens, axis, type_name, default_is_nan, typed, status, groups)
            if default_is_nan:
                assert outs[(0, 0)].get_status().all()  # every output cell has its members


def small_block_cases():
    """under OLAP_VARIANCE_BLOCK=100: groups of 133 items with exactly 128 set (lanes of the workgroup without a member),
    of 300 with 256, interleaved groups, a strided series"""
    exact_everywhere([3, 133], 1, 128)
    exact_everywhere([2, 300], 1, 256, types=("float32", "int32"))
    exact_everywhere([2, 600], 1, 256, groups=np.arange(600) % 2, types=("float64", "uint32"))
    exact_everywhere([520, 3], 0, 512, types=("float32", "float64"))


def test_the_workgroup_form_on_small_cubes_is_exact_on_exact_data():
    with_env(small_block_cases, OLAP_VARIANCE_BLOCK=100)


def test_the_workgroup_form_at_the_real_cut_is_exact_with_4096_set_members():
    assert choice("float64", False, BLOCK_SHAPE)[0] == DIRECT_BLOCK
    exact_everywhere(BLOCK_SHAPE, 1, 4096)
    exact_everywhere([2, 9000], 1, 4096, groups=np.arange(9000) % 2, types=("float64", "int32"))


def test_the_workgroup_form_on_uniform_float64_within_the_two_pass_bound():
    N, u = BLOCK_SHAPE[1], 2.0 ** -53
    rng = np.random.default_rng(N)
    typed = (rng.random(BLOCK_SHAPE) + 1.0).ravel()
    for default_is_nan in (False, True):
        assert choice("float64", default_is_nan, BLOCK_SHAPE)[0] == DIRECT_BLOCK
        s = make_store(typed, None, "float64", default_is_nan)
        before = raw(s.get_data())
        outs, again = run_all(s, BLOCK_SHAPE, 1, None, None), run_all(s, BLOCK_SHAPE, 1, None, None)
        wants = variance_reference_all(typed, None, BLOCK_SHAPE, 1, "float64", default_is_nan)
        for o in range(BLOCK_SHAPE[0]):
            n, mean, m2 = moments_of(typed.reshape(BLOCK_SHAPE)[o])
            tol = 4.0 * (n * u + n * n * (1.0 + mean * mean / (m2 / n)) * u * u)
            assert n == N and 1e-12 < tol < 4e-12
            for c in COMBOS:
                got, want = float(outs[c].get_data()[o]), float(wants[c][0][o])
                print("output cell %d kind %d ddof %d: relative difference %.3g (allowed %.3g)" % (o, c[0], c[1], abs(got - want) / want, tol))
                assert outs[c].get_status()[o] == 2 and abs(got - want) <= tol * want, (o, c, got, want)
        for c in COMBOS:
            assert raw(again[c].get_data()) == raw(outs[c].get_data())  # fixed by the plan, not by timing
        assert raw(s.get_data()) == before


# ---- values where a wrong implementation shows ----------------------------------------------------------------------
def series(type_name, default_is_nan, kind, ddof, values, lens=None, axis=0, status=None):
    values = np.asarray(values, dtype=NP[type_name])
    out = check(lens or [values.size], axis, type_name, default_is_nan, values, status)[(kind, ddof)]
    return out.get_data(), out.get_status()


EIGHT = [2, 4, 4, 4, 5, 5, 7, 9]


def test_hand_worked_literals_in_every_layout():
    for type_name in TYPES:
        assert series(type_name, False, 0, 0, EIGHT)[0].tolist() == [4]
        assert series(type_name, False, 1, 0, EIGHT)[0].tolist() == [2]
    assert series("float64", False, 0, 1, EIGHT)[0].tolist() == [32 / 7]
    assert series("float64", True, 1, 1, EIGHT)[0].tolist() == [math.sqrt(32 / 7)]
    assert series("float64", False, 0, 1, np.repeat(EIGHT, 8), lens=[8, 8])[0].tolist() == [32 / 7] * 8  # the column form
    assert series("float32", False, 0, 1, np.tile(EIGHT, 5), lens=[5, 8], axis=1)[0].tolist() == [np.float32(32 / 7)] * 5


def test_a_large_common_offset_and_float32_members_whose_float32_sum_would_round():
    for lens, axis, values in (([8], 0, 1e9 + np.arange(8.0)), ([8, 16], 0, np.repeat(1e9 + np.arange(8.0), 16)), ([5, 8], 1, np.tile(1e9 + np.arange(8.0), 5))):
        assert set(series("float64", False, 0, 0, values, lens, axis)[0].tolist()) == {5.25}  # E[x^2] - mean^2: 0 or garbage
        assert set(series("float64", True, 0, 1, values, lens, axis)[0].tolist()) == {6.0}
    members = [16777216.0, 16777218.0, 16777220.0, 16777222.0]  # their sum, 2^26 + 12, is no float32: a float32 accumulator misses the mean 16777219
    assert series("float32", False, 0, 0, members)[0].tolist() == [5.0]
    assert series("float32", True, 0, 1, np.repeat(members, 16), lens=[4, 16])[0].tolist() == [np.float32(20 / 3)] * 16


def test_special_floats():
    inf = np.inf
    for type_name in ("float32", "float64"):
        for kind in (0, 1):
            for members in ([inf, 1, 2], [-inf, 1, 2], [inf, -inf], [1, np.nan, 2], [1, -np.nan, 2]):
                v, s = series(type_name, False, kind, 0, members)  # a set NaN under a 0 default
                assert s.tolist() == [2] and np.isnan(v[0])
            v, s = series(type_name, True, kind, 1, [inf, 1, 2])  # NaN is the default: unset
            assert s.tolist() == [0] and np.isnan(v[0])
        v, s = series(type_name, True, 0, 0, [1, np.nan, 2])  # a NaN cell under the NaN default is no member
        assert v.tolist() == [0.25] and s.tolist() == [2]
        v, s = series(type_name, True, 0, 0, [-0.0, -0.0, 0.0])  # members under a NaN default: a SET +0
        assert v.tolist() == [0.0] and not np.signbit(v[0]) and s.tolist() == [2]
        v, s = series(type_name, False, 0, 0, [-0.0, 0.0, -0.0])  # all equal to the 0 default: no member
        assert s.tolist() == [0]
        v, s = series(type_name, True, 1, 0, [-0.0, 3.0, -0.0, 3.0])
        assert v.tolist() == [1.5]
    assert series("float64", False, 0, 0, [1e200, -1e200])[0].tolist() == [inf]


def test_integer_cells_convert_once():
    assert series("int32", False, 0, 0, [1, 2])[1].tolist() == [0]  # 0.25 truncates to the default: unset
    assert series("int32", True, 0, 0, [1, 2], status=np.array([2, 2], np.int32))[1].tolist() == [2]  # a SET 0 under the NaN default
    assert series("int32", False, 1, 1, [-5, 5])[0].tolist() == [7]  # sqrt(50)
    assert series("int32", False, 0, 0, [-5, -7, -9])[0].tolist() == [2]  # 8 / 3
    assert series("uint32", False, 0, 0, [2 ** 32 - 1, 2 ** 32 - 5])[0].tolist() == [4]
    v, s = series("uint32", False, 1, 0, [2 ** 31 + 5, 2 ** 32 - 1, 1])  # the members stay unsigned: a stddev of about 1.75e9
    assert 1.7e9 < v[0] < 1.8e9 and s.tolist() == [2]
    series("int32", False, 0, 0, [-(2 ** 31), 2 ** 31 - 1])  # 2^62: wraps as the typed conversion wraps (against the restatement)


def test_all_unset_and_single_members():
    for type_name in TYPES:
        for default_is_nan in (False, True):
            lens = [3, 6, 4]
            typed, status = random_cells(lens, type_name, default_is_nan, seed=1, unset=1.0)
            outs = check(lens, 1, type_name, default_is_nan, typed, status)
            assert not any(out.get_status().any() for out in outs.values())
            typed, status = random_cells(lens, type_name, default_is_nan, seed=2, unset=0.85)
            outs = check(lens, 1, type_name, default_is_nan, typed, status, [0, 1, 0, 1, 2, 2])
            # one member: variance 0 — unset under the 0 default, a SET 0 under the NaN default — and unset with ddof 1
            typed, status = random_cells([4, 1, 5], type_name, True, seed=3, unset=0.0)
            if status is None:
                typed[np.isnan(typed)] = 1
            outs = check([4, 1, 5], 1, type_name, True, typed, status)
            assert outs[(0, 0)].get_status().tolist() == [2] * 20 and not outs[(0, 0)].get_data().any()
            assert not outs[(0, 1)].get_status().any() and not outs[(1, 1)].get_status().any()


# ---- batches, tracked stores --------------------------------------------------------------------------------------------
def test_nine_measures_of_mixed_types_and_defaults():
    lens = [4, 9, 6]
    kinds = [("float32", False)] * 9
    inputs = [random_cells(lens, t, d, seed=100 + i) for i, (t, d) in enumerate(kinds)]
    stores = [make_store(v, st, t, d) for (v, st), (t, d) in zip(inputs, kinds)]
    groups = [0, 0, 0, 1, 1, 2, 2, 2, 2]
    outs, launches = pkg.HipStore.variance_multi(stores, lens, 1, 0, 1, groups)
    assert launches == 2  # nine of one kind: 8 + 1
    kinds = [("float32", False), ("int32", True), ("float32", False), ("float64", True), ("uint32", False), ("int32", True), ("float32", True),
             ("float64", True), ("int32", False)]
    inputs = [random_cells(lens, t, d, seed=200 + i) for i, (t, d) in enumerate(kinds)]
    stores = [make_store(v, st, t, d) for (v, st), (t, d) in zip(inputs, kinds)]
    outs, launches = pkg.HipStore.variance_multi(stores, lens, 1, 1, 1, groups)
    assert launches == len(set(kinds)) == 6
    for (v, st), (t, d), out in zip(inputs, kinds, outs):
        want_v, want_s = variance_reference(v, st, lens, 1, 1, 1, t, d, groups)
        assert out.type == t and out.default_is_nan == d and out.size == 4 * 3 * 6
        assert raw(out.get_data()) == raw(want_v) and np.array_equal(out.get_status(), want_s), (t, d)
    outs, launches = pkg.HipStore.variance_multi([], lens, 1)
    assert outs == [] and launches == 0


def test_a_dimension_without_items_gives_unset_cells():
    s = pkg.HipStore(0, "float32", 0.0)
    outs, launches = pkg.HipStore.variance_multi([s], [3, 0, 2], 1)
    assert outs[0].size == 6 and not outs[0].get_status().any() and not outs[0].get_data().any()
    outs, launches = pkg.HipStore.variance_multi([s], [3, 0, 2], 0)  # no output cell: nothing to launch
    assert launches == 0 and outs[0].size == 0

    def column_form_without_rows():  # a tile below one slot: slices of one cell
        assert choice("float32", False, [3, 0, 64])[::4] == (COLUMN, 1)
        outs, launches = pkg.HipStore.variance_multi([s], [3, 0, 64], 1, 1, 0)
        assert launches == 1 and outs[0].size == 192 and not outs[0].get_status().any() and not outs[0].get_data().any()

    with_env(column_form_without_rows, OLAP_VARIANCE_TILE=1)


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
    a, b = plain.variance(lens, 1, 1, 1, groups), tracked.variance(lens, 1, 1, 1, groups)  # item order, not insertion order
    assert tracked.order_tracked and not b.order_tracked
    assert raw(a.get_data()) == raw(b.get_data()) and raw(a.get_status()) == raw(b.get_status())
    outs, launches = pkg.HipStore.variance_multi([plain, tracked], lens, 1, 1, 1, groups)
    assert launches == 1 and raw(outs[1].get_data()) == raw(a.get_data())


def test_kind_and_ddof_outside_0_1_are_refused():
    s = pkg.HipStore(6, "float32", 0.0)
    for kind, ddof, message in ((2, 0, "variance: kind must be 0 or 1 (got 2)"), (-1, 0, "variance: kind must be 0 or 1 (got -1)"),
                                (0, 2, "variance: ddof must be 0 or 1 (got 2)"), (1, -1, "variance: ddof must be 0 or 1 (got -1)"),
                                (3, 3, "variance: kind must be 0 or 1 (got 3)")):
        with pytest.raises(pkg.capi.OlapError) as e:
            s.variance([2, 3], 1, kind, ddof)
        assert e.value.code == pkg.capi.ERR_INVALID_ARGUMENT and message in str(e.value)
