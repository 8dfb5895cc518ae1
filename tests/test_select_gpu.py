"""olap_store_select_total / olap_store_copy_select (getTotalForDimensionItems, copyMeasureData: src/cube.js:679-707,
:859-888) through the Python store API.  The total must equal, bit for bit, the left-to-right float64 sum of getValue
over the combinations in nesting order; the copy must equal a per-cell set_value(get_value) loop on a clone."""
import itertools
import math
import struct

import numpy as np
import pytest

from conftest import load_package

pytestmark = pytest.mark.gpu

pkg = load_package()
DTYPES = ["int32", "uint32", "float32", "float64"]


def bits(x):
    return struct.pack("<d", x) if x == x else b"nan"


def get_values(store):
    """getValue of every cell (the default where unset)"""
    data, st = store.get_data_f64(), store.get_status()
    default = float("nan") if store.default_is_nan else 0.0
    return np.where((st & 2) != 0, data, default)


def combos(lens, levels):
    """flat positions (or None: a cell that does not exist) of every combination, in nesting order"""
    strides = [int(np.prod(lens[d + 1:])) for d in range(len(lens))]
    for digits in itertools.product(*[list(e) for _, e in levels]):
        pos = 0
        for (axis, _), e in zip(levels, digits):
            if axis < 0:
                continue
            if e < 0:
                pos = None
                break
            pos += e * strides[axis]
        yield pos


def sequential_total(values, default, lens, levels):
    acc = 0.0
    for pos in combos(lens, levels):
        acc += default if pos is None else float(values[pos])  # Python float addition is IEEE float64
    return acc


def random_cube(rng, dtype, nan_default, ndim=None):
    ndim = ndim or int(rng.integers(1, 6))
    lens = [int(rng.choice([1, 3, 5, 7])) for _ in range(ndim)]
    n = int(np.prod(lens))
    vals = rng.integers(-40, 40, size=n).astype(np.float64)
    if dtype == "uint32":
        vals = np.abs(vals)
    if dtype in ("float32", "float64"):
        vals = vals * 0.25
    vals[rng.random(n) < 0.4] = 0.0  # sparse: unset under a 0 default
    if nan_default:
        vals[rng.random(n) < 0.3] = np.nan
    s = pkg.HipStore(n, dtype, float("nan") if nan_default else 0.0)
    s.set_data_f64(vals)
    return s, lens


def random_levels(rng, lens, allow_missing=True, allow_free=True):
    order = list(rng.permutation(len(lens)))
    levels = []
    for d in order:
        k = int(rng.integers(0, lens[d] + 3)) if rng.random() < 0.9 else 0
        if rng.random() < 0.35:
            e = list(range(lens[d]))  # the whole dimension in order (folds into the contiguous run)
        else:
            e = [int(x) for x in rng.integers(0, lens[d], size=k)]
            if allow_missing and e and rng.random() < 0.3:
                e[int(rng.integers(0, len(e)))] = -1
        levels.append((int(d), e))
    if allow_free and rng.random() < 0.4:
        levels.insert(int(rng.integers(0, len(levels) + 1)), (-1, [0] * int(rng.integers(0, 4))))
    return levels


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nan_default", [False, True])
def test_select_total_matches_sequential_sum(dtype, nan_default):
    rng = np.random.default_rng(11 + DTYPES.index(dtype) * 2 + int(nan_default))
    for trial in range(40):
        s, lens = random_cube(rng, dtype, nan_default)
        values = get_values(s)
        default = float("nan") if nan_default else 0.0
        levels = random_levels(rng, lens)
        got, path = s.select_total(lens, levels)
        want = sequential_total(values, default, lens, levels)
        assert bits(got) == bits(want), (trial, lens, levels, got, want)
        assert path == "device", (trial, levels)  # ordinary (small-integer / quarter) data is certified


def test_select_total_long_runs_and_permuted_rows():
    """row mode (runs >= 1024 cells, 16-byte loads) with gathered outer levels, against the sequential sum"""
    rng = np.random.default_rng(5)
    for dtype in DTYPES:
        lens = [5, 3, 1031]
        n = int(np.prod(lens))
        vals = rng.integers(0, 9, size=n).astype(np.float64)
        s = pkg.HipStore(n, dtype, 0.0)
        s.set_data_f64(vals)
        for levels in ([(1, [2, 0, 2]), (0, [4, 1]), (2, list(range(1031)))], [(0, [0, 1, 2, 3, 4]), (1, [0, 1, 2]), (2, list(range(1031)))],
                       [(2, list(range(1031))), (-1, [0, 0]), (0, [3, -1]), (1, [1])]):
            got, path = s.select_total(lens, levels)
            assert got == sequential_total(vals, 0.0, lens, levels) and path == "device", (dtype, levels)


@pytest.mark.parametrize("terms, want", [([2.0 ** 53, 1.0, -(2.0 ** 53)], 0.0), ([1e16, 1.0, -1e16], 0.0),
                                         ([1e308, 1e308, -math.inf], float("nan")), ([3.0, 1e308, 1e308, -1e308], math.inf)])
def test_sequential_path_for_order_dependent_sums(terms, want):
    s = pkg.HipStore(len(terms), "float64", 0.0)
    s.set_data_f64(np.array(terms))
    got, path = s.select_total([len(terms)], [(0, list(range(len(terms))))])
    assert path == "sequential"
    assert bits(got) == bits(want) == bits(sequential_total(np.array(terms), 0.0, [len(terms)], [(0, list(range(len(terms))))]))
    # the reversed nesting order is another left-to-right sum
    rev = [(0, list(range(len(terms)))[::-1])]
    got, path = s.select_total([len(terms)], rev)
    assert bits(got) == bits(sequential_total(np.array(terms), 0.0, [len(terms)], rev))


@pytest.mark.parametrize("terms", [[math.inf, 1.0, -math.inf], [math.inf, 2.0, 3.0], [-math.inf, -5.0], [-0.0, -0.0], [float("nan"), 1.0],
                                   [0.5, -0.5]])
def test_non_finite_and_signed_zero_terms(terms):
    s = pkg.HipStore(len(terms), "float64", float("nan"))
    s.set_data_f64(np.array(terms))
    levels = [(0, list(range(len(terms)))), (-1, [0, 0, 0])]
    got, path = s.select_total([len(terms)], levels)
    assert bits(got) == bits(sequential_total(get_values(s), float("nan"), [len(terms)], levels))
    assert path == "device"


def test_unset_cells_of_a_nan_default_and_missing_cells():
    s = pkg.HipStore(6, "float32", float("nan"))
    s.set_value(1, 2.5)
    got, path = s.select_total([2, 3], [(0, [0]), (1, [1])])
    assert got == 2.5 and path == "device"
    got, _ = s.select_total([2, 3], [(0, [0]), (1, [1, 2])])
    assert math.isnan(got)
    z = pkg.HipStore(6, "int32", 0.0)
    z.set_value(4, 7)
    assert z.select_total([2, 3], [(1, [1, -1, 1]), (0, [1, -1])]) == (14.0, "device")
    assert z.select_total([2, 3], [(0, []), (1, [1])]) == (0.0, "device")
    assert z.select_total([2, 3], [(0, [1]), (-1, []), (1, [1])]) == (0.0, "device")


def test_argument_errors():
    s = pkg.HipStore(6, "float32", 0.0)
    with pytest.raises(pkg.OlapError, match="has no level"):
        s.select_total([2, 3], [(0, [0]), (-1, [0])])
    with pytest.raises(pkg.OlapError, match="two levels"):
        s.select_total([2, 3], [(0, [0]), (1, [0]), (0, [1])])
    with pytest.raises(pkg.OlapError, match="outside dimension"):
        s.select_total([2, 3], [(0, [2]), (1, [0])])
    with pytest.raises(pkg.OlapError, match="outside dimension"):
        s.clone().copy_select(s, [2, 3], [(0, [-1]), (1, [0])])
    with pytest.raises(pkg.OlapError):
        s.select_total([2, 2], [(0, [0]), (1, [0])])


def per_cell_copy(target, source, lens, levels):
    for pos in combos(lens, levels):
        v, _ = source.get_value(pos)
        target.set_value(pos, v)


def assert_same_store(a, b):
    assert np.array_equal(a.get_status(), b.get_status())
    assert np.array_equal(a.get_data_f64(), b.get_data_f64(), equal_nan=True)
    assert np.array_equal(a.keys(), b.keys())
    ia, va = a.to_sparse()
    ib, vb = b.to_sparse()
    assert ia.tobytes() == ib.tobytes() and va.tobytes() == vb.tobytes()


def test_copy_select_matches_per_cell_loop():
    rng = np.random.default_rng(3)
    for trial in range(48):
        src_type, dst_type = DTYPES[trial % 4], DTYPES[(trial // 4) % 4]
        src, lens = random_cube(rng, src_type, bool(rng.integers(0, 2)), ndim=int(rng.integers(1, 5)))
        n = int(np.prod(lens))
        dst_nan = bool(rng.integers(0, 2))
        dst = pkg.HipStore(n, dst_type, float("nan") if dst_nan else 0.0)
        dst.set_data_f64(np.where(rng.random(n) < 0.5, rng.integers(1, 9, size=n).astype(np.float64), 0.0))
        tracked = trial % 3
        if tracked:
            dst.track_order()
            if tracked == 2:  # an order that is already explicit
                for i in rng.permutation(n)[: max(1, n // 3)]:
                    dst.set_value(int(i), float(rng.integers(1, 5)))
        levels = random_levels(rng, lens, allow_missing=False)
        want = dst.clone()
        per_cell_copy(want, src, lens, levels)
        dst.copy_select(src, lens, levels)
        assert_same_store(dst, want)


def test_copy_select_onto_itself_and_empty_selection():
    s = pkg.HipStore(12, "float32", 0.0)
    s.set_data_f64(np.arange(12.0))
    before = s.get_data_f64().copy()
    s.copy_select(s, [3, 4], [(1, [3, 0]), (0, [2, 1, 2])])
    assert np.array_equal(s.get_data_f64(), before)
    s.copy_select(pkg.HipStore(12, "float32", 0.0), [3, 4], [(0, []), (1, [0])])
    assert np.array_equal(s.get_data_f64(), before)


def test_sharded_select_total_and_copy():
    from olap_in_memory_amd.sharded import Comm, ShardedStore

    comm = Comm.init_all([0, 0])
    rng = np.random.default_rng(9)
    lens = [7, 5, 3]
    n = int(np.prod(lens))
    for dtype in DTYPES:
        vals = rng.integers(0, 6, size=n).astype(np.float64)
        sh = ShardedStore(comm, lens, dtype, 0.0).set_data_f64(vals)
        whole = pkg.HipStore(n, dtype, 0.0)
        whole.set_data_f64(vals)
        for _ in range(10):
            levels = random_levels(rng, lens)
            got, path = sh.select_total(levels)
            assert bits(got) == bits(whole.select_total(lens, levels)[0]) and path == "device"
        src = ShardedStore(comm, lens, dtype, 0.0).set_data_f64(rng.integers(0, 4, size=n).astype(np.float64))
        levels = random_levels(rng, lens, allow_missing=False)
        want = sh.gather()
        per_cell_copy(want, src.gather(), lens, levels)
        sh.copy_select(src, levels)
        assert np.array_equal(sh.get_data_f64(), want.get_data_f64())
    # a total only the sequential order can give: the whole measure is needed
    sh = ShardedStore(comm, [3], "float64", 0.0).set_data_f64(np.array([2.0 ** 53, 1.0, -(2.0 ** 53)]))
    with pytest.raises(pkg.OlapError, match="^sharded:"):
        sh.select_total([(0, [0, 1, 2])])


def test_hundred_million_cells_take_the_device_path():
    lens = [100, 1000, 1000]
    s = pkg.HipStore(10 ** 8, "float32", 0.0)
    s.fill(3.0)
    got, path = s.select_total(lens, [(0, list(range(100))), (1, list(range(1000))), (2, list(range(1000)))])
    assert path == "device" and got == s.total == 3.0e8
    got, path = s.select_total(lens, [(2, [999]), (0, list(range(100))), (1, list(range(1000)))])
    assert path == "device" and got == 3.0e5
