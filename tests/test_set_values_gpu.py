"""olap_store_set_values / olap_sharded_store_set_values (n setValue calls in one, in-memory.js:122-133) against the same
entries written one set_value at a time on a clone: the values bit for bit, the status mask, the key order of a tracked
store and whether that order is still the lazy ascending one."""
import zlib

import numpy as np
import pytest

from conftest import load_package

pytestmark = pytest.mark.gpu

pkg = load_package()
DTYPES = ["int32", "uint32", "float32", "float64"]


def assert_same_store(a, b):
    assert a.get_data().tobytes() == b.get_data().tobytes()
    assert np.array_equal(a.get_status(), b.get_status())
    assert np.array_equal(a.keys(), b.keys())
    assert a.order_tracked == b.order_tracked


def special_values(default):
    """values whose conversion or place is delicate: NaN, signed zeros, the default, Float32 underflow to 0, integers
    outside the 32-bit ranges, fractions"""
    return [float("nan"), 0.0, -0.0, default, 1e-50, -1e-50, 3e9, -3e9, 2.0 ** 40, 4294967296.0, -1.0, 0.5, -2.75, 1e300, None]


def random_entries(rng, size, n, default):
    specials = special_values(default)
    idx = rng.integers(0, size, size=n)
    if n > 8:  # a few cells written many times: set -> null -> set chains and repeated defaults
        hot = rng.integers(0, size, size=max(1, n // 16))
        pick = rng.random(n) < 0.3
        idx[pick] = rng.choice(hot, size=int(pick.sum()))
    values = []
    for _ in range(n):
        r = rng.random()
        if r < 0.15:
            values.append(None)
        elif r < 0.35:
            values.append(specials[int(rng.integers(0, len(specials)))])
        else:
            values.append(float(rng.integers(-50, 50)) * (0.25 if rng.random() < 0.5 else 1.0))
    return [int(i) for i in idx], values


def make_store(rng, size, dtype, default, form):
    """form: "plain" (untracked), "lazy" (tracked, still ascending), "seq" (tracked, explicit order after a reorder)"""
    s = pkg.HipStore(size, dtype, default)
    data = np.where(rng.random(size) < 0.4, rng.integers(1, 9, size=size).astype(np.float64), default)
    if form == "seq":
        s.track_order()
        s.set_data_f64(data)
        t = s.reorder([size // 4, 4], [1, 0])
        assert t.order_tracked == 2
        return t
    if form == "lazy":
        s.track_order()
    s.set_data_f64(data)
    if form == "lazy":
        assert s.order_tracked == 1
    return s


def check_batch(store, indexes, values):
    want = store.clone()
    for i, v in zip(indexes, values):
        want.set_value(i, v)
    store.set_values(indexes, values)
    assert_same_store(store, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("default", [0.0, float("nan")])
@pytest.mark.parametrize("form", ["plain", "lazy", "seq"])
def test_random_batches_match_sequential_set_value(dtype, default, form):
    rng = np.random.default_rng(zlib.crc32(("%s %s %s" % (dtype, default, form)).encode()))
    for n in (1, 2, 7, 300):
        size = 64 if n < 300 else 400
        store = make_store(rng, size, dtype, default, form)
        check_batch(store, *random_entries(rng, size, n, default))
        check_batch(store, *random_entries(rng, size, n, default))  # a second batch over the first one's result


def test_set_null_set_chains_take_the_place_of_the_last_revival():
    s = pkg.HipStore(8, "float32", 0.0).track_order()
    s.set_values([5, 2, 6], [1.0, 2.0, 3.0])
    # 2 stays set (keeps its place); 5 is unset then set again (appended at its revival); 6 is set to a Float32 zero
    # (deleted) and set again; 1 is set, nulled, set twice (appended at the first set after the null)
    idx = [2, 5, 1, 5, 1, 6, 1, 5, 1, 6, 2]
    vals = [7.0, None, 4.0, 0.0, None, 1e-50, 8.0, 9.0, 10.0, 11.0, 12.0]
    want = s.clone()
    for i, v in zip(idx, vals):
        want.set_value(i, v)
    s.set_values(idx, vals)
    assert_same_store(s, want)
    assert list(s.keys()) == [2, 1, 5, 6]


@pytest.mark.parametrize("dtype", DTYPES)
def test_ascending_hydration_of_a_tracked_store_stays_lazy(dtype):
    s = pkg.HipStore(1000, dtype, float("nan")).track_order()
    check_batch(s, list(range(3, 1000, 7)), [float(i % 5) for i in range(3, 1000, 7)])
    assert s.order_tracked == 1
    check_batch(s, [998, 999], [None, 1.0])  # above every key: still ascending
    assert s.order_tracked == 1
    check_batch(s, [500, 10], [1.0, 2.0])  # below a key: the order becomes explicit, as it would per cell
    assert s.order_tracked == 2


@pytest.mark.parametrize("dtype,form", [("float32", "seq"), ("int32", "plain"), ("float64", "lazy")])
def test_many_workgroups(dtype, form):
    rng = np.random.default_rng(11)
    size = 1 << 18
    n = 200_000
    store = make_store(rng, size, dtype, float("nan") if dtype == "float64" else 0.0, form)
    check_batch(store, *random_entries(rng, size, n, 0.0))


def test_numpy_entries_without_nulls():
    s = pkg.HipStore(100, "float64", 0.0)
    want = s.clone()
    idx = np.arange(99, -1, -3, dtype=np.uint64)
    vals = np.linspace(-2.0, 2.0, len(idx))
    for i, v in zip(idx, vals):
        want.set_value(int(i), float(v))
    s.set_values(idx, vals)
    assert_same_store(s, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_shards_on_one_device(dtype):
    from olap_in_memory_amd.sharded import Comm, ShardedStore

    comm = Comm.init_all([0, 0])
    rng = np.random.default_rng(5)
    lens = [7, 5, 3]
    size = int(np.prod(lens))
    for default in (0.0, float("nan")):
        data = np.where(rng.random(size) < 0.5, rng.integers(1, 9, size=size).astype(np.float64), default)
        got = ShardedStore(comm, lens, dtype, default).set_data_f64(data)
        want = ShardedStore(comm, lens, dtype, default).set_data_f64(data)
        for n in (1, 40, 500):
            idx, vals = random_entries(rng, size, n, default)
            got.set_values(idx, vals)
            for i, v in zip(idx, vals):
                want.set_value(i, v)
            assert got.gather().get_data().tobytes() == want.gather().get_data().tobytes()
            assert np.array_equal(got.get_status(), want.get_status())
        before = got.gather().get_data().tobytes()
        with pytest.raises(pkg.OlapError, match=r"entry 1: cell index 105 out of bounds"):
            got.set_values([0, size], [1.0, 2.0])
        assert got.gather().get_data().tobytes() == before


def last_writes(idx, vals, size):
    """the numpy last-write-wins model: (value of each cell's last entry, or NaN where none; whether it has one)"""
    last_pos = np.full(size, -1, dtype=np.int64)
    np.maximum.at(last_pos, np.asarray(idx, dtype=np.int64), np.arange(len(idx), dtype=np.int64))
    has = last_pos >= 0
    return np.where(has, np.asarray(vals)[np.maximum(last_pos, 0)], np.nan), has


def test_batches_compose_across_the_2_26_split():
    """2^26 + 2^12 entries are written as two batches: the second must see the first one's result, as the sequential
    setValue calls would (numpy entries, a plain Float32 store with a 0 default: a cell ends set exactly when its last
    value is non-zero)"""
    size = 1 << 20
    split = 1 << 26
    k = 1 << 12
    n = split + k
    rng = np.random.default_rng(26)
    idx = rng.integers(0, size, size=n).astype(np.uint64)
    vals = rng.integers(-3, 4, size=n).astype(np.float64)
    # the tail revisits cells the first batch leaves set and cells it leaves unset: it unsets, overwrites and sets them
    before, _ = last_writes(idx[:split], vals[:split], size)
    picks = np.concatenate([rng.choice(np.nonzero(before != 0)[0], size=k // 2), rng.choice(np.nonzero(before == 0)[0], size=k // 2)])
    idx[split:] = picks.astype(np.uint64)
    vals[split:] = np.where(rng.random(k) < 0.3, 0.0, rng.integers(5, 9, size=k).astype(np.float64))
    last, has = last_writes(idx, vals, size)
    assert has.all()
    assert np.any((before[picks] != 0) & (last[picks] == 0)) and np.any((before[picks] == 0) & (last[picks] != 0))
    assert np.any((before[picks] != 0) & (last[picks] != 0) & (last[picks] != before[picks]))
    s = pkg.HipStore(size, "float32", 0.0)
    s.set_values(idx, vals)
    assert np.array_equal((s.get_status() & 2) != 0, last != 0)
    assert np.array_equal(s.get_data(), last.astype(np.float32))


def test_set_values_beyond_2_32_cells():
    """a 5x10^9-cell Float32 store (20 GB): the sort runs on 33 key bits; the written cells are read back one by one, and
    a filtered total over rows that straddle cell 2^32 is the exact sum of the generator's values"""
    from fractions import Fraction

    from select_reference import mulberry_cell_values

    shape = [5000, 1000, 1000]
    n = int(np.prod(shape))
    s = pkg.HipStore(n, "float32", 0.0)
    pkg.capi.check(pkg.lib().olap_fill_seeded(s.values_ptr, None, n, 0, 2, 20240807, 1.0, None))
    two32 = 1 << 32
    idx = [two32 + 1, two32 - 1, two32, n - 1, two32, two32 + 1, 7, two32 - 1, two32 + 1]
    vals = [3.0, 5.0, 0.0, 11.0, 6.0, None, 2.5, 9.0, 4.0]
    s.set_values(idx, vals)
    want = {two32 - 1: 9.0, two32: 6.0, two32 + 1: 4.0, n - 1: 11.0, 7: 2.5}
    for cell, v in want.items():
        assert s.get_value(cell) == (v, True), cell
    assert s.get_value(two32 + 2) == (float(mulberry_cell_values([two32 + 2])[0]), True)
    # rows 4 294 and 4 293 (cell 2^32 is row 4 294, column 967 296), ROW mode; then three cells around 2^32, FLAT mode
    r0 = two32 // 1_000_000
    cells = np.concatenate([np.arange(r0 * 10 ** 6, (r0 + 1) * 10 ** 6), np.arange((r0 - 1) * 10 ** 6, r0 * 10 ** 6)]).astype(np.uint64)
    terms = mulberry_cell_values(cells).astype(np.float64)
    for cell, v in want.items():
        terms[cells == cell] = v
    scaled = terms * 2 ** 24  # Float32 values in [0.5, 1.5) and small integers: multiples of 2^-24
    assert np.array_equal(scaled, np.floor(scaled))
    exact = Fraction(int(scaled.astype(np.int64).sum()), 2 ** 24)
    got, path = s.select_total(shape, [(0, [r0, r0 - 1]), (1, list(range(1000))), (2, list(range(1000)))])
    assert path == "device" and got == float(exact)
    i1, i2 = (two32 % 10 ** 6) // 1000, two32 % 1000
    got, path = s.select_total(shape, [(2, [i2 + 1, i2, i2 - 1]), (0, [r0]), (1, [i1])])
    assert path == "device" and got == 4.0 + 6.0 + 9.0
    del s
