"""olap_store_compose_multi: the measures of one source cube on the dimensions of a composed cube in one pass per group of
up to 8 — bit for bit (values and mask) what olap_store_create [+ olap_store_fill] + olap_store_load leave on the device,
and what the oracle's create [+ fill] + load give.  The sources share their type with the new stores, so every case here
is a same-type case and is compared with both (check() names the two places where only one of them applies).  The
64-bit index instantiations need a store of 2^32 cells and are not reached here."""
import numpy as np
import pytest

from conftest import load_package
from golden_util import same_typed
from oracle.oracle import OracleStore

pytestmark = pytest.mark.gpu

pkg = load_package()
NAN = float("nan")
LANES = "compose_gather (16-byte lanes)"
CELLS = "compose_gather (16-byte runs of this store)"


def ident(n):
    return np.arange(n, dtype=np.int32)


# name -> (my lengths, his lengths, his item -> my item per dimension, the form the plan takes)
SHAPES = {
    # the two inner dimensions left alone: 96 cells in a row, whole 16-byte lanes for every cell type
    "lanes": ([6, 8, 12], [4, 8, 12], [[4, -1, 0, 2], ident(8), ident(12)], LANES),
    # every dimension remapped, items of his that I lack, items of mine that he lacks
    "remapped": ([4, 10], [6, 10], [[3, -1, 0, 2, -1, 1], [9, 3, 0, 7, 1, 8, 2, 6, 4, 5]], CELLS),
    # 35 cells: a ragged tail in the last lane, rows that end inside a lane
    "ragged": ([5, 7], [5, 7], [ident(5), [3, 0, 6, 1, 5, 2, 4]], CELLS),
    "one dimension": ([3], [2], [[2, 0]], CELLS),
    # maps that name an item of mine more than once: the last of his items wins, in every dimension
    "twice, both dimensions": ([3, 4], [4, 4], [[0, 2, 0, 1], [1, 1, 3, 0]], CELLS),
    "three times": ([2, 3], [3, 5], [[1, 1, 1], [2, -1, 2, 0, 0]], CELLS),
}
TYPES = ["float32", "float64", "int32", "uint32"]
DEFAULTS = [0.0, NAN]
FILLS = [None, 7.0, 2.5, 0.0, NAN]  # 2.5 into integer cells is 2; 0 under a 0 default and NaN under a NaN default are dropped


def cells(rng, n, default):
    """n cells of which about 40 % are unset, the set ones distinct enough to tell which cell of his arrived"""
    return np.where(rng.random(n) < 0.4, default, rng.integers(1, 1000, size=n).astype(np.float64))


def store(type_name, default, dense):
    s = pkg.HipStore(len(dense), type_name, default)
    s.set_data_f64(dense)
    return s


def same_store(a, b):
    return np.array_equal(a.get_status(), b.get_status()) and same_typed(a.get_data(), b.get_data())


def on_the_device(type_name, default, fill, source, my_len, his_len, maps):
    """create [+ fill] + load, the three calls the new one replaces"""
    ref = pkg.HipStore(int(np.prod(my_len, dtype=np.int64)) if len(my_len) else 1, type_name, default)
    if fill is not None:
        ref.fill(fill)
    ref.load(source, my_len, his_len, maps)
    return ref


def on_the_oracle(type_name, default, fill, dense, my_len, his_len, maps):
    his = OracleStore(len(dense), type_name, default)
    his.set_data(dense)
    mine = OracleStore(int(np.prod(my_len, dtype=np.int64)) if len(my_len) else 1, type_name, default)
    if fill is not None:
        mine.fill(fill)
    mine.load(his, my_len, his_len, maps)
    return mine.typed()


def written_once(my_len, his_len, maps):
    """my cells that at most one cell of his lands on.  Where several do, the reference's load keeps the last one in
    flat order (the oracle, and the compose pass); olap_store_load on the device writes them from several lanes at once
    and keeps whichever store lands last, so its result is compared on the other cells only.  Cube never builds such
    maps (a dimension lists an item once)."""
    once = np.ones(1, dtype=bool)
    for mine, his, m in zip(my_len, his_len, maps):
        m = np.asarray(m, dtype=np.int64)[:his]
        hits = np.bincount(m[m >= 0], minlength=mine)
        once = np.multiply.outer(once, hits <= 1).reshape(-1)
    return once


def check(out, type_name, default, fill, source, dense, my_len, his_len, maps, tag):
    assert (out.type, out.size) == (type_name, int(np.prod(my_len, dtype=np.int64)) if len(my_len) else 1), tag
    assert out.default_is_nan == (default != default), tag
    ref = on_the_device(type_name, default, fill, source, my_len, his_len, maps)
    once = written_once(my_len, his_len, maps)
    assert np.array_equal(out.get_status()[once], ref.get_status()[once]) and same_typed(out.get_data()[once], ref.get_data()[once]), ("device", tag)
    # An integer CELL cannot hold NaN: olap_store_fill(NaN) under a 0 default converts it to 0, the default, and leaves the
    # cells unset, where the reference's Map keeps a NaN number until serialize() (tests/test_typed_storage_differences.py
    # pins this kind of difference); that one combination is compared with the device calls only.
    if type_name in ("int32", "uint32") and default == 0.0 and fill is not None and fill != fill:
        return
    values, status = on_the_oracle(type_name, default, fill, dense, my_len, his_len, maps)
    assert np.array_equal(out.get_status(), status) and same_typed(out.get_data(), values), ("oracle", tag)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_type_default_and_fill_as_create_fill_load(shape):
    """One call per (type, default) carries five sources, one per fill — so only some measures of the call have one."""
    my_len, his_len, maps, kernel = SHAPES[shape]
    n_his = int(np.prod(his_len))
    rng = np.random.default_rng(5100)
    for type_name in TYPES:
        for default in DEFAULTS:
            assert pkg.Plan.compose(type_name, default, my_len, his_len, maps).kernel_name == kernel, (shape, type_name)
            dense = [cells(rng, n_his, default) for _ in FILLS]
            sources = [store(type_name, default, d) for d in dense]
            before = [(s.get_status(), s.get_data()) for s in sources]
            outs, launches = pkg.HipStore.compose_many(sources, my_len, his_len, maps, FILLS)
            assert launches == 1, (shape, type_name, default)
            for out, fill, source, d in zip(outs, FILLS, sources, dense):
                check(out, type_name, default, fill, source, d, my_len, his_len, maps, (shape, type_name, default, fill))
            for s, (status, values) in zip(sources, before):  # the sources are only read
                assert np.array_equal(s.get_status(), status) and same_typed(s.get_data(), values)


def test_the_last_of_several_items_wins():
    """[2, 3] <- [3, 5] by [1, 1, 1], [2, -1, 2, 0, 0]: my row 0 has no row of his; my (1, 0) takes his (2, 4), my (1, 2)
    his (2, 2), my (1, 1) nothing — the cells a load writes last."""
    my_len, his_len, maps, _ = SHAPES["three times"]
    source = store("float64", NAN, np.arange(1, 16, dtype=np.float64))
    (out,), _ = pkg.HipStore.compose_many([source], my_len, his_len, maps, [-1.0])
    assert out.get_data().tolist() == [-1.0, -1.0, -1.0, 15.0, -1.0, 13.0]


@pytest.mark.parametrize("type_name,default", [("float32", 0.0), ("int32", NAN), ("float64", NAN)])
def test_results_without_a_cell_of_his(type_name, default):
    rng = np.random.default_rng(5200)
    # a target of 0 cells: stores of size 0, nothing launched
    sources = [store(type_name, default, cells(rng, 6, default)) for _ in range(2)]
    outs, launches = pkg.HipStore.compose_many(sources, [0, 3], [2, 3], [[-1, -1], ident(3)], [7.0, None])
    assert launches == 0 and [o.size for o in outs] == [0, 0] and [o.type for o in outs] == [type_name] * 2
    # no stores: nothing to do
    assert pkg.HipStore.compose_many([], [2, 3], [2, 3], [ident(2), ident(3)]) == ([], 0)
    assert pkg.HipStore.compose_many([], [2, 3], [2, 3], [ident(2), ident(3)], []) == ([], 0)
    # no common dimension: a single cell, set and unset, with and without a fill
    for value in (5.0, default):
        for fill in (None, 7.0):
            one = store(type_name, default, np.array([value]))
            (out,), launches = pkg.HipStore.compose_many([one], [], [], [], [fill])
            assert launches == 1
            check(out, type_name, default, fill, one, np.array([value]), [], [], [], ("one cell", value, fill))
    # a source with no set cell, and one with no cell at all
    my_len, his_len, maps, _ = SHAPES["remapped"]
    for fill in (None, 7.0):
        dense = np.full(60, default)
        empty = store(type_name, default, dense)
        (out,), _ = pkg.HipStore.compose_many([empty], my_len, his_len, maps, [fill])
        check(out, type_name, default, fill, empty, dense, my_len, his_len, maps, ("nothing set", fill))
        nothing = pkg.HipStore(0, type_name, default)
        (out,), _ = pkg.HipStore.compose_many([nothing], [2, 3], [0, 3], [[], ident(3)], [fill])
        check(out, type_name, default, fill, nothing, np.zeros(0), [2, 3], [0, 3], [[], ident(3)], ("no cells", fill))
    # maps of only -1: every cell is the fill (or unset)
    dense = cells(rng, 6, default)
    source = store(type_name, default, dense)
    for fill in (None, 7.0, 2.5):
        for my_len in ([2, 3], [4, 8]):  # the per-cell form and whole lanes
            maps = [[-1, -1], [-1, -1, -1]]
            (out,), _ = pkg.HipStore.compose_many([source], my_len, [2, 3], maps, [fill])
            check(out, type_name, default, fill, source, dense, my_len, [2, 3], maps, ("all fill", fill, my_len))
            want = 0 if fill is None else (2 if fill == 2.5 and type_name == "int32" else fill)
            if fill is not None:
                assert np.all(out.get_data() == want) and np.all(out.get_status() == 2)
            else:
                assert np.all(out.get_status() == 0)


@pytest.mark.parametrize("shape", ["lanes", "remapped"])
def test_launches_of_up_to_eight(shape):
    my_len, his_len, maps, _ = SHAPES[shape]
    n_his = int(np.prod(his_len))
    rng = np.random.default_rng(5300)
    for n, want in [(1, 1), (2, 1), (8, 1), (9, 2)]:
        dense = [cells(rng, n_his, 0.0) for _ in range(n)]
        sources = [store("float32", 0.0, d) for d in dense]
        fills = [None if i % 3 else float(i + 1) for i in range(n)]
        outs, launches = pkg.HipStore.compose_many(sources, my_len, his_len, maps, fills)
        assert launches == want, (shape, n)
        for i in range(n):
            check(outs[i], "float32", 0.0, fills[i], sources[i], dense[i], my_len, his_len, maps, (shape, n, i))


def test_groups_by_type_and_default_in_list_order_and_a_repeat_gives_the_same():
    """{f32 / 0, f64 / NaN, f32 / 0, i32 / NaN}: three groups, three launches, the results in list order.  The repeat finds
    its three plans in the plan cache (which shows nothing to a test): the same launches and the same cells."""
    my_len, his_len, maps, _ = SHAPES["lanes"]
    n_his = int(np.prod(his_len))
    rng = np.random.default_rng(5400)
    kinds = [("float32", 0.0), ("float64", NAN), ("float32", 0.0), ("int32", NAN)]
    fills = [3.0, None, None, 2.5]
    dense = [cells(rng, n_his, d) for _, d in kinds]
    sources = [store(t, d, v) for (t, d), v in zip(kinds, dense)]
    for attempt in range(2):
        outs, launches = pkg.HipStore.compose_many(sources, my_len, his_len, maps, fills)
        assert launches == 3, attempt
        for i, (t, d) in enumerate(kinds):
            check(outs[i], t, d, fills[i], sources[i], dense[i], my_len, his_len, maps, (attempt, i))


@pytest.mark.parametrize("shape", ["lanes", "ragged"])
@pytest.mark.parametrize("type_name,default", [("float32", 0.0), ("int32", NAN)])
def test_the_plan_runs_as_a_compose_without_a_fill(shape, type_name, default):
    """olap_plan_run over an olap_compose_plan writes every cell of `out`: a store full of other cells ends as a new one."""
    my_len, his_len, maps, _ = SHAPES[shape]
    rng = np.random.default_rng(5500)
    dense = cells(rng, int(np.prod(his_len)), default)
    source = store(type_name, default, dense)
    out = store(type_name, default, rng.integers(1, 9, size=int(np.prod(my_len))).astype(np.float64))
    plan = pkg.Plan.compose(type_name, default, my_len, his_len, maps)
    assert (plan.in_cells, plan.out_cells) == (int(np.prod(his_len)), int(np.prod(my_len)))
    masks = type_name == "int32"
    plan.run(source.values_ptr, source.status_ptr if masks else 0, out.values_ptr, out.status_ptr if masks else 0)
    (want,), _ = pkg.HipStore.compose_many([source], my_len, his_len, maps)
    assert same_typed(out.get_data(), want.get_data())
    if masks:
        assert np.array_equal(out.get_status(), want.get_status())
