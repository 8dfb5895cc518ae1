"""load between stores of different cell types on the device (olap_load_plan_typed / olap_store_load_multi with n == 1).

The yardstick is the two-step path through calls that predate the converting kernel, on the same GPU: the other store's
float64 values written into a store of MY cell type under HIS default (set_data_f64: from_f64_kernel), then a same-type
load.  load_many must leave the same mask and bit-equal cells for all 12 ordered type pairs x the 4 default pairings, on
the smallest shapes where the two forms of the kernel can go wrong, with values where the conversion shows."""
import numpy as np
import pytest

from conftest import load_package
from golden_util import expected_typed, same_typed
from oracle.oracle import OracleStore

pytestmark = pytest.mark.gpu

pkg = load_package()
NAN = float("nan")
TYPES = ["int32", "uint32", "float32", "float64"]
PAIRS = [(s, t) for s in TYPES for t in TYPES if s != t]  # (his type, my type)
DEFAULTS = [(0.0, 0.0), (NAN, 0.0), (0.0, NAN), (NAN, NAN)]  # (my default, his default)
# (my lengths, his lengths, which dimensions are remapped, what the shape is there for)
SHAPES = [
    ([6, 8, 12], [4, 8, 12], "outer", "outer dimension remapped, contiguous inner runs"),
    ([5, 7], [5, 7], "inner", "inner remapped, rows of 7 that end inside a lane's run"),
    ([37], [41], "inner", "a cube that ends inside a run, items I lack (-1)"),
    ([3, 5, 7], [3, 5, 7], "all", "all odd, so runs of 2 and of 4 cells both straddle rows"),
    ([3, 5, 4095], [3, 5, 4095], "inner", "only the last dimension permuted, over one tile"),
    ([1, 2], [1, 2], "inner", "one row of two cells"),
]
SPECIAL_F64 = [0.1, -1.5, 0.4, 2.0 ** 24 + 1, 2.0 ** 31 + 5, -2.0 ** 31 - 7, 1e40, -0.0]


def maps_for(rng, my_len, his_len, what):
    maps = []
    for d, (ml, hl) in enumerate(zip(my_len, his_len)):
        remap = ml != hl or what == "all" or (what == "outer" and d == 0) or (what == "inner" and d == len(my_len) - 1)
        if remap:
            m = rng.permutation(max(ml, hl))[:hl]
            if hl == 2 and ml == 2:
                m = np.array([1, 0])
            m = np.where(m < ml, m, -1)
        else:
            m = np.arange(hl)
        maps.append(m.astype(np.int32))
    return maps


def his_values(rng, n, his_type, his_default, integers_only=False):
    """float64 values of the source: ~40 % unset (his default), small integers elsewhere, and where the type can hold
    them the values on which a conversion shows"""
    lo = 1 if his_type == "uint32" else -5
    v = rng.integers(lo, 60, size=n).astype(np.float64)
    v[v == 0] = 7.0
    if not integers_only:
        if his_type == "float64":
            k = min(n, 2 * len(SPECIAL_F64))
            v[:k] = (SPECIAL_F64 * 2)[:k]
        if his_type in ("float32", "float64") and his_default == 0.0 and n > 1:
            v[n - 1] = NAN  # a set NaN
    unset = rng.random(n) < 0.4
    if n <= 2 or not integers_only:
        unset[: min(n, len(SPECIAL_F64))] = False
        unset[n - 1] = False
    return np.where(unset, his_default, v)


def my_values(rng, n, my_default):
    return np.where(rng.random(n) < 0.5, my_default, rng.integers(1, 50, size=n).astype(np.float64))


def store(type_name, default, dense):
    s = pkg.HipStore(len(dense), type_name, default)
    s.set_data_f64(dense)
    return s


@pytest.mark.parametrize("his_type,my_type", PAIRS)
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_load_many_of_one_pair_equals_the_two_step_path(shape, his_type, my_type):
    my_len, his_len, what, tag = SHAPES[shape]
    rng = np.random.default_rng(9100 + shape)
    maps = maps_for(rng, my_len, his_len, what)
    n_my, n_his = int(np.prod(my_len)), int(np.prod(his_len))
    for my_default, his_default in DEFAULTS:
        his_dense = his_values(rng, n_his, his_type, his_default)
        mine_dense = my_values(rng, n_my, my_default)
        his = store(his_type, his_default, his_dense)
        mine, mine_ref = store(my_type, my_default, mine_dense), store(my_type, my_default, mine_dense)
        # the yardstick: re-type through float64 under HIS default, then the same-type load
        tmp = pkg.HipStore(n_his, my_type, his_default)
        tmp.set_data_f64(his.get_data_f64())
        mine_ref.load(tmp, my_len, his_len, maps)
        his_before = (his.get_data().tobytes(), his.get_status().tobytes())
        launches = pkg.HipStore.load_many([mine], [his], my_len, his_len, maps)
        where = (tag, his_type, my_type, my_default, his_default)
        assert launches == 1, where
        assert np.array_equal(mine.get_status(), mine_ref.get_status()), where
        assert same_typed(mine.get_data(), mine_ref.get_data()), where
        assert (his.get_data().tobytes(), his.get_status().tobytes()) == his_before, where


@pytest.mark.parametrize("his_type,my_type", [("float32", "float64"), ("float64", "float32")])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_float_pairs_on_integer_values_equal_the_reference(shape, his_type, my_type):
    """Integer-valued data is exact in both float types, so typed storage and the reference's float64 Map coincide:
    OracleStore.load between oracle stores of the two declared types."""
    my_len, his_len, what, tag = SHAPES[shape]
    rng = np.random.default_rng(9200 + shape)
    maps = maps_for(rng, my_len, his_len, what)
    n_my, n_his = int(np.prod(my_len)), int(np.prod(his_len))
    for my_default, his_default in DEFAULTS:
        his_dense = his_values(rng, n_his, his_type, his_default, integers_only=True)
        mine_dense = my_values(rng, n_my, my_default)
        oh = OracleStore(n_his, his_type, his_default)
        oh.set_data(his_dense)
        om = OracleStore(n_my, my_type, my_default)
        om.set_data(mine_dense)
        om.load(oh, my_len, his_len, maps)
        ev, es = expected_typed(om)
        mine = store(my_type, my_default, mine_dense)
        pkg.HipStore.load_many([mine], [store(his_type, his_default, his_dense)], my_len, his_len, maps)
        where = (tag, his_type, my_type, my_default, his_default)
        assert np.array_equal(mine.get_status(), es), where
        assert same_typed(mine.get_data(), ev), where


LANES, RUNS = "load_convert (16-byte lanes of the other store)", "load_convert (16-byte runs of the other store)"


@pytest.mark.parametrize("his_type,my_type,shape,name", [
    ("float32", "float64", 0, LANES),  # 96 contiguous cells: 24 lanes of four 4-byte cells
    ("float64", "int32", 0, LANES),    # 48 lanes of two float64 cells
    ("int32", "float32", 1, RUNS),     # the innermost dimension is remapped
    ("float64", "float32", 2, RUNS),
    ("uint32", "float64", 3, RUNS),
    ("float32", "int32", 4, RUNS),     # only the last dimension permuted: the row form through LDS is same-type only
    ("float64", "uint32", 5, RUNS),
])
def test_plan_names_the_form(his_type, my_type, shape, name):
    my_len, his_len, what, tag = SHAPES[shape]
    maps = maps_for(np.random.default_rng(9300 + shape), my_len, his_len, what)
    plan = pkg.Plan.load_typed(my_type, his_type, 0.0, NAN, my_len, his_len, maps)
    assert plan.kernel_name == name, tag
    assert (plan.in_cells, plan.out_cells) == (int(np.prod(his_len)), int(np.prod(my_len)))


def test_contiguous_rows_that_are_no_whole_lanes_run_as_runs_and_same_types_keep_their_plans():
    ident = [np.arange(l, dtype=np.int32) for l in [3, 5, 7]]
    assert pkg.Plan.load_typed("float32", "float64", 0.0, 0.0, [3, 5, 7], [3, 5, 7], ident).kernel_name == RUNS  # 105 cells, 2 per lane
    assert pkg.Plan.load_typed("float64", "float32", 0.0, 0.0, [3, 5, 8], [3, 5, 8], [np.arange(l, dtype=np.int32) for l in [3, 5, 8]]).kernel_name == LANES
    maps = maps_for(np.random.default_rng(1), [3, 5, 4095], [3, 5, 4095], "inner")
    for t in TYPES:
        same = pkg.Plan.load_typed(t, t, 0.0, 0.0, [3, 5, 4095], [3, 5, 4095], maps).kernel_name
        assert same == pkg.Plan.load(t, 0.0, 0.0, [3, 5, 4095], [3, 5, 4095], maps).kernel_name
        assert same == ("load_permute_rows_kernel" if t != "float64" else "load_scatter (16-byte runs of the other store)")


def test_one_cell_and_the_single_store_call_still_refuses_mixed_types():
    mine, his = store("float32", 0.0, np.array([0.0])), store("float64", NAN, np.array([0.1]))
    assert pkg.HipStore.load_many([mine], [his], [], [], []) == 1
    assert mine.get_data()[0] == np.float32(0.1) and mine.get_status()[0] == 2
    with pytest.raises(pkg.capi.OlapError, match="different cell types"):
        mine.load(his, [], [], [])
