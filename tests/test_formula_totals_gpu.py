"""olap_formula_totals (getNestedObject(computed measure, withTotals)): the extended cube of a formula over stored
measures must hold, for every one of the 2^D subsets of dimensions, the formula applied cell by cell to what the chain
drillUp(dim, 'all') over the subset's dimensions leaves of each input (each input with its own rules).

The expectation never comes from the code under test: every input runs the ORACLE chain exactly as tests/test_totals.py
does (typed rounding after every step, golden_util.expected_typed), and the formula is applied with numpy float64.  The
formulas use only operations IEEE-754 defines exactly and numpy implements so (+ - * /, min, max, abs, sqrt, unary
minus, ?:), so numpy is an independent oracle and every comparison is on float64 bit patterns (NaN equal to NaN).  The
formula language has no comparison operators; `?:` tests truthiness (non-zero and not NaN), so a comparison a > b is
written max(a - b, 0) ? x : y.  Input values are small integers (quarters for float cells): every stage of the oracle
chain is exact in the cell type."""
import itertools

import numpy as np
import pytest

from conftest import load_package
from golden_util import expected_typed, same_f64
from oracle.oracle import OracleStore

pytestmark = pytest.mark.gpu

pkg = load_package()
capi = pkg.capi
hs = pkg.hipstore
METHODS = ["sum", "average", "highest", "lowest", "first", "last", "product"]
NAN = float("nan")
KINDS = [("float32", 0.0), ("uint32", NAN), ("float64", 0.0), ("int32", NAN), ("float32", NAN), ("int32", 0.0), ("float64", NAN), ("uint32", 0.0)]
LDS_CELLS = 12288

# ---- formulas as trees; compiled to the postfix program of js/formula.js and evaluated by numpy ---------------------
OPCODE = {"const": 0, "in": 1, "add": 3, "sub": 4, "mul": 5, "div": 6, "neg": 9, "select": 11, "min": 12, "max": 13, "abs": 20, "sqrt": 25}


def I(k):
    return ("in", k)


def K(v):
    return ("const", float(v))


def compile_tree(tree):
    code, consts = [], []

    def walk(t):
        if t[0] == "in":
            code.extend([OPCODE["in"], t[1]])
        elif t[0] == "const":
            if t[1] not in consts:
                consts.append(t[1])
            code.extend([OPCODE["const"], consts.index(t[1])])
        else:
            for arg in t[1:]:
                walk(arg)
            code.append(OPCODE[t[0]])

    walk(tree)
    return code, consts


def np_min(a, b):
    """IEEE-754 minimum: NaN propagates, -0 < +0"""
    r = np.where(a < b, a, b)
    r = np.where((a == 0) & (b == 0), np.where(np.signbit(a), a, b), r)
    return np.where(np.isnan(a) | np.isnan(b), np.nan, r)


def np_max(a, b):
    r = np.where(a > b, a, b)
    r = np.where((a == 0) & (b == 0), np.where(np.signbit(a), b, a), r)
    return np.where(np.isnan(a) | np.isnan(b), np.nan, r)


def evaluate(tree, inputs):
    with np.errstate(all="ignore"):
        op = tree[0]
        if op == "in":
            return inputs[tree[1]]
        if op == "const":
            return np.full(inputs[0].shape, tree[1], np.float64)
        a = [evaluate(t, inputs) for t in tree[1:]]
        if op == "add":
            return a[0] + a[1]
        if op == "sub":
            return a[0] - a[1]
        if op == "mul":
            return a[0] * a[1]
        if op == "div":
            return a[0] / a[1]
        if op == "neg":
            return -a[0]
        if op == "abs":
            return np.abs(a[0])
        if op == "sqrt":
            return np.sqrt(a[0])
        if op == "min":
            return np_min(a[0], a[1])
        if op == "max":
            return np_max(a[0], a[1])
        assert op == "select"
        return np.where(~np.isnan(a[0]) & (a[0] != 0), a[1], a[2])


THIRD = ("div", I(0), K(3))                                                      # a / 3: full mantissas
MULADD = ("add", ("mul", I(0), I(1)), K(1))                                      # a * b + 1
RATIO = ("div", I(0), I(1))                                                      # a / b: unset and zero cells give inf and NaN
GREATER = ("select", ("max", ("sub", I(0), I(1)), K(0)), ("sqrt", ("abs", I(2))), ("neg", ("min", I(0), I(2))))  # a > b ? sqrt|c| : -min(a, c)
EIGHT = ("sub", ("add", ("div", ("sub", ("mul", ("add", I(0), I(1)), I(2)), I(3)), ("add", I(4), K(1.5))), ("max", I(5), I(6))), ("abs", I(7)))
BY_INPUTS = {1: [THIRD], 2: [MULADD, RATIO], 3: [GREATER], 8: [EIGHT]}


# ---- the oracle chain of tests/test_totals.py, restated ----------------------------------------------------------------
def chain(vals, type_name, default, lens, methods, subset):
    """oracle: drillUp(dim, 'all') for every dimension of `subset`, ascending; returns (typed values, mask)."""
    cur_lens = list(lens)
    o = OracleStore(len(vals), type_name, default)
    o.set_data(vals)
    ev, es = expected_typed(o)
    for d in sorted(subset):
        new_lens = list(cur_lens)
        new_lens[d] = 1
        maps = [np.zeros(l, np.uint32) if i == d else np.arange(l, dtype=np.uint32) for i, l in enumerate(cur_lens)]
        o = OracleStore(int(np.prod(cur_lens)), type_name, default)
        o.set_data(np.where(es == 2, ev.astype(np.float64), default))
        ev, es = expected_typed(o.drill_up(cur_lens, new_lens, maps, methods[d]))
        cur_lens = new_lens
    return ev, es


def get_value(ev, es, default):
    """getValue of every cell (in-memory.js:118-120): the value, or the default where unset"""
    return np.where(es == 2, ev.astype(np.float64), default)


def random_values(rng, n, type_name, default, frac):
    vals = rng.integers(-6, 7, size=n).astype(np.float64) if type_name != "uint32" else rng.integers(0, 9, size=n).astype(np.float64)
    if type_name.startswith("float"):
        vals = vals / 4.0
    return np.where(rng.random(n) < frac, vals, default)


def make_inputs(lens, kinds, seed, frac=0.7):
    rng = np.random.default_rng(seed)
    n = int(np.prod(lens)) if len(lens) else 1
    out = []
    for type_name, default in kinds:
        vals = random_values(rng, n, type_name, default, frac)
        g = pkg.HipStore(n, type_name, default)
        g.set_data_f64(vals)
        out.append((g, vals, type_name, default))
    return out


def check(tree, lens, inputs, methods, order=None, expect=True):
    """inputs: [(HipStore, float64 values, type, default)]; methods[i]: input i's rule per dimension; order: which entry
    of `inputs` each formula operand reads (default: one each)."""
    order = list(range(len(inputs))) if order is None else order
    code, consts = compile_tree(tree)
    stores = [inputs[k][0] for k in order]
    before = [inputs[k][0].get_data_f64().tobytes() for k in order]
    got, launches, nbytes = hs.formula_totals(code, consts, stores, lens, [methods[k] for k in order])
    assert [inputs[k][0].get_data_f64().tobytes() for k in order] == before  # the inputs are unchanged
    ext_shape = [l + 1 for l in lens]
    ext_cells = int(np.prod(ext_shape)) if lens else 1
    assert got.size == ext_cells
    # what ran (include/olap_hip.h): per-input figures from olap_store_totals on the same store
    alone = [inputs[k][0].totals(lens, methods[k]) for k in order]
    sum_launches, sum_bytes = sum(a[2] for a in alone), sum(a[3] for a in alone)
    if ext_cells <= LDS_CELLS:
        distinct = len({inputs[k][2] for k in order})
        print("small: launches", launches, "distinct cell types", distinct, "bytes", nbytes)
        assert launches <= distinct + 1, (launches, distinct)
    else:
        print("large: launches", launches, "sum of the inputs' launches", sum_launches, "bytes", nbytes, "sum", sum_bytes)
        assert launches == sum_launches + 1, (launches, sum_launches)
    assert nbytes == sum_bytes + len(order) * ext_cells * 8, (nbytes, sum_bytes)
    if not expect:
        return got
    got = got.reshape(ext_shape)
    for r in range(len(lens) + 1):
        for subset in itertools.combinations(range(len(lens)), r):
            cache = {}
            for k in set(order):
                _g, vals, type_name, default = inputs[k]
                ev, es = chain(vals, type_name, default, lens, methods[k], subset)
                cache[k] = get_value(ev, es, default)
            want = evaluate(tree, [cache[k] for k in order])
            index = tuple(lens[d] if d in subset else slice(0, lens[d]) for d in range(len(lens)))
            have = np.asarray(got[index], dtype=np.float64).ravel()
            assert same_f64(have, want), (subset, have[:8], want[:8])
    return got


def rules(n_inputs, nd, shift=0):
    """a different rule list per input: input i, dimension d -> METHODS[(shift + 3 i + d) mod 7]"""
    return [[METHODS[(shift + 3 * i + d) % 7] for d in range(nd)] for i in range(n_inputs)]


# ---- every cell type x both defaults, 1 / 2 / 3 / 8 inputs --------------------------------------------------------------
@pytest.mark.parametrize("kind", range(8))
def test_one_input_every_cell_type_and_default(kind):
    lens = [4, 3, 5]
    check(THIRD, lens, make_inputs(lens, [KINDS[kind]], seed=kind), rules(1, 3, kind))


@pytest.mark.parametrize("tree", BY_INPUTS[2], ids=["muladd", "ratio"])
@pytest.mark.parametrize("kind", range(8))
def test_two_inputs_mixed_cell_types(kind, tree):
    lens = [4, 3, 5]
    check(tree, lens, make_inputs(lens, [KINDS[kind], KINDS[(kind + 3) % 8]], seed=10 + kind, frac=0.6), rules(2, 3, kind))


@pytest.mark.parametrize("first", range(8))
def test_three_inputs_mixed_cell_types(first):
    """first = 0: Float32 0-default with uint32 NaN-default with Float64"""
    lens = [4, 3, 5]
    kinds = [KINDS[(first + j) % 8] for j in range(3)]
    check(GREATER, lens, make_inputs(lens, kinds, seed=20 + first), rules(3, 3, first))


@pytest.mark.parametrize("shift", [0, 4])
def test_eight_inputs_every_kind_at_once(shift):
    lens = [4, 3, 5]
    kinds = [KINDS[(shift + j) % 8] for j in range(8)]
    check(EIGHT, lens, make_inputs(lens, kinds, seed=30 + shift, frac=0.8), rules(8, 3, shift))


# ---- a different rule list per input, sparse data -----------------------------------------------------------------------
def test_rule_lists_cover_all_seven_rules():
    used = {m for seed in range(12) for per_input in rules(3, 5, seed) for m in per_input}
    assert used == set(METHODS)


@pytest.mark.parametrize("seed", range(12))
def test_rules_per_input_on_sparse_data(seed):
    """average of sums differs from sum of averages on sparse cells: each input's own rule list is part of the result"""
    rng = np.random.default_rng(200 + seed)
    nd = int(rng.integers(1, 6))
    lens = [int(x) for x in rng.integers(1, 6, size=nd)]
    n_inputs = [2, 3, 1][seed % 3]
    tree = [MULADD, GREATER, THIRD][seed % 3] if seed % 2 == 0 else [RATIO, GREATER, THIRD][seed % 3]
    kinds = [KINDS[(seed + 2 * j) % 8] for j in range(n_inputs)]
    check(tree, lens, make_inputs(lens, kinds, seed=300 + seed, frac=[1.0, 0.6, 0.3][seed % 3]), rules(n_inputs, nd, seed))


def test_the_rule_of_each_input_matters():
    """one store read as two operands with two rule lists: sum-then-average against average-then-sum"""
    lens = [3, 4]
    inputs = make_inputs(lens, [("float32", 0.0)], seed=5, frac=0.5)
    both = [inputs[0], inputs[0]]
    got = check(("sub", I(0), I(1)), lens, both, [["sum", "average"], ["average", "sum"]])
    assert np.any(got != 0)


# ---- shapes on both sides of the LDS bound and through every large-case form -------------------------------------------
SHAPES = [([4, 3, 5], ["sum", "average", "last"]),
          ([7, 6, 5, 4, 3, 2], ["sum"] * 6),
          ([40, 30, 12], ["sum", "average", "last"]),          # groups of dimensions through LDS
          ([3, 5000, 4], ["highest", "sum", "average"]),       # a dimension too long for a tile, between two groups
          ([2, 3, 13000], ["sum", "sum", "average"]),          # a tile that owns a CU
          ([2, 3, 40000], ["sum", "sum", "average"]),          # innermost dimension beyond any tile: scatter + stages + export
          ([], []),                                            # no dimension: one cell
          ([3, 1, 4], ["average", "product", "lowest"])]       # a dimension of length 1


@pytest.mark.parametrize("lens,methods", SHAPES, ids=[str(s[0]) for s in SHAPES])
def test_shapes(lens, methods):
    nd = len(lens)
    kinds = [("float32", 0.0), ("uint32", NAN)]
    per_input = [list(methods), [methods[(d + 1) % nd] for d in range(nd)]]
    check(MULADD, lens, make_inputs(lens, kinds, seed=40 + nd), per_input)


@pytest.mark.parametrize("lens,methods", [([40, 30, 12], ["average", "sum", "highest"]), ([2, 3, 13000], ["sum", "average", "sum"])], ids=["groups", "owns-a-cu"])
def test_large_three_inputs_of_one_cell_type(lens, methods):
    kinds = [("float64", NAN), ("float64", 0.0), ("float64", NAN)]
    check(GREATER, lens, make_inputs(lens, kinds, seed=50), [methods, methods[::-1], methods])


def test_small_launches_share_a_cell_type():
    """inputs of one cell type: one launch builds every extended cube, one evaluates"""
    lens = [4, 3, 5]
    inputs = make_inputs(lens, [("float32", 0.0), ("float32", NAN), ("float32", 0.0)], seed=60)
    code, consts = compile_tree(GREATER)
    _v, launches, _b = hs.formula_totals(code, consts, [x[0] for x in inputs], lens, rules(3, 3))
    assert launches == 2
    inputs = make_inputs(lens, [("float32", 0.0), ("int32", NAN), ("float64", 0.0)], seed=61)
    _v, launches, _b = hs.formula_totals(code, consts, [x[0] for x in inputs], lens, rules(3, 3))
    assert launches == 4
    # at the LDS bound: 12288 = 16 * 24 * 32 extended cells
    lens = [15, 23, 31]
    inputs = make_inputs(lens, [("float64", 0.0), ("float64", NAN)], seed=62)
    check(MULADD, lens, inputs, [["sum", "average", "sum"], ["highest", "sum", "average"]])


# ---- the same store twice, an empty input, a tracked input --------------------------------------------------------------
def test_same_store_as_two_inputs():
    lens = [4, 3, 5]
    inputs = make_inputs(lens, [("int32", 0.0)], seed=70)
    check(MULADD, lens, inputs, [["sum", "highest", "average"]], order=[0, 0])
    lens = [40, 30, 12]
    inputs = make_inputs(lens, [("float32", NAN)], seed=71)
    check(RATIO, lens, inputs, [["sum", "average", "last"]], order=[0, 0])


@pytest.mark.parametrize("kind", [("float32", 0.0), ("uint32", NAN), ("float64", NAN)], ids=["f32-0", "u32-nan", "f64-nan"])
def test_an_input_whose_every_cell_is_unset(kind):
    lens = [4, 3, 5]
    inputs = make_inputs(lens, [("float32", 0.0)], seed=80)
    empty = pkg.HipStore(60, kind[0], kind[1])
    inputs.append((empty, np.full(60, kind[1]), kind[0], kind[1]))
    check(RATIO, lens, inputs, [["sum", "sum", "average"], ["average", "sum", "product"]])
    check(MULADD, lens, inputs, [["sum", "sum", "average"], ["average", "sum", "product"]], order=[1, 0])


def test_tracked_input_is_refused_and_nothing_else_happens():
    lens = [4, 3, 5]
    inputs = make_inputs(lens, [("float32", 0.0), ("float32", 0.0)], seed=90)
    capi.check(capi.lib().olap_store_track_order(inputs[1][0]._h, 1))
    before = [x[0].get_data_f64().tobytes() for x in inputs]
    code, consts = compile_tree(MULADD)
    with pytest.raises(pkg.OlapError) as err:
        hs.formula_totals(code, consts, [x[0] for x in inputs], lens, rules(2, 3))
    assert str(err.value).split(": ", 1)[-1].startswith("ordered:") or "ordered:" in str(err.value)
    assert capi.last_error().startswith("ordered:")
    assert [x[0].get_data_f64().tobytes() for x in inputs] == before
    assert capi.lib().olap_store_order_tracked(inputs[1][0]._h) == 1  # still tracked, still ascending
    with pytest.raises(pkg.OlapError, match="Unsupported aggregation method"):
        hs.formula_totals(code, consts, [inputs[0][0], inputs[0][0]], lens, [[0, 1, 2], [0, 1, 9]])
    assert [x[0].get_data_f64().tobytes() for x in inputs] == before


def test_reference_literals():
    """test/cube-accessors.js: antennas [[1,2],[4,8],[16,32]], routers [[3,2],[4,9],[16,32]], routers / antennas"""
    a = pkg.HipStore(6, "uint32", 0.0)
    a.set_data_f64([1, 2, 4, 8, 16, 32])
    r = pkg.HipStore(6, "uint32", 0.0)
    r.set_data_f64([3, 2, 4, 9, 16, 32])
    code, consts = compile_tree(("div", I(0), I(1)))
    got, launches, nbytes = hs.formula_totals(code, consts, [r, a], [3, 2], [["sum", "sum"], ["sum", "sum"]])
    want = [[3 / 1, 2 / 2, 5 / 3], [4 / 4, 9 / 8, 13 / 12], [16 / 16, 32 / 32, 48 / 48], [23 / 21, 43 / 42, 66 / 63]]
    assert got.reshape(4, 3).tolist() == want and launches == 2 and nbytes == 48 + 2 * 12 * 8
