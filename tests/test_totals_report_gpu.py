"""olap_totals_report (getNestedObjects(ids, withTotals)): several stored and computed measures of one cube in one call.

Every output slot is compared on float64 bit patterns (NaN equal to NaN) with what olap_store_totals or
olap_formula_totals gives when it is called alone on the same stores, and `launches` / `bytes_read` with the contract of
include/olap_hip.h.  Sibling code is not the only expectation: the small cases are also compared with the ORACLE chain
of drillUp(dim, 'all') per input and subset (typed rounding after every step, golden_util.expected_typed) plus the formula
in numpy float64, restated from tests/test_formula_totals_gpu.py.  The formulas use only operations IEEE-754 defines
exactly (+ - * /, min, max, abs, unary minus), and the values are small integers (quarters for float cells), so every
stage of the oracle chain is exact in the cell type."""
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
LDS_CELLS = 12288
BATCH = 8  # inputs of one cell type per launch of the LDS regime

# ---- formulas as trees; compiled to the postfix program of js/formula.js and evaluated by numpy ---------------------
OPCODE = {"const": 0, "in": 1, "add": 3, "sub": 4, "mul": 5, "div": 6, "neg": 9, "min": 12, "max": 13, "abs": 20}


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
        return {"add": lambda: a[0] + a[1], "sub": lambda: a[0] - a[1], "mul": lambda: a[0] * a[1], "div": lambda: a[0] / a[1],
                "neg": lambda: -a[0], "abs": lambda: np.abs(a[0]), "min": lambda: np_min(a[0], a[1]), "max": lambda: np_max(a[0], a[1])}[op]()


THIRD = ("div", I(0), K(3))                                                      # a / 3: full mantissas
MARGIN = ("sub", I(0), I(1))                                                     # a - b
RATIO = ("div", ("sub", I(0), I(1)), I(0))                                       # (a - b) / a: unset and zero cells give inf and NaN
THREE = ("add", ("mul", I(0), I(1)), ("max", I(2), K(0.5)))                      # a * b + max(c, 0.5)
EIGHT = ("sub", ("add", ("div", ("sub", ("mul", ("add", I(0), I(1)), I(2)), I(3)), ("add", I(4), K(1.5))), ("max", I(5), I(6))), ("abs", I(7)))


# ---- the oracle chain of tests/test_totals.py, restated ----------------------------------------------------------------
def chain(vals, type_name, default, lens, methods, subset):
    """oracle: drillUp(dim, 'all') for every dimension of `subset`, ascending; returns getValue of every cell"""
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
    return np.where(es == 2, ev.astype(np.float64), default)


def random_values(rng, n, type_name, default, frac):
    vals = rng.integers(-6, 7, size=n).astype(np.float64) if type_name != "uint32" else rng.integers(0, 9, size=n).astype(np.float64)
    if type_name.startswith("float"):
        vals = vals / 4.0
    return np.where(rng.random(n) < frac, vals, default)


def make_inputs(lens, kinds, seed, frac=0.7):
    """[(HipStore, float64 values, type, default)]"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(lens)) if len(lens) else 1
    out = []
    for type_name, default in kinds:
        vals = random_values(rng, n, type_name, default, frac)
        g = pkg.HipStore(n, type_name, default)
        g.set_data_f64(vals)
        out.append((g, vals, type_name, default))
    return out


def rules(n_inputs, nd, shift=0):
    """a different rule list per input: input i, dimension d -> METHODS[(shift + 3 i + d) mod 7]"""
    return [[METHODS[(shift + 3 * i + d) % 7] for d in range(nd)] for i in range(n_inputs)]


def check(lens, inputs, methods, outputs, oracle=True):
    """outputs: an int (the extended cube of that input) or (tree, picks).  The report against the two per-measure calls
    alone, slot by slot on bit patterns; its launches and bytes against the contract; and, when `oracle`, against the
    oracle chain + numpy."""
    stores = [x[0] for x in inputs]
    before = [s.get_data_f64().tobytes() for s in stores]
    spec = [o if isinstance(o, int) else (*compile_tree(o[0]), o[1]) for o in outputs]
    got, launches, nbytes = hs.totals_report(stores, lens, methods, spec)
    assert [s.get_data_f64().tobytes() for s in stores] == before  # the inputs are unchanged
    ext_shape = [l + 1 for l in lens]
    ext = int(np.prod(ext_shape)) if lens else 1
    assert got.shape == (len(outputs), ext)
    # ---- each slot against the per-measure call, alone on the same stores
    alone = [s.totals(lens, methods[i]) for i, s in enumerate(stores)]
    for k, o in enumerate(outputs):
        if isinstance(o, int):
            want = alone[o][0]
        else:
            code, consts = compile_tree(o[0])
            want = hs.formula_totals(code, consts, [stores[i] for i in o[1]], lens, [methods[i] for i in o[1]])[0]
        assert same_f64(got[k], want), ("slot", k, got[k][:8], want[:8])
    # ---- what ran (include/olap_hip.h)
    formulas = [o for o in outputs if not isinstance(o, int)]
    if ext <= LDS_CELLS:
        per_type = {}
        for x in inputs:
            per_type[x[2]] = per_type.get(x[2], 0) + 1
        want_launches = sum(-(-n // BATCH) for n in per_type.values()) + (1 if formulas else 0)
    else:
        want_launches = sum(a[2] for a in alone) + (1 if formulas else 0)
    want_bytes = sum(a[3] for a in alone) + sum(len(o[1]) * ext * 8 for o in formulas)
    print("ext", ext, "launches", launches, "expected", want_launches, "bytes", nbytes, "expected", want_bytes)
    assert launches == want_launches
    assert nbytes == want_bytes
    if not oracle:
        return got
    # ---- every marginal against the oracle chain and numpy
    for r in range(len(lens) + 1):
        for subset in itertools.combinations(range(len(lens)), r):
            marginal = [chain(vals, type_name, default, lens, methods[i], subset) for i, (_g, vals, type_name, default) in enumerate(inputs)]
            index = tuple(lens[d] if d in subset else slice(0, lens[d]) for d in range(len(lens)))
            for k, o in enumerate(outputs):
                want = marginal[o] if isinstance(o, int) else evaluate(o[0], [marginal[i] for i in o[1]])
                have = np.asarray(got[k].reshape(ext_shape)[index], dtype=np.float64).ravel()
                assert same_f64(have, want), ("slot", k, "subset", subset, have[:8], want[:8])
    return got


# ---- odd extended cubes: the packed slots 1 and 3 start on an 8-byte boundary only, and hold formulas -----------------
@pytest.mark.parametrize("lens", [[], [1], [2, 2]], ids=["ext1", "ext2", "ext9"])
def test_two_stored_and_three_formulas_on_tiny_cubes(lens):
    nd = len(lens)
    inputs = make_inputs(lens, [("float32", 0.0), ("float64", NAN)], seed=7 + nd, frac=0.8)
    check(lens, inputs, rules(2, nd, 1), [0, (MARGIN, [0, 1]), 1, (RATIO, [1, 0]), (THIRD, [1])])


# ---- four cell types, outputs in another order than the inputs, shared and formula-only inputs ---------------------------
def test_four_cell_types_shared_inputs_and_all_seven_rules():
    lens = [4, 3, 5]
    kinds = [("int32", NAN), ("uint32", 0.0), ("float32", NAN), ("float64", 0.0)]
    methods = rules(4, 3)
    assert {m for per_input in methods for m in per_input} == set(METHODS)
    # input 2: three formulas and a stored output; input 1: formulas only
    outputs = [(MARGIN, [2, 0]), 3, (RATIO, [1, 2]), 2, (THREE, [2, 3, 1]), 0]
    check(lens, make_inputs(lens, kinds, seed=11, frac=0.6), methods, outputs)


# ---- more inputs of one cell type than one launch holds; a formula that picks 8 of 12 inputs -----------------------------
def test_nine_float32_inputs_and_a_formula_over_eight_of_twelve():
    lens = [3, 4]
    kinds = [("float32", 0.0 if j % 3 else NAN) for j in range(9)] + [("float64", 0.0), ("int32", NAN), ("float64", NAN)]
    picks = [11, 3, 7, 0, 9, 5, 10, 2]
    outputs = [1, (EIGHT, picks), 4, 6, 8, 11, 0]
    check(lens, make_inputs(lens, kinds, seed=13, frac=0.8), rules(12, 2, 2), outputs)


# ---- the last shape that stays in LDS and the first that takes the pass plan ------------------------------------------
@pytest.mark.parametrize("lens", [[95, 127], [96, 127]], ids=["ext12288-lds", "ext12416-passes"])
def test_lds_boundary(lens):
    ext = (lens[0] + 1) * (lens[1] + 1)
    assert (ext <= LDS_CELLS) == (lens[0] == 95)
    inputs = make_inputs(lens, [("float32", 0.0), ("float64", NAN)], seed=17)
    check(lens, inputs, [["sum", "average"], ["highest", "sum"]], [0, (MARGIN, [1, 0]), 1], oracle=False)


def test_pass_plan_with_an_odd_extended_cube_and_a_formula_only_input():
    """above LDS with odd ext (131 * 101 = 13231): the misaligned slot 1 is a formula, input 1 lives in scratch"""
    lens = [130, 100]
    inputs = make_inputs(lens, [("float32", NAN), ("uint32", 0.0)], seed=19)
    check(lens, inputs, [["sum", "lowest"], ["average", "sum"]], [0, (RATIO, [0, 1]), (THIRD, [1])], oracle=False)


def test_stored_outputs_only():
    lens = [4, 3, 5]
    inputs = make_inputs(lens, [("float32", 0.0), ("float32", NAN), ("int32", 0.0)], seed=23)
    check(lens, inputs, rules(3, 3, 4), [2, 0, 1])


# ---- a tracked input ------------------------------------------------------------------------------------------------------
def test_tracked_input_is_refused_and_the_next_call_succeeds():
    """the refusal is a host check: it comes before the slab is allocated, so there is nothing to give back"""
    lens = [4, 3, 5]
    inputs = make_inputs(lens, [("float32", 0.0), ("float32", 0.0)], seed=29)
    stores = [x[0] for x in inputs]
    capi.check(capi.lib().olap_store_track_order(stores[1]._h, 1))
    before = [s.get_data_f64().tobytes() for s in stores]
    code, consts = compile_tree(MARGIN)
    with pytest.raises(pkg.OlapError):
        hs.totals_report(stores, lens, rules(2, 3), [0, (code, consts, [0, 1])])
    assert capi.last_error().startswith("ordered:")
    assert [s.get_data_f64().tobytes() for s in stores] == before
    assert capi.lib().olap_store_order_tracked(stores[1]._h) == 1  # still tracked, still ascending
    check(lens, [inputs[0]] + make_inputs(lens, [("float32", 0.0)], seed=31), rules(2, 3), [0, (MARGIN, [0, 1])])
