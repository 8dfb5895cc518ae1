"""olap_formula_select_total / olap_store_copy_select_formula (getTotalForDimensionItems and copyMeasureData of a
computed measure) through the Python store API.  Every value is checked against a numpy float64 restatement of the
formula at the selection's positions (tests/select_reference.py): the total bit for bit against the left-to-right
sum, on the path predict_path says; the copy against a loop of set_value calls."""
import math
import struct

import numpy as np
import pytest

from conftest import load_package
from select_reference import nesting_positions, predict_path, sequential_total, split_free

pytestmark = pytest.mark.gpu

pkg = load_package()
hs = pkg.hipstore
DTYPES = ["int32", "uint32", "float32", "float64"]

# opcodes (js/formula.js OP, csrc FormulaOp)
CONST, INPUT, ADD, SUB, MUL, DIV, MOD, NEG, NANADD, SELECT, MIN, MAX, ISNAN = 0, 1, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 17
ABS, CEIL, FLOOR, TRUNC, SQRT, SIGN, NOT = 20, 21, 22, 24, 25, 31, 38
UNARY = [NEG, ISNAN, ABS, CEIL, FLOOR, TRUNC, SQRT, SIGN, NOT]
BINARY = [ADD, SUB, MUL, DIV, MOD, NANADD, MIN, MAX]


def bits(x):
    return struct.pack("<d", x) if x == x else b"nan"


def _js_minmax(a, b, lo):
    both_zero = (a == 0) & (b == 0)
    pick_a = np.where(both_zero, np.signbit(a) == lo, (a < b) if lo else (a > b))
    r = np.where(pick_a, a, b)
    return np.where(np.isnan(a) | np.isnan(b), np.nan, r)


def evaluate(code, consts, inputs):
    """the postfix program over float64 arrays, with the JS semantics of js/formula.js evaluate()"""
    st = []
    pc = 0
    with np.errstate(all="ignore"):
        while pc < len(code):
            op = code[pc]
            if op == CONST:
                pc += 1
                st.append(np.full_like(inputs[0], consts[code[pc]]))
            elif op == INPUT:
                pc += 1
                st.append(np.asarray(inputs[code[pc]], dtype=np.float64))
            elif op == SELECT:
                c, a, b = st[-3], st[-2], st[-1]
                del st[-3:]
                st.append(np.where((c == c) & (c != 0), a, b))
            elif op in UNARY:
                a = st.pop()
                st.append({NEG: lambda: -a, ISNAN: lambda: np.isnan(a).astype(np.float64), ABS: lambda: np.abs(a), CEIL: lambda: np.ceil(a),
                           FLOOR: lambda: np.floor(a), TRUNC: lambda: np.trunc(a), SQRT: lambda: np.sqrt(a),
                           SIGN: lambda: np.where(np.isnan(a), a, np.where(a > 0, 1.0, np.where(a < 0, -1.0, a))),
                           NOT: lambda: np.where((a == a) & (a != 0), 0.0, 1.0)}[op]())
            else:
                b = st.pop()
                a = st.pop()
                st.append({ADD: lambda: a + b, SUB: lambda: a - b, MUL: lambda: a * b, DIV: lambda: a / b, MOD: lambda: np.fmod(a, b),
                           NANADD: lambda: np.where(np.isnan(a) & ~np.isnan(b), b, np.where(~np.isnan(a) & np.isnan(b), a, a + b)),
                           MIN: lambda: _js_minmax(a, b, True), MAX: lambda: _js_minmax(a, b, False)}[op]())
            pc += 1
    return st[-1]


def get_values(store):
    data, st = store.get_data_f64(), store.get_status()
    default = float("nan") if store.default_is_nan else 0.0
    return np.where((st & 2) != 0, data, default)


def formula_terms(code, consts, inputs, positions):
    """the formula's value at every position (-1: every input reads its own default)"""
    vals = []
    for s in inputs:
        v = get_values(s)
        d = float("nan") if s.default_is_nan else 0.0
        vals.append(np.where(positions < 0, d, v[np.maximum(positions, 0)]))
    return evaluate(code, consts, vals)


def random_input(rng, n, dtype, nan_default):
    vals = rng.integers(-40, 40, size=n).astype(np.float64)
    if dtype == "uint32":
        vals = np.abs(vals)
    if dtype in ("float32", "float64"):
        vals = vals * 0.25
    vals[rng.random(n) < 0.3] = 0.0
    if nan_default:
        vals[rng.random(n) < 0.3] = np.nan
    s = pkg.HipStore(n, dtype, float("nan") if nan_default else 0.0)
    s.set_data_f64(vals)
    return s


def random_levels(rng, lens, allow_missing=True, allow_free=True, max_extra=3):
    levels = []
    for d in rng.permutation(len(lens)):
        if rng.random() < 0.35:
            e = list(range(lens[d]))
        else:
            e = [int(x) for x in rng.integers(0, lens[d], size=int(rng.integers(0, lens[d] + max_extra)))]
            if allow_missing and e and rng.random() < 0.3:
                e[int(rng.integers(0, len(e)))] = -1
        levels.append((int(d), e))
    if allow_free and rng.random() < 0.4:
        levels.insert(int(rng.integers(0, len(levels) + 1)), (-1, [0] * int(rng.integers(0, 4))))
    return levels


# integer-valued programs (certified on small data) and ones whose terms carry full mantissas
FORMULAS = [
    ([INPUT, 0, INPUT, 1, ADD], []),
    ([INPUT, 0, INPUT, 1, MUL, INPUT, 2, SUB], []),
    ([INPUT, 0, INPUT, 1, NANADD, CONST, 0, MAX, INPUT, 2, MIN], [1.5]),
    ([INPUT, 0, INPUT, 1, INPUT, 2, SELECT, ABS, NEG], []),
    ([INPUT, 0, ISNAN, INPUT, 1, NOT, ADD, INPUT, 2, SIGN, ADD], []),
    ([INPUT, 0, CONST, 0, MOD, INPUT, 1, FLOOR, ADD, INPUT, 2, CEIL, SUB, INPUT, 0, TRUNC, ADD], [3.0]),
    ([INPUT, 0, CONST, 0, DIV], [3.0]),
    ([INPUT, 0, ABS, SQRT, INPUT, 1, DIV], []),
]


def check_total(code, consts, inputs, lens, levels):
    got, path = hs.select_total_formula(code, consts, inputs, lens, levels)
    positions = nesting_positions(lens, levels)
    terms = formula_terms(code, consts, inputs, positions)
    want = sequential_total(terms, 0.0, np.arange(terms.size))
    assert bits(got) == bits(want), (code, lens, levels, got, want)
    dims, m = split_free(levels)
    if m:
        one = formula_terms(code, consts, inputs, nesting_positions(lens, dims))
        assert path == predict_path(one, m), (code, lens, levels, path)
    return path


@pytest.mark.parametrize("dtypes", [("int32", "uint32", "float32"), ("float64", "int32", "uint32"), ("float32", "float64", "float32"),
                                    ("uint32", "float32", "float64")])
def test_total_matches_reference(dtypes):
    rng = np.random.default_rng(7 + DTYPES.index(dtypes[0]))
    paths = set()
    for trial in range(24):
        ndim = int(rng.integers(1, 5))
        lens = [int(rng.choice([1, 3, 5, 7])) for _ in range(ndim)]
        n = int(np.prod(lens))
        inputs = [random_input(rng, n, t, bool(rng.integers(0, 2))) for t in dtypes]
        code, consts = FORMULAS[trial % len(FORMULAS)]
        paths.add(check_total(code, consts, inputs, lens, random_levels(rng, lens)))
    assert "device" in paths  # (test_uncertified_totals_take_the_sequential_path forces the other path)


def test_row_regime_and_long_lists():
    """runs of >= 1024 cells (ROW), missing rows in ROW mode, and lists above the 512-entry inline limit"""
    rng = np.random.default_rng(21)
    lens = [600, 3, 1031]
    n = int(np.prod(lens))
    inputs = [random_input(rng, n, "float32", False), random_input(rng, n, "int32", True)]
    whole = list(range(1031))
    long_list = [int(x) for x in rng.integers(0, 600, size=700)]
    for code, consts in FORMULAS[:2] + FORMULAS[6:7]:
        code = [w if not (code[i - 1] == INPUT and w == 2) else 1 for i, w in enumerate(code)]  # two inputs only
        for levels in ([(0, long_list[:40]), (1, [2, 0]), (2, whole)], [(1, [1, -1]), (0, [5, 3]), (2, whole)],
                       [(0, long_list), (1, [0, 1, 2]), (2, [4, 1030, 0])], [(2, [7]), (0, long_list), (-1, [0, 0]), (1, [2])]):
            check_total(code, consts, inputs, lens, levels)


def test_missing_cells_read_each_inputs_default():
    a = pkg.HipStore(6, "float64", float("nan"))
    b = pkg.HipStore(6, "int32", 0.0)
    a.set_data_f64(np.arange(1.0, 7.0))
    b.set_data_f64(np.arange(6.0))
    nanadd = [INPUT, 0, INPUT, 1, CONST, 0, ADD, NANADD]  # a || (b + 1): a missing cell gives NaN || (0 + 1) = 1
    got, path = hs.select_total_formula(nanadd, [1.0], [a, b], [2, 3], [(0, [-1, 1]), (1, [0, -1])])
    assert got == 1.0 + 1.0 + (4.0 + 4.0) + 1.0 and path == "device"  # cell (1, 0): 4 || 3 + 1 = 8
    got, _ = hs.select_total_formula([INPUT, 1, CONST, 0, ADD], [2.0], [a, b], [2, 3], [(0, [-1]), (1, [0, 1, 2])])
    assert got == 6.0


def test_uncertified_totals_take_the_sequential_path():
    lens = [3, 4]
    a = pkg.HipStore(12, "float64", 0.0)
    a.set_data_f64(np.array([2.0 ** 53, 1.0, -(2.0 ** 53), 5.0] * 3))
    b = pkg.HipStore(12, "float64", 0.0)
    b.set_data_f64(np.zeros(12))
    for code, consts in (([INPUT, 0, INPUT, 1, SUB], []), ([INPUT, 0, CONST, 0, DIV], [3.0])):
        assert check_total(code, consts, [a, b], lens, [(0, [0, 1, 2]), (1, [0, 1, 2, 3])]) == "sequential"
    assert hs.select_total_formula([INPUT, 0, CONST, 0, DIV], [3.0], [a], lens, [(0, []), (1, [0])]) == (0.0, "device")


SPECIALS = [0.0, -0.0, math.inf, -math.inf, math.nan, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-310, -1e-310, 2.0 ** 53 - 1, 2.0 ** 53,
            2.0 ** 53 + 2, -(2.0 ** 53) - 2, 0.49999999999999994, -0.49999999999999994, 0.5, -0.5, 1.5, -2.5, 3.0, -1.0, 7.25, 1e308, 2.0]


def test_every_op_bit_for_bit():
    """each op of the exact set over specials: the copy into a NaN-default float64 target keeps -0 and every bit"""
    k = len(SPECIALS)
    lens = [k, k]
    grid_a = np.repeat(np.array(SPECIALS), k)
    grid_b = np.tile(np.array(SPECIALS), k)
    a = pkg.HipStore(k * k, "float64", float("nan"))
    b = pkg.HipStore(k * k, "float64", float("nan"))
    a.set_data_f64(grid_a)
    b.set_data_f64(grid_b)
    everything = [(0, list(range(k))), (1, list(range(k)))]
    programs = [[INPUT, 0, op] for op in UNARY] + [[INPUT, 0, INPUT, 1, op] for op in BINARY] + [[INPUT, 0, INPUT, 1, CONST, 0, SELECT]]
    for code in programs:
        want = evaluate(code, [7.0], [grid_a, grid_b])
        out = pkg.HipStore(k * k, "float64", float("nan"))
        out.copy_select_formula(code, [7.0], [a, b], lens, everything)
        got = get_values(out)
        bad = [(grid_a[i], grid_b[i], got[i], want[i]) for i in range(k * k) if bits(float(got[i])) != bits(float(want[i]))]
        assert not bad, (code, bad[:5])
        for i in range(0, k * k, 7):  # the reduction's values: one cell, 0 + x
            got_t, _ = hs.select_total_formula(code, [7.0], [a, b], lens, [(0, [i // k]), (1, [i % k])])
            assert bits(got_t) == bits(0.0 + float(want[i])), (code, grid_a[i], grid_b[i])


def assert_same_store(x, y):
    assert np.array_equal(x.get_status(), y.get_status())
    assert np.array_equal(x.get_data_f64(), y.get_data_f64(), equal_nan=True)
    assert np.array_equal(x.keys(), y.keys())
    ix, vx = x.to_sparse()
    iy, vy = y.to_sparse()
    assert ix.tobytes() == iy.tobytes() and vx.tobytes() == vy.tobytes()


def test_copy_matches_a_set_value_loop():
    rng = np.random.default_rng(5)
    for trial in range(48):
        ndim = int(rng.integers(1, 5))
        lens = [int(rng.choice([1, 3, 5, 7])) for _ in range(ndim)]
        n = int(np.prod(lens))
        inputs = [random_input(rng, n, DTYPES[(trial + j) % 4], bool(rng.integers(0, 2))) for j in range(2)]
        dst_nan = bool(rng.integers(0, 2))
        dst = pkg.HipStore(n, DTYPES[(trial // 4) % 4], float("nan") if dst_nan else 0.0)
        dst.set_data_f64(np.where(rng.random(n) < 0.5, rng.integers(1, 9, size=n).astype(np.float64), 0.0))
        tracked = trial % 3
        if tracked:
            dst.track_order()
            if tracked == 2:
                for i in rng.permutation(n)[: max(1, n // 3)]:
                    dst.set_value(int(i), float(rng.integers(1, 5)))
        code, consts = FORMULAS[trial % len(FORMULAS)]
        code = [w if not (code[i - 1] == INPUT and w == 2) else 0 for i, w in enumerate(code)]
        as_input = trial % 5 == 0  # the target is one of the inputs (no repeats: every cell is visited once)
        if as_input:
            inputs[1] = dst
        levels = random_levels(rng, lens, allow_missing=False, allow_free=not as_input, max_extra=0 if as_input else 3)
        if as_input:
            levels = [(d, list(dict.fromkeys(e))) for d, e in levels]
        positions = nesting_positions(lens, levels)
        values = formula_terms(code, consts, inputs, positions)
        want = dst.clone()
        for p, v in zip(positions.tolist(), values.tolist()):
            want.set_value(p, v)
        dst.copy_select_formula(code, consts, inputs, lens, levels)
        assert_same_store(dst, want)


def test_copy_of_an_empty_selection_writes_nothing():
    a = pkg.HipStore(6, "float32", 0.0)
    a.set_data_f64(np.arange(6.0))
    before = a.get_data_f64().copy()
    a.copy_select_formula([INPUT, 0, CONST, 0, ADD], [1.0], [a], [2, 3], [(0, []), (1, [0, 1])])
    assert np.array_equal(a.get_data_f64(), before)
