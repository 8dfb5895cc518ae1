"""The formula interpreter's library opcodes (ROUND, POW, ROUNDTO, HYPOT, ATAN2, CBRT, EXP, LN, LOG10, LOG2, SIN, COS, TAN,
ASIN, ACOS, ATAN, and MOD at large ratios) against tests/formula_reference.py, which shares no code with the kernels and
is pinned to V8 by tests/test_formula_reference.py.  Inputs are Float64 stores with a NaN default (they keep -0 and every
bit); the result is the float64 cube of olap_store_eval_formula.

A result that the reference gives as NaN, an infinity or a zero must be exactly that, sign included.  ROUND, MOD and
ROUNDTO (digits NaN, -0, -22 .. 22, +-400) are exact operations and must match bit for bit, and so must integer powers
and 10^k.  Everywhere else the bound is the 1e-12 of tests/js/gpu_test.js as a pure relative error (1e-12 * 2^-1022
absolute where the result is subnormal): some 4 500 ulp, which catches a wrong function, a wrong special case, a float32
routine, a broken range reduction or cancellation, and is not the accuracy claim.  The accuracy is measured by
tools/formula_ulp.py (profiles/formula_ulp_r33.txt, NOTEBOOK.md): at most 1.3 ulp (ATAN, ATAN2, POW) over these sweeps.

olap_store_copy_select_formula refuses -1 entries, so the cell that does not exist (formula_at_missing) is reached through
olap_formula_select_total."""
import ctypes as C
import math

import numpy as np
import pytest

import formula_cases as fc
import formula_reference as fr
from conftest import load_package

pytestmark = pytest.mark.gpu

pkg = load_package()
capi = pkg.capi
hs = pkg.hipstore
NAN = math.nan

# opcodes (js/formula.js OP, csrc FormulaOp)
CONST, INPUT, SCALAR, ADD, SUB, MUL, DIV, MOD, POW, NEG, NANADD, SELECT, MIN, MAX, ATAN2, HYPOT, ROUNDTO, ISNAN = range(18)
ABS, CEIL, FLOOR, ROUND, TRUNC, SQRT, CBRT, EXP, LN, LOG10, LOG2, SIGN, SIN, COS, TAN, ASIN, ACOS, ATAN, NOT = range(20, 39)
ALL_UNARY = [NEG, ISNAN] + list(range(ABS, NOT + 1))
ALL_BINARY = [ADD, SUB, MUL, DIV, MOD, POW, NANADD, MIN, MAX, ATAN2, HYPOT, ROUNDTO]
OPS = fr.UNARY_OPS + fr.BINARY_OPS
IDS = [fr.NAMES[o] for o in OPS]
BIT_FOR_BIT = (ROUND, MOD)


def store_of(values):
    s = pkg.HipStore(len(values), "float64", NAN)
    s.set_data_f64(np.asarray(values, np.float64))
    return s


def eval_formula(code, consts, inputs, scalars=()):
    """olap_store_eval_formula: the float64 cube the host path carries"""
    prog = hs._formula(code, consts, inputs)
    sc = (C.c_double * max(len(scalars), 1))(*scalars)
    out = np.zeros(inputs[0].size, np.float64)
    capi.check(capi.lib().olap_store_eval_formula(*prog[:-1], sc, len(scalars), out.ctypes.data_as(capi._pdbl)))
    return out


def program(op, n_args):
    """op(a), op(a, b), or the left fold op(op(a, b), c) as formula.js lowers hypot(a, b, c)"""
    code = [INPUT, 0] + ([op] if n_args == 1 else [])
    for k in range(1, n_args):
        code += [INPUT, k, op]
    return code


def opcodes(code):
    """the program's opcodes, without the operand words of CONST / INPUT / SCALAR"""
    out, pc = [], 0
    while pc < len(code):
        out.append(code[pc])
        pc += 2 if code[pc] <= SCALAR else 1
    return out


def run(op, arrays):
    return eval_formula(program(op, len(arrays)), [], [store_of(x) for x in arrays])


def get_values(store):
    data, st = store.get_data_f64(), store.get_status()
    return np.where((st & 2) != 0, data, NAN if store.default_is_nan else 0.0)


def check(op, got, want, arrays, exact_bits):
    """prints the largest relative error, then asserts class and sign, the bound, and bit equality where it is due"""
    with np.errstate(all="ignore"):
        rel = np.abs(got - want) / np.maximum(np.abs(want), fc.MIN_NORMAL)
    rel = np.where(np.isfinite(want) & (want != 0) & np.isfinite(got), rel, 0.0)
    i = int(np.argmax(rel))
    print("%s: largest relative error %.3g at %r" % (fr.NAMES.get(op, op), rel[i], [float(x[i]) for x in arrays]))
    ok = fc.same_bits(got, want) if exact_bits else fc.within_bound(got, want)
    assert ok.all(), (fr.NAMES.get(op, op), int((~ok).sum()), fc.failures(ok, got, want, *arrays))


# ------------------------------------------------------------------------------------------------ a. the specials grid
def test_the_grid_extends_the_exact_opcodes_specials():
    from test_select_formula_gpu import SPECIALS

    assert fc.same_bits(np.array(fc.SPECIALS[: len(SPECIALS)]), np.array(SPECIALS)).all() and len(set(fc.bits(np.array(fc.SPECIALS)).tolist())) == len(fc.SPECIALS)


@pytest.mark.parametrize("op", OPS, ids=IDS)
def test_specials_grid(op):
    arrays = fc.grid() if op in fr.BINARY_OPS else (np.array(fc.SPECIALS),)
    check(op, run(op, arrays), fc.rounded(fc.grid_exact(op)), arrays, op in BIT_FOR_BIT)


def test_round_to_at_every_kind_of_digits():
    a, d = fc.roundto_grid()
    want = np.array([fr.reference(ROUNDTO, x, y) for x, y in zip(a.tolist(), d.tolist())])
    check(ROUNDTO, run(ROUNDTO, (a, d)), want, (a, d), True)


# ------------------------------------------------------------------ b. results that the specification makes exact
def test_integer_powers_are_exact():
    """x^y for integers: one wrong bit turns 2 ^ n, stored into an Int32 measure, into 2^n - 1"""
    pairs = [(x, y) for x in range(-12, 13) for y in range(41) if abs(x ** y) < 2 ** 48]
    x, y = (np.array([p[i] for p in pairs], np.float64) for i in (0, 1))
    check(POW, run(POW, (x, y)), np.array([float(a ** b) for a, b in pairs]), (x, y), True)


def test_powers_of_ten_are_correctly_rounded():
    """10^k, k = -22 .. 22: a wrong 10^-2 flips roundTo at halves"""
    k = np.arange(-22, 23).astype(np.float64)
    ten = np.full(k.size, 10.0)
    check(POW, run(POW, (ten, k)), np.array([float("1e%d" % i) for i in range(-22, 23)]), (ten, k), True)


# ------------------------------------------------------------------------------------------------- c. accuracy sweeps
@pytest.mark.parametrize("op", OPS, ids=IDS)
def test_sweep(op):
    arrays = fc.sweep(op)
    check(op, run(op, arrays), fc.rounded(fc.sweep_exact(op)), arrays, op in BIT_FOR_BIT + (ROUNDTO,))


def test_hypot_of_three_folds_left():
    arrays = fc.hypot3()
    want = np.array([fr.hypot_fold(*xs) for xs in zip(*(x.tolist() for x in arrays))])
    check(HYPOT, run(HYPOT, arrays), want, arrays, False)


# ------------------------------------------------------------------------- d. the other paths compute the same bits
@pytest.fixture(scope="module")
def grid_stores():
    a, b = fc.grid()
    return a, b, store_of(a), store_of(b)


def test_set_formula_and_copy_give_the_cube_bit_for_bit(grid_stores):
    """every opcode through formula_store_kernel (both instantiations) and through FormulaSource, against eval_formula_kernel"""
    a, b, sa, sb = grid_stores
    k = len(fc.SPECIALS)
    everything = [(0, list(range(k))), (1, list(range(k)))]
    programs = [([INPUT, 0, op], ()) for op in ALL_UNARY] + [([INPUT, 0, INPUT, 1, op], ()) for op in ALL_BINARY]
    programs += [([INPUT, 0, INPUT, 1, CONST, 0, SELECT], ()), ([INPUT, 0, CONST, 1, ROUNDTO], ()), ([INPUT, 0, SCALAR, 1, POW], (2.0, NAN)),
                 ([INPUT, 1, SCALAR, 0, HYPOT, INPUT, 0, ROUND, MOD], (-0.0, 0.5))]
    assert {w for code, _s in programs for w in opcodes(code)} == set(range(18)) | set(range(20, 39))  # all 37 opcodes
    consts = [7.0, -2.0]
    for code, scalars in programs:
        cube = eval_formula(code, consts, [sa, sb], scalars)
        target = pkg.HipStore(k * k, "float64", NAN).set_formula(code, consts, [sa, sb], scalars)
        same = fc.same_bits(get_values(target), cube)
        assert same.all(), ("set_formula", code, fc.failures(same, get_values(target), cube, a, b))
        if SCALAR in opcodes(code):
            continue  # a selection's formula reads no totals
        target = pkg.HipStore(k * k, "float64", NAN).copy_select_formula(code, consts, [sa, sb], [k, k], everything)
        same = fc.same_bits(get_values(target), cube)
        assert same.all(), ("copy_select_formula", code, fc.failures(same, get_values(target), cube, a, b))


def test_round_in_both_instantiations_of_the_store_kernel(grid_stores):
    """ROUND alone runs formula_store_kernel<ALL = false>, ROUND next to a library opcode <ALL = true>: both against the
    reference, bit for bit (fmod is exact)"""
    a, b, sa, sb = grid_stores
    rounded = np.array([fr.reference(ROUND, x) for x in a.tolist()])
    plain = get_values(pkg.HipStore(a.size, "float64", NAN).set_formula([INPUT, 0, ROUND], [], [sa, sb]))
    same = fc.same_bits(plain, rounded)
    assert same.all(), fc.failures(same, plain, rounded, a)
    want = np.array([fr.reference(MOD, x, y) for x, y in zip(rounded.tolist(), b.tolist())])
    both = get_values(pkg.HipStore(a.size, "float64", NAN).set_formula([INPUT, 0, ROUND, INPUT, 1, MOD], [], [sa, sb]))
    same = fc.same_bits(both, want)
    assert same.all(), fc.failures(same, both, want, a, b)
    (x,) = fc.sweep(ROUND)
    want = fc.rounded(fc.sweep_exact(ROUND))
    got = get_values(pkg.HipStore(x.size, "float64", NAN).set_formula([INPUT, 0, ROUND], [], [store_of(x)]))
    same = fc.same_bits(got, want)
    assert same.all(), fc.failures(same, got, want, x)


def test_one_to_the_power_of_an_unset_cell_stays_unset():
    """1 ^ a over a NaN default: NaN (C's pow gives 1), at a cell that is unset and at one that does not exist"""
    a = pkg.HipStore(6, "float64", NAN)
    a.set_value(2, 3.0)
    code, consts = [CONST, 0, INPUT, 0, POW], [1.0]
    target = pkg.HipStore(6, "float64", NAN).copy_select_formula(code, consts, [a], [6], [(0, list(range(6)))])
    assert ((target.get_status() & 2) != 0).tolist() == [False, False, True, False, False, False] and target.get_data_f64()[2] == 1.0
    for entries in ([-1], [0], [2, -1]):
        total, _path = hs.select_total_formula(code, consts, [a], [6], [(0, entries)])
        assert math.isnan(total), entries
    assert hs.select_total_formula(code, consts, [a], [6], [(0, [2])])[0] == 1.0
    with pytest.raises(pkg.OlapError):  # a copy has no cell to write a -1 entry to
        pkg.HipStore(6, "float64", NAN).copy_select_formula(code, consts, [a], [6], [(0, [-1])])
