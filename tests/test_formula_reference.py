"""tests/formula_reference.py against V8: the reference the device's library opcodes are held to computes what
js/formula.js's evaluate() computes.  On the grid of special values the two agree in class and sign (NaN, the infinities,
the zeros) and bit for bit wherever ECMA-262 fixes the result (round, roundTo, %, integer powers); on the sweeps V8's
Math stays within 4 ulp of the correctly rounded value (measured with node 12 on these inputs: log10 1.7 ulp, hypot 1.7,
atan2 1.1, everything else below 0.9), which no wrong function, rule or sign would."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import formula_cases as fc
import formula_reference as fr

HERE = os.path.dirname(os.path.abspath(__file__))
NODE = shutil.which("node")

V8 = {fr.ROUND: "round", fr.CBRT: "cbrt", fr.EXP: "exp", fr.LN: "log", fr.LOG10: "log10", fr.LOG2: "log2", fr.SIN: "sin", fr.COS: "cos",
      fr.TAN: "tan", fr.ASIN: "asin", fr.ACOS: "acos", fr.ATAN: "atan", fr.MOD: "f:a % b", fr.POW: "f:a ^ b", fr.ATAN2: "atan2",
      fr.HYPOT: "hypot", fr.ROUNDTO: "f:roundTo(a, b)"}
BIT_FOR_BIT = (fr.ROUND, fr.MOD, fr.ROUNDTO)
OPS = fr.UNARY_OPS + fr.BINARY_OPS
MAX_ULPS = 4.0


def integer_powers():
    pairs = [(x, y) for x in range(-12, 13) for y in range(41) if abs(x ** y) < 2 ** 48]
    return np.array([p[0] for p in pairs], np.float64), np.array([p[1] for p in pairs], np.float64), np.array([float(x ** y) for x, y in pairs])


def powers_of_ten():
    k = np.arange(-22, 23).astype(np.float64)
    return np.full(k.size, 10.0), k, np.array([float("1e%d" % i) for i in range(-22, 23)])  # a decimal literal is correctly rounded


def hexes(x):
    return ["%016x" % v for v in fc.bits(x).tolist()]


@pytest.fixture(scope="module")
def v8():
    """every job in one node process: name -> float64 array"""
    if NODE is None:
        pytest.skip("node is not installed")
    jobs = {}
    for op in OPS:
        jobs["grid", op] = (V8[op], fc.grid() if op in fr.BINARY_OPS else (np.array(fc.SPECIALS),))
        jobs["sweep", op] = (V8[op], fc.sweep(op))
    jobs["pow()"] = ("f:pow(a, b)", fc.grid())
    jobs["Math.pow"] = ("pow", fc.grid())
    jobs["roundTo digits"] = ("f:roundTo(a, b)", fc.roundto_grid())
    jobs["integer powers"] = ("f:a ^ b", integer_powers()[:2])
    jobs["powers of ten"] = ("f:a ^ b", powers_of_ten()[:2])
    jobs["hypot3"] = ("f:hypot(a, b, c)", fc.hypot3())
    names = list(jobs)
    doc = json.dumps([{"fn": jobs[k][0], "args": [hexes(x) for x in jobs[k][1]]} for k in names])
    r = subprocess.run([NODE, os.path.join(HERE, "js", "dump_math.js")], input=doc, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return {k: np.array([int(h, 16) for h in col], np.uint64).view(np.float64) for k, col in zip(names, json.loads(r.stdout))}


def worst_ulps(got, exact_values):
    errs = [fr.ulps(g, e) for g, e in zip(got.tolist(), exact_values)]
    i = int(np.argmax(errs))
    return errs[i], i


@pytest.mark.parametrize("op", OPS, ids=[fr.NAMES[o] for o in OPS])
def test_specials_grid(v8, op):
    got = v8["grid", op]
    exact = fc.grid_exact(op)
    want = fc.rounded(exact)
    inputs = fc.grid() if op in fr.BINARY_OPS else (np.array(fc.SPECIALS),)
    classes = np.array([fr.classify(g) == fr.classify(w) for g, w in zip(got.tolist(), want.tolist())])
    assert classes.all(), (fr.NAMES[op], fc.failures(classes, got, want, *inputs))
    if op in BIT_FOR_BIT:
        same = fc.same_bits(got, want)
        assert same.all(), (fr.NAMES[op], fc.failures(same, got, want, *inputs))
    worst, i = worst_ulps(got, exact)
    assert worst <= MAX_ULPS, (fr.NAMES[op], worst, [float(x[i]) for x in inputs], float(got[i]), float(want[i]))


def test_pow_by_all_three_spellings(v8):
    """a ^ b, pow(a, b) and Math.pow are one function"""
    assert fc.same_bits(v8["grid", fr.POW], v8["pow()"]).all() and fc.same_bits(v8["grid", fr.POW], v8["Math.pow"]).all()


def test_round_to_over_the_digits_the_device_test_uses(v8):
    a, d = fc.roundto_grid()
    want = np.array([fr.reference(fr.ROUNDTO, x, y) for x, y in zip(a.tolist(), d.tolist())])
    same = fc.same_bits(v8["roundTo digits"], want)
    assert same.all(), fc.failures(same, v8["roundTo digits"], want, a, d)
    assert fr.reference(fr.ROUNDTO, 2.5, math.nan) == 3.0 and fr.reference(fr.ROUNDTO, 1.005, 2.0) == 1.0  # 1.005 * 100 = 100.49999999999999


def test_integer_powers_are_exact(v8):
    x, y, want = integer_powers()
    for got in (v8["integer powers"], np.array([fr.reference(fr.POW, a, b) for a, b in zip(x.tolist(), y.tolist())])):
        same = fc.same_bits(got, want)
        assert same.all(), fc.failures(same, got, want, x, y)
    # 10^k: the reference is the correctly rounded value throughout, and so is V8 where the result is an integer.  Below 1
    # ECMA-262 leaves the last bit to the implementation: node 12's V8 is one ulp off at k = -4, -5 and a few more.
    x, k, want = powers_of_ten()
    ref = np.array([fr.reference(fr.POW, 10.0, b) for b in k.tolist()])
    assert fc.same_bits(ref, want).all()
    got = v8["powers of ten"]
    same = fc.same_bits(got, want) | (k < 0)
    assert same.all(), fc.failures(same, got, want, x, k)
    assert max(fr.ulps(g, w) for g, w in zip(got.tolist(), want.tolist())) <= 1.0


@pytest.mark.parametrize("op", OPS, ids=[fr.NAMES[o] for o in OPS])
def test_sweep_within_4_ulps(v8, op):
    got = v8["sweep", op]
    exact = fc.sweep_exact(op)
    if op in BIT_FOR_BIT:
        want = fc.rounded(exact)
        same = fc.same_bits(got, want)
        if op == fr.ROUNDTO:  # V8's own 10^k is only certain to be the correctly rounded one where it is an integer
            same = same | (fc.sweep(op)[1] < 0)
        assert same.all(), (fr.NAMES[op], fc.failures(same, got, want, *fc.sweep(op)))
    worst, i = worst_ulps(got, exact)
    print("%s: V8 is within %.2f ulp of the reference (at %r)" % (fr.NAMES[op], worst, [float(x[i]) for x in fc.sweep(op)]))
    assert worst <= MAX_ULPS, (fr.NAMES[op], worst, [float(x[i]) for x in fc.sweep(op)], float(got[i]))


def test_hypot_of_three_is_the_fold_of_two(v8):
    a, b, c = fc.hypot3()
    errs = [fr.ulps(g, fr.hypot_fold(x, y, z)) for g, x, y, z in zip(v8["hypot3"].tolist(), a.tolist(), b.tolist(), c.tolist())]
    assert max(errs) <= MAX_ULPS, max(errs)


def test_the_rules_the_device_used_to_miss():
    """spot checks of the reference itself, readable without node"""
    nan, inf = math.nan, math.inf
    for b, e in ((1.0, nan), (1.0, inf), (1.0, -inf), (-1.0, inf), (-1.0, -inf), (nan, 1.0), (-8.0, 1 / 3)):
        assert math.isnan(fr.reference(fr.POW, b, e)), (b, e)
    assert fr.reference(fr.POW, nan, 0.0) == 1.0 and fr.reference(fr.POW, nan, -0.0) == 1.0
    assert fr.classify(fr.reference(fr.POW, -0.0, 3.0)) == "-0" and fr.reference(fr.POW, -0.0, -3.0) == -inf and fr.reference(fr.POW, -0.0, -2.0) == inf
    assert fr.reference(fr.POW, -inf, -3.0) == 0 and fr.classify(fr.reference(fr.POW, -inf, -3.0)) == "-0"
    for x, want in ((0.49999999999999994, "+0"), (-0.2, "-0"), (-0.5, "-0"), (-0.0, "-0"), (0.0, "+0")):
        assert fr.classify(fr.reference(fr.ROUND, x)) == want, x
    assert fr.reference(fr.ROUND, 2.0 ** 52 + 1) == 2.0 ** 52 + 1 and fr.reference(fr.ROUND, 2.5) == 3.0 and fr.reference(fr.ROUND, -2.5) == -2.0
    assert fr.reference(fr.HYPOT, nan, -inf) == inf and math.isnan(fr.reference(fr.HYPOT, nan, 1.0))
    assert fr.reference(fr.ATAN2, 0.0, -0.0) == math.pi and fr.reference(fr.ATAN2, -0.0, -1.0) == -math.pi
    assert fr.classify(fr.reference(fr.ATAN2, -0.0, 0.0)) == "-0" and fr.reference(fr.ATAN2, inf, -inf) == 3 * math.pi / 4
    assert fr.reference(fr.LN, -0.0) == -inf and math.isnan(fr.reference(fr.LN, -1.0)) and math.isnan(fr.reference(fr.ASIN, 1.0000000000000002))
    assert fr.reference(fr.MOD, 1e308, 3.0) == 2.0 and fr.classify(fr.reference(fr.MOD, -6.0, 3.0)) == "-0" and fr.reference(fr.MOD, 5.0, inf) == 5.0
    assert fr.ulps(1.0000000000000002, 1.0) == 1.0 and fr.ulps(math.nan, math.nan) == 0.0 and fr.ulps(0.0, -0.0) == inf
