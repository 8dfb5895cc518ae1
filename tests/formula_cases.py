"""The inputs on which the formula interpreter's library opcodes are compared with tests/formula_reference.py, shared by
the V8 check (test_formula_reference.py), the device check (test_formula_ops_gpu.py) and tools/formula_ulp.py: a grid of
special values and, per opcode, a seeded sweep of 4 096 cells at the arguments where math libraries go wrong.  The
reference of each is computed once per process."""
import functools
import math

import numpy as np

import formula_reference as fr
from formula_reference import ACOS, ASIN, ATAN, ATAN2, CBRT, COS, EXP, HYPOT, LN, LOG2, LOG10, MOD, POW, ROUND, ROUNDTO, SIN, TAN

N_SWEEP = 4096
HALF_PI = 1.5707963267948966

# SPECIALS of test_select_formula_gpu.py, then the values at which the library opcodes have a boundary
SPECIALS = [0.0, -0.0, math.inf, -math.inf, math.nan, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-310, -1e-310, 2.0 ** 53 - 1, 2.0 ** 53,
            2.0 ** 53 + 2, -(2.0 ** 53) - 2, 0.49999999999999994, -0.49999999999999994, 0.5, -0.5, 1.5, -2.5, 3.0, -1.0, 7.25, 1e308, 2.0,
            1.0, -2.0, 10.0, -10.0, HALF_PI, -HALF_PI, 709.78, 709.79, -745.13, -745.14, 1e22, 2.0 ** 1023, 2.0 ** 52 + 1, -(2.0 ** 52 + 1),
            0.9999999999999999, 1.0000000000000002, 0.1, -0.2, 2.5]
ROUNDTO_DIGITS = [math.nan, -0.0, -3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0, 400.0, -400.0]

REL_BOUND = 1e-12  # tests/js/gpu_test.js's figure, as a relative error
MIN_NORMAL = 2.0 ** -1022


def grid():
    """(a, b): every pair of SPECIALS"""
    s = np.array(SPECIALS)
    return np.repeat(s, s.size), np.tile(s, s.size)


def roundto_grid():
    s, d = np.array(SPECIALS), np.array(ROUNDTO_DIGITS)
    return np.repeat(s, d.size), np.tile(d, s.size)


def _parts(n, k):
    return [n // k + (1 if i < n % k else 0) for i in range(k)]


def _signs(rng, n):
    return np.where(rng.random(n) < 0.5, -1.0, 1.0)


def _pow_pairs(rng):
    n = _parts(N_SWEEP, 4)
    a = [rng.uniform(0, 10, n[0]), 10.0 ** rng.uniform(-100, 100, n[1]), 1.0 + rng.uniform(-1e-6, 1e-6, n[2]),
         -rng.integers(1, 13, n[3]).astype(np.float64)]
    b = [rng.uniform(-30, 30, n[0]), rng.uniform(-3, 3, n[1]), rng.uniform(-1e8, 1e8, n[2]), rng.integers(-20, 21, n[3]).astype(np.float64)]
    return np.concatenate(a), np.concatenate(b)


def _log_magnitudes(rng):
    n = _parts(N_SWEEP, 3)
    return np.concatenate([10.0 ** rng.uniform(-320, 308, n[0]), 1.0 + rng.uniform(-1e-3, 1e-3, n[1]), rng.uniform(0.5, 2, n[2])])


@functools.lru_cache(maxsize=None)
def sweep(op):
    """the opcode's sweep: a tuple of one or two float64 arrays of N_SWEEP cells"""
    rng = np.random.default_rng(1000 + op)
    if op in (SIN, COS, TAN):
        near = []
        for k in range(1, 201):
            x = fr.to_double(k * fr.mp.pi / 2)
            near += [np.nextafter(x, -math.inf), x, np.nextafter(x, math.inf)]
        n = _parts(N_SWEEP - len(near), 3)
        return (np.concatenate([rng.uniform(-10, 10, n[0]), rng.uniform(-1e6, 1e6, n[1]), _signs(rng, n[2]) * 10.0 ** rng.uniform(6, 300, n[2]),
                                np.array(near)]),)
    if op == EXP:
        return (np.concatenate([rng.uniform(-745, 709.7, N_SWEEP // 2), rng.uniform(-1e-3, 1e-3, N_SWEEP // 2)]),)
    if op in (LN, LOG10, LOG2):
        return (_log_magnitudes(rng),)
    if op == CBRT:
        return (_log_magnitudes(rng) * _signs(rng, N_SWEEP),)
    if op in (ASIN, ACOS):
        h = N_SWEEP // 2
        return (np.concatenate([rng.uniform(-1, 1, h), _signs(rng, h) * (1.0 - 10.0 ** -rng.uniform(1, 16, h))]),)
    if op == ATAN:
        h = N_SWEEP // 2
        return (np.concatenate([rng.uniform(-10, 10, h), _signs(rng, h) * 10.0 ** rng.uniform(-300, 300, h)]),)
    if op == ROUND:
        h = N_SWEEP // 4
        halves = rng.integers(-2 ** 20, 2 ** 20, h).astype(np.float64) + 0.5
        return (np.concatenate([rng.uniform(-10, 10, h), halves, np.nextafter(halves, math.inf), np.nextafter(halves, -math.inf)]),)
    if op in (POW, ATAN2):
        return _pow_pairs(rng)
    if op == HYPOT:
        a, b = _pow_pairs(rng)
        a[:3], b[:3] = [1e300, 3e-320, 1e308], [1e300, 4e-320, 1e-308]
        return a, b
    if op == MOD:
        a = _signs(rng, N_SWEEP) * rng.uniform(1, 10, N_SWEEP) * 10.0 ** rng.uniform(-300, 307, N_SWEEP)
        b = _signs(rng, N_SWEEP) * rng.uniform(1, 10, N_SWEEP) * 10.0 ** rng.uniform(-300, 300, N_SWEEP)
        named = [(1e308, 3.0), (2.0 ** 1023, 10.0), (1e308, 1e-300), (-7.25, 1e-300), (2.0 ** 1023, 5e-324), (-1e308, 2.2250738585072014e-308),
                 (1e22, 0.1), (5e-324, 1e308)]
        for i, (x, y) in enumerate(named):
            a[i], b[i] = x, y
        return a, b
    if op == ROUNDTO:
        return rng.uniform(-1000, 1000, N_SWEEP), rng.integers(-22, 23, N_SWEEP).astype(np.float64)
    raise KeyError(op)


def hypot3():
    """512 triples for hypot(a, b, c), folded from the left"""
    a, b = sweep(HYPOT)
    return a[:512], b[:512], a[512:1024][::-1].copy()


def _exact(op, arrays):
    return [fr.exact(op, *xs) for xs in zip(*(x.tolist() for x in arrays))]


@functools.lru_cache(maxsize=None)
def sweep_exact(op):
    return _exact(op, sweep(op))


@functools.lru_cache(maxsize=None)
def grid_exact(op):
    return _exact(op, grid() if op in fr.BINARY_OPS else (np.array(SPECIALS),))


def rounded(exact_values):
    return np.array([fr.to_double(v) for v in exact_values], np.float64)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same_bits(got, want):
    """cell by cell: the same bits, or both NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def within_bound(got, want):
    """cell by cell: `got` is `want` where that is NaN, an infinity or a zero (sign included); elsewhere |got - want| is within
    REL_BOUND of |want|, or of the smallest normal number where `want` is subnormal"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    special = np.isnan(want) | np.isinf(want) | (want == 0)
    with np.errstate(all="ignore"):
        close = np.abs(got - want) <= REL_BOUND * np.maximum(np.abs(want), MIN_NORMAL)
    return np.where(special, same_bits(got, want), close & np.isfinite(got))


def failures(ok, got, want, *inputs, limit=6):
    """the first few cells where `ok` is false, readable in an assertion message"""
    bad = np.flatnonzero(~ok)
    return [tuple(float(x[i]) for x in inputs) + (float(got[i]), float(want[i])) for i in bad[:limit]]
