"""Plain high-precision references for the filtered total (getTotalForDimensionItems, src/cube.js:679-707) and its
exactness certificate (DESIGN K8), shared by the select tests.  A selection is a list of levels in nesting order,
[(axis, entries), ...]: axis = cube dimension or -1 (a free filter key, which only repeats the product), entries =
item indices (-1 = a cell that does not exist, read as the default)."""
import math
from fractions import Fraction

import numpy as np

# below this many terms the sequential sum is a Python loop; above, np.add.accumulate (also strictly left to right)
_LOOP_MAX = 1 << 16


def nesting_positions(lens, levels):
    """int64 flat position of every combination in nesting order (the first level outermost), -1 where the cell does
    not exist.  A free level repeats the product of the levels inside it."""
    strides = [int(np.prod(lens[d + 1:], dtype=np.int64)) for d in range(len(lens))]
    pos = np.zeros(1, dtype=np.int64)
    missing = np.zeros(1, dtype=bool)
    for axis, entries in levels:
        e = np.asarray(entries, dtype=np.int64).reshape(-1)
        if axis < 0:
            contrib, miss = np.zeros(e.size, dtype=np.int64), np.zeros(e.size, dtype=bool)
        else:
            contrib, miss = np.where(e < 0, 0, e * strides[axis]), e < 0
        pos = (pos[:, None] + contrib[None, :]).reshape(-1)
        missing = (missing[:, None] | miss[None, :]).reshape(-1)
    return np.where(missing, -1, pos)


def split_free(levels):
    """(the dimension levels, m = product of the free levels' lengths): one copy of the terms and how often it repeats"""
    m = 1
    dims = []
    for axis, entries in levels:
        if axis < 0:
            m *= len(entries)
        else:
            dims.append((axis, entries))
    return dims, m


def terms_at(values, default, positions):
    """getValue of every combination as float64 (values: getValue of every cell)"""
    values = np.asarray(values, dtype=np.float64)
    positions = np.asarray(positions, dtype=np.int64)
    if values.size == 0:
        return np.full(positions.size, default, dtype=np.float64)
    return np.where(positions < 0, default, values[np.maximum(positions, 0)])


def sequential_total(values, default, positions):
    """0.0 + x0 + x1 + ... in float64, in nesting order: the reference's `total += getSingleData(...)`.  The leading
    +0.0 is JS's starting value (so an all -0 sum is +0)."""
    v = terms_at(values, default, positions)
    if v.size <= _LOOP_MAX:
        acc = 0.0
        for x in v.tolist():
            acc += x
        return acc
    return float(np.cumsum(np.concatenate([[0.0], v]))[-1])


def _scaled(terms):
    """(E, [(|x| / 2^E as int, sign, count)]) over the distinct non-zero finite terms; E = None when there is none"""
    v = np.asarray(terms, dtype=np.float64).reshape(-1)
    v = v[np.isfinite(v) & (v != 0)]
    uniq, counts = np.unique(v, return_counts=True)
    parts = []
    e_min = None
    for x, c in zip(uniq.tolist(), counts.tolist()):
        n, d = x.as_integer_ratio()  # x = n / 2^k
        k = d.bit_length() - 1
        low = ((n & -n).bit_length() - 1) - k  # exponent of the lowest set bit
        e_min = low if e_min is None else min(e_min, low)
        parts.append((n, k, c))
    if e_min is None:
        return None, []
    out = []
    for n, k, c in parts:
        shift = -k - e_min  # n * 2^-k / 2^E, an integer since E <= the lowest set bit of n * 2^-k
        a = abs(n) << shift if shift >= 0 else abs(n) >> -shift
        out.append((a, 1 if n > 0 else -1, c))
    return e_min, out


def exact_total(terms):
    """the exact sum of the terms as a Fraction, or None when a NaN or an infinity is present"""
    v = np.asarray(terms, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(v)):
        return None
    e, parts = _scaled(v)
    if e is None:
        return Fraction(0)
    return Fraction(sum(s * a * c for a, s, c in parts)) * Fraction(2) ** e


def predict_path(terms, m):
    """K8 restated in exact arithmetic: "device" when the order-free total is certified, else "sequential".  `terms` is
    one copy of the selection's values (the free levels removed); the free levels repeat it m times.

    The prediction does not depend on the device's order of addition.  Let A be the exact sum of |x| over the finite
    terms and E the exponent of their lowest set mantissa bit, so that every term is a multiple of 2^E.  While
    A < 2^(53+E), every partial sum of |x|, in any order, is a multiple of 2^E below 2^(53+E), hence representable:
    the device's computed A is exactly A.  Once the exact A reaches 2^(53+E), the computed A does too, because
    rounding is monotone: the partial sums are exact until one first reaches 2^(53+E), which is representable, so
    it rounds to at least 2^(53+E), and adding further |x| never decreases it.  Such an A fails the bound 2^(52+E)
    whatever m is, so the answer is "sequential" in exact and in device arithmetic alike."""
    v = np.asarray(terms, dtype=np.float64).reshape(-1)
    nan = bool(np.isnan(v).any())
    pos_inf, neg_inf = bool((v == math.inf).any()), bool((v == -math.inf).any())
    if nan or (pos_inf and neg_inf):
        return "device"  # NaN in any order
    e, parts = _scaled(v)
    if e is None:
        return "device"  # no non-zero finite term: 0 or a single-signed inf
    a_int = sum(a * c for a, _, c in parts)  # A / 2^E
    if a_int >= 1 << 53:
        return "sequential"
    try:
        a = math.ldexp(float(a_int), e)  # exact: A is a multiple of 2^E below 2^(53+E)
    except OverflowError:
        a = math.inf
    am = a * m
    if not math.isfinite(am):
        return "sequential"
    if e + 52 <= 1023 and am > math.ldexp(1.0, e + 52):
        return "sequential"
    return "device"


def mulberry_cell_values(cells, seed=20240807):
    """fround(0.5 + u(2*cell + 1)) for arbitrary (64-bit) cell indices: what olap_fill_seeded(code 2, frac 1) writes
    to a Float32 measure, in closed form."""
    cells = np.asarray(cells, dtype=np.uint64)
    a = ((np.uint64(seed) + (np.uint64(2) * cells + np.uint64(1)) * np.uint64(0x6D2B79F5)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    with np.errstate(over="ignore"):
        t = (a ^ (a >> np.uint32(15))) * (np.uint32(1) | a)
        t = (t + ((t ^ (t >> np.uint32(7))) * (np.uint32(61) | t))) ^ t
        r = t ^ (t >> np.uint32(14))
    return (0.5 + r.astype(np.float64) / 4294967296.0).astype(np.float32)
