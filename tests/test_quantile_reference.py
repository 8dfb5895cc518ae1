"""tests/quantile_reference.py (the NumPy restatement of Cube.quantile that tests/test_quantile_gpu.py compares the device
with) pinned by hand-worked literals and, where float64 arithmetic is exact, by numpy.quantile(method="linear").  No
tolerance anywhere."""
import math
import struct

import numpy as np
import pytest

from quantile_reference import quantile_of, quantile_reference, sort_key

NAN, INF = math.nan, math.inf


def bits(x):
    return struct.pack("<d", x)


def one(values, q, type_name="float64", default_is_nan=False, status=None):
    v, s = quantile_reference(np.asarray(values, dtype=type_name), status, [len(values)], 0, q, type_name, default_is_nan)
    return v[0], int(s[0])


def test_the_order_is_the_total_order_with_every_nan_last():
    values = [NAN, 1.0, -0.0, 0.0, -INF, -NAN, INF, -1.0, 5e-324, -5e-324]
    got = sorted(values, key=sort_key)
    assert [bits(x) for x in got[:8]] == [bits(x) for x in (-INF, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, INF)]
    assert all(x != x for x in got[8:])
    assert sort_key(NAN) == sort_key(-NAN) == 2 ** 64 - 1 > sort_key(INF)


@pytest.mark.parametrize("members,q,want", [
    ([7.0], 0, 7.0), ([7.0], 0.3, 7.0), ([7.0], 1, 7.0),
    ([4.0, 2.0], 0, 2.0), ([4.0, 2.0], 0.25, 2.5), ([4.0, 2.0], 0.5, 3.0), ([4.0, 2.0], 1, 4.0),
    ([4.0, 2.0], 0.3, 2.6), ([4.0, 2.0], 0.9, 3.8),  # h = 0.3: 2 + 0.3 * 2; h = 0.9: 2 + 0.9 * 2
    ([9.0, 1.0, 5.0], 0, 1.0), ([9.0, 1.0, 5.0], 0.25, 3.0), ([9.0, 1.0, 5.0], 0.5, 5.0), ([9.0, 1.0, 5.0], 1, 9.0),
    ([9.0, 1.0, 5.0], 0.3, 1.0 + 0.6 * 4.0),  # h = 0.6, lo = 0
    ([9.0, 1.0, 5.0], 0.9, 5.0 + (1.8 - 1) * 4.0),  # h = 1.8, lo = 1, frac = 0.8 as 1.8 - 1 rounds it
    ([0.1, 0.7], 0.3, 0.28), ([0.7, 0.1], 0.3, 0.28),  # fused: 0.27999999999999997
    ([2.0, 2.0, 2.0, 5.0], 0.5, 2.0), ([2.0, 2.0, 5.0, 5.0], 0.5, 3.5),  # ties
])
def test_hand_worked_quantiles(members, q, want):
    assert bits(quantile_of(members, q)) == bits(want)


def test_the_fused_result_differs():
    """the case of the issue in exact rational arithmetic: the unfused chain rounds three times, a fused one twice"""
    from fractions import Fraction as F
    lo, hi, q = 0.1, 0.7, 0.3
    h = q * 1
    d = hi - lo
    m = h * d
    assert lo + m == 0.28
    fused = float(F(lo) + F(h) * F(d))  # fma(h, d, lo): one rounding of the exact sum
    assert fused == 0.27999999999999997 != 0.28


def test_unset_cells_are_no_members():
    assert one([0, 0, 0], 0.5) == (0.0, 0)  # all unset under the 0 default
    v, s = one([NAN, NAN], 0.5, default_is_nan=True)
    assert s == 0 and v != v
    assert one([0, 3, 0, 1, 0], 0.5) == (2.0, 2)  # members 1, 3
    assert one([5, 3, 9], 0.5, "int32", True, np.array([2, 0, 2], np.int32)) == (7, 2)  # the mask is primary: 3 is no member
    v, s = quantile_reference(np.zeros(0, np.float32), None, [2, 0, 3], 1, 0.5, "float32", False)
    assert v.tolist() == [0.0] * 6 and s.tolist() == [0] * 6  # a dimension without items: every group is empty
    v, s = quantile_reference(np.array([1, 2, 3, 4], np.float32), None, [4], 0, 0.5, "float32", False, [0, 0, 2, 2], 4)
    assert v.tolist() == [1.5, 0.0, 3.5, 0.0] and s.tolist() == [2, 0, 2, 0]  # groups nobody maps to


def test_special_values():
    assert one([INF, -INF, 1, 2], 0.5, default_is_nan=True) == (1.5, 2)
    v, s = one([INF, -INF], 0.5, default_is_nan=True)  # -inf + 0.5 * inf = NaN = the default: unset
    assert s == 0 and bits(v) == bits(np.nan)
    v, s = one([INF, -INF], 0.5)  # ... a set NaN under the 0 default, and the one quiet NaN
    assert s == 2 and bits(v) == bits(np.nan)
    assert one([INF, -INF], 0) == (-INF, 2) and one([INF, -INF], 1) == (INF, 2)
    v, s = one([1, NAN, 2, 0, 3], 1)  # a NaN member under a 0 default sorts last
    assert s == 2 and v != v
    assert one([1, -NAN, 2, 0, 3], 0.5) == (2.5, 2)  # members 1 2 3 NaN, h = 1.5
    v, s = one([1, NAN, 2, 0, 3], 0.75)
    assert s == 2 and bits(v) == bits(np.nan)
    v, s = one([0.0, -0.0, 0.0], 0, default_is_nan=True)  # -0 before +0 under a NaN default
    assert (bits(v), s) == (bits(-0.0), 2)
    v, s = one([-0.0, 0.0, -0.0], 1, default_is_nan=True)
    assert (bits(v), s) == (bits(0.0), 2)
    assert one([-0.0, 0.0], 0.5)[1] == 0  # both equal the 0 default
    v, s = one([np.float32(0.1), np.float32(0.7)], 0.3, "float32")  # rounded to Float32 once, from the float64 result
    assert v == np.float32(float(np.float32(0.1)) + 0.3 * (float(np.float32(0.7)) - float(np.float32(0.1))))


def test_integer_cells_truncate_the_result_once():
    assert one([1, 2], 0.5, "int32") == (1, 2)  # 1.5
    assert one([-1, -2], 0.5, "int32") == (-1, 2)  # -1.5
    assert one([-1, 1], 0.5, "int32") == (0, 0)  # 0 is the default: unset
    assert one([-1, 1], 0.5, "int32", True, np.array([2, 2], np.int32)) == (0, 2)  # a SET 0 under the NaN default
    assert one([2 ** 32 - 1, 2 ** 32 - 2], 0.5, "uint32") == (2 ** 32 - 2, 2)
    assert one([-(2 ** 31), 2 ** 31 - 1], 0.5, "int32") == (0, 0)  # -0.5
    assert one([1, 2], 0.5, "float64") == (1.5, 2)


@pytest.mark.parametrize("n", [1, 5, 9, 13, 101])
@pytest.mark.parametrize("q", [0, 0.25, 0.5, 0.75, 1])
def test_numpy_quantile_exactly_where_float64_is_exact(n, q):
    """small integers, q a multiple of 1/4, n - 1 a multiple of 4: h is an integer or the interpolation is exact in both"""
    rng = np.random.default_rng(n)
    for trial in range(20):
        members = rng.integers(-50, 50, size=n).astype(np.float64)
        members[members == 0] = 7  # (0 would be unset under the 0 default)
        want = np.quantile(members, q) if np.__version__ < "1.22" else np.quantile(members, q, method="linear")
        assert bits(quantile_of(members, q)) == bits(float(want))
        v, s = one(members, q)
        assert (bits(v), s) == (bits(float(want)), 2) or (want == 0 and s == 0)
    cube = rng.integers(1, 9, size=(3, n, 4)).astype(np.float32)
    v, s = quantile_reference(cube.ravel(), None, [3, n, 4], 1, q, "float32", False)
    assert np.array_equal(v.reshape(3, 4), np.quantile(cube.astype(np.float64), q, axis=1).astype(np.float32)) and s.tolist() == [2] * 12
