"""tests/variance_reference.py (the NumPy / Python restatement of Cube.variance and Cube.stddev that
tests/test_variance_gpu.py compares the device with) pinned by hand-worked literals, by statistics.pvariance / variance
over Fractions where the data is exactly representable, and by numpy.var within the two-pass bound.  Also the CPU side of
the re-associated form's two cases: on exact-arithmetic data every summation order gives the same bits, on uniform
[1, 2) data the orders differ by far less than the bound the GPU test allows."""
import math
import statistics
import struct
from fractions import Fraction

import numpy as np
import pytest

from variance_reference import COMBOS, moments_of, variance_of, variance_reference, variance_reference_all

NAN, INF = math.nan, math.inf
U = 2.0 ** -53


def bits(x):
    return struct.pack("<d", x)


def one(values, kind=0, ddof=0, type_name="float64", default_is_nan=False, status=None):
    v, s = variance_reference(np.asarray(values, dtype=type_name), status, [len(values)], 0, kind, ddof, type_name, default_is_nan)
    return v[0], int(s[0])


def bound(members):
    """4 (N u + N^2 k^2 u^2): twice the sum of two Chan-Golub-LeVeque two-pass bounds, k^2 = 1 + mean^2 / variance"""
    n, mean, m2 = moments_of(members)
    kappa2 = 1.0 + mean * mean / (m2 / n)
    return 4.0 * (n * U + n * n * kappa2 * U * U)


# ---- hand-worked literals ---------------------------------------------------------------------------------------------
EIGHT = [2, 4, 4, 4, 5, 5, 7, 9]  # sum 40, mean 5, squared deviations 9 1 1 1 0 0 4 16 = 32


def test_hand_worked_literals():
    assert bits(variance_of(EIGHT, 0, 0)) == bits(4.0)
    assert bits(variance_of(EIGHT, 1, 0)) == bits(2.0)
    assert bits(variance_of(EIGHT, 0, 1)) == bits(32 / 7)
    assert bits(variance_of(EIGHT, 1, 1)) == bits(math.sqrt(32 / 7))
    assert one(EIGHT) == (4.0, 2) and one(EIGHT, kind=1) == (2.0, 2) and one(EIGHT, ddof=1) == (32 / 7, 2)
    assert one(EIGHT, 0, 0, "int32") == (4, 2) and one(EIGHT, 0, 1, "int32") == (4, 2)  # 4.57 truncates once
    assert one(EIGHT, 0, 1, "float32") == (np.float32(32 / 7), 2)
    assert moments_of([1.0, 2.0, 4.0]) == (3, 7.0 / 3, (1.0 - 7.0 / 3) ** 2 + (2.0 - 7.0 / 3) ** 2 + (4.0 - 7.0 / 3) ** 2)


def test_a_single_member():
    assert bits(variance_of([7.0], 0, 0)) == bits(0.0) and bits(variance_of([7.0], 1, 0)) == bits(0.0)
    assert variance_of([7.0], 0, 1) is None and variance_of([7.0], 1, 1) is None
    assert one([7.0]) == (0.0, 0)  # a variance of 0 is the 0 default: unset
    v, s = one([7.0], default_is_nan=True)  # ... and a SET 0 under the NaN default
    assert (bits(v), s) == (bits(0.0), 2)
    assert one([7.0], ddof=1) == (0.0, 0)
    v, s = one([7.0], ddof=1, default_is_nan=True)
    assert s == 0 and v != v
    assert one([7, 0, 0], 0, 0, "int32") == (0, 0)
    assert one([7, 1, 1], 0, 0, "int32", True, np.array([2, 0, 0], np.int32)) == (0, 2)  # the mask is primary
    assert one([7, 1, 1], 0, 1, "int32", True, np.array([2, 0, 0], np.int32)) == (0, 0)
    assert one([3.0, 3.0, 3.0], 1, 1) == (0.0, 0)  # equal members: 0
    v, s = one([3.0, 3.0, 3.0], 1, 1, default_is_nan=True)
    assert (bits(v), s) == (bits(0.0), 2)


def test_unset_cells_are_no_members():
    assert one([0, 0, 0]) == (0.0, 0)  # all unset under the 0 default
    v, s = one([NAN, NAN], default_is_nan=True)
    assert s == 0 and v != v
    assert one([0, 3, 0, 1, 0]) == (1.0, 2)  # members 3, 1: mean 2
    assert one([0, 3, 0, 1, 0], ddof=1) == (2.0, 2)
    assert one([5, 3, 9], 0, 0, "int32", True, np.array([2, 0, 2], np.int32)) == (4, 2)  # 3 is no member
    v, s = variance_reference(np.zeros(0, np.float32), None, [2, 0, 3], 1, 0, 0, "float32", False)
    assert v.tolist() == [0.0] * 6 and s.tolist() == [0] * 6  # a dimension without items: every group is empty
    v, s = variance_reference(np.array([1, 3, 3, 7], np.float32), None, [4], 0, 0, 0, "float32", False, [0, 0, 2, 2], 4)
    assert v.tolist() == [1.0, 0.0, 4.0, 0.0] and s.tolist() == [2, 0, 2, 0]  # groups nobody maps to
    v, s = variance_reference(np.array([1, 3, 3, 7], np.float32), None, [4], 0, 1, 1, "float32", False, [0, 2, 0, 2], 3)
    assert v.tolist() == [np.float32(math.sqrt(2.0)), 0.0, np.float32(math.sqrt(8.0))] and s.tolist() == [2, 0, 2]  # interleaved


def test_special_values():
    for kind in (0, 1):
        for members in ([INF, 1, 2], [-INF, 1, 2], [INF, -INF], [1, NAN, 2]):
            v, s = one(members, kind)  # a set NaN under the 0 default, and the one quiet NaN
            assert s == 2 and bits(v) == bits(np.nan), members
            if INF in members or -INF in members:
                v, s = one(members, kind, default_is_nan=True)  # NaN is the default: unset
                assert s == 0 and bits(v) == bits(np.nan)
    assert one([1, NAN, 2], default_is_nan=True) == (0.25, 2)  # a NaN cell under the NaN default is no member
    assert one([-0.0, 0.0])[1] == 0  # both equal the 0 default
    v, s = one([-0.0, -0.0, 0.0], default_is_nan=True)  # members under the NaN default: variance +0, set
    assert (bits(v), s) == (bits(0.0), 2)
    assert one([1e200, -1e200]) == (INF, 2)  # the squares overflow
    assert one([1e200, -1e200], kind=1) == (INF, 2)
    a, b = float(np.float32(0.1)), float(np.float32(0.7))
    v, s = one([np.float32(0.1), np.float32(0.7)], 1, 1, "float32")  # rounded to Float32 once, from the float64 result
    mean = (a + b) / 2
    assert v == np.float32(math.sqrt(((a - mean) * (a - mean) + (b - mean) * (b - mean)) / 1))


def test_a_large_common_offset_does_not_cancel():
    members = [1e9 + k for k in range(8)]  # E[x^2] - mean^2 loses every digit here
    assert variance_of(members, 0, 0) == 5.25 and variance_of(members, 0, 1) == 6.0
    naive = sum(x * x for x in members) / 8 - (sum(members) / 8) ** 2
    assert naive != 5.25


def test_integer_cells_convert_the_result_once():
    assert one([1, 2], 0, 0, "int32") == (0, 0)  # 0.25 truncates to the default
    assert one([1, 2], 0, 0, "int32", True, np.array([2, 2], np.int32)) == (0, 2)
    assert one([-5, 5], 0, 0, "int32") == (25, 2) and one([-5, 5], 1, 1, "int32") == (7, 2)  # sqrt(50) = 7.07
    assert one([2 ** 32 - 1, 2 ** 32 - 5], 0, 0, "uint32") == (4, 2)
    big = one([-(2 ** 31), 2 ** 31 - 1], 0, 0, "int32")  # (2^32 - 1)^2 / 4 wraps as ToInt32 wraps
    want = int(variance_of([-(2.0 ** 31), 2.0 ** 31 - 1]))
    assert big[0] == ((want + 2 ** 31) % 2 ** 32) - 2 ** 31


# ---- against statistics over Fractions, and numpy.var ----------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 8, 64, 257])
def test_exactly_representable_data_gives_the_rational_result_rounded_once(n):
    """dyadic members and a power-of-two count: sum, mean, deviations, squares and their sum are exact, so the result is
    the exact variance, rounded by the one division (ddof 1) or not at all"""
    rng = np.random.default_rng(n)
    count = 1 << (n.bit_length() - 1)
    for trial in range(10):
        members = (rng.integers(-64, 64, size=count) / 8.0).tolist()
        fr = [Fraction(x) for x in members]
        assert bits(variance_of(members, 0, 0)) == bits(float(statistics.pvariance(fr)))
        assert bits(variance_of(members, 0, 1)) == bits(float(statistics.variance(fr)))
        assert bits(variance_of(members, 1, 0)) == bits(math.sqrt(float(statistics.pvariance(fr))))


@pytest.mark.parametrize("n", [2, 5, 31, 100, 1000])
def test_numpy_var_within_the_two_pass_bound(n):
    rng = np.random.default_rng(n)
    for members in (rng.random(n) + 1.0, rng.normal(size=n) * 100, 1e6 + rng.random(n)):
        tol = bound(members)
        for ddof in (0, 1):
            got, want = variance_of(members, 0, ddof), float(np.var(members, ddof=ddof))
            assert abs(got - want) <= tol * want, (n, ddof, got, want)
            assert abs(variance_of(members, 1, ddof) - float(np.std(members, ddof=ddof))) <= tol * math.sqrt(want)
    cube = rng.integers(1, 9, size=(3, n, 4)).astype(np.float32)
    for (kind, ddof), (v, s) in variance_reference_all(cube.ravel(), None, [3, n, 4], 1, "float32", True).items():
        want = np.var(cube.astype(np.float64), axis=1, ddof=ddof)
        want = np.sqrt(want) if kind else want
        assert np.allclose(v.reshape(3, 4), want, rtol=1e-6) and s.tolist() == [2] * 12


# ---- the re-associated form's data, on the CPU -----------------------------------------------------------------------
def orders(members):
    """the same two passes with the additions grouped differently: reversed, in 256 strided partial sums added by a
    butterfly (what a workgroup per output cell does), pairwise"""
    v = np.asarray(members, dtype=np.float64)

    def strided(x):
        lanes = [math.fsum([]) for _ in range(256)]
        first = [True] * 256
        for j, e in enumerate(x.tolist()):
            lanes[j % 256] = e if first[j % 256] else lanes[j % 256] + e
            first[j % 256] = False
        lanes = np.array(lanes).reshape(4, 64)
        d = 1
        while d < 64:
            lanes = lanes + lanes[:, np.arange(64) ^ d]
            d <<= 1
        return float(((lanes[0, 0] + lanes[1, 0]) + lanes[2, 0]) + lanes[3, 0])

    def pairwise(x):
        return float(x[0]) if len(x) == 1 else pairwise(x[: len(x) // 2]) + pairwise(x[len(x) // 2:])

    def backwards(x):
        s = 0.0
        for e in x[::-1].tolist():
            s += e
        return s

    results = []
    for add in (backwards, strided, pairwise):
        mean = add(v) / len(v)
        d = v - mean
        results.append(add(d * d) / len(v))
    return results


@pytest.mark.parametrize("n", [4096, 8192])
def test_exact_arithmetic_data_gives_the_same_bits_in_any_order(n):
    rng = np.random.default_rng(n)
    for low in (-8, 0):
        members = rng.integers(low, low + 16, size=n).astype(np.float64)
        want = variance_of(members)
        assert all(bits(r) == bits(want) for r in orders(members))
        assert bits(float(np.var(members))) == bits(want)


def test_uniform_data_differs_between_orders_by_far_less_than_the_bound():
    rng = np.random.default_rng(5000)
    members = rng.random(5000) + 1.0
    want = variance_of(members)
    tol = bound(members)
    assert 1e-12 < tol < 4e-12  # about 2.2e-12 here
    worst = max(abs(r - want) / want for r in orders(members))
    assert worst <= 1e-14 < tol  # measured: a few 1e-15
    dropped = variance_of(np.delete(members, members.argmax()))  # what a lost member does: about 4e-4
    assert abs(dropped - want) / want > 1e6 * tol
    assert COMBOS == ((0, 0), (0, 1), (1, 0), (1, 1))
