"""The plain references of tests/select_reference.py on worked cases (no GPU): the certificate predictor (DESIGN K8) at
its bounds, the sequential sum and the nesting order."""
import itertools
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

from select_reference import exact_total, nesting_positions, predict_path, sequential_total, split_free, terms_at


def bits(x):
    return struct.pack("<d", x) if x == x else b"nan"


def f32(x):
    assert float(np.float32(x)) == x
    return x


P = math.ldexp
# (terms, m, path, sequential total): the exact sums were worked out with Fraction
WORKED = [
    ([P(1, 51), P(1, 51) - 1, 1.0], 1, "device", P(1, 52)),
    ([P(1, 51), P(1, 51), 1.0], 1, "sequential", P(1, 52) + 1),
    ([P(1, 52), 1.0, P(1, 52), 1.0], 1, "sequential", P(1, 53)),  # exact: 2^53 + 2
    ([P(1, 40) + 1, P(1, 40) - 1], 2048, "device", None),
    ([P(1, 40) + 1, P(1, 40) - 1], 2049, "sequential", None),
    ([P(1, -1023), P(1, -1074)], 1, "device", None),
    ([P(1, -1022), P(1, -1074)], 1, "sequential", None),
    ([P(1, 1023), -P(1, 1022)], 1, "device", P(1, 1022)),  # E + 52 > 1023
    ([P(1, 1023), P(1, 1022), -P(1, 1022)], 1, "sequential", P(1, 1023)),  # A overflows
    ([P(1, 1023), P(1, 1023), -P(1, 1023)], 1, "sequential", math.inf),  # exact: 2^1023
    ([f32(3 * P(1, -149)), f32(P(1, -127))], 1, "device", None),
    ([f32(P(1, -149)), 1.5], 1, "sequential", None),
    ([float(2 ** 32 - 1)] * (1 << 20), 1, "device", None),
]


@pytest.mark.parametrize("terms, m, path, total", WORKED)
def test_predictor_on_worked_cases(terms, m, path, total):
    assert predict_path(terms, m) == path
    exact = exact_total(terms) * m
    if len(terms) < 100:
        assert exact == sum(Fraction(x) for x in terms) * m
    # the reference's order: the m copies one after the other
    want = sequential_total(np.tile(np.asarray(terms), m), 0.0, np.arange(len(terms) * m))
    if total is not None:
        assert bits(want) == bits(total)
    if path == "device":
        assert want == float(exact)  # the certificate's promise: the sequential sum is the exact one


def test_exact_sums_of_the_worked_cases():
    assert exact_total([P(1, 52), 1.0, P(1, 52), 1.0]) == 2 ** 53 + 2
    assert exact_total([P(1, 1023), P(1, 1023), -P(1, 1023)]) == 2 ** 1023
    assert exact_total([P(1, -1022), P(1, -1074)]) == Fraction(2 ** 52 + 1, 2 ** 1074)
    assert exact_total([1.0, math.nan]) is None and exact_total([math.inf]) is None
    assert exact_total([]) == 0 and exact_total([0.0, -0.0]) == 0


def test_predictor_on_non_finite_and_zero_terms():
    assert predict_path([math.nan, P(1, 60), 1.0], 1) == "device"
    assert predict_path([math.inf, -math.inf, P(1, 60), 1.0], 1) == "device"
    assert predict_path([math.inf, 2.0], 1) == "device"
    assert predict_path([math.inf, P(1, 53), 1.0], 1) == "sequential"  # the finite terms decide
    assert predict_path([0.0, -0.0], 5) == "device" and predict_path([], 1) == "device"
    assert predict_path([1e308], 2) == "sequential"  # A*m overflows
    assert predict_path([-P(1, 52)], 2) == "device"  # E = 52: one term is always exact
    assert predict_path([-P(1, 51), -1.0], 1) == "device" and predict_path([-P(1, 51), -1.0], 2) == "sequential"


def test_signed_zero_and_non_finite_sequential_sums():
    assert bits(sequential_total([-0.0, -0.0], 0.0, [0, 1])) == bits(0.0)
    assert math.isnan(sequential_total([1.0, 2.0], math.nan, [0, -1, 1]))
    big = np.full(100_000, 0.1)
    assert sequential_total(big, 0.0, np.arange(big.size)) == _loop(big)  # (the accumulate path)


def _loop(v):
    acc = 0.0
    for x in v.tolist():
        acc += x
    return acc


def test_nesting_positions_match_itertools():
    rng = np.random.default_rng(1)
    for _ in range(50):
        lens = [int(x) for x in rng.integers(1, 5, size=int(rng.integers(1, 4)))]
        levels = [(d, [int(x) for x in rng.integers(-1, lens[d], size=int(rng.integers(0, 4)))]) for d in rng.permutation(len(lens))]
        if rng.random() < 0.5:
            levels.insert(int(rng.integers(0, len(levels) + 1)), (-1, [0] * int(rng.integers(0, 3))))
        strides = [int(np.prod(lens[d + 1:])) for d in range(len(lens))]
        want = []
        for digits in itertools.product(*[e for _, e in levels]):
            pos = 0
            for (axis, _), e in zip(levels, digits):
                if axis >= 0:
                    pos = -1 if pos < 0 or e < 0 else pos + e * strides[axis]
            want.append(pos)
        assert nesting_positions(lens, levels).tolist() == want, (lens, levels)
        dims, m = split_free(levels)
        assert m * len(nesting_positions(lens, dims)) == len(want)


def test_terms_at_reads_the_default_for_missing_cells():
    assert terms_at([5.0, 6.0], 0.0, [1, -1, 0]).tolist() == [6.0, 0.0, 5.0]
