"""olap_formula_totals (getNestedObject(computed measure, withTotals)) checks its arguments on the host before any
device work — the same codes and messages with and without a GPU — and Cube sends only eligible computed measures to it
(tests/js/formula_totals_host_test.js, with a stubbed addon)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import load_package

pkg = load_package()
capi = pkg.capi
HERE = os.path.dirname(os.path.abspath(__file__))
NODE = shutil.which("node")

CONST, INPUT, SCALAR, ADD = 0, 1, 2, 3


def call(code, n_inputs, inputs, lens=(2, 3), methods=None, n_consts=0, consts=True, values=True, ndim=None):
    c = (C.c_int32 * max(len(code), 1))(*code)
    k = (C.c_double * 1)(0.0) if consts else None
    table = (C.c_void_p * max(len(inputs), 1))(*inputs) if inputs is not None else None
    nd = len(lens) if ndim is None else ndim
    lv = (C.c_uint32 * max(len(lens), 1))(*lens)
    if methods is None:
        methods = [0] * (max(n_inputs, 1) * len(lens))
    m = (C.c_int * max(len(methods), 1))(*methods)
    n = int(np.prod([l + 1 for l in lens], dtype=np.float64)) if len(lens) else 1
    out = (C.c_double * min(max(n, 1), 4096))() if values else None
    launches, nbytes = C.c_int(-1), C.c_uint64(0)
    rc = capi.lib().olap_formula_totals(c, len(code), k, n_consts, n_inputs, table, nd, lv, m, out, C.byref(launches), C.byref(nbytes))
    return rc


def test_symbol_is_bound():
    assert hasattr(capi.lib(), "olap_formula_totals")
    assert callable(pkg.hipstore.formula_totals)


def test_argument_errors_without_stores():
    """Everything that can be refused without looking at a store: the same answers on a machine with no device."""
    assert call([INPUT, 0], 1, None) == capi.ERR_INVALID_ARGUMENT
    assert capi.last_error() == "formula inputs are NULL"
    assert call([INPUT, 0], 1, [None]) == capi.ERR_INVALID_ARGUMENT
    assert capi.last_error() == "formula input 0 is NULL"
    for n_inputs in (0, 9, -1):
        assert call([INPUT, 0], n_inputs, [None] * max(n_inputs, 1)) == capi.ERR_INVALID_ARGUMENT
        assert "needs 1..8 stored measures" in capi.last_error()
    assert call([INPUT, 0, SCALAR, 0, ADD], 1, [None]) == capi.ERR_INVALID_ARGUMENT
    assert "SCALAR" in capi.last_error()
    # check_formula, with its messages
    assert call([INPUT, 3], 1, [None]) == capi.ERR_INDEX_RANGE
    assert capi.last_error() == "formula operand 3 out of range"
    assert call([INPUT, 0, ADD], 1, [None]) == capi.ERR_INVALID_ARGUMENT
    assert capi.last_error() == "formula program underflows its stack"
    assert call([], 1, [None]) == capi.ERR_INVALID_ARGUMENT
    assert "formula program has 0 words" in capi.last_error()
    assert call([INPUT, 0] * 49, 1, [None]) == capi.ERR_INVALID_ARGUMENT  # 98 words
    assert call([INPUT, 0, INPUT, 0], 1, [None]) == capi.ERR_INVALID_ARGUMENT
    assert capi.last_error() == "formula program leaves 2 values on its stack"
    assert call([INPUT, 0, CONST, 0, ADD], 1, [None], n_consts=1, consts=False) == capi.ERR_INVALID_ARGUMENT
    assert capi.last_error() == "formula constants are NULL"


def store_errors(a, b, tracked):
    """every refusal that needs a store handle: [(what, rc, message), ...]"""
    A, B, T = a._h.value, b._h.value, tracked._h.value
    two = [INPUT, 0, INPUT, 1, ADD]
    calls = [
        ("rule code above product", lambda: call([INPUT, 0], 1, [A], methods=[0, 7])),
        ("rule code below sum", lambda: call([INPUT, 0], 1, [A], methods=[-1, 0])),
        ("the second input's rules are checked too", lambda: call(two, 2, [A, A], methods=[0, 0, 0, 9])),
        ("6 cells, dimensions describe 8", lambda: call([INPUT, 0], 1, [A], lens=(2, 4))),
        ("the second input holds 8 cells", lambda: call(two, 2, [A, B])),
        ("17 dimensions", lambda: call([INPUT, 0], 1, [A], lens=(1,) * 17)),
        ("4.9e9 extended cells", lambda: call([INPUT, 0], 1, [A], lens=(70000, 70000))),
        ("no result array", lambda: call([INPUT, 0], 1, [A], values=False)),
        ("tracked input", lambda: call(two, 2, [A, T])),
        ("SCALAR", lambda: call([INPUT, 0, SCALAR, 0, ADD], 1, [A])),
        ("nine inputs", lambda: call([INPUT, 0], 9, [A] * 9)),
    ]
    return [(what, f(), capi.last_error()) for what, f in calls]


EXPECTED_STORE_ERRORS = [
    (capi.ERR_UNSUPPORTED_METHOD, "Unsupported aggregation method: 7"),
    (capi.ERR_UNSUPPORTED_METHOD, "Unsupported aggregation method: -1"),
    (capi.ERR_UNSUPPORTED_METHOD, "Unsupported aggregation method: 9"),
    (capi.ERR_LENGTH_MISMATCH, "6 cells but the dimensions describe 8"),
    (capi.ERR_LENGTH_MISMATCH, "8 cells but the dimensions describe 6"),
    (capi.ERR_INVALID_ARGUMENT, "totals: at most 16 dimensions"),
    (capi.ERR_INVALID_ARGUMENT, "totals: the extended cube would hold"),
    (capi.ERR_INVALID_ARGUMENT, "values is NULL"),
    (capi.ERR_INVALID_ARGUMENT, "ordered:"),
    (capi.ERR_INVALID_ARGUMENT, "SCALAR"),
    (capi.ERR_INVALID_ARGUMENT, "needs 1..8 stored measures"),
]


@pytest.mark.gpu
def test_argument_errors_with_stores_leave_the_inputs_unchanged():
    """Store handles exist only where a device does.  Every refusal comes with the code and message the host checks
    give, leaves the inputs as they were, and the store-free refusals answer as they do without a device."""
    a = pkg.HipStore(6, "float32", 0.0)
    a.set_data_f64(np.arange(6.0))
    b = pkg.HipStore(8, "float32", 0.0)
    t = pkg.HipStore(6, "float32", 0.0)
    capi.check(capi.lib().olap_store_track_order(t._h, 1))
    t.set_data_f64(np.arange(6.0) + 1)
    before = [x.get_data_f64().tobytes() for x in (a, b, t)]
    got = store_errors(a, b, t)
    assert len(got) == len(EXPECTED_STORE_ERRORS)
    for (what, rc, message), (want_rc, want_message) in zip(got, EXPECTED_STORE_ERRORS):
        assert rc == want_rc and want_message in message, (what, rc, message)
    assert [m for w, _, m in got if w == "tracked input"][0].startswith("ordered:")
    test_argument_errors_without_stores()
    assert [x.get_data_f64().tobytes() for x in (a, b, t)] == before
    vals, launches, nbytes = pkg.hipstore.formula_totals([INPUT, 0], [], [a], [2, 3], [["sum", "sum"]])
    assert vals.reshape(3, 4).tolist() == [[0, 1, 2, 3], [3, 4, 5, 12], [3, 5, 7, 15]] and launches == 2


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_cube_eligibility_predicate():
    r = subprocess.run([NODE, os.path.join(HERE, "js", "formula_totals_host_test.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " 0 failed" in r.stdout
