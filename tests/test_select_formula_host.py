"""olap_formula_select_total / olap_store_copy_select_formula check their arguments on the host before any device work
(the same codes with and without a GPU), and js/formula.js isDeviceExact says which formulas take the device route."""
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

INPUT, SCALAR, ADD = 1, 2, 3


def call_total(code, n_inputs, inputs, lens=(2, 3), levels=((0, (0, 1)), (1, (0,)))):
    c = (C.c_int32 * len(code))(*code)
    k = (C.c_double * 1)(0.0)
    table = (C.c_void_p * max(len(inputs), 1))(*inputs) if inputs is not None else None
    lv = (C.c_uint32 * len(lens))(*lens)
    ax = (C.c_int * len(levels))(*[a for a, _ in levels])
    n = (C.c_uint32 * len(levels))(*[len(e) for _, e in levels])
    keep = [(C.c_int32 * max(len(e), 1))(*e) for _, e in levels]
    sel = (C.POINTER(C.c_int32) * len(levels))(*[C.cast(x, C.POINTER(C.c_int32)) for x in keep])
    total, path = C.c_double(), C.c_int()
    return capi.lib().olap_formula_select_total(c, len(code), k, 0, n_inputs, table, len(lens), lv, len(levels), ax, n, sel, C.byref(total),
                                                C.byref(path))


def call_copy(target, code, n_inputs, inputs, lens=(2, 3), levels=((0, (0, 1)), (1, (0,)))):
    c = (C.c_int32 * len(code))(*code)
    k = (C.c_double * 1)(0.0)
    table = (C.c_void_p * max(len(inputs), 1))(*inputs) if inputs is not None else None
    lv = (C.c_uint32 * len(lens))(*lens)
    ax = (C.c_int * len(levels))(*[a for a, _ in levels])
    n = (C.c_uint32 * len(levels))(*[len(e) for _, e in levels])
    keep = [(C.c_int32 * max(len(e), 1))(*e) for _, e in levels]
    sel = (C.POINTER(C.c_int32) * len(levels))(*[C.cast(x, C.POINTER(C.c_int32)) for x in keep])
    return capi.lib().olap_store_copy_select_formula(target, c, len(code), k, 0, n_inputs, table, len(lens), lv, len(levels), ax, n, sel)


def test_argument_errors_without_a_device():
    assert call_total([INPUT, 0], 1, None) == capi.ERR_INVALID_ARGUMENT
    assert capi.last_error() == "formula inputs are NULL"
    assert call_total([INPUT, 0], 1, [None]) == capi.ERR_INVALID_ARGUMENT
    assert capi.last_error() == "formula input 0 is NULL"
    for n_inputs in (0, 9):
        assert call_total([INPUT, 0], n_inputs, [None] * max(n_inputs, 1)) == capi.ERR_INVALID_ARGUMENT
        assert "needs 1..8 stored measures" in capi.last_error()
    assert call_total([INPUT, 0, SCALAR, 0, ADD], 1, [None]) == capi.ERR_INVALID_ARGUMENT
    assert "SCALAR" in capi.last_error()
    assert call_total([INPUT, 3], 1, [None]) == capi.ERR_INDEX_RANGE  # check_formula: operand out of range
    assert call_total([INPUT, 0, ADD], 1, [None]) == capi.ERR_INVALID_ARGUMENT  # stack underflow
    assert call_copy(None, [INPUT, 0], 1, [None]) == capi.ERR_INVALID_ARGUMENT
    assert capi.last_error() == "store is NULL"


@pytest.mark.gpu
def test_argument_errors_with_stores_leave_the_target_unchanged():
    a = pkg.HipStore(6, "float32", 0.0)
    a.set_data_f64(np.arange(6.0))
    b = pkg.HipStore(8, "float32", 0.0)
    t = pkg.HipStore(6, "float64", float("nan"))
    t.set_data_f64(np.arange(6.0) + 1)
    before = t.get_data_f64().tobytes()
    assert call_total([INPUT, 0, INPUT, 1, ADD], 2, [a._h.value, b._h.value]) == capi.ERR_LENGTH_MISMATCH
    assert call_total([INPUT, 0], 1, [a._h.value], levels=((0, (0, 1)), (2, (0,)))) == capi.ERR_INVALID_ARGUMENT  # bad axis
    assert call_total([INPUT, 0], 1, [a._h.value], levels=((0, (0, 2)), (1, (0,)))) == capi.ERR_INDEX_RANGE
    assert call_total([INPUT, 0, SCALAR, 0, ADD], 1, [a._h.value]) == capi.ERR_INVALID_ARGUMENT
    assert call_total([INPUT, 0], 9, [a._h.value] * 9) == capi.ERR_INVALID_ARGUMENT
    assert call_copy(t._h.value, [INPUT, 0, INPUT, 1, ADD], 2, [a._h.value, b._h.value]) == capi.ERR_LENGTH_MISMATCH
    assert call_copy(t._h.value, [INPUT, 0], 1, [a._h.value], levels=((0, (0, -1)), (1, (0,)))) == capi.ERR_INDEX_RANGE  # copies need >= 0
    assert call_copy(t._h.value, [INPUT, 0], 1, [None]) == capi.ERR_INVALID_ARGUMENT
    assert t.get_data_f64().tobytes() == before


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_device_exact_predicate():
    r = subprocess.run([NODE, os.path.join(HERE, "js", "select_formula_host_test.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " 0 failed" in r.stdout
