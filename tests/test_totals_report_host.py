"""olap_totals_report (getNestedObjects(ids, withTotals): several measures in one device call) checks its arguments on
the host before any device work — the same codes and messages with and without a GPU — and Cube sends the eligible ids
of one call through one report (tests/js/totals_report_host_test.js, with a stubbed addon)."""
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


def S(i):
    """a stored output: the extended cube of input i"""
    return i


def F(code, picks, n_consts=0):
    """a formula output: INPUT operand j reads report input picks[j]"""
    return (code, n_consts, picks)


def ints(a):
    return (C.c_int * max(len(a), 1))(*a)


def call(inputs, outputs, lens=(2, 3), methods=None, tables=True, code=True, consts=True, picks=True, values=True, n_inputs=None, n_outputs=None,
         stored_counts=(0, 0, 0)):
    """inputs: store handles (or None); outputs: S(i) | F(code, picks)"""
    n_in = (len(inputs) if inputs is not None else 1) if n_inputs is None else n_inputs
    table = (C.c_void_p * max(len(inputs), 1))(*inputs) if inputs is not None else None
    lv = (C.c_uint32 * max(len(lens), 1))(*lens)
    if methods is None:
        methods = [0] * (max(n_in, 1) * len(lens))
    stored, n_code, n_consts, n_picks, words, chosen = [], [], [], [], [], []
    for out in outputs:
        if isinstance(out, int):
            stored.append(out), n_code.append(stored_counts[0]), n_consts.append(stored_counts[1]), n_picks.append(stored_counts[2])
        else:
            stored.append(-1), n_code.append(len(out[0])), n_consts.append(out[1]), n_picks.append(len(out[2]))
            words.extend(out[0]), chosen.extend(out[2])
    ext = int(np.prod([l + 1 for l in lens], dtype=np.float64)) if len(lens) else 1
    out = (C.c_double * min(max(ext * max(len(outputs), 1), 1), 1 << 16))() if values else None
    launches, nbytes = C.c_int(-1), C.c_uint64(0)
    return capi.lib().olap_totals_report(
        n_in, table, len(lens), lv, ints(methods), len(outputs) if n_outputs is None else n_outputs, ints(stored) if tables else None, ints(n_code),
        (C.c_int32 * max(len(words), 1))(*words) if code else None, ints(n_consts), (C.c_double * 4)() if consts else None, ints(n_picks),
        ints(chosen) if picks else None, out, C.byref(launches), C.byref(nbytes))


def expect(got, expected):
    assert len(got) == len(expected)
    for (what, rc, message), (want_rc, want_message) in zip(got, expected):
        assert rc == want_rc and want_message in message, (what, rc, message)


def test_symbol_is_bound():
    assert hasattr(capi.lib(), "olap_totals_report")
    assert callable(pkg.hipstore.totals_report)


def table_errors(A, A2):
    """every refusal decided before a store is looked into (A, A2: any two handles, or None): [(what, rc, message), ...]"""
    one = F([INPUT, 0], [0])
    calls = [
        ("no input", lambda: call([A], [one], n_inputs=0)),
        ("33 inputs", lambda: call([A], [one], n_inputs=33)),
        ("no output", lambda: call([A], [one], n_outputs=0)),
        ("33 outputs", lambda: call([A], [one], n_outputs=33)),
        ("no input table", lambda: call(None, [one])),
        ("no output tables", lambda: call([A], [one], tables=False)),
        # formulas: olap_formula_totals' refusals, prefixed with the output's number
        ("SCALAR", lambda: call([A], [S(0), F([INPUT, 0, SCALAR, 0, ADD], [0])])),
        ("operand out of range", lambda: call([A], [F([INPUT, 3], [0])])),
        ("stack underflow", lambda: call([A, A2], [S(1), S(0), F([INPUT, 0, ADD], [0])])),
        ("empty program", lambda: call([A], [F([], [0])])),
        ("98 words", lambda: call([A], [F([INPUT, 0] * 49, [0])])),
        ("two values left", lambda: call([A], [F([INPUT, 0, INPUT, 0], [0])])),
        ("constants are NULL", lambda: call([A], [F([INPUT, 0, CONST, 0, ADD], [0], n_consts=1)], consts=False)),
        ("programs are NULL", lambda: call([A], [one], code=False)),
        ("formula inputs are NULL", lambda: call([A], [one], picks=False)),
        ("no formula input", lambda: call([A], [S(0), F([CONST, 0], [], n_consts=1)])),
        ("nine formula inputs", lambda: call([A], [F([INPUT, 0], [0] * 9)])),
        # the tables
        ("a stored output with a program", lambda: call([A], [S(0)], stored_counts=(2, 0, 0))),
        ("stored index past the inputs", lambda: call([A], [S(1)])),
        ("stored index below -1", lambda: call([A], [-2])),
        ("formula input past the inputs", lambda: call([A], [S(0), F([INPUT, 0], [1])])),
        ("formula input below 0", lambda: call([A], [F([INPUT, 0], [-1])])),
        ("a formula names one input twice", lambda: call([A, A2], [S(0), F([INPUT, 0, INPUT, 1, ADD], [1, 1])])),
        ("a stored input named by two outputs", lambda: call([A, A2], [S(1), S(0), S(1)])),
        ("an input no output uses", lambda: call([A, A2], [S(0), one])),
    ]
    return [(what, f(), capi.last_error()) for what, f in calls]


EXPECTED_TABLE_ERRORS = [
    (capi.ERR_INVALID_ARGUMENT, "a totals report needs 1..32 stored measures, got 0"),
    (capi.ERR_INVALID_ARGUMENT, "a totals report needs 1..32 stored measures, got 33"),
    (capi.ERR_INVALID_ARGUMENT, "a totals report needs 1..32 outputs, got 0"),
    (capi.ERR_INVALID_ARGUMENT, "a totals report needs 1..32 outputs, got 33"),
    (capi.ERR_INVALID_ARGUMENT, "report inputs are NULL"),
    (capi.ERR_INVALID_ARGUMENT, "report output tables are NULL"),
    (capi.ERR_INVALID_ARGUMENT, "output 1: a formula with totals cannot read a measure total (SCALAR)"),
    (capi.ERR_INDEX_RANGE, "output 0: formula operand 3 out of range"),
    (capi.ERR_INVALID_ARGUMENT, "output 2: formula program underflows its stack"),
    (capi.ERR_INVALID_ARGUMENT, "output 0: formula program has 0 words"),
    (capi.ERR_INVALID_ARGUMENT, "output 0: formula program has 98 words"),
    (capi.ERR_INVALID_ARGUMENT, "output 0: formula program leaves 2 values on its stack"),
    (capi.ERR_INVALID_ARGUMENT, "output 0: formula constants are NULL"),
    (capi.ERR_INVALID_ARGUMENT, "output 0: formula programs are NULL"),
    (capi.ERR_INVALID_ARGUMENT, "output 0: formula inputs are NULL"),
    (capi.ERR_INVALID_ARGUMENT, "output 1: a formula with totals needs 1..8 stored measures, got 0"),
    (capi.ERR_INVALID_ARGUMENT, "output 0: a formula with totals needs 1..8 stored measures, got 9"),
    (capi.ERR_INVALID_ARGUMENT, "output 0: a stored output carries no program"),
    (capi.ERR_INDEX_RANGE, "output 0: input 1 out of range"),
    (capi.ERR_INDEX_RANGE, "output 0: input -2 out of range"),
    (capi.ERR_INDEX_RANGE, "output 1: input 1 out of range"),
    (capi.ERR_INDEX_RANGE, "output 0: input -1 out of range"),
    (capi.ERR_INVALID_ARGUMENT, "output 1: input 1 is named twice"),
    (capi.ERR_INVALID_ARGUMENT, "output 2: input 1 is output 0 already"),
    (capi.ERR_INVALID_ARGUMENT, "report input 1 is used by no output"),
]


def test_argument_errors_without_stores():
    """Everything that is refused without looking into a store — the outputs' tables and every formula: the same answers
    on a machine with no device.  Then the first look at a store: a NULL handle."""
    expect(table_errors(None, None), EXPECTED_TABLE_ERRORS)
    assert call([None], [S(0)]) == capi.ERR_INVALID_ARGUMENT and capi.last_error() == "report input 0 is NULL"
    assert call([None, None], [S(1), F([INPUT, 0, INPUT, 1, ADD], [0, 1])]) == capi.ERR_INVALID_ARGUMENT
    assert capi.last_error() == "report input 0 is NULL"


def store_errors(a, a2, b, tracked):
    """every refusal that needs a store handle: [(what, rc, message), ...]"""
    A, A2, B, T = a._h.value, a2._h.value, b._h.value, tracked._h.value
    two = F([INPUT, 0, INPUT, 1, ADD], [0, 1])
    calls = [
        ("a NULL handle behind a good one", lambda: call([A, None], [two])),
        ("tracked input", lambda: call([A, T], [S(0), two])),
        ("rule code above product", lambda: call([A], [S(0)], methods=[0, 7])),
        ("the second input's rules are checked too", lambda: call([A, A2], [two], methods=[0, 0, 0, -1])),
        ("6 cells, dimensions describe 8", lambda: call([A], [S(0)], lens=(2, 4))),
        ("the second input holds 8 cells", lambda: call([A, B], [two])),
        ("17 dimensions", lambda: call([A], [S(0)], lens=(1,) * 17)),
        ("4.9e9 extended cells", lambda: call([A], [S(0)], lens=(70000, 70000))),
        ("2 outputs + 1 scratch input of 1.6e9 extended cells each", lambda: call([A, A2], [S(0), F([INPUT, 0], [1])], lens=(40000, 40000))),
        ("no result array", lambda: call([A], [S(0)], values=False)),
    ]
    return [(what, f(), capi.last_error()) for what, f in calls]


EXPECTED_STORE_ERRORS = [
    (capi.ERR_INVALID_ARGUMENT, "report input 1 is NULL"),
    (capi.ERR_INVALID_ARGUMENT, "ordered:"),
    (capi.ERR_UNSUPPORTED_METHOD, "Unsupported aggregation method: 7"),
    (capi.ERR_UNSUPPORTED_METHOD, "Unsupported aggregation method: -1"),
    (capi.ERR_LENGTH_MISMATCH, "6 cells but the dimensions describe 8"),
    (capi.ERR_LENGTH_MISMATCH, "8 cells but the dimensions describe 6"),
    (capi.ERR_INVALID_ARGUMENT, "totals: at most 16 dimensions"),
    (capi.ERR_INVALID_ARGUMENT, "totals: the report would hold"),
    (capi.ERR_INVALID_ARGUMENT, "totals: the report would hold"),
    (capi.ERR_INVALID_ARGUMENT, "values is NULL"),
]


@pytest.mark.gpu
def test_argument_errors_with_stores_leave_the_inputs_unchanged():
    """Store handles exist only where a device does.  Every refusal comes with the code and message the host checks
    give, leaves the inputs as they were, and the store-free refusals answer as they do without a device."""
    a = pkg.HipStore(6, "float32", 0.0)
    a.set_data_f64(np.arange(6.0))
    a2 = pkg.HipStore(6, "float32", 0.0)
    a2.set_data_f64(np.arange(6.0) * 2)
    b = pkg.HipStore(8, "float32", 0.0)
    t = pkg.HipStore(6, "float32", 0.0)
    capi.check(capi.lib().olap_store_track_order(t._h, 1))
    t.set_data_f64(np.arange(6.0) + 1)
    before = [x.get_data_f64().tobytes() for x in (a, a2, b, t)]
    got = store_errors(a, a2, b, t)
    expect(got, EXPECTED_STORE_ERRORS)
    assert [m for w, _, m in got if w == "tracked input"][0].startswith("ordered:")
    expect(table_errors(a._h.value, a2._h.value), EXPECTED_TABLE_ERRORS)
    test_argument_errors_without_stores()
    assert [x.get_data_f64().tobytes() for x in (a, a2, b, t)] == before
    vals, launches, nbytes = pkg.hipstore.totals_report([a, a2], [2, 3], [["sum", "sum"]] * 2, [0, ([INPUT, 0, INPUT, 1, ADD], [], [1, 0])])
    assert vals[0].reshape(3, 4).tolist() == [[0, 1, 2, 3], [3, 4, 5, 12], [3, 5, 7, 15]]
    assert vals[1].tolist() == (vals[0] * 3).tolist() and launches == 2 and nbytes == 2 * 24 + 2 * 12 * 8


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_cube_sends_the_eligible_ids_through_one_report():
    r = subprocess.run([NODE, os.path.join(HERE, "js", "totals_report_host_test.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " 0 failed" in r.stdout
