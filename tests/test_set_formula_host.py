"""olap_store_set_formula / olap_sharded_store_set_formula (a computed measure written straight into a stored one) refuse
bad arguments on the host before any device work: the same codes and messages with and without a GPU.  The refusals that
look into a store are driven with host-side stand-ins of the handle, which the library only reads (size, device) before
it answers."""
import ctypes as C
import os
import re

from conftest import load_package

pkg = load_package()
capi = pkg.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONST, INPUT, SCALAR, ADD = 0, 1, 2, 3


class FakeStore(C.Structure):
    """struct olap_store (csrc/olap_internal.hpp), for refusals decided from its first fields: no buffer is attached, so
    a call that got past its checks would fail on the device requirement, never touch memory"""
    _fields_ = [("size", C.c_uint64), ("dtype", C.c_int), ("default_kind", C.c_int), ("device", C.c_int), ("values", C.c_void_p),
                ("status", C.c_void_p), ("track_order", C.c_bool), ("seq", C.c_void_p), ("next_seq", C.c_uint64), ("maybe_nonempty", C.c_bool),
                ("hi_index", C.c_uint64)]


def fake(size, device=0, dtype=2, default_kind=0):
    s = FakeStore()
    s.size, s.dtype, s.default_kind, s.device, s.next_seq = size, dtype, default_kind, device, 1
    return s


def call(fn, target, code, inputs, n_inputs=None, n_consts=0, consts=True, scalars=(), scalar_table=True):
    """fn(target, code, consts, inputs, scalars) with ctypes tables; inputs: handles (FakeStore, int or None) or None"""
    c = (C.c_int32 * max(len(code), 1))(*code)
    k = (C.c_double * 4)() if consts else None
    sc = (C.c_double * max(len(scalars), 1))(*scalars) if scalar_table else None
    addr = lambda h: C.addressof(h) if isinstance(h, FakeStore) else h
    table = (C.c_void_p * max(len(inputs), 1))(*[addr(h) for h in inputs]) if inputs is not None else None
    n_in = (len(inputs) if inputs is not None else 1) if n_inputs is None else n_inputs
    return fn(addr(target), c if code else None, len(code), k, n_consts, n_in, table, sc, len(scalars))


def both():
    L = capi.lib()
    return (L.olap_store_set_formula, L.olap_sharded_store_set_formula)


def test_symbols_are_declared():
    header = open(os.path.join(ROOT, "include", "olap_hip.h")).read()
    for name in ("olap_store_set_formula", "olap_sharded_store_set_formula"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.SIGNATURES and len(capi.SIGNATURES[name][1]) == 9
        assert len(getattr(capi.lib(), name).argtypes) == 9
    assert callable(pkg.HipStore.set_formula)
    from olap_in_memory_amd.sharded import ShardedStore

    assert callable(ShardedStore.set_formula)


def test_program_checks_come_first():
    """check_formula's refusals, whatever the handles are"""
    for fn in both():
        assert call(fn, None, [], [None]) == capi.ERR_INVALID_ARGUMENT
        assert "formula program has 0 words" in capi.last_error()
        assert call(fn, None, [INPUT, 0] * 49, [None]) == capi.ERR_INVALID_ARGUMENT  # 98 words
        assert call(fn, None, [INPUT], [None]) == capi.ERR_INVALID_ARGUMENT
        assert capi.last_error() == "formula program truncated"
        assert call(fn, None, [INPUT, 1], [None]) == capi.ERR_INDEX_RANGE
        assert capi.last_error() == "formula operand 1 out of range"
        assert call(fn, None, [CONST, 0], [None]) == capi.ERR_INDEX_RANGE  # no constants given
        assert call(fn, None, [SCALAR, 0], [None]) == capi.ERR_INDEX_RANGE  # no scalars given
        assert call(fn, None, [INPUT, 0, ADD], [None]) == capi.ERR_INVALID_ARGUMENT
        assert capi.last_error() == "formula program underflows its stack"
        assert call(fn, None, [INPUT, 0, INPUT, 0], [None]) == capi.ERR_INVALID_ARGUMENT
        assert capi.last_error() == "formula program leaves 2 values on its stack"
        assert call(fn, None, [INPUT, 0, 99], [None]) == capi.ERR_INVALID_ARGUMENT
        assert capi.last_error() == "unknown formula opcode 99"
        assert call(fn, None, [INPUT, 0] * 17 + [ADD] * 16, [None]) == capi.ERR_INVALID_ARGUMENT
        assert capi.last_error() == "formula needs a stack deeper than 16"
        assert call(fn, None, [INPUT, 0], [None] * 9) == capi.ERR_INVALID_ARGUMENT
        assert "too many" in capi.last_error()


def test_null_handles():
    t = fake(6)
    for fn in both():
        assert call(fn, None, [INPUT, 0], [None]) == capi.ERR_INVALID_ARGUMENT
        assert capi.last_error() == "store is NULL"
    for fn, target in zip(both(), (t, 1)):  # (the sharded form looks into no handle before these answers)
        assert call(fn, target, [CONST, 0], [], n_consts=1) == capi.ERR_INVALID_ARGUMENT
        assert capi.last_error() == "a formula needs at least one stored measure to read"
        assert call(fn, target, [CONST, 0], None, n_inputs=0, n_consts=1) == capi.ERR_INVALID_ARGUMENT
        assert call(fn, target, [INPUT, 0], None) == capi.ERR_INVALID_ARGUMENT
        assert capi.last_error() == "a formula needs at least one stored measure to read"
        assert call(fn, target, [INPUT, 0, CONST, 0, ADD], [None], n_consts=1, consts=False) == capi.ERR_INVALID_ARGUMENT
        assert capi.last_error() == "formula argument arrays must not be NULL"
        assert call(fn, target, [INPUT, 0, SCALAR, 0, ADD], [None], scalars=(1.0,), scalar_table=False) == capi.ERR_INVALID_ARGUMENT
        assert call(fn, target, [INPUT, 0], [None]) == capi.ERR_INVALID_ARGUMENT
        assert capi.last_error() == "formula input 0 is NULL"
    a = fake(6)
    assert call(both()[0], t, [INPUT, 0, INPUT, 1, ADD], [a, None]) == capi.ERR_INVALID_ARGUMENT
    assert capi.last_error() == "formula input 1 is NULL"


def test_store_refusals_without_a_device():
    fn = both()[0]
    t, a, short, far = fake(6), fake(6), fake(5), fake(6, device=1)
    assert call(fn, t, [INPUT, 0, INPUT, 1, ADD], [a, short]) == capi.ERR_LENGTH_MISMATCH
    assert capi.last_error() == "formula input 1 holds 5 cells, the target 6"
    assert call(fn, short, [INPUT, 0], [a]) == capi.ERR_LENGTH_MISMATCH
    assert call(fn, t, [INPUT, 0, INPUT, 1, ADD], [a, t]) == capi.ERR_INVALID_ARGUMENT
    assert capi.last_error() == "formula input 1 is the target itself"
    assert call(fn, t, [INPUT, 0], [t]) == capi.ERR_INVALID_ARGUMENT
    assert call(fn, t, [INPUT, 0, INPUT, 1, ADD], [a, far]) == capi.ERR_INVALID_ARGUMENT
    assert capi.last_error() == "the formula's inputs and the target live on different devices"
    assert call(fn, far, [INPUT, 0], [a]) == capi.ERR_INVALID_ARGUMENT
    # the same input twice is no alias of the target
    empty_t, empty_a = fake(0), fake(0)
    assert call(fn, empty_t, [INPUT, 0, INPUT, 1, ADD], [empty_a, empty_a]) == capi.OK  # no cells: nothing to do, no device needed
    assert call(fn, empty_t, [INPUT, 0], [a]) == capi.ERR_LENGTH_MISMATCH
