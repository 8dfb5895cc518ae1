"""olap_store_cumulate_multi (running aggregates along a dimension) is declared in every layer and refuses bad arguments
on the host before any device work: the same codes and messages with and without a GPU.  The refusals that look into a
store are driven with host-side stand-ins of the handle, which the library only reads; they must stay byte-identical.
Cube.cumulate sends its eligible measures through one many-call (tests/js/cumulate_host_test.js, with a stubbed addon)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import load_package

pkg = load_package()
capi = pkg.capi
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NODE = shutil.which("node")
NAME = "olap_store_cumulate_multi"


class FakeStore(C.Structure):
    """struct olap_store (csrc/olap_internal.hpp): no buffer is attached, so a call that got past its checks would fail on
    the device requirement, never touch memory"""
    _fields_ = [("size", C.c_uint64), ("dtype", C.c_int), ("default_kind", C.c_int), ("device", C.c_int), ("values", C.c_void_p),
                ("status", C.c_void_p), ("track_order", C.c_bool), ("seq", C.c_void_p), ("next_seq", C.c_uint64), ("maybe_nonempty", C.c_bool),
                ("hi_index", C.c_uint64)]


def fake(size, device=0, dtype=2, default_kind=0, tracked=False):
    s = FakeStore()
    s.size, s.dtype, s.default_kind, s.device, s.next_seq, s.track_order = size, dtype, default_kind, device, 1, tracked
    return s


def call(handles, n=None, methods=None, lens=(2, 3), ndim=None, axis=1, n_groups=2, groups=(0, 1, 0), out=True, method_list=True, lens_there=True):
    """handles: FakeStore / address / None entries, or None for a NULL list -> (rc, message, result handles)"""
    addr = lambda h: C.addressof(h) if isinstance(h, FakeStore) else h
    count = (len(handles) if handles is not None else 1) if n is None else n
    hs = (C.c_void_p * max(len(handles), 1))(*[addr(h) for h in handles]) if handles is not None else None
    outs = (C.c_void_p * max(count, 1))() if out else None
    codes = (C.c_int * max(count, 1))(*(methods if methods is not None else [0] * max(count, 1))) if method_list else None
    lv = (C.c_uint32 * max(len(lens), 1))(*lens) if lens_there else None
    g = (C.c_uint32 * max(len(groups), 1))(*groups) if groups is not None else None
    launches = C.c_int(-1)
    rc = capi.lib().olap_store_cumulate_multi(count, hs, codes, outs, len(lens) if ndim is None else ndim, lv, axis, n_groups, g, C.byref(launches))
    return rc, capi.last_error(), [outs[i] for i in range(count)] if out and count > 0 else []


def test_the_call_is_declared_in_every_layer():
    header = open(os.path.join(ROOT, "include", "olap_hip.h")).read()
    assert re.search(r"\bint %s\(" % NAME, header)
    assert NAME in capi.SIGNATURES and len(capi.SIGNATURES[NAME][1]) == 10
    assert len(getattr(capi.lib(), NAME).argtypes) == 10
    assert callable(pkg.HipStore.cumulate) and callable(pkg.HipStore.cumulate_multi)
    assert capi.lib().olap_abi_version() == 2
    assert "cumulateMulti" in open(os.path.join(ROOT, "olap-in-memory_amd", "napi", "olap_napi.cc")).read()


def test_list_errors_without_stores():
    assert call(None)[:2] == (capi.ERR_INVALID_ARGUMENT, "store / method list is NULL")
    assert call([None], out=False)[:2] == (capi.ERR_INVALID_ARGUMENT, "store / method list is NULL")
    assert call([None], method_list=False)[:2] == (capi.ERR_INVALID_ARGUMENT, "store / method list is NULL")
    assert call([None], n=-1)[:2] == (capi.ERR_INVALID_ARGUMENT, "store / method list is NULL")
    assert call([None])[:2] == (capi.ERR_INVALID_ARGUMENT, "store 0 of the batch is NULL")
    rc, message, outs = call([], n=0)  # nothing to do is no error
    assert rc == capi.OK, message


def test_rules_lengths_axis_and_map_are_refused_before_a_store_is_looked_into():
    """The handles here are addresses of nothing: a call that looked into them, or at a device, would not answer like this."""
    nothing = (C.c_char * 8)()
    f = C.addressof(nothing)
    assert call([f, f], methods=[0, 7])[:2] == (capi.ERR_UNSUPPORTED_METHOD, "Unsupported aggregation method: 7")
    assert call([f, f], methods=[-1, 0], ndim=33)[:2] == (capi.ERR_UNSUPPORTED_METHOD, "Unsupported aggregation method: -1")
    assert call([f, f], ndim=33)[:2] == (capi.ERR_INVALID_ARGUMENT, "ndim 33 out of range [0, 32]")
    assert call([f, f], ndim=-1)[:2] == (capi.ERR_INVALID_ARGUMENT, "ndim -1 out of range [0, 32]")
    assert call([f, f], lens_there=False)[:2] == (capi.ERR_INVALID_ARGUMENT, "dimension length vectors must not be NULL")
    assert call([f, f], axis=2)[:2] == (capi.ERR_INVALID_ARGUMENT, "axis 2 out of range [0, 2)")
    assert call([f, f], axis=-1)[:2] == (capi.ERR_INVALID_ARGUMENT, "axis -1 out of range [0, 2)")
    assert call([f, f], lens=(), axis=0)[:2] == (capi.ERR_INVALID_ARGUMENT, "axis 0 out of range [0, 0)")
    assert call([f, f], groups=(0, 2, 1))[:2] == (capi.ERR_INDEX_RANGE, "cumulate map: entry 1 = 2 is outside the groups (2)")
    assert call([f, f], groups=(0, 0, 0), n_groups=0)[:2] == (capi.ERR_INDEX_RANGE, "cumulate map: entry 0 = 0 is outside the groups (0)")
    assert call([f, f], n_groups=4)[:2] == (capi.ERR_INVALID_ARGUMENT, "cumulate: 4 groups for the 3 items of the dimension")
    assert call([f, f], n_groups=0xFFFFFFFF)[:2] == (capi.ERR_INVALID_ARGUMENT, "cumulate: 4294967295 groups for the 3 items of the dimension")


def test_refusals_that_read_a_store_leave_the_stand_ins_untouched():
    a, a2, b, t, far = fake(6), fake(6, dtype=3), fake(8), fake(6, tracked=True), fake(6, device=1)
    everyone = (a, a2, b, t, far)
    before = [bytes(x) for x in everyone]
    cases = [
        ([a, None], dict(), capi.ERR_INVALID_ARGUMENT, "store 1 of the batch is NULL"),
        ([a, a2], dict(methods=[0, 7]), capi.ERR_UNSUPPORTED_METHOD, "Unsupported aggregation method: 7"),
        ([a, a2], dict(ndim=33), capi.ERR_INVALID_ARGUMENT, "ndim 33 out of range [0, 32]"),
        ([a, a2], dict(axis=2), capi.ERR_INVALID_ARGUMENT, "axis 2 out of range [0, 2)"),
        ([a, a2], dict(groups=(0, 1, 2)), capi.ERR_INDEX_RANGE, "cumulate map: entry 2 = 2 is outside the groups (2)"),
        ([a, t], dict(), capi.ERR_INVALID_ARGUMENT, "ordered: store 1 of the batch tracks its insertion order; its key order needs the per-item chain"),
        ([a, b], dict(), capi.ERR_LENGTH_MISMATCH, "store holds 8 cells but the dimensions describe 6"),
        ([a, a2], dict(lens=(2, 4), groups=(0, 1, 0, 1)), capi.ERR_LENGTH_MISMATCH, "store holds 6 cells but the dimensions describe 8"),
        ([a, a2, far], dict(), capi.ERR_INVALID_ARGUMENT, "cumulate: the stores live on different devices (0 and 1)"),
        ([a, far], dict(groups=None, n_groups=0xFFFFFFFF), capi.ERR_INVALID_ARGUMENT,  # (n_groups is not read without a map)
         "cumulate: the stores live on different devices (0 and 1)"),
    ]
    for handles, kw, want_rc, want_message in cases:
        rc, message, outs = call(handles, **kw)
        assert (rc, message) == (want_rc, want_message), (kw, rc, message)
        assert all(h is None for h in outs), want_message  # nothing is created
    assert [bytes(x) for x in everyone] == before


def test_what_the_plan_keys_of_the_calls_along_a_dimension_hold():
    """cumulate, rolling, quantile and variance side by side (tests/_along_keys_dry_worker.py, under OLAP_PLAN_DRY=1)"""
    env = {k: v for k, v in os.environ.items() if not re.match(r"OLAP_(CUMULATE|ROLLING|QUANTILE|VARIANCE)_", k)}
    env["OLAP_PLAN_DRY"] = "1"
    r = subprocess.run([sys.executable, os.path.join(HERE, "_along_keys_dry_worker.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0 and "along-axis plan keys ok" in r.stdout, r.stdout[-4000:]


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_cube_sends_its_eligible_measures_through_one_call():
    r = subprocess.run([NODE, os.path.join(HERE, "js", "cumulate_host_test.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " 0 failed" in r.stdout
