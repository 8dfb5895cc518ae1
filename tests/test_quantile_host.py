"""olap_store_quantile_multi (order statistics along a dimension) is declared in every layer and refuses bad arguments on
the host before any device work: the same codes and messages with and without a GPU, in cumulate's order with `quantile`
in place of `cumulate`, q after the axis and before the groups.  The refusals that look into a store are driven with
host-side stand-ins of the handle, which the library only reads; they must stay byte-identical.  A store that tracks its
insertion order is NOT refused.  olap_diag_quantile_choice (host only) shows that the shape lists of
tests/test_quantile_gpu.py reach every form.  Cube.quantile sends its eligible measures through one many-call
(tests/js/quantile_host_test.js, with a stubbed addon)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import load_package
from test_cumulate_host import FakeStore, fake
from test_quantile_gpu import (COLUMN, COLUMN_SHAPES, DIRECT_BLOCK, DIRECT_BLOCK_SHAPES, DIRECT_LANES, DIRECT_LANES_SHAPE, GROUP_SHAPES, ROW, ROW_SHAPES,
                               SIZED_GROUPS, SMALL_TILE, TYPES, choice, expected_form)

pkg = load_package()
capi = pkg.capi
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NODE = shutil.which("node")
NAME = "olap_store_quantile_multi"


def call(handles, n=None, lens=(2, 3), ndim=None, axis=1, q=0.5, n_groups=2, groups=(0, 1, 0), out=True, lens_there=True):
    """handles: FakeStore / address / None entries, or None for a NULL list -> (rc, message, result handles)"""
    addr = lambda h: C.addressof(h) if isinstance(h, FakeStore) else h
    count = (len(handles) if handles is not None else 1) if n is None else n
    hs = (C.c_void_p * max(len(handles), 1))(*[addr(h) for h in handles]) if handles is not None else None
    outs = (C.c_void_p * max(count, 1))() if out else None
    lv = (C.c_uint32 * max(len(lens), 1))(*lens) if lens_there else None
    g = (C.c_uint32 * max(len(groups), 1))(*groups) if groups is not None else None
    launches = C.c_int(-1)
    rc = capi.lib().olap_store_quantile_multi(count, hs, outs, len(lens) if ndim is None else ndim, lv, axis, q, n_groups, g, C.byref(launches))
    return rc, capi.last_error(), [outs[i] for i in range(count)] if out and count > 0 else []


def test_the_call_is_declared_in_every_layer():
    header = open(os.path.join(ROOT, "include", "olap_hip.h")).read()
    assert re.search(r"\bint %s\(" % NAME, header) and re.search(r"\bint olap_diag_quantile_choice\(", header)
    assert NAME in capi.SIGNATURES and len(capi.SIGNATURES[NAME][1]) == 10
    assert len(getattr(capi.lib(), NAME).argtypes) == 10
    assert len(capi.lib().olap_diag_quantile_choice.argtypes) == 9
    assert callable(pkg.HipStore.quantile) and callable(pkg.HipStore.quantile_multi)
    assert capi.lib().olap_abi_version() == 2
    assert "quantileMulti" in open(os.path.join(ROOT, "olap-in-memory_amd", "napi", "olap_napi.cc")).read()
    assert os.path.exists(os.path.join(ROOT, "olap-in-memory_amd", "csrc", "olap_quantile.hip"))  # (the library binds the symbol: the unit is linked)


def test_median_stays_refused_as_a_rule():
    """the seven-rule list is closed: the quantile is a call, not an eighth rule"""
    with pytest.raises(Exception) as e:
        pkg.hipstore._method_code("median")
    assert "median" in str(e.value)
    nothing = (C.c_char * 8)()
    codes = (C.c_int * 1)(7)
    hs, outs = (C.c_void_p * 1)(C.addressof(nothing)), (C.c_void_p * 1)()
    lv = (C.c_uint32 * 2)(2, 3)
    assert capi.lib().olap_store_cumulate_multi(1, hs, codes, outs, 2, lv, 1, 1, None, None) == capi.ERR_UNSUPPORTED_METHOD


def test_list_errors_without_stores():
    assert call(None)[:2] == (capi.ERR_INVALID_ARGUMENT, "store list is NULL")
    assert call([None], out=False)[:2] == (capi.ERR_INVALID_ARGUMENT, "store list is NULL")
    assert call([None], n=-1)[:2] == (capi.ERR_INVALID_ARGUMENT, "store list is NULL")
    assert call([None])[:2] == (capi.ERR_INVALID_ARGUMENT, "store 0 of the batch is NULL")
    rc, message, outs = call([], n=0)  # nothing to do is no error
    assert rc == capi.OK, message
    rc, message, outs = call([], n=0, q=7.0, axis=9)  # ... but the arguments are still checked
    assert (rc, message) == (capi.ERR_INVALID_ARGUMENT, "axis 9 out of range [0, 2)")


def test_lengths_axis_q_and_map_are_refused_before_a_store_is_looked_into():
    """The handles here are addresses of nothing: a call that looked into them, or at a device, would not answer like this."""
    nothing = (C.c_char * 8)()
    f = C.addressof(nothing)
    assert call([f, f], ndim=33)[:2] == (capi.ERR_INVALID_ARGUMENT, "ndim 33 out of range [0, 32]")
    assert call([f, f], ndim=-1, q=2.0)[:2] == (capi.ERR_INVALID_ARGUMENT, "ndim -1 out of range [0, 32]")
    assert call([f, f], lens_there=False)[:2] == (capi.ERR_INVALID_ARGUMENT, "dimension length vectors must not be NULL")
    assert call([f, f], axis=2)[:2] == (capi.ERR_INVALID_ARGUMENT, "axis 2 out of range [0, 2)")
    assert call([f, f], axis=-1, q=-0.1)[:2] == (capi.ERR_INVALID_ARGUMENT, "axis -1 out of range [0, 2)")  # the axis comes first
    assert call([f, f], lens=(), axis=0)[:2] == (capi.ERR_INVALID_ARGUMENT, "axis 0 out of range [0, 0)")
    assert call([f, f], q=-0.1)[:2] == (capi.ERR_INVALID_ARGUMENT, "quantile: q must lie in [0, 1] (got -0.1)")
    assert call([f, f], q=1.5, n_groups=4)[:2] == (capi.ERR_INVALID_ARGUMENT, "quantile: q must lie in [0, 1] (got 1.5)")  # before the groups
    rc, message, outs = call([f, f], q=float("nan"), groups=(0, 2, 1))
    assert rc == capi.ERR_INVALID_ARGUMENT and re.fullmatch(r"quantile: q must lie in \[0, 1\] \(got -?nan\)", message), message
    assert call([f, f], q=float("inf"))[:2] == (capi.ERR_INVALID_ARGUMENT, "quantile: q must lie in [0, 1] (got inf)")
    assert call([f, f], groups=(0, 2, 1))[:2] == (capi.ERR_INDEX_RANGE, "quantile map: entry 1 = 2 is outside the groups (2)")
    assert call([f, f], groups=(0, 0, 0), n_groups=0)[:2] == (capi.ERR_INDEX_RANGE, "quantile map: entry 0 = 0 is outside the groups (0)")
    assert call([f, f], n_groups=4)[:2] == (capi.ERR_INVALID_ARGUMENT, "quantile: 4 groups for the 3 items of the dimension")
    assert call([f, f], n_groups=0xFFFFFFFF)[:2] == (capi.ERR_INVALID_ARGUMENT, "quantile: 4294967295 groups for the 3 items of the dimension")


def test_refusals_that_read_a_store_leave_the_stand_ins_untouched():
    a, a2, b, t, far = fake(6), fake(6, dtype=3), fake(8), fake(6, tracked=True), fake(6, device=1)
    everyone = (a, a2, b, t, far)
    before = [bytes(x) for x in everyone]
    cases = [
        ([a, None], dict(), capi.ERR_INVALID_ARGUMENT, "store 1 of the batch is NULL"),
        ([a, a2], dict(ndim=33), capi.ERR_INVALID_ARGUMENT, "ndim 33 out of range [0, 32]"),
        ([a, a2], dict(axis=2), capi.ERR_INVALID_ARGUMENT, "axis 2 out of range [0, 2)"),
        ([a, a2], dict(q=1.5), capi.ERR_INVALID_ARGUMENT, "quantile: q must lie in [0, 1] (got 1.5)"),
        ([a, a2], dict(groups=(0, 1, 2)), capi.ERR_INDEX_RANGE, "quantile map: entry 2 = 2 is outside the groups (2)"),
        ([a, b], dict(), capi.ERR_LENGTH_MISMATCH, "store holds 8 cells but the dimensions describe 6"),
        ([t, b], dict(), capi.ERR_LENGTH_MISMATCH, "store holds 8 cells but the dimensions describe 6"),
        ([a, a2], dict(lens=(2, 4), groups=(0, 1, 0, 1)), capi.ERR_LENGTH_MISMATCH, "store holds 6 cells but the dimensions describe 8"),
        ([a, a2, far], dict(), capi.ERR_INVALID_ARGUMENT, "quantile: the stores live on different devices (0 and 1)"),
        # a tracked store is not refused: the call goes on to the next check
        ([a, t, far], dict(), capi.ERR_INVALID_ARGUMENT, "quantile: the stores live on different devices (0 and 1)"),
        ([a, far], dict(groups=None, n_groups=0xFFFFFFFF), capi.ERR_INVALID_ARGUMENT,  # (n_groups is not read without a map)
         "quantile: the stores live on different devices (0 and 1)"),
    ]
    for handles, kw, want_rc, want_message in cases:
        rc, message, outs = call(handles, **kw)
        assert (rc, message) == (want_rc, want_message), (kw, rc, message)
        assert all(h is None for h in outs), want_message  # nothing is created
    assert [bytes(x) for x in everyone] == before


def test_the_planner_reaches_every_form_with_the_shapes_of_the_gpu_test(monkeypatch):
    monkeypatch.delenv("OLAP_QUANTILE_TILE", raising=False)
    seen = set()
    for lens in COLUMN_SHAPES + ROW_SHAPES + GROUP_SHAPES:
        groups = SIZED_GROUPS if lens in GROUP_SHAPES else None
        for type_name in TYPES:
            for default_is_nan in (False, True):
                c = choice(type_name, default_is_nan, lens, 1, groups)
                assert c[0] == expected_form(lens, type_name), (lens, type_name, c)
                assert c[1] == 32768 // (np.dtype(type_name).itemsize + (4 if default_is_nan and "int" in type_name else 0))
                if c[0] == COLUMN:
                    assert c[4] * c[5] <= c[1] and c[5] >= (max(np.bincount(groups)) if groups is not None else lens[1]), (lens, c)  # the largest group fits
                else:
                    assert c[3] % 2 == 1 and c[2] * lens[1] * int(np.prod(lens[2:])) <= c[1], (lens, c)  # odd pitch, whole series
                seen.add(c[0])
    assert choice("float32", False, [2, 3, 1030])[4] == 256 and choice("int32", True, [2, 300, 18])[4] == 12  # slices of the row; whole slots
    assert choice("float32", False, [3, 8192])[0] == ROW and choice("float32", False, [3, 8193])[0] == DIRECT_BLOCK
    assert choice("float64", False, [3, 4096])[0] == ROW and choice("float64", False, [3, 4097])[0] == DIRECT_BLOCK
    assert choice("float32", False, [100, 100, 10000], 2, np.arange(10000) // 12)[::4] == (COLUMN, 1)
    assert choice("float32", False, [100, 2049, 10000])[0] == DIRECT_LANES and choice("float32", False, [100, 2048, 10000])[0] == COLUMN
    monkeypatch.setenv("OLAP_QUANTILE_TILE", str(SMALL_TILE))
    for type_name in TYPES:
        for default_is_nan in (False, True):
            for lens in DIRECT_BLOCK_SHAPES:
                c = choice(type_name, default_is_nan, lens)
                assert c[:2] == ((ROW if lens[1] <= SMALL_TILE else DIRECT_BLOCK), SMALL_TILE), (lens, c)
                seen.add(c[0])
            K = SMALL_TILE + 1
            assert choice(type_name, default_is_nan, [2, K], 1, np.arange(K) % 3)[::4] == (COLUMN, 1)  # narrow rows beyond a tile: the row a slice
            assert choice(type_name, default_is_nan, [2, K, 3], 1, np.arange(K) // 9)[::4] == (COLUMN, 3)
            assert choice(type_name, default_is_nan, [2, 2 * K + 3], 1, np.arange(2 * K + 3) % 2)[0] == DIRECT_BLOCK
            assert choice(type_name, default_is_nan, [2, K, 16], 1, np.arange(K) % 2)[0] == DIRECT_BLOCK
            assert choice(type_name, default_is_nan, DIRECT_LANES_SHAPE)[0] == DIRECT_LANES
            seen.add(DIRECT_LANES)
            assert choice(type_name, default_is_nan, [2, 30, 16], 1, np.arange(30) // 3)[4:] == (16, 4)  # one group of three rows per tile
            assert choice(type_name, default_is_nan, [40, 7])[:3] == (ROW, SMALL_TILE, 9)
    assert seen == {COLUMN, ROW, DIRECT_LANES, DIRECT_BLOCK}
    monkeypatch.setenv("OLAP_QUANTILE_TILE", "1000000")  # the knob only lowers the tile
    assert choice("float32", False, [3, 5])[1] == 8192


def test_the_choice_call_refuses_what_it_cannot_plan():
    c = (C.c_uint32 * 6)()
    L = capi.lib()
    assert L.olap_diag_quantile_choice(2, 0, 1, 8, 1, 1, 8, 1, c) == capi.ERR_INVALID_ARGUMENT
    assert L.olap_diag_quantile_choice(4, 0, 1, 8, 1, 1, 8, 1, None) == capi.ERR_INVALID_ARGUMENT
    assert L.olap_diag_quantile_choice(4, 0, 1, 2 ** 32, 1, 1, 8, 1, c) == capi.ERR_INVALID_ARGUMENT
    assert L.olap_diag_quantile_choice(4, 0, 1, 8, 1, 1, 9, 1, c) == capi.ERR_INVALID_ARGUMENT
    assert capi.last_error() == "quantile choice: a group of 9 of the dimension's 8 items"


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_cube_sends_its_eligible_measures_through_one_call():
    r = subprocess.run([NODE, os.path.join(HERE, "js", "quantile_host_test.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " 0 failed" in r.stdout
