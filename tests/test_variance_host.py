"""olap_store_variance_multi (variance and standard deviation along a dimension) is declared in every layer and refuses
bad arguments on the host before any device work: the same codes and messages with and without a GPU, in cumulate's order
with `variance` in place of `cumulate`, kind and then ddof after the axis and before the groups.  The refusals that look
into a store are driven with host-side stand-ins of the handle, which the library only reads; they must stay
byte-identical.  A store that tracks its insertion order is NOT refused.  olap_diag_variance_choice (host only) shows that
the shape lists of tests/test_variance_gpu.py reach every form, and where the re-associated workgroup form begins.  kind
and ddof are not part of the plan-cache key (tests/_variance_dry_worker.py, under OLAP_PLAN_DRY=1).  Cube.variance sends
its eligible measures through one many-call (tests/js/variance_host_test.js, with a stubbed addon)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_package
from test_cumulate_host import FakeStore, fake
from test_cumulate_host import call as cumulate_call
from test_variance_gpu import (AROUND_SMALL_TILE, BLOCK_CELLS, BLOCK_MEMBERS, BLOCK_SHAPE, COLUMN, COLUMN_SHAPES, DIRECT_BLOCK, DIRECT_LANES, DIRECT_LANES_SHAPE,
                               GROUP_SHAPES, NEVER, ROW, ROW_SHAPES, SIZED_GROUPS, SMALL_TILE, TYPES, choice, expected_form)

pkg = load_package()
capi = pkg.capi
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NODE = shutil.which("node")
NAME = "olap_store_variance_multi"
KNOBS = ("OLAP_VARIANCE_TILE", "OLAP_VARIANCE_BLOCK", "OLAP_VARIANCE_GRID")


def call(handles, n=None, lens=(2, 3), ndim=None, axis=1, kind=0, ddof=0, n_groups=2, groups=(0, 1, 0), out=True, lens_there=True):
    """handles: FakeStore / address / None entries, or None for a NULL list -> (rc, message, result handles)"""
    addr = lambda h: C.addressof(h) if isinstance(h, FakeStore) else h
    count = (len(handles) if handles is not None else 1) if n is None else n
    hs = (C.c_void_p * max(len(handles), 1))(*[addr(h) for h in handles]) if handles is not None else None
    outs = (C.c_void_p * max(count, 1))() if out else None
    lv = (C.c_uint32 * max(len(lens), 1))(*lens) if lens_there else None
    g = (C.c_uint32 * max(len(groups), 1))(*groups) if groups is not None else None
    launches = C.c_int(-1)
    rc = capi.lib().olap_store_variance_multi(count, hs, outs, len(lens) if ndim is None else ndim, lv, axis, kind, ddof, n_groups, g, C.byref(launches))
    return rc, capi.last_error(), [outs[i] for i in range(count)] if out and count > 0 else []


def test_the_call_is_declared_in_every_layer():
    header = open(os.path.join(ROOT, "include", "olap_hip.h")).read()
    assert re.search(r"\bint %s\(" % NAME, header) and re.search(r"\bint olap_diag_variance_choice\(", header)
    assert NAME in capi.SIGNATURES and len(capi.SIGNATURES[NAME][1]) == 11
    assert len(getattr(capi.lib(), NAME).argtypes) == 11
    assert len(capi.lib().olap_diag_variance_choice.argtypes) == 9
    assert callable(pkg.HipStore.variance) and callable(pkg.HipStore.variance_multi)
    assert capi.lib().olap_abi_version() == 2  # the ABI only grew
    assert "varianceMulti" in open(os.path.join(ROOT, "olap-in-memory_amd", "napi", "olap_napi.cc")).read()
    assert os.path.exists(os.path.join(ROOT, "olap-in-memory_amd", "csrc", "olap_variance.hip"))  # (the library binds the symbol: the unit is linked)
    for text in (header, open(os.path.join(ROOT, "DESIGN.md")).read(), open(os.path.join(ROOT, "olap-in-memory_amd", "csrc", "olap_variance.hip")).read()):
        assert "RE-ASSOCIATED" in text  # the fourth form says what it is wherever K1r does
    cube = open(os.path.join(ROOT, "olap-in-memory_amd", "js", "cube.js")).read()
    assert all(("  %s(" % name) in cube for name in ("variance", "stddev", "_varianceHost"))


def test_list_errors_without_stores():
    assert call(None)[:2] == (capi.ERR_INVALID_ARGUMENT, "store list is NULL")
    assert call([None], out=False)[:2] == (capi.ERR_INVALID_ARGUMENT, "store list is NULL")
    assert call([None], n=-1)[:2] == (capi.ERR_INVALID_ARGUMENT, "store list is NULL")
    assert call([None])[:2] == (capi.ERR_INVALID_ARGUMENT, "store 0 of the batch is NULL")
    rc, message, outs = call([], n=0)  # nothing to do is no error
    assert rc == capi.OK, message
    rc, message, outs = call([], n=0, kind=7, axis=9)  # ... but the arguments are still checked
    assert (rc, message) == (capi.ERR_INVALID_ARGUMENT, "axis 9 out of range [0, 2)")
    assert call([], n=0, ddof=2)[:2] == (capi.ERR_INVALID_ARGUMENT, "variance: ddof must be 0 or 1 (got 2)")


def test_lengths_axis_kind_ddof_and_map_are_refused_before_a_store_is_looked_into():
    """The handles here are addresses of nothing: a call that looked into them, or at a device, would not answer like this."""
    nothing = (C.c_char * 8)()
    f = C.addressof(nothing)
    assert call([f, f], ndim=33)[:2] == (capi.ERR_INVALID_ARGUMENT, "ndim 33 out of range [0, 32]")
    assert call([f, f], ndim=-1, kind=2)[:2] == (capi.ERR_INVALID_ARGUMENT, "ndim -1 out of range [0, 32]")
    assert call([f, f], lens_there=False)[:2] == (capi.ERR_INVALID_ARGUMENT, "dimension length vectors must not be NULL")
    assert call([f, f], axis=2)[:2] == (capi.ERR_INVALID_ARGUMENT, "axis 2 out of range [0, 2)")
    assert call([f, f], axis=-1, kind=-1, ddof=5)[:2] == (capi.ERR_INVALID_ARGUMENT, "axis -1 out of range [0, 2)")  # the axis comes first
    assert call([f, f], lens=(), axis=0)[:2] == (capi.ERR_INVALID_ARGUMENT, "axis 0 out of range [0, 0)")
    assert call([f, f], kind=2)[:2] == (capi.ERR_INVALID_ARGUMENT, "variance: kind must be 0 or 1 (got 2)")
    assert call([f, f], kind=-1, ddof=2)[:2] == (capi.ERR_INVALID_ARGUMENT, "variance: kind must be 0 or 1 (got -1)")  # kind before ddof
    assert call([f, f], ddof=2)[:2] == (capi.ERR_INVALID_ARGUMENT, "variance: ddof must be 0 or 1 (got 2)")
    assert call([f, f], kind=1, ddof=-1, n_groups=4)[:2] == (capi.ERR_INVALID_ARGUMENT, "variance: ddof must be 0 or 1 (got -1)")  # before the groups
    assert call([f, f], ddof=2 ** 31 - 1, groups=(0, 2, 1))[:2] == (capi.ERR_INVALID_ARGUMENT, "variance: ddof must be 0 or 1 (got 2147483647)")
    assert call([f, f], groups=(0, 2, 1))[:2] == (capi.ERR_INDEX_RANGE, "variance map: entry 1 = 2 is outside the groups (2)")
    assert call([f, f], groups=(0, 0, 0), n_groups=0)[:2] == (capi.ERR_INDEX_RANGE, "variance map: entry 0 = 0 is outside the groups (0)")
    assert call([f, f], n_groups=4)[:2] == (capi.ERR_INVALID_ARGUMENT, "variance: 4 groups for the 3 items of the dimension")
    assert call([f, f], n_groups=0xFFFFFFFF)[:2] == (capi.ERR_INVALID_ARGUMENT, "variance: 4294967295 groups for the 3 items of the dimension")


def test_the_checks_come_in_cumulates_order_with_cumulates_messages():
    """the same bad arguments to both calls: the same code, and the same message but for the call's name"""
    nothing = (C.c_char * 8)()
    f = C.addressof(nothing)
    a, b, far = fake(6), fake(8), fake(6, device=1)
    cases = [
        ([f, f], dict(ndim=33, axis=5, n_groups=4)), ([f, f], dict(lens_there=False, axis=5)), ([f, f], dict(axis=2, n_groups=4)),
        ([f, f], dict(n_groups=4, groups=(0, 9, 1))), ([f, f], dict(groups=(0, 9, 1))), ([a, None], dict(axis=2)), ([a, b, far], dict()),
        ([a, b], dict(groups=(0, 1, 2))), ([a, far], dict()), ([a, far], dict(lens=(2, 4), groups=(0, 1, 0, 1))),
    ]
    for handles, kw in cases:
        mine, his = call(handles, **kw), cumulate_call(handles, **kw)
        assert mine[0] == his[0] != capi.OK and mine[1] == his[1].replace("cumulate", "variance"), (kw, mine, his)
        assert all(h is None for h in mine[2])


def test_refusals_that_read_a_store_leave_the_stand_ins_untouched():
    a, a2, b, t, far = fake(6), fake(6, dtype=3), fake(8), fake(6, tracked=True), fake(6, device=1)
    everyone = (a, a2, b, t, far)
    before = [bytes(x) for x in everyone]
    cases = [
        ([a, None], dict(), capi.ERR_INVALID_ARGUMENT, "store 1 of the batch is NULL"),
        ([a, a2], dict(ndim=33), capi.ERR_INVALID_ARGUMENT, "ndim 33 out of range [0, 32]"),
        ([a, a2], dict(axis=2), capi.ERR_INVALID_ARGUMENT, "axis 2 out of range [0, 2)"),
        ([a, a2], dict(kind=2), capi.ERR_INVALID_ARGUMENT, "variance: kind must be 0 or 1 (got 2)"),
        ([a, a2], dict(ddof=2), capi.ERR_INVALID_ARGUMENT, "variance: ddof must be 0 or 1 (got 2)"),
        ([a, a2], dict(groups=(0, 1, 2)), capi.ERR_INDEX_RANGE, "variance map: entry 2 = 2 is outside the groups (2)"),
        ([a, b], dict(), capi.ERR_LENGTH_MISMATCH, "store holds 8 cells but the dimensions describe 6"),
        ([t, b], dict(), capi.ERR_LENGTH_MISMATCH, "store holds 8 cells but the dimensions describe 6"),
        ([a, a2], dict(lens=(2, 4), groups=(0, 1, 0, 1)), capi.ERR_LENGTH_MISMATCH, "store holds 6 cells but the dimensions describe 8"),
        ([a, a2, far], dict(), capi.ERR_INVALID_ARGUMENT, "variance: the stores live on different devices (0 and 1)"),
        # a tracked store is not refused: the call goes on to the next check
        ([a, t, far], dict(kind=1, ddof=1), capi.ERR_INVALID_ARGUMENT, "variance: the stores live on different devices (0 and 1)"),
        ([a, far], dict(groups=None, n_groups=0xFFFFFFFF), capi.ERR_INVALID_ARGUMENT,  # (n_groups is not read without a map)
         "variance: the stores live on different devices (0 and 1)"),
    ]
    for handles, kw, want_rc, want_message in cases:
        rc, message, outs = call(handles, **kw)
        assert (rc, message) == (want_rc, want_message), (kw, rc, message)
        assert all(h is None for h in outs), want_message  # nothing is created
    assert [bytes(x) for x in everyone] == before


def test_the_planner_reaches_every_form_with_the_shapes_of_the_gpu_test(monkeypatch):
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
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
    assert choice("float32", False, [100, 100, 10000], 2, np.arange(10000) // 12)[::4] == (COLUMN, 1)
    assert choice("float32", False, [100, 2049, 10000])[0] == DIRECT_LANES and choice("float32", False, [100, 2048, 10000])[0] == COLUMN
    # the re-associated form: at most BLOCK_CELLS output cells whose largest group has BLOCK_MEMBERS members or more
    assert (BLOCK_CELLS, BLOCK_MEMBERS) == (65536, 1024)
    for type_name in TYPES:
        for default_is_nan in (False, True):
            assert choice(type_name, default_is_nan, BLOCK_SHAPE)[0] == DIRECT_BLOCK
            assert choice(type_name, default_is_nan, [2, 9000], 1, np.arange(9000) % 2)[0] == DIRECT_BLOCK
            assert choice(type_name, default_is_nan, [1, 10 ** 6])[0] == DIRECT_BLOCK
            assert choice(type_name, default_is_nan, [BLOCK_CELLS, BLOCK_MEMBERS])[0] == DIRECT_BLOCK
            assert choice(type_name, default_is_nan, [BLOCK_CELLS + 1, BLOCK_MEMBERS])[0] == ROW
            assert choice(type_name, default_is_nan, [BLOCK_CELLS, BLOCK_MEMBERS - 1])[0] == ROW
            assert choice(type_name, default_is_nan, [2, BLOCK_MEMBERS, BLOCK_CELLS // 2])[0] == DIRECT_BLOCK
            assert choice(type_name, default_is_nan, [2, BLOCK_MEMBERS, BLOCK_CELLS // 2 + 1])[0] == COLUMN
            assert choice(type_name, default_is_nan, [2, 2 * BLOCK_MEMBERS, 16], 1, np.arange(2 * BLOCK_MEMBERS) % 3)[0] == COLUMN  # groups of 683
            seen.add(DIRECT_BLOCK)
    # the series around the real tile stay in the one-lane forms only with the block cut out of reach
    assert choice("float32", False, [3, 8192])[0] == DIRECT_BLOCK
    monkeypatch.setenv("OLAP_VARIANCE_BLOCK", NEVER)
    assert choice("float32", False, [3, 8192])[0] == ROW and choice("float32", False, [3, 8193])[0] == DIRECT_LANES
    assert choice("float64", False, [3, 4096])[0] == ROW and choice("float64", False, [3, 4097])[0] == DIRECT_LANES
    assert choice("int32", True, [2, 4097], 1, np.arange(4097) % 3)[0] == COLUMN and choice("int32", True, [2, 8197], 1, np.arange(8197) % 2)[0] == DIRECT_LANES
    assert choice("float64", False, BLOCK_SHAPE)[0] == DIRECT_LANES
    monkeypatch.setenv("OLAP_VARIANCE_BLOCK", "100")
    for type_name in TYPES:
        for lens, axis, groups in (([3, 133], 1, None), ([2, 300], 1, None), ([2, 600], 1, np.arange(600) % 2), ([520, 3], 0, None)):
            assert choice(type_name, False, lens, axis, groups)[0] == DIRECT_BLOCK
        assert choice(type_name, False, [3, 99])[0] == ROW
    monkeypatch.delenv("OLAP_VARIANCE_BLOCK")
    monkeypatch.setenv("OLAP_VARIANCE_TILE", str(SMALL_TILE))
    for type_name in TYPES:
        for default_is_nan in (False, True):
            for lens in AROUND_SMALL_TILE:
                c = choice(type_name, default_is_nan, lens)
                assert c[:2] == ((ROW if lens[1] <= SMALL_TILE else DIRECT_LANES), SMALL_TILE), (lens, c)
                seen.add(c[0])
            K = SMALL_TILE + 1
            assert choice(type_name, default_is_nan, [2, K], 1, np.arange(K) % 3)[::4] == (COLUMN, 1)  # narrow rows beyond a tile: the row a slice
            assert choice(type_name, default_is_nan, [2, K, 3], 1, np.arange(K) // 9)[::4] == (COLUMN, 3)
            assert choice(type_name, default_is_nan, [2, 2 * K + 3], 1, np.arange(2 * K + 3) % 2)[0] == DIRECT_LANES
            assert choice(type_name, default_is_nan, [2, K, 16], 1, np.arange(K) % 2)[0] == DIRECT_LANES
            assert choice(type_name, default_is_nan, DIRECT_LANES_SHAPE)[0] == DIRECT_LANES
            assert choice(type_name, default_is_nan, [2, 30, 16], 1, np.arange(30) // 3)[4:] == (16, 4)  # one group of three rows per tile
            assert choice(type_name, default_is_nan, [40, 7])[:3] == (ROW, SMALL_TILE, 9)
    assert seen == {COLUMN, ROW, DIRECT_LANES, DIRECT_BLOCK}
    monkeypatch.setenv("OLAP_VARIANCE_TILE", "1000000")  # the knob only lowers the tile
    assert choice("float32", False, [3, 5])[1] == 8192
    monkeypatch.setenv("OLAP_VARIANCE_TILE", "1")  # a tile below one slot and a dimension without items: a slice of one cell, no division by zero
    assert choice("float32", False, [3, 0, 64])[:2] == (COLUMN, 1) and choice("float32", False, [3, 0, 64])[4:] == (1, 1)
    assert choice("float64", True, [3, 0, 3])[0] == ROW and choice("float32", False, [3, 2, 64])[0] == DIRECT_LANES


def test_the_choice_call_refuses_what_it_cannot_plan():
    c = (C.c_uint32 * 6)()
    L = capi.lib()
    assert L.olap_diag_variance_choice(2, 0, 1, 8, 1, 1, 8, 1, c) == capi.ERR_INVALID_ARGUMENT
    assert L.olap_diag_variance_choice(4, 0, 1, 8, 1, 1, 8, 1, None) == capi.ERR_INVALID_ARGUMENT
    assert L.olap_diag_variance_choice(4, 0, 1, 2 ** 32, 1, 1, 8, 1, c) == capi.ERR_INVALID_ARGUMENT
    assert L.olap_diag_variance_choice(4, 0, 1, 8, 1, 1, 9, 1, c) == capi.ERR_INVALID_ARGUMENT
    assert capi.last_error() == "variance choice: a group of 9 of the dimension's 8 items"


def test_kind_and_ddof_are_not_part_of_the_plan_key():
    env = dict(os.environ, OLAP_PLAN_DRY="1")
    for knob in KNOBS:
        env.pop(knob, None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_variance_dry_worker.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0 and "variance plan keys ok" in r.stdout, r.stdout[-4000:]


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_cube_sends_its_eligible_measures_through_one_call():
    r = subprocess.run([NODE, os.path.join(HERE, "js", "variance_host_test.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " 0 failed" in r.stdout
