"""olap_store_rolling_multi (rolling windows along a dimension) is declared in every layer and refuses bad arguments on
the host before any device work: the same codes and messages with and without a GPU.  The refusals that look into a
store are driven with host-side stand-ins of the handle, which the library only reads; they must stay byte-identical.
olap_diag_rolling_choice (host only) shows that the shape lists of tests/test_rolling_gpu.py reach every form and every
tile border.  Cube.rolling sends its eligible measures through one many-call (tests/js/rolling_host_test.js, with a
stubbed addon)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import load_package
from test_cumulate_host import FakeStore, fake
from test_rolling_gpu import (COLUMNS, DIRECT, EDGE_SHAPES, FORM_SHAPES, GRID_SHAPES, SERIES, STRADDLE_BEFORE, STRADDLE_SHAPES, TYPES, WINDOWS, choice,
                              first_direct, tiles)

pkg = load_package()
capi = pkg.capi
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NODE = shutil.which("node")
NAME = "olap_store_rolling_multi"


def call(handles, n=None, methods=None, lens=(2, 3), ndim=None, axis=1, before=1, after=0, n_groups=2, groups=(0, 1, 0), out=True, method_list=True,
         lens_there=True):
    """handles: FakeStore / address / None entries, or None for a NULL list -> (rc, message, result handles)"""
    addr = lambda h: C.addressof(h) if isinstance(h, FakeStore) else h
    count = (len(handles) if handles is not None else 1) if n is None else n
    hs = (C.c_void_p * max(len(handles), 1))(*[addr(h) for h in handles]) if handles is not None else None
    outs = (C.c_void_p * max(count, 1))() if out else None
    codes = (C.c_int * max(count, 1))(*(methods if methods is not None else [0] * max(count, 1))) if method_list else None
    lv = (C.c_uint32 * max(len(lens), 1))(*lens) if lens_there else None
    g = (C.c_uint32 * max(len(groups), 1))(*groups) if groups is not None else None
    launches = C.c_int(-1)
    rc = capi.lib().olap_store_rolling_multi(count, hs, codes, outs, len(lens) if ndim is None else ndim, lv, axis, before, after, n_groups, g,
                                             C.byref(launches))
    return rc, capi.last_error(), [outs[i] for i in range(count)] if out and count > 0 else []


def test_the_call_is_declared_in_every_layer():
    header = open(os.path.join(ROOT, "include", "olap_hip.h")).read()
    assert re.search(r"\bint %s\(" % NAME, header) and re.search(r"\bint olap_diag_rolling_choice\(", header)
    assert NAME in capi.SIGNATURES and len(capi.SIGNATURES[NAME][1]) == 12
    assert len(getattr(capi.lib(), NAME).argtypes) == 12
    assert len(capi.lib().olap_diag_rolling_choice.argtypes) == 8
    assert callable(pkg.HipStore.rolling) and callable(pkg.HipStore.rolling_multi)
    assert capi.lib().olap_abi_version() == 2
    assert "rollingMulti" in open(os.path.join(ROOT, "olap-in-memory_amd", "napi", "olap_napi.cc")).read()


def test_list_errors_without_stores():
    assert call(None)[:2] == (capi.ERR_INVALID_ARGUMENT, "store / method list is NULL")
    assert call([None], out=False)[:2] == (capi.ERR_INVALID_ARGUMENT, "store / method list is NULL")
    assert call([None], method_list=False)[:2] == (capi.ERR_INVALID_ARGUMENT, "store / method list is NULL")
    assert call([None], n=-1)[:2] == (capi.ERR_INVALID_ARGUMENT, "store / method list is NULL")
    assert call([None])[:2] == (capi.ERR_INVALID_ARGUMENT, "store 0 of the batch is NULL")
    rc, message, outs = call([], n=0)  # nothing to do is no error
    assert rc == capi.OK, message


def test_rules_lengths_axis_window_and_map_are_refused_before_a_store_is_looked_into():
    """The handles here are addresses of nothing: a call that looked into them, or at a device, would not answer like this."""
    nothing = (C.c_char * 8)()
    f = C.addressof(nothing)
    assert call([f, f], methods=[0, 7])[:2] == (capi.ERR_UNSUPPORTED_METHOD, "Unsupported aggregation method: 7")
    assert call([f, f], methods=[-1, 0], ndim=33)[:2] == (capi.ERR_UNSUPPORTED_METHOD, "Unsupported aggregation method: -1")
    assert call([f, f], ndim=33)[:2] == (capi.ERR_INVALID_ARGUMENT, "ndim 33 out of range [0, 32]")
    assert call([f, f], ndim=-1)[:2] == (capi.ERR_INVALID_ARGUMENT, "ndim -1 out of range [0, 32]")
    assert call([f, f], lens_there=False)[:2] == (capi.ERR_INVALID_ARGUMENT, "dimension length vectors must not be NULL")
    assert call([f, f], axis=2)[:2] == (capi.ERR_INVALID_ARGUMENT, "axis 2 out of range [0, 2)")
    assert call([f, f], axis=-1, before=0, after=-1)[:2] == (capi.ERR_INVALID_ARGUMENT, "axis -1 out of range [0, 2)")  # the axis comes first
    assert call([f, f], lens=(), axis=0)[:2] == (capi.ERR_INVALID_ARGUMENT, "axis 0 out of range [0, 0)")
    assert call([f, f], before=1, after=-2)[:2] == (capi.ERR_INVALID_ARGUMENT, "rolling: empty window (before 1, after -2)")
    assert call([f, f], before=-3, after=2, n_groups=4)[:2] == (capi.ERR_INVALID_ARGUMENT, "rolling: empty window (before -3, after 2)")  # before the groups
    assert call([f, f], before=-(2 ** 31), after=-(2 ** 31))[:2] == (capi.ERR_INVALID_ARGUMENT,
                                                                       "rolling: empty window (before -2147483648, after -2147483648)")
    assert call([f, f], groups=(0, 2, 1))[:2] == (capi.ERR_INDEX_RANGE, "rolling map: entry 1 = 2 is outside the groups (2)")
    assert call([f, f], groups=(0, 0, 0), n_groups=0)[:2] == (capi.ERR_INDEX_RANGE, "rolling map: entry 0 = 0 is outside the groups (0)")
    assert call([f, f], n_groups=4)[:2] == (capi.ERR_INVALID_ARGUMENT, "rolling: 4 groups for the 3 items of the dimension")
    assert call([f, f], n_groups=0xFFFFFFFF)[:2] == (capi.ERR_INVALID_ARGUMENT, "rolling: 4294967295 groups for the 3 items of the dimension")


def test_refusals_that_read_a_store_leave_the_stand_ins_untouched():
    a, a2, b, t, far = fake(6), fake(6, dtype=3), fake(8), fake(6, tracked=True), fake(6, device=1)
    everyone = (a, a2, b, t, far)
    held = [bytes(x) for x in everyone]
    cases = [
        ([a, None], dict(), capi.ERR_INVALID_ARGUMENT, "store 1 of the batch is NULL"),
        ([a, a2], dict(methods=[0, 7]), capi.ERR_UNSUPPORTED_METHOD, "Unsupported aggregation method: 7"),
        ([a, a2], dict(ndim=33), capi.ERR_INVALID_ARGUMENT, "ndim 33 out of range [0, 32]"),
        ([a, a2], dict(axis=2), capi.ERR_INVALID_ARGUMENT, "axis 2 out of range [0, 2)"),
        ([a, a2], dict(before=0, after=-1), capi.ERR_INVALID_ARGUMENT, "rolling: empty window (before 0, after -1)"),
        ([a, a2], dict(groups=(0, 1, 2)), capi.ERR_INDEX_RANGE, "rolling map: entry 2 = 2 is outside the groups (2)"),
        ([a, t], dict(), capi.ERR_INVALID_ARGUMENT, "ordered: store 1 of the batch tracks its insertion order; its key order needs the per-item chain"),
        ([a, b], dict(), capi.ERR_LENGTH_MISMATCH, "store holds 8 cells but the dimensions describe 6"),
        ([a, a2], dict(lens=(2, 4), groups=(0, 1, 0, 1)), capi.ERR_LENGTH_MISMATCH, "store holds 6 cells but the dimensions describe 8"),
        ([a, a2, far], dict(), capi.ERR_INVALID_ARGUMENT, "rolling: the stores live on different devices (0 and 1)"),
        ([a, far], dict(groups=None, n_groups=0xFFFFFFFF), capi.ERR_INVALID_ARGUMENT,  # (n_groups is not read without a map)
         "rolling: the stores live on different devices (0 and 1)"),
    ]
    for handles, kw, want_rc, want_message in cases:
        rc, message, outs = call(handles, **kw)
        assert (rc, message) == (want_rc, want_message), (kw, rc, message)
        assert all(h is None for h in outs), want_message  # nothing is created
    assert [bytes(x) for x in everyone] == held


def test_the_choice_diagnostic_refuses_what_the_call_refuses():
    c = (C.c_uint32 * 4)()
    L = capi.lib()
    assert L.olap_diag_rolling_choice(2, 1, 8, 1, 1, 0, 0, c) == capi.ERR_INVALID_ARGUMENT
    assert L.olap_diag_rolling_choice(4, 1, 8, 1, 1, 0, 0, None) == capi.ERR_INVALID_ARGUMENT
    assert L.olap_diag_rolling_choice(4, 1, 8, 1, 1, -2, 0, c) == capi.ERR_INVALID_ARGUMENT
    assert capi.last_error() == "rolling: empty window (before 1, after -2)"
    assert L.olap_diag_rolling_choice(4, 1, 8, 1, 2 ** 31 - 1, 2 ** 31 - 1, 1, c) == capi.OK and tuple(c) == (SERIES, 1, 8, 1)  # beyond +-K: as +-K


def test_the_gpu_shapes_reach_every_form_and_every_tile_border():
    """If the planner's constants change, the assertion that fails names the list whose shapes are to be replaced."""
    forms = {choice(t, lens, b, a)[0] for t in TYPES for lens in FORM_SHAPES for b, a in WINDOWS}
    assert forms == {SERIES, COLUMNS}, "FORM_SHAPES: both tiled forms"
    along = lambda form, d: [(t, lens) for t in TYPES for lens in FORM_SHAPES + STRADDLE_SHAPES for b in (2,) + STRADDLE_BEFORE
                             if choice(t, lens, b)[0] == form and tiles(t, lens, b)[d] > 1]
    assert along(SERIES, 0) and along(COLUMNS, 0), "several tiles along outer"
    assert along(COLUMNS, 2), "FORM_SHAPES: several tiles along inner"
    for form in (SERIES, COLUMNS):
        # windows that straddle a tile border along K: more than one tile there, every float type and window
        cut = [lens for lens in STRADDLE_SHAPES
               if all(choice(t, lens, b)[0] == form and tiles(t, lens, b)[1] > 1 for t in ("float32", "float64") for b in STRADDLE_BEFORE)]
        assert cut, ("STRADDLE_SHAPES", form)
    assert any(choice(t, lens, b)[1] > 1 and -(-lens[0] // choice(t, lens, b)[1]) * choice(t, lens, b)[1] != lens[0]
               for t in TYPES for lens in FORM_SHAPES for b in (2,)), "FORM_SHAPES: a partial last tile of series"
    for t, lens in EDGE_SHAPES:
        over = first_direct(t, lens)
        assert 0 < over < lens[1] and choice(t, lens, over - 1)[0] != DIRECT and choice(t, lens, over) == (DIRECT, 0, 0, 0), (t, lens)
    assert {choice(t, lens, first_direct(t, lens) - 1)[0] for t, lens in EDGE_SHAPES} == {SERIES, COLUMNS}, "EDGE_SHAPES: both tiled forms at their widest"
    for lens in GRID_SHAPES:
        for t in ("float32", "int32"):
            for b, a in ((2, 0), (1, 1)):
                n = tiles(t, lens, b, a)
                assert choice(t, lens, b, a)[0] != DIRECT and n[0] * n[1] * n[2] >= 6, ("GRID_SHAPES", lens, n)


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_cube_sends_its_eligible_measures_through_one_call():
    r = subprocess.run([NODE, os.path.join(HERE, "js", "rolling_host_test.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " 0 failed" in r.stdout
