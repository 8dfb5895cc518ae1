"""olap_store_load_multi / olap_store_reorder_multi (the measures of a cube loaded / reordered in one call) check their
arguments on the host before any device work — the same codes and messages with and without a GPU — and Cube sends the
measures of hydrateFromCube / reorderDimensions through one many-call (tests/js/load_many_host_test.js, with a stubbed
addon).  The store handles here are ctypes stand-ins without buffers: a call that got past its checks would fail on the
device requirement and never touch memory."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import load_package

pkg = load_package()
capi = pkg.capi
HERE = os.path.dirname(os.path.abspath(__file__))
NODE = shutil.which("node")


class FakeStore(C.Structure):
    """struct olap_store (csrc/olap_internal.hpp)"""
    _fields_ = [("size", C.c_uint64), ("dtype", C.c_int), ("default_kind", C.c_int), ("device", C.c_int), ("values", C.c_void_p),
                ("status", C.c_void_p), ("track_order", C.c_bool), ("seq", C.c_void_p), ("next_seq", C.c_uint64), ("maybe_nonempty", C.c_bool),
                ("hi_index", C.c_uint64)]


def fake(size, device=0, dtype=2, default_kind=0, tracked=False):
    s = FakeStore()
    s.size, s.dtype, s.default_kind, s.device, s.next_seq, s.track_order = size, dtype, default_kind, device, 1, tracked
    return s


def snapshot(stores):
    return [bytes(s) for s in stores]


def u32(a):
    return (C.c_uint32 * max(len(a), 1))(*a)


def handles(hs):
    if hs is None:
        return None
    return (C.c_void_p * max(len(hs), 1))(*[C.addressof(h) if isinstance(h, FakeStore) else h for h in hs])


def load(targets, sources, n=None, my=(2, 3), his=(2, 2), maps=None, ndim=None, lens=True):
    """olap_store_load_multi over fakes (None: a NULL list / entry); the default maps put his 2 x 2 cells into my 2 x 3"""
    count = (len(targets) if targets is not None else 1) if n is None else n
    rows = maps if maps not in (None, "null") else [list(range(l)) for l in his]
    keep = [(C.c_int32 * max(len(r), 1))(*r) for r in rows]
    arr = (C.POINTER(C.c_int32) * max(len(rows), 1))(*[C.cast(k, C.POINTER(C.c_int32)) for k in keep])
    launches = C.c_int(-1)
    rc = capi.lib().olap_store_load_multi(count, handles(targets), handles(sources), len(my) if ndim is None else ndim,
                                          u32(my) if lens else None, u32(his) if lens else None, arr if maps != "null" else None,
                                          C.byref(launches))
    return rc, capi.last_error()


def reorder(stores, n=None, old=(2, 3), perm=(1, 0), ndim=None, out=True, with_perm=True):
    count = (len(stores) if stores is not None else 1) if n is None else n
    outs = (C.c_void_p * max(count, 1))() if out else None
    launches = C.c_int(-1)
    p = (C.c_int32 * max(len(perm), 1))(*perm)
    rc = capi.lib().olap_store_reorder_multi(count, handles(stores), outs, len(old) if ndim is None else ndim, u32(old), p if with_perm else None,
                                             C.byref(launches))
    return rc, capi.last_error(), [outs[i] for i in range(count)] if out and count > 0 else []


def test_symbols_are_bound():
    for name in ("olap_store_load_multi", "olap_store_reorder_multi", "olap_load_plan_typed"):
        assert hasattr(capi.lib(), name), name
    for wrapper in ("load_many", "reorder_many"):
        assert callable(getattr(pkg.HipStore, wrapper))
    assert callable(pkg.Plan.load_typed)
    header = open(os.path.join(os.path.dirname(HERE), "include", "olap_hip.h")).read()
    for name in ("olap_store_load_multi", "olap_store_reorder_multi", "olap_load_plan_typed"):
        assert ("int %s(" % name) in header


def test_load_multi_refuses_its_lists_on_the_host():
    t, s = fake(6), fake(4)
    assert load(None, [s]) == (capi.ERR_INVALID_ARGUMENT, "store list is NULL")
    assert load([t], None) == (capi.ERR_INVALID_ARGUMENT, "store list is NULL")
    assert load([t], [s], n=-1) == (capi.ERR_INVALID_ARGUMENT, "store list is NULL")
    assert load([None], [s]) == (capi.ERR_INVALID_ARGUMENT, "store 0 of the batch is NULL")
    assert load([t, fake(6)], [s, None]) == (capi.ERR_INVALID_ARGUMENT, "store 1 of the batch is NULL")
    rc, message = load([], [], n=0)  # nothing to do is no error
    assert rc == capi.OK, message


def test_load_multi_refuses_lengths_maps_sizes_devices_order_and_aliases_on_the_host():
    t, t2, s, s2 = fake(6), fake(6, dtype=3), fake(4), fake(4, dtype=0, default_kind=1)
    stores = [t, t2, s, s2]
    before = snapshot(stores)
    good = ([t, t2], [s, s2])
    assert load(*good, ndim=33) == (capi.ERR_INVALID_ARGUMENT, "ndim 33 out of range [0, 32]")
    assert load(*good, ndim=-1) == (capi.ERR_INVALID_ARGUMENT, "ndim -1 out of range [0, 32]")
    assert load(*good, lens=False) == (capi.ERR_INVALID_ARGUMENT, "dimension length vectors must not be NULL")
    assert load(*good, maps="null") == (capi.ERR_INVALID_ARGUMENT, "his_to_mine is NULL")
    assert load(*good, maps=[[0, 1], [0, 3]]) == (
        capi.ERR_INDEX_RANGE, "load map of dimension 1: entry 1 = 3 is outside this store's dimension (3 items)")
    assert load([t, fake(8)], [s, s2]) == (capi.ERR_LENGTH_MISMATCH, "load: store sizes do not match the dimensions")
    assert load([t, t2], [s, fake(6)]) == (capi.ERR_LENGTH_MISMATCH, "load: store sizes do not match the dimensions")
    assert load([t, t2], [s, fake(4, device=1)]) == (capi.ERR_INVALID_ARGUMENT, "load: the stores live on different devices (0 and 1)")
    rc, message = load([t, fake(6, tracked=True)], [s, s2])
    assert rc == capi.ERR_INVALID_ARGUMENT and message.startswith("ordered: store 1 of the batch tracks its insertion order")
    assert load([t, t], [s, s2]) == (capi.ERR_INVALID_ARGUMENT, "load: store 0 of the batch is a target twice, or a target and a source")
    six = fake(6)
    assert load([t, six], [fake(6), t], his=(2, 3)) == (capi.ERR_INVALID_ARGUMENT, "load: store 0 of the batch is a target twice, or a target and a source")
    assert load([t], [t], his=(2, 3))[0] == capi.ERR_INVALID_ARGUMENT
    # the order of the checks: a map out of range is reported before a size, a size before a tracked target
    assert load([t, fake(8, tracked=True)], [s, s2], maps=[[0, 1], [0, 3]])[0] == capi.ERR_INDEX_RANGE
    assert load([t, fake(8, tracked=True)], [s, s2])[0] == capi.ERR_LENGTH_MISMATCH
    assert snapshot(stores) == before


def test_good_arguments_get_past_the_checks_to_the_device_requirement():
    """Without a device, arguments that are in order (-1 in a map skips an item) reach the device requirement: the refusals
    above were decided before it.  With a device nothing is called: the stand-ins have no buffers to run on."""
    if capi.lib().olap_device_count() > 0:
        return
    rc, message = load([fake(6)], [fake(4, dtype=3)], maps=[[0, -1], [2, -1]])
    assert rc == capi.ERR_NO_DEVICE, message


def test_reorder_multi_refuses_its_arguments_on_the_host():
    a, a2, b, t = fake(6), fake(6), fake(8), fake(6, tracked=True)
    before = snapshot([a, a2, b, t])
    assert reorder(None)[:2] == (capi.ERR_INVALID_ARGUMENT, "store / method list is NULL")
    assert reorder([a], out=False)[:2] == (capi.ERR_INVALID_ARGUMENT, "store / method list is NULL")
    assert reorder([a], n=-1)[:2] == (capi.ERR_INVALID_ARGUMENT, "store / method list is NULL")
    assert reorder([None])[:2] == (capi.ERR_INVALID_ARGUMENT, "store 0 of the batch is NULL")
    assert reorder([a, None])[:2] == (capi.ERR_INVALID_ARGUMENT, "store 1 of the batch is NULL")
    assert reorder([a, a2], ndim=33)[:2] == (capi.ERR_INVALID_ARGUMENT, "ndim 33 out of range [0, 32]")
    rc, message, outs = reorder([a, t])
    assert rc == capi.ERR_INVALID_ARGUMENT and message.startswith("ordered: store 1 of the batch tracks its insertion order") and outs == [None, None]
    rc, message, outs = reorder([a, b])
    assert (rc, message) == (capi.ERR_LENGTH_MISMATCH, "store holds 8 cells but the dimensions describe 6") and outs == [None, None]
    assert reorder([a, a2], with_perm=False)[:2] == (capi.ERR_INVALID_ARGUMENT, "perm is NULL")
    rc, message, outs = reorder([], n=0)
    assert rc == capi.OK, message
    assert snapshot([a, a2, b, t]) == before


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_cube_sends_its_measures_through_one_many_call():
    r = subprocess.run([NODE, os.path.join(HERE, "js", "load_many_host_test.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " 0 failed" in r.stdout
