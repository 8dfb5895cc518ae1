"""olap_store_compose_multi (the measures of one source cube brought onto a composed cube's dimensions in one call)
checks its arguments on the host before any device work — the same codes and messages with and without a GPU, no store
created and out[] untouched — and Cube.compose sends the measures of each source cube through one composeMulti
(tests/js/compose_many_host_test.js, with a stubbed addon).  The store handles here are ctypes stand-ins without
buffers: a call that got past its checks would fail on the device requirement and never touch memory."""
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
SENTINEL = 0x5A5A5A5A


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


def compose(sources, n=None, my=(2, 3), his=(2, 2), maps=None, ndim=None, lens=True, out=True, fills=True):
    """olap_store_compose_multi over fakes (None: a NULL list / entry); the default maps put his 2 x 2 cells into my 2 x 3.
    Returns (code, message, out[] afterwards, launches)."""
    count = (len(sources) if sources is not None else 1) if n is None else n
    rows = maps if maps not in (None, "null") else [list(range(l)) for l in his]
    keep = [(C.c_int32 * max(len(r), 1))(*r) for r in rows]
    arr = (C.POINTER(C.c_int32) * max(len(rows), 1))(*[C.cast(k, C.POINTER(C.c_int32)) for k in keep])
    slots = max(count, 1)
    outs = (C.c_void_p * slots)(*[SENTINEL] * slots) if out else None
    launches = C.c_int(-1)
    values = (C.c_double * slots)(*[7.0] * slots) if fills else None
    has = (C.c_uint8 * slots)(*[1] * slots) if fills else None
    rc = capi.lib().olap_store_compose_multi(count, handles(sources), values, has, outs, len(my) if ndim is None else ndim,
                                             u32(my) if lens else None, u32(his) if lens else None, arr if maps != "null" else None,
                                             C.byref(launches))
    return rc, capi.last_error(), [outs[i] for i in range(slots)] if out else None, launches.value


def refused(result, code, message=None, starts=None):
    rc, text, outs, launches = result
    assert rc == code, (rc, text)
    if message is not None:
        assert text == message
    if starts is not None:
        assert text.startswith(starts), text
    assert outs is None or all(o == SENTINEL for o in outs), "out[] was written"
    assert launches == 0
    return True


def test_symbols_are_bound():
    for name in ("olap_store_compose_multi", "olap_compose_plan"):
        assert hasattr(capi.lib(), name), name
    assert callable(pkg.HipStore.compose_many) and callable(pkg.Plan.compose)
    header = open(os.path.join(os.path.dirname(HERE), "include", "olap_hip.h")).read()
    for name in ("olap_store_compose_multi", "olap_compose_plan"):
        assert ("int %s(" % name) in header


def test_compose_multi_refuses_its_arguments_on_the_host_in_order():
    s, s2 = fake(4), fake(4, dtype=0, default_kind=1)
    stores = [s, s2]
    before = snapshot(stores)
    # 1. the list, 2. its entries
    assert refused(compose(None), capi.ERR_INVALID_ARGUMENT, "store list is NULL")
    assert refused(compose([s], n=-1), capi.ERR_INVALID_ARGUMENT, "store list is NULL")
    assert refused(compose([None]), capi.ERR_INVALID_ARGUMENT, "store 0 of the batch is NULL")
    assert refused(compose([s, None]), capi.ERR_INVALID_ARGUMENT, "store 1 of the batch is NULL")
    # 3. ndim, the length vectors and the map entries: the load checks
    assert refused(compose(stores, ndim=33), capi.ERR_INVALID_ARGUMENT, "ndim 33 out of range [0, 32]")
    assert refused(compose(stores, ndim=-1), capi.ERR_INVALID_ARGUMENT, "ndim -1 out of range [0, 32]")
    assert refused(compose(stores, lens=False), capi.ERR_INVALID_ARGUMENT, "dimension length vectors must not be NULL")
    assert refused(compose(stores, maps="null"), capi.ERR_INVALID_ARGUMENT, "his_to_mine is NULL")
    assert refused(compose(stores, maps=[[0, 1], [0, 3]]), capi.ERR_INDEX_RANGE,
                   "load map of dimension 1: entry 1 = 3 is outside this store's dimension (3 items)")
    # 4. sizes, 5. devices, 6. tracked sources, 7. out
    assert refused(compose([s, fake(6)]), capi.ERR_LENGTH_MISMATCH, "compose: store sizes do not match the dimensions")
    assert refused(compose([s, fake(4, device=1)]), capi.ERR_INVALID_ARGUMENT, "compose: the stores live on different devices (0 and 1)")
    assert refused(compose([s, fake(4, tracked=True)]), capi.ERR_INVALID_ARGUMENT, starts="ordered: store 1 of the batch tracks its insertion order")
    assert refused(compose(stores, out=False), capi.ERR_INVALID_ARGUMENT, "out is NULL")
    # the order: a NULL entry before ndim, a map before a size, a size before a device, a device before a tracked source,
    # a tracked source before a NULL out
    assert refused(compose([s, None], ndim=33), capi.ERR_INVALID_ARGUMENT, "store 1 of the batch is NULL")
    assert refused(compose([s, fake(6, device=1)], maps=[[0, 1], [0, 3]]), capi.ERR_INDEX_RANGE)
    assert refused(compose([s, fake(6, device=1, tracked=True)]), capi.ERR_LENGTH_MISMATCH)
    assert refused(compose([s, fake(4, device=1, tracked=True)]), capi.ERR_INVALID_ARGUMENT, starts="compose: the stores live on different devices")
    assert refused(compose([s, fake(4, tracked=True)], out=False), capi.ERR_INVALID_ARGUMENT, starts="ordered:")
    assert snapshot(stores) == before


def test_nothing_to_do_is_no_error():
    rc, message, outs, launches = compose([], n=0)
    assert rc == capi.OK, message
    assert outs == [SENTINEL] and launches == 0
    rc, message, _, launches = compose(None, n=0, out=False, fills=False)
    assert rc == capi.OK and launches == 0, message


def test_good_arguments_get_past_the_checks_to_the_device_requirement():
    """Without a device, arguments that are in order (-1 in a map skips an item; no fills) reach the device requirement: the
    refusals above were decided before it.  With a device nothing is called: the stand-ins have no buffers to run on."""
    if capi.lib().olap_device_count() > 0:
        return
    assert refused(compose([fake(4, dtype=3)], maps=[[0, -1], [2, -1]], fills=False), capi.ERR_NO_DEVICE)
    assert refused(compose([fake(1)], my=(), his=(), maps=[]), capi.ERR_NO_DEVICE)


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_cube_sends_the_measures_of_each_source_through_one_compose_call():
    r = subprocess.run([NODE, os.path.join(HERE, "js", "compose_many_host_test.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " 0 failed" in r.stdout
