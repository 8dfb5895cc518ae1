"""olap_store_blocks_report (Cube.scan / iterateOverDimension in one device pass) checks its arguments on the host before
any device work — the same codes and messages with and without a GPU — and Cube sends a scan through one blocksReport
call and serves the handed-out cubes from the host (tests/js/scan_blocks_host_test.js, with a stubbed addon).  The store
handles here are ctypes stand-ins without buffers: a call that got past its checks would fail on the device requirement
and never touch memory."""
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


def handles(hs):
    if hs is None:
        return None
    return (C.c_void_p * max(len(hs), 1))(*[C.addressof(h) if isinstance(h, FakeStore) else h for h in hs])


def blocks(stores, n=None, lens=(2, 3), scanned=(1, 0), ndim=None, with_lens=True, with_flags=True, out=True):
    """olap_store_blocks_report over fakes (None: a NULL list / entry)"""
    count = (len(stores) if stores is not None else 1) if n is None else n
    lv = (C.c_uint32 * max(len(lens), 1))(*lens)
    flags = (C.c_uint8 * max(len(scanned), 1))(*scanned)
    cells = 1
    for l in lens:
        cells *= l
    result = (C.c_double * max(count * cells, 1))() if out else None
    launches = C.c_int(-1)
    rc = capi.lib().olap_store_blocks_report(count, handles(stores), len(lens) if ndim is None else ndim, lv if with_lens else None,
                                             flags if with_flags else None, result, C.byref(launches))
    return rc, capi.last_error()


def test_symbol_is_bound():
    assert hasattr(capi.lib(), "olap_store_blocks_report")
    import sys
    assert callable(sys.modules[pkg.HipStore.__module__].blocks_report)
    header = open(os.path.join(os.path.dirname(HERE), "include", "olap_hip.h")).read()
    assert "int olap_store_blocks_report(" in header
    assert "#define OLAP_BLOCKS_MAX_BYTES (1ull << 30)" in header


def test_refuses_its_lists_and_lengths_on_the_host():
    a, b = fake(6), fake(6, dtype=0, default_kind=1)
    before = [bytes(a), bytes(b)]
    assert blocks(None) == (capi.ERR_INVALID_ARGUMENT, "store list is NULL")
    assert blocks([a], n=-1) == (capi.ERR_INVALID_ARGUMENT, "store list is NULL")
    assert blocks([a], out=False) == (capi.ERR_INVALID_ARGUMENT, "store list is NULL")
    assert blocks([None]) == (capi.ERR_INVALID_ARGUMENT, "store 0 of the batch is NULL")
    assert blocks([a, None]) == (capi.ERR_INVALID_ARGUMENT, "store 1 of the batch is NULL")
    assert blocks([a, b], ndim=33) == (capi.ERR_INVALID_ARGUMENT, "ndim 33 out of range [0, 32]")
    assert blocks([a, b], ndim=-1) == (capi.ERR_INVALID_ARGUMENT, "ndim -1 out of range [0, 32]")
    assert blocks([a, b], with_lens=False) == (capi.ERR_INVALID_ARGUMENT, "dimension length vectors must not be NULL")
    assert blocks([a, b], with_flags=False) == (capi.ERR_INVALID_ARGUMENT, "scanned flags are NULL")
    assert blocks([a, b], scanned=(0, 0)) == (capi.ERR_INVALID_ARGUMENT, "blocks: no dimension is scanned")
    assert blocks([a, b], lens=(), scanned=()) == (capi.ERR_INVALID_ARGUMENT, "blocks: no dimension is scanned")
    assert blocks([fake(0)], lens=(0, 3), scanned=(1, 0)) == (capi.ERR_INVALID_ARGUMENT, "blocks: a dimension has no items")  # C == 0
    assert blocks([fake(0)], lens=(2, 0), scanned=(1, 0)) == (capi.ERR_INVALID_ARGUMENT, "blocks: a dimension has no items")  # B == 0
    rc, message = blocks([], n=0)  # nothing to do is no error
    assert rc == capi.OK, message
    assert [bytes(a), bytes(b)] == before


def test_refuses_sizes_devices_order_and_the_cap_on_the_host(monkeypatch):
    a, b = fake(6), fake(6, dtype=3)
    assert blocks([a, fake(8)]) == (capi.ERR_LENGTH_MISMATCH, "store holds 8 cells but the dimensions describe 6")
    assert blocks([a, fake(6, device=1)]) == (capi.ERR_INVALID_ARGUMENT, "blocks: the stores live on different devices (0 and 1)")
    rc, message = blocks([a, fake(6, tracked=True)])
    assert rc == capi.ERR_INVALID_ARGUMENT and message.startswith("ordered: store 1 of the batch tracks its insertion order")
    monkeypatch.setenv("OLAP_BLOCKS_MAX_BYTES", "95")  # two stores of 6 cells are 96 bytes
    rc, message = blocks([a, b])
    assert rc == capi.ERR_INVALID_ARGUMENT and message.startswith("blocks: 2 stores of 6 cells")
    # the environment only lowers the cap: the compiled one (1 GiB) holds against a larger value
    monkeypatch.setenv("OLAP_BLOCKS_MAX_BYTES", str(1 << 40))
    big, big2 = fake(1 << 27), fake(1 << 27)
    lv = (1 << 13, 1 << 14)
    launches = C.c_int(-1)
    one = (C.c_double * 1)()  # never written: the call is refused
    rc = capi.lib().olap_store_blocks_report(2, handles([big, big2]), 2, (C.c_uint32 * 2)(*lv), (C.c_uint8 * 2)(1, 0), one, C.byref(launches))
    assert rc == capi.ERR_INVALID_ARGUMENT and capi.last_error().startswith("blocks: 2 stores of 134217728 cells")
    monkeypatch.delenv("OLAP_BLOCKS_MAX_BYTES")
    # the order of the checks: no scanned dimension before a size, a size before a device, a device before a tracked
    # store, a tracked store before the cap
    monkeypatch.setenv("OLAP_BLOCKS_MAX_BYTES", "8")
    assert blocks([a, fake(8, device=1, tracked=True)], scanned=(0, 0))[1] == "blocks: no dimension is scanned"
    assert blocks([a, fake(8, device=1, tracked=True)])[0] == capi.ERR_LENGTH_MISMATCH
    assert blocks([a, fake(6, device=1, tracked=True)])[1].startswith("blocks: the stores live on different devices")
    assert blocks([a, fake(6, tracked=True)])[1].startswith("ordered: ")
    assert blocks([a, b])[1].startswith("blocks: 2 stores")


def test_good_arguments_get_past_the_checks_to_the_device_requirement():
    """Without a device, arguments that are in order reach the device requirement: the refusals above were decided before
    it.  With a device nothing is called: the stand-ins have no buffers to run on."""
    if capi.lib().olap_device_count() > 0:
        return
    rc, message = blocks([fake(6), fake(6, dtype=0, default_kind=1)])
    assert rc == capi.ERR_NO_DEVICE, message


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_cube_scans_through_one_device_call():
    r = subprocess.run([NODE, os.path.join(HERE, "js", "scan_blocks_host_test.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " 0 failed" in r.stdout
