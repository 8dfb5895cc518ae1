"""olap_store_dice_multi / olap_store_dice_drillup_multi / olap_store_drilldown_multi (dice, slice and drillDown of ALL
stored measures of a cube in one call) check their arguments on the host before any device work — the same codes and
messages with and without a GPU — and Cube sends the measures of one operation through one many-call
(tests/js/multi_gather_host_test.js, with a stubbed addon)."""
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

NAMES = ["olap_store_dice_multi", "olap_store_dice_drillup_multi", "olap_store_drilldown_multi"]


def u32(a):
    return (C.c_uint32 * max(len(a), 1))(*a)


def tables(rows, ctype):
    keep = [(ctype * max(len(r), 1))(*r) for r in rows]
    arr = (C.POINTER(ctype) * max(len(rows), 1))(*[C.cast(k, C.POINTER(ctype)) for k in keep])
    return keep, arr


def call(name, handles, n=None, methods=None, old=(2, 3), new=(2, 2), ndim=None, out=True):
    """handles: a list of store handles / None entries, or None for a NULL list.  The tables select / refine dimension 1."""
    count = (len(handles) if handles is not None else 1) if n is None else n
    hs = (C.c_void_p * max(len(handles), 1))(*handles) if handles is not None else None
    outs = (C.c_void_p * max(count, 1))() if out else None
    launches = C.c_int(-1)
    codes = (C.c_int * max(count, 1))(*(methods if methods is not None else [0] * max(count, 1)))
    nd = len(old) if ndim is None else ndim
    L = capi.lib()
    if name == "olap_store_dice_multi":
        keep, sel = tables([range(l) for l in new], C.c_int32)
        rc = L.olap_store_dice_multi(count, hs, outs, nd, u32(old), u32(new), sel, C.byref(launches))
    elif name == "olap_store_dice_drillup_multi":
        keep, sel = tables([range(l) for l in new], C.c_int32)
        keep2, maps = tables([[0] * l for l in new], C.c_uint32)
        rc = L.olap_store_dice_drillup_multi(count, hs, codes, outs, nd, u32(old), u32(new), u32([1] * len(new)), sel, maps, C.byref(launches))
    else:
        keep, maps = tables([[j % o for j in range(l)] for o, l in zip(old, new)], C.c_uint32)
        rc = L.olap_store_drilldown_multi(count, hs, codes, outs, nd, u32(old), u32(new), maps, C.byref(launches))
    return rc, capi.last_error(), [outs[i] for i in range(count)] if out and count > 0 else []


def test_symbols_are_bound():
    for name in NAMES:
        assert hasattr(capi.lib(), name), name
    for wrapper in ("dice_multi", "dice_drillup_multi", "drill_down_multi"):
        assert callable(getattr(pkg.HipStore, wrapper))


@pytest.mark.parametrize("name", NAMES)
def test_list_errors_without_stores(name):
    """Everything that is refused without looking into a store: the same answers on a machine with no device."""
    assert call(name, None)[:2] == (capi.ERR_INVALID_ARGUMENT, "store / method list is NULL")
    assert call(name, [None], out=False)[:2] == (capi.ERR_INVALID_ARGUMENT, "store / method list is NULL")
    assert call(name, [None], n=-1)[:2] == (capi.ERR_INVALID_ARGUMENT, "store / method list is NULL")
    assert call(name, [None])[:2] == (capi.ERR_INVALID_ARGUMENT, "store 0 of the batch is NULL")
    rc, message, outs = call(name, [], n=0)  # nothing to do is no error
    assert rc == capi.OK, message


@pytest.mark.parametrize("name", NAMES)
def test_rules_and_lengths_are_refused_before_a_store_is_looked_into(name):
    """A rule out of range and ndim out of range are decided from the lists alone: the entries only have to be there.  The
    handles here are addresses of nothing — a call that looked into them, or at a device, would not answer like this."""
    nothing = (C.c_char * 8)()
    fake = C.addressof(nothing)
    assert call(name, [fake, fake], ndim=33)[:2] == (capi.ERR_INVALID_ARGUMENT, "ndim 33 out of range [0, 32]")
    assert call(name, [fake, fake], ndim=-1)[:2] == (capi.ERR_INVALID_ARGUMENT, "ndim -1 out of range [0, 32]")
    if name != "olap_store_dice_multi":
        assert call(name, [fake, fake], methods=[0, 7])[:2] == (capi.ERR_UNSUPPORTED_METHOD, "Unsupported aggregation method: 7")
        assert call(name, [fake, fake], methods=[-1, 0], ndim=33)[:2] == (capi.ERR_UNSUPPORTED_METHOD, "Unsupported aggregation method: -1")


def store_errors(name, a, a2, b, tracked):
    """every refusal that needs a store handle: [(what, rc, message, results), ...]"""
    A, A2, B, T = a._h.value, a2._h.value, b._h.value, tracked._h.value
    calls = [
        ("a NULL handle behind a good one", lambda: call(name, [A, None])),
        ("tracked store", lambda: call(name, [A, T])),
        ("8 cells, dimensions describe 6", lambda: call(name, [A, B])),
        ("6 cells, dimensions describe 8", lambda: call(name, [A, A2], old=(2, 4), new=(2, 4))),
        ("33 dimensions", lambda: call(name, [A, A2], ndim=33)),
    ]
    if name != "olap_store_dice_multi":
        calls += [("rule code above product", lambda: call(name, [A, A2], methods=[0, 7])),
                  ("rule code below sum", lambda: call(name, [A, A2], methods=[-1, 0]))]
    return [(what,) + f() for what, f in calls]


EXPECTED_STORE_ERRORS = [
    (capi.ERR_INVALID_ARGUMENT, "store 1 of the batch is NULL"),
    (capi.ERR_INVALID_ARGUMENT, "ordered: store 1 of the batch tracks its insertion order"),
    (capi.ERR_LENGTH_MISMATCH, "store holds 8 cells but the dimensions describe 6"),
    (capi.ERR_LENGTH_MISMATCH, "store holds 6 cells but the dimensions describe 8"),
    (capi.ERR_INVALID_ARGUMENT, "ndim 33 out of range"),
    (capi.ERR_UNSUPPORTED_METHOD, "Unsupported aggregation method: 7"),
    (capi.ERR_UNSUPPORTED_METHOD, "Unsupported aggregation method: -1"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_argument_errors_with_stores_return_no_store_and_leave_the_inputs_unchanged(name):
    """Store handles exist only where a device does.  Every refusal comes with the code and message of the host checks,
    returns no store, leaves the inputs as they were, and the store-free refusals answer as they do without a device."""
    a = pkg.HipStore(6, "float32", 0.0)
    a.set_data_f64(np.arange(6.0))
    a2 = pkg.HipStore(6, "float32", 0.0)
    a2.set_data_f64(np.arange(6.0) * 2)
    b = pkg.HipStore(8, "float32", 0.0)
    t = pkg.HipStore(6, "float32", 0.0)
    capi.check(capi.lib().olap_store_track_order(t._h, 1))
    t.set_data_f64(np.arange(6.0) + 1)
    before = [x.get_data_f64().tobytes() for x in (a, a2, b, t)]
    got = store_errors(name, a, a2, b, t)
    assert len(got) == (5 if name == "olap_store_dice_multi" else 7)
    for (what, rc, message, outs), (want_rc, want_message) in zip(got, EXPECTED_STORE_ERRORS):
        assert rc == want_rc and want_message in message, (what, rc, message)
        assert all(h is None for h in outs), what
    assert [m for w, _, m, _ in got if w == "tracked store"][0].startswith("ordered:")
    test_list_errors_without_stores(name)
    assert [x.get_data_f64().tobytes() for x in (a, a2, b, t)] == before


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_cube_sends_its_measures_through_one_many_call():
    r = subprocess.run([NODE, os.path.join(HERE, "js", "multi_gather_host_test.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-6000:]
    assert " 0 failed" in r.stdout
