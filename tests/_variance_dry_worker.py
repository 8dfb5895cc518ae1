"""Worker of tests/test_variance_host.py: with OLAP_PLAN_DRY=1 (no device: plans are built, their tables land in host
memory, nothing is launched) olap_store_variance_multi gets as far as the launch, so its plans land in the plan cache.
olap_diag_plan_cache_count then shows what the plan-cache key holds — cell type, default, shape, axis, map, the tile and
the block cut — and what it does not: kind and ddof."""
import ctypes as C
import os
import sys

assert os.environ.get("OLAP_PLAN_DRY") == "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from conftest import load_package  # noqa: E402
from test_cumulate_host import fake  # noqa: E402

pkg = load_package()
capi = pkg.capi
L = capi.lib()


def call(store, kind, ddof, lens=(2, 3), axis=1, groups=(0, 1, 0), n_groups=2):
    hs, outs = (C.c_void_p * 1)(C.addressof(store)), (C.c_void_p * 1)()
    lv = (C.c_uint32 * len(lens))(*lens)
    g = (C.c_uint32 * len(groups))(*groups) if groups is not None else None
    launches = C.c_int(-1)
    rc = L.olap_store_variance_multi(1, hs, outs, len(lens), lv, axis, kind, ddof, n_groups, g, C.byref(launches))
    assert rc == capi.ERR_NO_DEVICE and "OLAP_PLAN_DRY is set" in capi.last_error(), (rc, capi.last_error())  # planned, not launched
    assert outs[0] is None and launches.value == 0
    return L.olap_diag_plan_cache_count()


a, b = fake(6), fake(6, dtype=3)
start = L.olap_diag_plan_cache_count()
first = call(a, 0, 0)
assert first == start + 1
for kind, ddof in ((0, 1), (1, 0), (1, 1), (0, 0)):
    assert call(a, kind, ddof) == first, (kind, ddof)  # kind and ddof travel as launch arguments
hs, outs = (C.c_void_p * 1)(C.addressof(a)), (C.c_void_p * 1)()
lv, g = (C.c_uint32 * 2)(2, 3), (C.c_uint32 * 3)(0, 1, 0)
assert L.olap_store_variance_multi(1, hs, outs, 2, lv, 1, 2, 0, 2, g, None) == capi.ERR_INVALID_ARGUMENT  # refused before any plan
assert L.olap_diag_plan_cache_count() == first
assert call(b, 1, 1) == first + 1  # another cell type
assert call(a, 1, 0, groups=(0, 0, 1)) == first + 2  # another map
assert call(a, 0, 1, groups=None) == first + 3  # no map
assert call(a, 0, 0, lens=(3, 2), axis=0) == first + 4  # another shape and axis
os.environ["OLAP_VARIANCE_TILE"] = "64"
assert call(a, 0, 0) == first + 5  # the tile is part of the key ...
assert call(a, 1, 1) == first + 5
del os.environ["OLAP_VARIANCE_TILE"]
assert call(a, 1, 1) == first + 5  # ... and the plan of the real tile is still there
os.environ["OLAP_VARIANCE_BLOCK"] = "2"
assert call(a, 0, 0) == first + 6  # so is the block cut
print("variance plan keys ok")
