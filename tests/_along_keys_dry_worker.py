"""Worker of tests/test_cumulate_host.py: with OLAP_PLAN_DRY=1 (no device: plans are built, their tables land in host
memory, nothing is launched) the four calls that run along one dimension get as far as the launch, so their plans land in
the plan cache.  olap_diag_plan_cache_count then shows what one key builder must keep apart and what it must not: the
rule (cumulate, rolling) and q (quantile) travel as launch arguments; shape, axis and map are in every key, rolling's
window as the plan holds it (clipped to the dimension), quantile's tile; and the tag keeps the calls apart.  (kind, ddof
and variance's knobs: tests/_variance_dry_worker.py)"""
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
a = fake(6)


def plans_after(name, extras, rule=None, lens=(2, 3), axis=1, groups=(0, 1, 0), n_groups=2):
    """one store through olap_store_<name>_multi, `extras` between the axis and the groups -> plans in the cache"""
    hs, outs = (C.c_void_p * 1)(C.addressof(a)), (C.c_void_p * 1)()
    rules = () if rule is None else ((C.c_int * 1)(rule),)
    lv = (C.c_uint32 * len(lens))(*lens)
    g = (C.c_uint32 * len(groups))(*groups) if groups is not None else None
    launches = C.c_int(-1)
    rc = getattr(L, "olap_store_%s_multi" % name)(1, hs, *rules, outs, len(lens), lv, axis, *extras, n_groups, g, C.byref(launches))
    assert rc == capi.ERR_NO_DEVICE and "OLAP_PLAN_DRY is set" in capi.last_error(), (name, rc, capi.last_error())  # planned, not launched
    assert outs[0] is None and launches.value == 0
    return L.olap_diag_plan_cache_count()


def cumulate(rule=0, **kw):
    return plans_after("cumulate", (), rule, **kw)


def rolling(before, after, rule=0, **kw):
    return plans_after("rolling", (before, after), rule, **kw)


def quantile(q, **kw):
    return plans_after("quantile", (q,), **kw)


def variance(kind, ddof, **kw):
    return plans_after("variance", (kind, ddof), **kw)


start = L.olap_diag_plan_cache_count()

# cumulate: the rule is not in the key; the map, the axis and shape, and "no map" are
first = cumulate()
assert first == start + 1
for rule in range(1, 7):
    assert cumulate(rule) == first, rule
assert cumulate(groups=(0, 0, 1)) == first + 1  # another map
assert cumulate(3, groups=(0, 0, 1)) == first + 1
assert cumulate(lens=(3, 2), axis=0) == first + 2  # another shape and axis
assert cumulate(groups=None) == first + 3  # no map
assert cumulate(5, groups=None, n_groups=7) == first + 3  # (n_groups is not read without a map)
count = first + 3
assert cumulate() == count  # the first plan is still there

# rolling: the rule is not in the key; before and after are, as the plan holds them (beyond +-K they act as +-K)
assert rolling(3, 0) == count + 1  # a cumulate plan of this shape and map is there already: the tag keeps them apart
for rule in range(1, 7):
    assert rolling(3, 0, rule) == count + 1, rule
assert rolling(2000000000, 0) == count + 1  # before = K and before >> K: one plan
assert rolling(2, 0) == count + 2
assert rolling(3, 1) == count + 3
assert rolling(3, 3) == count + 4
assert rolling(3, 2000000000) == count + 4  # after is clipped as before is
assert rolling(3, -3) == count + 5
assert rolling(2000000000, -2000000000) == count + 5  # ... on both sides
assert rolling(3, 0, groups=None) == count + 6  # no map
count += 6

# quantile: q is not in the key; OLAP_QUANTILE_TILE is
assert quantile(0.5) == count + 1
for q in (0.0, 0.25, 1.0):
    assert quantile(q) == count + 1, q
os.environ["OLAP_QUANTILE_TILE"] = "64"
assert quantile(0.5) == count + 2
assert quantile(0.9) == count + 2
del os.environ["OLAP_QUANTILE_TILE"]
assert quantile(0.9) == count + 2  # the plan of the real tile is still there
count += 2

# across the calls: one shape, one map, four plans
assert variance(0, 0) == count + 1
assert cumulate() == count + 1 and rolling(3, 0) == count + 1 and quantile(0.5) == count + 1 and variance(1, 1) == count + 1
count += 1
assert cumulate(groups=(1, 0, 1)) == count + 1
assert rolling(3, 0, groups=(1, 0, 1)) == count + 2
assert quantile(0.5, groups=(1, 0, 1)) == count + 3
assert variance(0, 0, groups=(1, 0, 1)) == count + 4
print("along-axis plan keys ok")
