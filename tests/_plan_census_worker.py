"""Worker of tests/test_plan_census.py: builds drillUp plans and prints

    shape -> axis | map kind | dtype/default pairs | rules -> kernel_name | Plan.describe()

(one line for the plans of a shape and map that agree in cell size, kernel name and describe())

so that a change to the planner or to the regime decision (drillup_form, olap_kernels.hpp) shows which shapes it moved:
tests/golden/drillup_plan_census.txt holds the lines of the commit before the planner became a unit of its own.

Without arguments (OLAP_PLAN_DRY=1, no device): the shapes of tests/_plan_dry_worker.py, every shape at which
tests/test_gpu_parity.py asserts a kernel name, and a pair of shapes on either side of every threshold the planner and
the launcher use.  With `--device`: the shapes that reach the segmented rows, which dry planning skips — plans only, no
store is allocated and nothing is launched; the first line tells the device's CU count (the sizing depends on it)."""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from conftest import load_package  # noqa: E402

DEVICE = "--device" in sys.argv
assert DEVICE or os.environ.get("OLAP_PLAN_DRY") == "1"
pkg = load_package()
ident = lambda l: np.arange(l, dtype=np.uint32)  # noqa: E731
NAN = float("nan")
TYPES = [("float32", 0.0), ("float32", NAN), ("int32", 0.0), ("uint32", NAN), ("float64", 0.0)]  # as tests/_plan_dry_worker.py
KINDS = ("all", "runs", "interleaved", "random")


def dry_worker_shapes():
    """SHAPES of tests/_plan_dry_worker.py (read, not imported: the module runs on import)"""
    tree = ast.parse(open(os.path.join(HERE, "_plan_dry_worker.py")).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "SHAPES":
            return eval(compile(ast.Expression(node.value), "SHAPES", "eval"), {})
    raise AssertionError("tests/_plan_dry_worker.py has no SHAPES")


def map_of(kind, K, rng):
    """the four map kinds of tests/_plan_dry_worker.py, and the ones the GPU tests build"""
    if K == 0:
        return np.zeros(0, np.uint32), 1
    if kind == "all":
        m = np.zeros(K, np.uint32)
    elif kind == "runs":
        G = max(1, min(K, 1 + K // 31))
        m = np.minimum(np.arange(K) // 31, G - 1)
    elif kind == "interleaved":
        m = np.arange(K) % max(1, min(K, 10))
    elif kind == "random":
        m = rng.integers(0, max(1, min(K, 7)), size=K)
        m = np.unique(m, return_inverse=True)[1]
    elif kind.startswith("mod"):
        m = np.arange(K) % int(kind[3:])
    elif kind.startswith("by"):  # contiguous groups of that many members
        m = np.arange(K) // int(kind[2:])
    elif kind.startswith("even"):  # that many contiguous groups of (nearly) equal length
        g = int(kind[4:])
        m = np.repeat(np.arange(g), np.diff(np.linspace(0, K, g + 1).astype(int)))
    elif kind == "thirds":
        m = np.arange(K) * 3 // K if K >= 3 else np.zeros(K)
    elif kind == "halves":
        m = (np.arange(K) >= K // 3).astype(int)
    elif kind == "calendar":
        days = np.arange(np.datetime64("2010-01-01"), np.datetime64("2010-01-01") + K)
        months = days.astype("datetime64[M]").astype(np.int64)
        m = months - months[0]
    elif kind.startswith("ragged"):  # contiguous groups of 1..n members
        m = np.repeat(np.arange(K), rng.integers(1, int(kind[6:]) + 1, size=K))[:K]
        m = np.unique(m, return_inverse=True)[1]
    elif kind == "scattered":  # many small groups, members anywhere
        first = {}
        m = np.array([first.setdefault(int(g), len(first)) for g in rng.integers(0, max(2, K // 7), size=K)])
    elif kind == "capped":  # all but the last item keep their own group
        m = np.minimum(np.arange(K), K - 2)
    else:
        raise AssertionError(kind)
    m = m.astype(np.uint32)
    return m, int(m.max()) + 1


def fmt_default(d):
    return "nan" if d != d else "0"


def census(cases):
    """cases: (lens, axis, kind, types, env).  Every plan is built; the plans of a case that agree in cell size, kernel name and
    describe() share a line, which lists their dtype/default pairs and rules."""
    rng = np.random.default_rng(46)
    for lens, axis, kind, types, env in cases:
        K = lens[axis]
        gmap, G = map_of(kind, K, rng)
        new = list(lens)
        new[axis] = G
        maps = [gmap if i == axis else ident(l) for i, l in enumerate(lens)]
        for k, v in env.items():
            os.environ[k] = v
        by_rule = {}  # (cell size, rule, name, describe) -> dtype/default pairs
        for t, d in types:
            methods = ["sum"]
            while methods:
                m = methods.pop(0)
                plan = pkg.Plan.drillup(t, d, m, lens, new, maps)
                name = plan.kernel_name
                by_rule.setdefault((np.dtype(t).itemsize, m, name, plan.describe()), []).append("%s/%s" % (t, fmt_default(d)))
                plan.destroy()
                if m == "sum" and any(w in name for w in ("reduce", "split", "segments")):
                    methods = ["product", "highest"]  # the segmented name depends on the rule
        lines = {}  # (cell size, pairs, name, describe) -> rules
        for (size, m, name, desc), pairs in by_rule.items():
            lines.setdefault((size, ",".join(pairs), name, desc), []).append(m)
        for (_size, pairs, name, desc), rules in lines.items():
            print("%s -> axis %d | %s%s | %s | %s -> %s | %s" % (lens, axis, kind, "".join(" %s=%s" % kv for kv in sorted(env.items())), pairs, ",".join(rules),
                                                              name, desc))
        for k in env:
            del os.environ[k]


NO_REDUCE = {"OLAP_REDUCE_MAX_CELLS": "0"}  # as the GPU tests of the tile / gtile / flat regimes set it
F32, F64 = [("float32", 0.0)], [("float64", 0.0)]
BOTH = F32 + F64

# the shapes that reach the segmented rows (wide rows of the few-outputs regime that are not one contiguous '-> all' group
# narrow enough for the 16-byte cooperative form); the first four lie on either side of inner * cell size = 2 048 bytes
SEGMENTED = [([2600, 511], 0, "halves", F32, {}), ([2600, 512], 0, "halves", F32, {}), ([2600, 255], 0, "halves", F64, {}), ([2600, 256], 0, "halves", F64, {}),
             ([3, 900, 516], 1, "interleaved", TYPES, {}), ([1100, 2052], 0, "all", TYPES, {}), ([1500, 514], 0, "all", F64, {}),
             ([10000, 10000], 0, "all", F32, {})]

if DEVICE:
    import torch

    print("# cus=%d" % torch.cuda.get_device_properties(0).multi_processor_count)
    census(SEGMENTED)
    sys.exit(0)

cases = []
# ---- tests/_plan_dry_worker.py ([10**8] as [10**6]: no table beyond a few MB)
for lens, axis in dry_worker_shapes():
    lens = [10 ** 6] if lens == [10 ** 8] else lens
    for kind in KINDS:
        cases.append((lens, axis, kind, TYPES, {}))
# ---- every shape at which tests/test_gpu_parity.py asserts a kernel name
for lens, g in (([7, 1500, 3], 4), ([3, 3652, 10], 10), ([5, 5200, 1], 5)):  # test_group_tile_long_groups_share_output_cells
    cases.append((lens, 1, "even%d" % g, TYPES, NO_REDUCE))
cases.append(([6000, 7], 0, "mod2", TYPES, {}))  # test_split_regime_few_outputs_long_groups
for lens, axis in (([300, 4000], 1), ([5, 70000], 1), ([40000, 200], 0), ([1, 100000], 1), ([100000], 0)):  # test_reduce_regime_shapes
    cases.append((lens, axis, "thirds", F32, {}))
for lens, axis in (([5000, 300], 1), ([4200, 260, 4], 1), ([1000, 264, 8], 1), ([3, 40000, 2], 1), ([100000], 0), ([2000000], 0), ([400000, 10], 0),
                   ([2, 40000, 64], 1), ([70000, 128], 0), ([3, 1000, 12], 1), ([7, 4097, 100], 1), ([2, 9000, 68], 1), ([1, 50000, 24], 1), ([5000, 301], 1),
                   ([3, 40001], 1), ([100001], 0), ([130000, 257], 1)):  # test_reduce_regime_to_all
    cases.append((lens, axis, "all", [("float32", 0.0), ("uint32", NAN), ("float64", NAN)], {}))
for lens, kind in (([7, 3652, 30], "calendar"), ([3, 3653, 5], "calendar"), ([5, 100000, 1], "by30"), ([2, 9000, 3], "ragged40"),
                   ([4, 5000, 127], "ragged30")):  # test_group_tile_regime
    cases.append((lens, 1, kind, [("float32", 0.0), ("float64", NAN), ("uint32", NAN)], {}))
for lens, kind in (([5, 1000, 100], "mod100"), ([3, 900, 12], "mod50"), ([2, 640, 64], "scattered"), ([4, 3000, 8], "mod10"),
                   ([3, 700, 6], "mod35")):  # test_flat_regime_interleaved_groups
    cases.append((lens, 1, kind, [("float32", 0.0), ("float64", NAN), ("uint32", NAN)], NO_REDUCE))
for lens in ([37, 5, 300], [9, 271], [3, 4, 1000]):  # test_tile_regime_long_rows_every_rule
    cases.append((lens, len(lens) - 1, "all", TYPES, NO_REDUCE))
for lens, axis, kind in (([64, 3], 1, "all"), ([2, 6000, 1], 1, "by3"), ([5, 9, 4], 1, "by3")):  # test_product_that_hits_the_default_restarts
    cases.append((lens, axis, kind, [("float64", 0.0), ("float64", NAN)], {}))
for K in (257, 1000):  # test_tile_regime_long_last_dimension
    cases.append(([131500, K], 1, "all", [("float32", 0.0), ("int32", 0.0)], {}))
for outer, K, inner, kind in ((1003, 1000, 1, "mod10"), (1001, 1000, 1, "mod100"), (501, 100, 10, "mod10"), (77, 4096, 1, "scattered"), (1999, 37, 3, "scattered"),
                              (260, 613, 5, "scattered")):  # test_tile_regime_permuted_groups
    cases.append(([outer, K, inner], 1, kind, TYPES, {}))
for lens, axis, kind in (([3000, 132], 0, "all"), ([2, 1500, 256], 1, "all"), ([2600, 200], 0, "halves"), ([3, 900, 516], 1, "interleaved"), ([2100, 250], 0, "all"),
                         ([1200, 1000], 0, "all"), ([1300, 1020], 0, "all"), ([1100, 2052], 0, "all"), ([2001, 251], 0, "all"),
                         ([1500, 514], 0, "all")):  # test_split_regime_wide_rows (dry: the split forms where the device plans segments)
    cases.append((lens, axis, kind, TYPES, {}))
# ---- either side of every threshold
for inner in (508, 512, 127, 129):  # inner / vec 127 | 128: the row regime
    cases.append(([3, 40, inner], 1, "runs", F32, {}))
for K in (4096, 4097):  # K * inner at the tile budget | one cell above, 4-byte cells
    cases += [([5, K, 1], 1, "runs", F32, {}), ([5, K, 1], 1, "mod100", F32, {})]
for K in (2048, 2049):  # ... 8-byte cells
    cases += [([5, K, 1], 1, "runs", F64, {}), ([5, K, 1], 1, "mod100", F64, {})]
cases += [([5, 64, 64], 1, "runs", F32, {}), ([5, 241, 17], 1, "runs", F32, {}), ([5, 32, 64], 1, "runs", F64, {}), ([5, 683, 3], 1, "runs", F64, {})]
# the tile's tables at 16 KiB | beyond (a row that fits the tile holds at most 4 096 members, so contiguous groups end AT 16 KiB:
# 4 095 groups; interleaved ones take 8 bytes per group: 2 048 | 2 049 groups)
cases += [([5, 4096, 1], 1, "capped", F32, {}), ([5, 4096, 1], 1, "mod2048", F32, {}), ([5, 4096, 1], 1, "mod2049", F32, {})]
for K in (255, 256):  # longest group 255 | 256: the few-outputs regime
    cases.append(([K, 7], 0, "all", BOTH, {}))
for outer in (131071, 131072):  # output cells 131 071 | 131 072
    cases.append(([outer, 300], 1, "all", BOTH, {}))
for inner in (128, 129, 1024, 1025, 512, 513, 514):  # the wide 16-byte reduce form: inner 128 | 129, 1 024 | 1 025 (8-byte cells: 512 | 513, 514)
    cases.append(([3000, inner], 0, "all", BOTH, {}))
for K in (1530, 1536):  # shortest group 255 | 256: the cooperative gtile
    cases.append(([8000, K, 3], 1, "even6", BOTH, {}))
for K in (6144, 6150):  # groups per tile 1 024 | 1 025 (groups of three members: the group count cuts the tiles)
    cases.append(([5, K, 1], 1, "by3", F32, {}))
cases += [c for c in SEGMENTED[:4]]  # inner * cell size 2 044 | 2 048: what dry planning makes of them
census(cases)


def null_map_of_an_empty_dimension():
    """The C ABI takes maps[d] == NULL for a dimension without items (the bindings always pass a pointer): K = 0 rolled up to
    three groups, all of them empty."""
    import ctypes as C

    capi = pkg.capi
    ol, nl, inner = (C.c_uint32 * 2)(0, 5), (C.c_uint32 * 2)(3, 5), ident(5)
    maps = (capi._pu32 * 2)(None, inner.ctypes.data_as(capi._pu32))
    h = C.c_void_p()
    capi.check(capi.lib().olap_drillup_plan(C.byref(h), capi.DTYPES["float32"], capi.DEFAULT_ZERO, capi.METHODS["sum"], 2, ol, nl, maps))
    plan = pkg.Plan(h)
    print("[0, 5] -> axis 0 | NULL map, 3 groups | float32/0 | sum -> %s | %s" % (plan.kernel_name, plan.describe()))
    plan.destroy()


null_map_of_an_empty_dimension()
print("census ok")
