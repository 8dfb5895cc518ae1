#!/usr/bin/env python3
"""Developer tool: load between cell types on the device and load of several measures in one call.

  (a) load float64 -> float32 of a 10^7-cell cube through olap_store_load_multi against the two-step path it replaces
      (the other store's cells to the host as float64, back into a store of my type, then a same-type load)
  (b) same-type load of 1, 4 and 8 measures of 10^6 cells as n olap_store_load calls and as one olap_store_load_multi,
      in alternating rounds (the two paths take turns at going first), with the per-measure path against itself (A/A)
  (c) the same multi call with tables it has not seen (the plan is built and its tables uploaded) against its repeat
      (the plan comes from the cache)
  (d) the converting kernels at 10^8 cells next to the same-type load_scatter kernels of the same target type and of
      the wider of the two types (a converting load moves no more bytes than the wider same-type one)

Host clock around REPS back-to-back calls that end in a device synchronise; medians over the rounds.
`--single-load` prints only the same-type single-store loads, tagged with the library in use (OLAP_LIBOLAPGPU selects
another build): run alternately with two builds inside one GPU call to compare them.
Usage: python tools/load_bench.py [out.txt] [--rounds N] [--single-load]
"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from conftest import load_package  # noqa: E402

pkg = load_package()
HipStore, Plan, capi = pkg.HipStore, pkg.Plan, pkg.capi
_tables = pkg.hipstore._tables
if "--single-load" in sys.argv:  # a build from before this tool lacks the newer symbols: bind what it has
    _probe = C.CDLL(capi.lib_path())
    capi.SIGNATURES = {k: v for k, v in capi.SIGNATURES.items() if hasattr(_probe, k)}
L = capi.lib()
SIZE = {"int32": 4, "uint32": 4, "float32": 4, "float64": 8}


def pu(a):
    return a.ctypes.data_as(capi._pu32)


def sync():
    capi.check(L.olap_device_synchronize())


def clock(fn, reps):
    """us per call: reps calls back to back, then a device synchronise"""
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) * 1e6 / reps


def filled(cells, type_name, default=0.0, seed=7):
    s = HipStore(cells, type_name, default)
    capi.check(L.olap_fill_seeded(s.values_ptr, None, cells, 0, capi.DTYPES[type_name], seed, 0.6, None))
    capi.check(L.olap_canonicalize(s.values_ptr, None, cells, capi.DTYPES[type_name], capi.DEFAULT_ZERO, 0, None))
    return s


def outer_maps(my_len, his_len, shift=1):
    """his items of dimension 0 land `shift` items further on in mine (which has more); the other dimensions are left alone"""
    return [np.arange(his_len[0], dtype=np.int32) + shift] + [np.arange(l, dtype=np.int32) for l in his_len[1:]]


def inner_maps(lens, seed=3):
    """the items of the last dimension scattered, the others left alone"""
    rng = np.random.default_rng(seed)
    return [np.arange(l, dtype=np.int32) for l in lens[:-1]] + [rng.permutation(lens[-1]).astype(np.int32)]


def medians(paths, rounds, reps):
    """paths: [(name, fn)]; alternating order, two warm-up rounds"""
    t = {name: [] for name, _ in paths}
    for r in range(-2, rounds):
        for name, fn in (paths if r % 2 == 0 else paths[::-1]):
            us = clock(fn, reps)
            if r >= 0:
                t[name].append(us)
    return {k: statistics.median(v) for k, v in t.items()}


def load_call(mine, his, my_len, his_len, maps, keep):
    ml, hl = np.asarray(my_len, np.uint32), np.asarray(his_len, np.uint32)
    k, arr = _tables(maps, np.int32, C.c_int32)
    keep.append((ml, hl, k, arr))
    return lambda: capi.check(L.olap_store_load(mine._h, his._h, len(ml), pu(ml), pu(hl), arr))


def multi_call(targets, sources, my_len, his_len, maps, keep):
    ml, hl = np.asarray(my_len, np.uint32), np.asarray(his_len, np.uint32)
    k, arr = _tables(maps, np.int32, C.c_int32)
    n = len(targets)
    ts, ss = (C.c_void_p * n)(*[s._h.value for s in targets]), (C.c_void_p * n)(*[s._h.value for s in sources])
    launches = C.c_int(0)
    keep.append((ml, hl, k, arr, ts, ss, launches))
    return lambda: capi.check(L.olap_store_load_multi(n, ts, ss, len(ml), pu(ml), pu(hl), arr, C.byref(launches))), launches


def single_loads(say, rounds):
    tag = "prev" if os.environ.get("OLAP_LIBOLAPGPU") else "this"
    keep = []
    for type_name in ("float32", "float64"):
        for label, my_len, his_len, maps in [("10^6 cells, outer dimension remapped", [12, 100, 1000], [10, 100, 1000], None),
                                             ("10^6 cells, innermost dimension scattered", [10, 100, 1000], [10, 100, 1000], "inner"),
                                             ("10^8 cells, outer dimension remapped", [12] + [10] * 7, [10] * 8, None)]:
            maps = inner_maps(his_len) if maps == "inner" else outer_maps(my_len, his_len)
            mine, his = filled(int(np.prod(my_len)), type_name), filled(int(np.prod(his_len)), type_name, seed=11)
            m = medians([("load", load_call(mine, his, my_len, his_len, maps, keep))], rounds, 20 if "10^6" in label else 5)
            say("%s %-8s %-44s %9.1f us" % (tag, type_name, label, m["load"]))
            del mine, his


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--") and not a.isdigit()]
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 15
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if "--single-load" in sys.argv:
        single_loads(say, rounds)
        return
    keep = []
    # (a)
    my_len, his_len = [12] + [10] * 6, [10] * 7
    maps = outer_maps(my_len, his_len)
    mine, his = filled(int(np.prod(my_len)), "float32"), filled(int(np.prod(his_len)), "float64", seed=11)
    device, _ = multi_call([mine], [his], my_len, his_len, maps, keep)

    def two_step():
        tmp = HipStore(his.size, "float32", 0.0)
        tmp.set_data_f64(his.get_data_f64())
        mine.load(tmp, my_len, his_len, maps)

    m = medians([("device", device), ("host", two_step)], 5, 3)
    say("(a) load float64 -> float32, 10^7 cells: olap_store_load_multi %.1f us, through the host %.1f us (x %.0f)" % (m["device"], m["host"], m["host"] / m["device"]))
    del mine, his
    # (b) and (c)
    say("")
    say("%-34s %3s | %12s %12s %6s | %12s %6s | launches | %14s" % ("(b) same-type load, 10^6 cells (us per call over all measures)", "n", "n x load", "load_multi", "ratio",
                                                                   "n x load'", "A/A", "(c) new tables"))
    my_len, his_len = [12, 100, 1000], [10, 100, 1000]
    for type_name in ("float32", "float64"):
        for n in (1, 4, 8):
            targets = [filled(int(np.prod(my_len)), type_name, seed=20 + i) for i in range(n)]
            sources = [filled(int(np.prod(his_len)), type_name, seed=40 + i) for i in range(n)]
            maps = outer_maps(my_len, his_len)
            singles = [load_call(t, s, my_len, his_len, maps, keep) for t, s in zip(targets, sources)]
            multi, launches = multi_call(targets, sources, my_len, his_len, maps, keep)

            def per():
                for f in singles:
                    f()

            m = medians([("per", per), ("multi", multi), ("again", per)], rounds, 20)
            # (c): every call with a map it has not seen (the two spare items of dimension 0 give few shifts: the
            # innermost map is rotated instead, by another amount each time)
            fresh = []
            for k in range(1, 13):
                mp = [np.arange(10, dtype=np.int32), np.arange(100, dtype=np.int32), np.roll(np.arange(1000, dtype=np.int32), 7 * k + 100 * n + (500 if type_name == "float64" else 0))]
                fresh.append(mp)
            small_targets = [filled(10 ** 6, type_name, seed=60 + i) for i in range(n)]
            first, repeat = [], []
            for mp in fresh:
                f, _ = multi_call(small_targets, sources, his_len, his_len, mp, keep)
                first.append(clock(f, 1))
                repeat.append(clock(f, 1))
            say("%-34s %3d | %9.1f us %9.1f us %6.2f | %9.1f us %6.2f | %d / %d | %6.1f -> %5.1f us" % (
                "    " + type_name, n, m["per"], m["multi"], m["multi"] / m["per"], m["again"], m["again"] / m["per"], n, launches.value,
                statistics.median(first), statistics.median(repeat)))
            del targets, sources, small_targets
    # (d)
    say("")
    say("(d) kernels at 10^8 cells (olap_plan_run, us per run; B/cell = bytes read + written)")
    his_len = [10] * 8
    for form, my_len, maps in [("lanes", [12] + [10] * 7, outer_maps([12] + [10] * 7, his_len)), ("runs", his_len, inner_maps(his_len))]:
        bufs = {t: (filled(10 ** 8, t, seed=5), HipStore(int(np.prod(my_len)), t, 0.0)) for t in ("float32", "float64", "int32")}
        times = {}
        pairs = [("float32", "float32"), ("float64", "float64"), ("float64", "float32"), ("float32", "float64"), ("int32", "float32"), ("float64", "int32")]
        if form == "runs":  # the same-type scatter form that the LDS row form replaced: the like-for-like yardstick of the run form
            pairs += [("float32", "float32", "scatter"), ("float64", "float64", "scatter")]
        for his_t, my_t, *scatter in pairs:
            if scatter:
                os.environ["OLAP_LOAD_NO_PERMUTE"] = "1"
            plan = Plan.load_typed(my_t, his_t, 0.0, 0.0, my_len, his_len, maps)
            os.environ.pop("OLAP_LOAD_NO_PERMUTE", None)
            src, dst = bufs[his_t][0], bufs[my_t][1]
            run = lambda: plan.run(src.values_ptr, None, dst.values_ptr, None)  # noqa: E731
            us = medians([("run", run)], rounds, 10)["run"]
            times[(his_t, my_t) + tuple(scatter)] = us
            bpc = SIZE[his_t] + SIZE[my_t]
            say("    %-6s %-8s -> %-8s %8.1f us  %2d B/cell  %5.2f TB/s  %s" % (form, his_t, my_t, us, bpc, bpc * 1e8 / us / 1e6, plan.kernel_name))
        for his_t, my_t in [("float64", "float32"), ("float32", "float64"), ("int32", "float32"), ("float64", "int32")]:
            wider = "float64" if "float64" in (his_t, my_t) else my_t
            say("    %-6s %s -> %s: x %.2f of the same-type load of %s (the wider type)" % (form, his_t, my_t, times[(his_t, my_t)] / times[(wider, wider)], wider))
            if form == "runs":
                say("    %-6s %s -> %s: x %.2f of the same-type scatter form of %s" % (form, his_t, my_t, times[(his_t, my_t)] / times[(wider, wider, "scatter")], wider))
        del bufs
    if args:
        with open(args[0], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
