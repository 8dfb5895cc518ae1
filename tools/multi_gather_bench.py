#!/usr/bin/env python3
"""Developer tool: dice, the fused dice -> drillUp and drillDown of 2, 4 and 8 Float32 measures as ONE multi call
(olap_store_dice_multi / _dice_drillup_multi / _drilldown_multi: one launch for the measures) against the per-measure
calls of the same build (olap_store_dice / _dice_drillup / _drilldown, one launch each), in the same process, in
alternating rounds (the two paths also take turns at going first); medians of the time per operation over all measures,
host clock around REPS back-to-back operations that end in a device synchronise.

A third column runs the per-measure path against itself: the spread of the run, below which a ratio says nothing.
Usage: python tools/multi_gather_bench.py [out.txt] [--rounds N]
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
HipStore, capi = pkg.HipStore, pkg.capi
_tables = pkg.hipstore._tables
REPS = 20


def ident(n):
    return np.arange(n)


def u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32))


def pu(a):
    return a.ctypes.data_as(capi._pu32)


def shapes():
    """(label, source shape, single(handle, out), multi(n, handles, outs, launches)): the C ABI calls with every argument
    marshalled once, so that the clock sees the library and the device, not the Python wrappers"""
    L = capi.lib()
    keep = []  # the arrays the pointer tables point into
    out = []

    def tables(rows, np_dtype, c_type):
        k, arr = _tables(rows, np_dtype, c_type)
        keep.append(k)
        return arr

    # config 3 of bench.py as the Node host issues it: slice(dimension1, item3) -> dice(dimension4, [1,4,7]) -> drillUp(dimension0, all)
    # composed into one selection over the [10]^8 cube
    shape = [10] * 8
    mid = [10, 1, 10, 10, 3, 10, 10, 10]
    sel = [ident(l) for l in shape]
    sel[1], sel[4] = [3], [1, 4, 7]
    ol, ml, nl = u32(shape), u32(mid), u32([1] + mid[1:])
    a_sel = tables(sel, np.int32, C.c_int32)
    a_map = tables([np.zeros(l, int) if d == 0 else ident(l) for d, l in enumerate(mid)], np.uint32, C.c_uint32)
    sums = (C.c_int * 8)()
    out.append(("config 3: slice -> dice -> drillUp of [10]^8", shape,
                lambda h, o: L.olap_store_dice_drillup(h, o, 8, pu(ol), pu(ml), pu(nl), a_sel, a_map, 0),
                lambda n, hs, outs, la: L.olap_store_dice_drillup_multi(n, hs, sums, outs, 8, pu(ol), pu(ml), pu(nl), a_sel, a_map, la)))

    def dice(label, old, new, sel):
        o, n_, arr = u32(old), u32(new), tables(sel, np.int32, C.c_int32)
        out.append((label, old, lambda h, res: L.olap_store_dice(h, res, len(old), pu(o), pu(n_), arr),
                    lambda n, hs, outs, la: L.olap_store_dice_multi(n, hs, outs, len(old), pu(o), pu(n_), arr, la)))

    some = np.arange(99, 19, -2)  # 40 of 100 items, in reversed order
    dice("dice of the middle dimension, 10^6 cells", [100, 100, 100], [100, 40, 100], [ident(100), some, ident(100)])
    dice("dice of the middle dimension, rows of 99 (dice_direct)", [100, 100, 99], [100, 40, 99], [ident(100), some, ident(99)])
    dice("dice of the innermost dimension, 10^6 cells", [100, 100, 100], [100, 100, 40], [ident(100), ident(100), some])

    def drilldown(label, old, new):
        o, n_, arr = u32(old), u32(new), tables([ident(old[0]), np.arange(100) // 2, ident(old[2])], np.uint32, C.c_uint32)
        out.append((label, old, lambda h, res: L.olap_store_drilldown(h, res, 3, pu(o), pu(n_), arr, 0, None, 0),
                    lambda n, hs, outs, la: L.olap_store_drilldown_multi(n, hs, sums, outs, 3, pu(o), pu(n_), arr, la)))

    # 50 parents to 100 children: over rows of 1000 cells (the row form) and of 20 cells (the two-pass form, pair by pair behind the call)
    drilldown("drillDown to 10^6 cells, row form", [10, 50, 1000], [10, 100, 1000])
    drilldown("drillDown to 10^6 cells, two-pass form", [500, 50, 20], [500, 100, 20])
    return out, keep


def clock(fn, n):
    """us per operation: REPS operations of n results each, back to back, then a device synchronise"""
    L = capi.lib()
    capi.check(L.olap_device_synchronize())
    outs = [(C.c_void_p * n)() for _ in range(REPS)]
    slots = [[C.cast(C.byref(o, i * C.sizeof(C.c_void_p)), capi._pvp) for i in range(n)] for o in outs]  # &o[i]
    t0 = time.perf_counter()
    for o, slot in zip(outs, slots):
        fn(o, slot)
    capi.check(L.olap_device_synchronize())
    us = (time.perf_counter() - t0) * 1e6 / REPS
    for o in outs:  # (results go back to the pool outside the clock)
        for h in o:
            L.olap_store_destroy(h)
    return us


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 30
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("%-54s %3s | %12s %12s %6s | %12s %6s | launches" % ("operation (us per operation over all measures)", "n", "per measure", "multi", "ratio", "per measure'", "A/A"))
    rng = np.random.default_rng(7)
    cases, keep = shapes()
    for label, shape, single, many in cases:
        cells = int(np.prod(shape))
        values = rng.integers(1, 9, size=cells).astype(np.float32)
        for n in (2, 4, 8):
            stores = []
            for _ in range(n):
                s = HipStore(cells, "float32", 0.0)
                s.set_data(values)
                stores.append(s)
            hs = (C.c_void_p * n)(*[s._h for s in stores])
            launches = C.c_int(0)

            def per(outs, slot):
                for i in range(n):
                    capi.check(single(hs[i], slot[i]))

            def multi(outs, slot):
                capi.check(many(n, hs, outs, C.byref(launches)))

            t = {"per": [], "multi": [], "again": []}
            for r in range(-2, rounds):  # (two rounds warm every path up)
                order = [("per", per), ("multi", multi), ("again", per)]
                for name, fn in (order if r % 2 == 0 else order[::-1]):
                    us = clock(fn, n)
                    if r >= 0:
                        t[name].append(us)
            m = {k: statistics.median(v) for k, v in t.items()}
            say("%-54s %3d | %9.1f us %9.1f us %6.2f | %9.1f us %6.2f | %d / %d" % (label, n, m["per"], m["multi"], m["multi"] / m["per"], m["again"],
                                                                                     m["again"] / m["per"], n * (2 if "two-pass" in label else 1), launches.value))
            del stores
    # the two forms of the batched gather (OLAP_GATHER_BATCH_FORM: blockIdx.y picks the pair | a lane loops over the pairs), the
    # blocks form also against itself
    say("")
    say("%-54s %3s | %12s %12s %6s | %12s %6s" % ("batched gather: blockIdx.y form against lane-loop form", "n", "blocks", "pairs", "ratio", "blocks'", "A/A"))
    for label, shape, single, many in cases:
        if not label.startswith("dice") or "dice_direct" in label:
            continue
        cells = int(np.prod(shape))
        values = rng.integers(1, 9, size=cells).astype(np.float32)
        for n in (2, 4, 8):
            stores = []
            for _ in range(n):
                s = HipStore(cells, "float32", 0.0)
                s.set_data(values)
                stores.append(s)
            hs = (C.c_void_p * n)(*[s._h for s in stores])
            launches = C.c_int(0)

            def form(which):
                def run(outs, slot):
                    capi.check(many(n, hs, outs, C.byref(launches)))

                def timed():
                    os.environ["OLAP_GATHER_BATCH_FORM"] = which
                    try:
                        return clock(run, n)
                    finally:
                        del os.environ["OLAP_GATHER_BATCH_FORM"]
                return timed

            t = {"blocks": [], "pairs": [], "again": []}
            for r in range(-2, rounds):
                order = [("blocks", form("blocks")), ("pairs", form("pairs")), ("again", form("blocks"))]
                for name, fn in (order if r % 2 == 0 else order[::-1]):
                    us = fn()
                    if r >= 0:
                        t[name].append(us)
            m = {k: statistics.median(v) for k, v in t.items()}
            say("%-54s %3d | %9.1f us %9.1f us %6.2f | %9.1f us %6.2f" % (label, n, m["blocks"], m["pairs"], m["pairs"] / m["blocks"], m["again"], m["again"] / m["blocks"]))
            del stores
    if args:
        with open(args[0], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
