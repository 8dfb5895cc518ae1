#!/usr/bin/env python3
"""Developer tool: olap_store_variance_multi (dispersion along a dimension, K16) through the C ABI at 10^8 cells in each of
its forms, Float32 and Float64, against (b) olap_store_drillup_batch with the `average` rule over the same shape and map —
the nearest existing roll-up: the same bytes read and written, one fold instead of two — (c) a device-to-device copy of
the INPUT bytes (olap_store_clone: a new store and one hipMemcpy) and (d) olap_store_quantile_multi (q = 0.5) of the same
shape and map, all timed in the same process in alternating rounds.  Host clock around REPS back-to-back calls that end
in a device synchronise; medians and [min .. max] over the rounds.  The shapes are those of tools/quantile_bench.py plus
one series of 10^6 cells.

A second table looks for the crossover between a lane and a workgroup per output cell: `cells` output cells of groups of
`members`, as [cells, members] (the members contiguous: the row form, beyond a tile the direct form) and as
[1, members, cells] (the members strided: the column form, beyond a tile the direct form), with OLAP_VARIANCE_BLOCK (read
at every call) forcing either side.

Usage: python tools/variance_bench.py [out.txt] [--rounds N]
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
REPS = 10
FORMS = ("column", "row", "direct/lanes", "direct/block")
AVERAGE = capi.METHODS["average"]


def u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32))


def clock(fn, reps=REPS):
    """us per call: `reps` calls back to back, then a device synchronise"""
    L = capi.lib()
    capi.check(L.olap_device_synchronize())
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    capi.check(L.olap_device_synchronize())
    return (time.perf_counter() - t0) / reps * 1e6


def along_call(name, stores, lens, axis, groups, n_groups, *scalars):
    """olap_store_variance_multi (scalars: kind, ddof) or olap_store_quantile_multi (scalars: q)"""
    L = capi.lib()
    n = len(stores)
    hs = (C.c_void_p * n)(*[s._h.value for s in stores])
    outs = (C.c_void_p * n)()
    lv = u32(lens)
    g = None if groups is None else u32(groups)
    launches = C.c_int()

    def call():
        capi.check(getattr(L, name)(n, hs, outs, len(lv), lv.ctypes.data_as(capi._pu32), axis, *scalars, n_groups,
                                    None if g is None else g.ctypes.data_as(capi._pu32), C.byref(launches)))
        for i in range(n):
            L.olap_store_destroy(C.c_void_p(outs[i]))
    return call, (lv, g, hs, outs)


def drillup_call(stores, lens, axis, groups, n_groups):
    """drillUp('average') of the same dimension by the same map, all stores in one batch call"""
    L = capi.lib()
    n = len(stores)
    hs = (C.c_void_p * n)(*[s._h.value for s in stores])
    outs = (C.c_void_p * n)()
    ol = u32(lens)
    nl = ol.copy()
    nl[axis] = n_groups
    maps = [np.arange(l, dtype=np.uint32) for l in lens]
    maps[axis] = np.zeros(lens[axis], dtype=np.uint32) if groups is None else u32(groups)
    arr = (C.POINTER(C.c_uint32) * len(maps))(*[m.ctypes.data_as(capi._pu32) for m in maps])

    def call():
        capi.check(L.olap_store_drillup_batch(n, hs, outs, len(ol), ol.ctypes.data_as(capi._pu32), nl.ctypes.data_as(capi._pu32), arr, AVERAGE))
        for i in range(n):
            L.olap_store_destroy(C.c_void_p(outs[i]))
    return call, (ol, nl, maps, arr, hs, outs)


def clone_call(stores):
    L = capi.lib()
    out = C.c_void_p()

    def call():
        for s in stores:
            capi.check(L.olap_store_clone(s._h, C.byref(out)))
            L.olap_store_destroy(out)
    return call


def form_of(type_name, lens, axis, groups, n_groups):
    outer, K, inner = int(np.prod(lens[:axis], dtype=np.int64)), lens[axis], int(np.prod(lens[axis + 1:], dtype=np.int64))
    longest = K if groups is None else int(np.bincount(groups, minlength=n_groups).max())
    c = (C.c_uint32 * 6)()
    capi.check(capi.lib().olap_diag_variance_choice(np.dtype(type_name).itemsize, 0, outer, K, inner, n_groups, longest, 1, c))
    return FORMS[c[0]]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)
        if args:
            with open(args[0], "w") as f:
                f.write("\n".join(lines) + "\n")

    L = capi.lib()
    capi.check(L.olap_set_device(0))
    n = 10 ** 8
    rng = np.random.default_rng(1)
    cells = rng.integers(-3, 9, size=n).astype(np.float32)  # zeros (unset) among them, mostly duplicates
    stores = {}
    for type_name in ("float32", "float64"):
        big = HipStore(n, type_name, 0.0)
        big.set_data(cells.astype(type_name))
        eight = [HipStore(n // 8, type_name, 0.0) for _ in range(8)]
        for k, s in enumerate(eight):
            s.set_data(cells[k * (n // 8):(k + 1) * (n // 8)].astype(type_name))
        million = HipStore(10 ** 6, type_name, 0.0)
        million.set_data(cells[:10 ** 6].astype(type_name))
        stores[type_name] = (big, eight, million)

    by = lambda K, per: np.arange(K) // per
    say("olap_store_variance_multi (kind 0, ddof 0) against (b) olap_store_drillup_batch('average') of the same shape and map, (c) olap_store_clone of the input")
    say("and (d) olap_store_quantile_multi (q = 0.5) of the same shape and map, 0 default")
    say("us per call, median [min .. max] of %d rounds of %d calls" % (rounds, REPS))
    say()
    for type_name in ("float32", "float64"):
        big, eight, million = stores[type_name]
        cases = [
            ("[100, 100, 10^4] axis 0, one group", [big], [100, 100, 10 ** 4], 0, None, 1),
            ("[100, 100, 10^4] axis 0, groups of 12", [big], [100, 100, 10 ** 4], 0, by(100, 12), 9),
            ("[100, 100, 10^4] axis 1, one group", [big], [100, 100, 10 ** 4], 1, None, 1),
            ("[100, 100, 10^4] axis 1, groups of 12", [big], [100, 100, 10 ** 4], 1, by(100, 12), 9),
            ("[100, 100, 10^4] axis 2, one group", [big], [100, 100, 10 ** 4], 2, None, 1),
            ("[100, 100, 10^4] axis 2, groups of 12", [big], [100, 100, 10 ** 4], 2, by(10 ** 4, 12), 834),
            ("[10^6, 100] axis 1, groups of 31", [big], [10 ** 6, 100], 1, by(100, 31), 4),
            ("[10^6, 100] axis 1, one group", [big], [10 ** 6, 100], 1, None, 1),
            ("[1, 10^6] axis 1, one group (10^6 cells)", [million], [1, 10 ** 6], 1, None, 1),
            ("8 measures [100, 100, 1250] each, axis 1, groups of 12", eight, [100, 100, 1250], 1, by(100, 12), 9),
            ("8 measures [125000, 100] each, axis 1, groups of 31", eight, [125000, 100], 1, by(100, 31), 4),
        ]
        for label, group, lens, axis, groups, ng in cases:
            vc, keep1 = along_call("olap_store_variance_multi", group, lens, axis, groups, ng, 0, 0)
            dc, keep2 = drillup_call(group, lens, axis, groups, ng)
            qc, keep3 = along_call("olap_store_quantile_multi", group, lens, axis, groups, ng, 0.5)
            cc = clone_call(group)
            vc(), dc(), cc(), qc()  # plans, pool and code objects
            tv, td, tc, tq = [], [], [], []
            for r in range(rounds):
                order = ((vc, tv), (dc, td), (cc, tc))
                for fn, into in (order if r % 2 == 0 else order[::-1]):
                    into.append(clock(fn))
                tq.append(clock(qc, 2))  # (tens of milliseconds in places: fewer repetitions)
            mv, md, mc, mq = statistics.median(tv), statistics.median(td), statistics.median(tc), statistics.median(tq)
            say("%-8s %-56s %-12s variance %9.1f [%9.1f .. %9.1f] us | drillUp average %8.1f [%8.1f .. %8.1f] us | copy %8.1f [%8.1f .. %8.1f] us | quantile %9.1f us"
                " | v / drillUp %6.2f | v / copy %6.2f | quantile / v %6.2f"
                % (type_name, label, form_of(type_name, lens, axis, groups, ng), mv, min(tv), max(tv), md, min(td), max(td), mc, min(tc), max(tc), mq, mv / md,
                   mv / mc, mq / mv))
        say()

    say("a lane against a workgroup per output cell (OLAP_VARIANCE_BLOCK = 4294967295 against 1,4294967295), Float64 and Float32, one group: us per call, median of %d rounds of %d calls"
        % (rounds, REPS))
    for type_name in ("float64", "float32"):
        big = stores[type_name][0]
        for layout in ("[cells, members]", "[1, members, cells]"):
            for members in (256, 1024, 4096, 16384, 65536):
                row = "%-8s %-20s members %6d" % (type_name, layout, members)
                for out_cells in (16, 256, 1024, 4096, 16384, 65536):
                    if members * out_cells > 2 ** 26:
                        continue
                    lens = [out_cells, members] if layout.startswith("[cells") else [1, members, out_cells]
                    size = members * out_cells
                    key = (type_name, size)
                    if key not in stores:
                        stores[key] = HipStore(size, type_name, 0.0)
                        stores[key].set_data(cells[:size].astype(type_name))
                    call, keep = along_call("olap_store_variance_multi", [stores[key]], lens, 1, None, 1, 0, 0)
                    t = {"4294967295": [], "1,4294967295": []}
                    form = {}
                    for knob in t:
                        os.environ["OLAP_VARIANCE_BLOCK"] = knob
                        form[knob] = form_of(type_name, lens, 1, None, 1)
                        call()
                    for r in range(rounds):
                        for knob in (("4294967295", "1,4294967295") if r % 2 == 0 else ("1,4294967295", "4294967295")):
                            os.environ["OLAP_VARIANCE_BLOCK"] = knob
                            t[knob].append(clock(call))
                    del os.environ["OLAP_VARIANCE_BLOCK"]
                    lane, block = statistics.median(t["4294967295"]), statistics.median(t["1,4294967295"])
                    row += " | cells %5d: %-12s %8.1f  block %8.1f  lane / block %6.2f" % (out_cells, form["4294967295"], lane, block, lane / block)
                say(row)
        say()


if __name__ == "__main__":
    main()
