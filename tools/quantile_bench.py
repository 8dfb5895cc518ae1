#!/usr/bin/env python3
"""Developer tool: olap_store_quantile_multi (order statistics along a dimension, K15) through the C ABI at 10^8 cells in
each of its forms (small integers with zeros among them, and values whose keys differ in every bit), against (b) olap_store_drillup with the `highest` rule over the same shape and map — the nearest
existing roll-up: the same bytes read and written — and (c) a device-to-device copy of the INPUT bytes (olap_store_clone:
a new store and one hipMemcpy), all timed in the same process in alternating rounds.  Host clock around REPS
back-to-back calls that end in a device synchronise; medians and [min .. max] over the rounds.  A second table times
rank counting against bisection on the key's bits (OLAP_QUANTILE_RANK, read at every launch) over group sizes.

Usage: python tools/quantile_bench.py [out.txt] [--rounds N]
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


def quantile_call(stores, lens, axis, groups, n_groups, q=0.5):
    L = capi.lib()
    n = len(stores)
    hs = (C.c_void_p * n)(*[s._h.value for s in stores])
    outs = (C.c_void_p * n)()
    lv = u32(lens)
    g = None if groups is None else u32(groups)
    launches = C.c_int()

    def call():
        capi.check(L.olap_store_quantile_multi(n, hs, outs, len(lv), lv.ctypes.data_as(capi._pu32), axis, q, n_groups,
                                               None if g is None else g.ctypes.data_as(capi._pu32), C.byref(launches)))
        for i in range(n):
            L.olap_store_destroy(C.c_void_p(outs[i]))
    return call, (lv, g, hs, outs)


def drillup_call(stores, lens, axis, groups, n_groups):
    """drillUp('highest') of the same dimension by the same map, all stores in one batch call"""
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
        capi.check(L.olap_store_drillup_batch(n, hs, outs, len(ol), ol.ctypes.data_as(capi._pu32), nl.ctypes.data_as(capi._pu32), arr, 2))
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
    capi.check(capi.lib().olap_diag_quantile_choice(np.dtype(type_name).itemsize, 0, outer, K, inner, n_groups, longest, 1, c))
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
        # values that differ in every bit of the key (the small integers above differ in a handful: the bisection skips the rest)
        noise = HipStore(n, type_name, 0.0)
        noise.set_data(((rng.random(n) - 0.5) * np.exp2(rng.integers(-20, 20, size=n))).astype(type_name))
        stores[type_name] = (big, eight, million, noise)

    by = lambda K, per: np.arange(K) // per
    say("olap_store_quantile_multi (q = 0.5) against (b) olap_store_drillup_batch('highest') of the same shape and map and (c) olap_store_clone of the input, 0 default")
    say("us per call, median [min .. max] of %d rounds of %d calls" % (rounds, REPS))
    say()
    for type_name in ("float32", "float64"):
        big, eight, million, noise = stores[type_name]
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
            ("[100, 100, 10^4] axis 1, one group, every key bit varies", [noise], [100, 100, 10 ** 4], 1, None, 1),
            ("[100, 100, 10^4] axis 1, groups of 31, every key bit varies", [noise], [100, 100, 10 ** 4], 1, by(100, 31), 4),
            ("[10^6, 100] axis 1, groups of 31, every key bit varies", [noise], [10 ** 6, 100], 1, by(100, 31), 4),
            ("8 measures [100, 100, 1250] each, axis 1, groups of 12", eight, [100, 100, 1250], 1, by(100, 12), 9),
            ("8 measures [125000, 100] each, axis 1, groups of 31", eight, [125000, 100], 1, by(100, 31), 4),
        ]
        for label, group, lens, axis, groups, ng in cases:
            qc, keep1 = quantile_call(group, lens, axis, groups, ng)
            dc, keep2 = drillup_call(group, lens, axis, groups, ng)
            cc = clone_call(group)
            qc(), dc(), cc()  # plans, pool and code objects
            slow = clock(qc, 1) > 20000  # a call of tens of milliseconds: fewer repetitions
            reps = 2 if slow else REPS
            tq, td, tc = [], [], []
            for r in range(rounds):
                order = ((qc, tq), (dc, td), (cc, tc))
                for fn, into in (order if r % 2 == 0 else order[::-1]):
                    into.append(clock(fn, reps))
            mq, md, mc = statistics.median(tq), statistics.median(td), statistics.median(tc)
            say("%-8s %-62s %-12s quantile %9.1f [%9.1f .. %9.1f] us | drillUp highest %8.1f [%8.1f .. %8.1f] us | copy %8.1f [%8.1f .. %8.1f] us | q / drillUp %6.2f | q / copy %6.2f"
                % (type_name, label, form_of(type_name, lens, axis, groups, ng), mq, min(tq), max(tq), md, min(td), max(td), mc, min(tc), max(tc), mq / md, mq / mc))
        say()

    say("rank counting against bisection on the key's bits: Float32, 10^8 cells, groups of n members along the middle (column form, [100, K, 10^4]) and the")
    say("last dimension (row form, [10^6, K]); K = the multiple of n nearest 96.  us per call, median of %d rounds of %d calls" % (rounds, REPS))
    big = stores["float32"][0]
    for n_members in (2, 4, 8, 12, 16, 24, 32, 48, 96):
        K = max(96 // n_members, 1) * n_members
        row = "n = %3d (K = %3d)" % (n_members, K)
        for lens in ([10 ** 8 // (K * 10 ** 4), K, 10 ** 4], [10 ** 8 // K, K]):
            size = int(np.prod(lens))
            if size not in stores:
                stores[size] = HipStore(size, "float32", 0.0)
                stores[size].set_data(cells[:size])
            call, keep = quantile_call([stores[size]], lens, 1, by(K, n_members), K // n_members)
            t = {"0": [], "1000000": []}
            for knob in t:
                os.environ["OLAP_QUANTILE_RANK"] = knob
                call()
            for r in range(rounds):
                for knob in (("0", "1000000") if r % 2 == 0 else ("1000000", "0")):
                    os.environ["OLAP_QUANTILE_RANK"] = knob
                    t[knob].append(clock(call))
            del os.environ["OLAP_QUANTILE_RANK"]
            b, k = statistics.median(t["0"]), statistics.median(t["1000000"])
            row += " | %-12s bisect %8.1f us  ranks %8.1f us  ranks / bisect %5.2f" % (form_of("float32", lens, 1, by(K, n_members), K // n_members), b, k, k / b)
        say(row)


if __name__ == "__main__":
    main()
