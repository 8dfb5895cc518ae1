#!/usr/bin/env python3
"""Developer tool: olap_store_rolling_multi (rolling windows along a dimension, K14) through the C ABI at 10^8 Float32
cells, against a device-to-device copy of the same bytes (olap_store_clone: a new store and one hipMemcpy) and against
olap_store_cumulate_multi of the same shape, timed in the same process in rotating rounds.  All three read every cell
once and write every cell once as far as device memory is concerned, so the copy is the yardstick.  Host clock around
REPS back-to-back calls that end in a device synchronise; medians and [min .. max] over the rounds; GB/s counts the
bytes read plus the bytes written.

Usage: python tools/rolling_bench.py [out.txt] [--rounds N]
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
FORMS = ("series", "columns", "direct")


def u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32))


def clock(fn):
    """us per call: REPS calls back to back, then a device synchronise"""
    L = capi.lib()
    capi.check(L.olap_device_synchronize())
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
    capi.check(L.olap_device_synchronize())
    return (time.perf_counter() - t0) / REPS * 1e6


def along_call(store, lens, axis, rule, window=None):
    """olap_store_rolling_multi with `window` = (before, after), olap_store_cumulate_multi without"""
    L = capi.lib()
    hs, outs, codes = (C.c_void_p * 1)(store._h.value), (C.c_void_p * 1)(), (C.c_int * 1)(rule)
    lv = u32(lens)
    launches = C.c_int()

    def call():
        if window is None:
            capi.check(L.olap_store_cumulate_multi(1, hs, codes, outs, len(lv), lv.ctypes.data_as(capi._pu32), axis, 1, None, C.byref(launches)))
        else:
            capi.check(L.olap_store_rolling_multi(1, hs, codes, outs, len(lv), lv.ctypes.data_as(capi._pu32), axis, window[0], window[1], 1, None,
                                                  C.byref(launches)))
        L.olap_store_destroy(C.c_void_p(outs[0]))
    return call, (lv, hs, outs, codes)


def clone_call(store):
    L = capi.lib()
    out = C.c_void_p()

    def call():
        capi.check(L.olap_store_clone(store._h, C.byref(out)))
        L.olap_store_destroy(out)
    return call


def chosen(lens, axis, window):
    c = (C.c_uint32 * 4)()
    outer, K, inner = int(np.prod(lens[:axis], dtype=np.int64)), lens[axis], int(np.prod(lens[axis + 1:], dtype=np.int64))
    capi.check(capi.lib().olap_diag_rolling_choice(4, outer, K, inner, window[0], window[1], 0, c))
    return "%s %u x %u x %u" % (FORMS[c[0]], c[1], c[2], c[3])


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
    rng = np.random.default_rng(1)
    stores = {}

    def store_of(size):
        if size not in stores:
            stores[size] = HipStore(size, "float32", 0.0)
            stores[size].set_data(rng.integers(-3, 9, size=size).astype(np.float32))  # zeros (unset) among them
        return stores[size]

    windows = [("(2, 0)", (2, 0)), ("(11, 0)", (11, 0)), ("(1, 1)", (1, 1)), ("lag 1", (1, -1))]
    cases = [(lens, axis, rule, w) for lens, axis in (([100, 100, 10 ** 4], 1), ([10 ** 6, 100], 1)) for rule in (0, 1) for w in windows]
    cases += [([100, 100, 12], axis, 0, w) for axis in (0, 1, 2) for w in (windows[0], windows[3])]
    say("olap_store_rolling_multi against olap_store_clone (device-to-device copy of the same bytes) and olap_store_cumulate_multi, Float32, 0 default, one group")
    say("us per call, median [min .. max] of %d rounds of %d calls; GB/s = (bytes read + bytes written) / median; tile: form, series x rows x cols" % (rounds, REPS))
    say()
    for lens, axis, rule, (wname, window) in cases:
        s = store_of(int(np.prod(lens)))
        roll, keep_r = along_call(s, lens, axis, rule, window)
        cum, keep_c = along_call(s, lens, axis, rule)
        calls = [roll, clone_call(s), cum]
        for fn in calls:
            fn()  # plan, pool and code objects
        t = [[], [], []]
        for r in range(rounds):
            for which in [(r + i) % 3 for i in range(3)]:
                t[which].append(clock(calls[which]))
        m = [statistics.median(x) for x in t]
        gbs = lambda us: s.size * 8 / us / 1e3
        say("%-18s axis %d %-7s %-8s %-22s rolling %8.1f [%8.1f .. %8.1f] us %6.0f GB/s | copy %7.1f [%7.1f .. %7.1f] us | cumulate %8.1f us | rolling / copy %5.2f | rolling / cumulate %5.2f"
            % (str(lens).replace("1000000", "10^6").replace("10000", "10^4"), axis, ("sum", "average")[rule], wname, chosen(lens, axis, window), m[0], min(t[0]),
               max(t[0]), gbs(m[0]), m[1], min(t[1]), max(t[1]), m[2], m[0] / m[1], m[0] / m[2]))


if __name__ == "__main__":
    main()
