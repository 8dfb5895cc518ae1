#!/usr/bin/env python3
"""Developer tool: olap_store_cumulate_multi (running aggregates along a dimension, K13) through the C ABI at 10^8
Float32 cells in each of its forms, against a device-to-device copy of the same bytes (olap_store_clone: a new store and
one hipMemcpy) timed in the same process, in alternating rounds.  Both read every cell once and write every cell once,
so the copy is the yardstick.  Host clock around REPS back-to-back calls that end in a device synchronise; medians and
[min .. max] over the rounds; GB/s counts the bytes read plus the bytes written.

Usage: python tools/cumulate_bench.py [out.txt] [--rounds N]
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


def cumulate_call(stores, lens, axis, groups, n_groups, rule=0):
    L = capi.lib()
    n = len(stores)
    hs = (C.c_void_p * n)(*[s._h.value for s in stores])
    outs = (C.c_void_p * n)()
    codes = (C.c_int * n)(*([rule] * n))
    lv = u32(lens)
    g = None if groups is None else u32(groups)
    launches = C.c_int()

    def call():
        capi.check(L.olap_store_cumulate_multi(n, hs, codes, outs, len(lv), lv.ctypes.data_as(capi._pu32), axis, n_groups,
                                               None if g is None else g.ctypes.data_as(capi._pu32), C.byref(launches)))
        for i in range(n):
            L.olap_store_destroy(C.c_void_p(outs[i]))
    return call, (lv, g, hs, outs, codes)


def clone_call(stores):
    L = capi.lib()
    out = C.c_void_p()

    def call():
        for s in stores:
            capi.check(L.olap_store_clone(s._h, C.byref(out)))
            L.olap_store_destroy(out)
    return call


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 7
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    L = capi.lib()
    capi.check(L.olap_set_device(0))
    n = 10 ** 8
    rng = np.random.default_rng(1)
    cells = rng.integers(-3, 9, size=n).astype(np.float32)  # zeros (unset) among them
    big = HipStore(n, "float32", 0.0)
    big.set_data(cells)
    eight = [HipStore(10 ** 7, "float32", 0.0) for _ in range(8)]
    for k, s in enumerate(eight):
        s.set_data(cells[k * 10 ** 7:(k + 1) * 10 ** 7])
    del cells

    year = lambda K, per: np.arange(K) // per
    cases = [
        ("column form      [100, 100, 10^4] axis 1, one group", [big], [100, 100, 10 ** 4], 1, None, 1, 0),
        ("column form      [100, 100, 10^4] axis 1, groups of 12 (average)", [big], [100, 100, 10 ** 4], 1, year(100, 12), 9, 1),
        ("column form      [100, 100, 10^4] axis 1, interleaved k % 3", [big], [100, 100, 10 ** 4], 1, np.arange(100) % 3, 3, 0),
        ("row form         [250000, 100, 4] axis 1, one group (one slot)", [big], [250000, 100, 4], 1, None, 1, 0),
        ("row form         [125000, 100, 8] axis 1, one group (two slots)", [big], [125000, 100, 8], 1, None, 1, 0),
        ("row form         [83333, 100, 12] of 99 999 600 cells (three slots)", None, [83333, 100, 12], 1, None, 1, 0),
        ("column, 4 slots  [62500, 100, 16] axis 1, one group", [big], [62500, 100, 16], 1, None, 1, 0),
        ("column, ragged   [100, 100, 9999] of 99 990 000 cells", None, [100, 100, 9999], 1, None, 1, 0),
        ("row form         [10^6, 100] axis 1, one group", [big], [10 ** 6, 100], 1, None, 1, 0),
        ("row form         [10^6, 100] axis 1, groups of 12", [big], [10 ** 6, 100], 1, year(100, 12), 9, 0),
        ("row form         [10^6, 100] axis 1, interleaved k % 3", [big], [10 ** 6, 100], 1, np.arange(100) % 3, 3, 0),
        ("row form         [10^6 / 3 * 3, 100, 3] inner 3", None, [333333, 100, 3], 1, None, 1, 0),
        ("row, chunked     [10^4, 10^4] axis 1, one group", [big], [10 ** 4, 10 ** 4], 1, None, 1, 0),
        ("row, chunked     [10^4, 10^4] axis 1, groups of 365", [big], [10 ** 4, 10 ** 4], 1, year(10 ** 4, 365), 28, 0),
        ("one-cell column  [10^4, 10^4] axis 1, interleaved k % 3 (uncoalesced)", [big], [10 ** 4, 10 ** 4], 1, np.arange(10 ** 4) % 3, 3, 0),
        ("latency-bound    [1, 10^6]: one series, one lane of the row form (10^6 cells)", None, [1, 10 ** 6], 1, None, 1, 0),
        ("latency-bound    [10^5, 4] axis 0: one lane of the column form (4 x 10^5 cells)", None, [10 ** 5, 4], 0, None, 1, 0),
        ("8 measures       [10^5, 100] each, one launch (8 x 10^7 cells)", eight, [10 ** 5, 100], 1, None, 1, 0),
        ("8 measures       [100, 100, 1000] each, one launch (8 x 10^7 cells)", eight, [100, 100, 1000], 1, None, 1, 0),
    ]
    say("olap_store_cumulate_multi against olap_store_clone (device-to-device copy of the same bytes), Float32, 0 default")
    say("us per call, median [min .. max] of %d rounds of %d calls; GB/s = (bytes read + bytes written) / median" % (rounds, REPS))
    say()
    odd = {}
    for label, stores, lens, axis, groups, ng, rule in cases:
        if stores is None:  # a size of its own
            size = int(np.prod(lens))
            if size not in odd:
                odd[size] = HipStore(size, "float32", 0.0)
                odd[size].set_data(rng.integers(-3, 9, size=size).astype(np.float32))
            stores = [odd[size]]
        total = sum(s.size for s in stores)
        cum, keep = cumulate_call(stores, lens, axis, groups, ng, rule)
        cop = clone_call(stores)
        cum(), cop()  # plan, pool and code objects
        tc, tk = [], []
        for r in range(rounds):
            for which in ((0, 1) if r % 2 == 0 else (1, 0)):
                (tc if which == 0 else tk).append(clock(cum if which == 0 else cop))
        mc, mk = statistics.median(tc), statistics.median(tk)
        gbs = lambda us: total * 8 / us / 1e3
        say("%-78s cumulate %9.1f [%9.1f .. %9.1f] us %7.0f GB/s | copy %8.1f [%8.1f .. %8.1f] us %7.0f GB/s | cumulate / copy %.2f"
            % (label, mc, min(tc), max(tc), gbs(mc), mk, min(tk), max(tk), gbs(mk), mc / mk))
    if args:
        with open(args[0], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
