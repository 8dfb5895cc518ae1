#!/usr/bin/env python3
"""Developer tool: olap_store_compose_multi through the C ABI next to the three calls it replaces and next to a plain
device-to-device copy, without the Node host around it (tools/compose_bench.js times the whole Cube.compose).

  three Float32 measures of [100, 1000, 100] (10^7 cells) into [150, 1000, 100] (1.5 * 10^7: the first 100 items of
  dimension 0 are his, the other 50 are fill or unset), with and without a fill:
    compose_many (one launch)  |  3 x (create [+ fill] + load)  |  3 x clone of a finished result (hipMemcpy)
  the same with the items of the last dimension permuted (the per-cell form).

Host clock around one pass over the three measures that ends in a device synchronise, results freed inside the clock
(their buffers go back to the pool, as they do for the old path); alternating rounds, medians.
Usage: python tools/compose_pass.py [out.txt] [--rounds N]
"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from conftest import load_package  # noqa: E402

pkg = load_package()
HipStore, Plan, capi = pkg.HipStore, pkg.Plan, pkg.capi
L = capi.lib()
OUT = [a for a in sys.argv[1:] if not a.startswith("--") and not a.isdigit()]
ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 15
lines = []


def say(text):
    print(text)
    lines.append(text)
    if OUT:
        with open(OUT[0], "w") as f:
            f.write("\n".join(lines) + "\n")


def clock(fn):
    capi.check(L.olap_device_synchronize())
    t0 = time.perf_counter()
    fn()
    capi.check(L.olap_device_synchronize())
    return (time.perf_counter() - t0) * 1e6


def source(cells, seed):
    s = HipStore(cells, "float32", 0.0)
    capi.check(L.olap_fill_seeded(s.values_ptr, None, cells, 0, capi.DTYPES["float32"], seed, 0.5, None))
    capi.check(L.olap_canonicalize(s.values_ptr, None, cells, capi.DTYPES["float32"], capi.DEFAULT_ZERO, 0, None))
    return s


my_len, his_len = [150, 1000, 100], [100, 1000, 100]
n_my, n_his = int(np.prod(my_len)), int(np.prod(his_len))
sources = [source(n_his, 11 + i) for i in range(3)]
ident = [np.arange(l, dtype=np.int32) for l in his_len]
permuted = ident[:2] + [np.random.default_rng(3).permutation(100).astype(np.int32)]
say("# olap_store_compose_multi, 3 Float32 measures, %s <- %s; us per pass over the three measures, medians of %d rounds" % (my_len, his_len, ROUNDS))
for name, maps in (("trailing dimensions left alone", ident), ("last dimension permuted", permuted)):
    kernel = Plan.compose("float32", 0.0, my_len, his_len, maps).kernel_name
    for fill in (None, 7.0):
        fills = [fill] * 3

        def one_pass():
            outs, launches = HipStore.compose_many(sources, my_len, his_len, maps, fills)
            assert launches == 1
            del outs

        def three_calls():
            for s in sources:
                t = HipStore(n_my, "float32", 0.0)
                if fill is not None:
                    t.fill(fill)
                t.load(s, my_len, his_len, maps)
                del t

        done, _ = HipStore.compose_many(sources, my_len, his_len, maps, fills)

        def copies():
            for d in done:
                c = d.clone()
                del c

        times = {"pass": [], "calls": [], "copy": []}
        for fn in (one_pass, three_calls, copies):
            fn()
        for r in range(ROUNDS):
            order = [("pass", one_pass), ("calls", three_calls), ("copy", copies)]
            for key, fn in (order if r % 2 else order[::-1]):
                times[key].append(clock(fn))
        p, c, k = (statistics.median(times[x]) for x in ("pass", "calls", "copy"))
        moved = 3 * (n_my + n_his) * 4
        say("%-32s fill %-4s | compose_many %8.1f us (%5.2f TB/s over %d MB) | create%s + load x3 %8.1f us (x %.2f) | clone x3 %8.1f us (pass / copy %.2f) | %s"
            % (name, fill, p, moved / p / 1e6, moved // 1000000, " + fill" if fill is not None else "", c, c / p, k, p / k, kernel))
