"""Developer tool: the accuracy of the formula interpreter's library opcodes on the device, in units in the last place of the
correctly rounded result (tests/formula_reference.py: mpmath at 400 bits), over the sweeps of tests/formula_cases.py
(4 096 cells per opcode, the arguments at which math libraries go wrong) and over the finite results of the specials grid.
Per opcode: the maximum, the 99.9th percentile and the input of the maximum.  A measurement, not a test: the suite asserts
a relative 1e-12 (tests/test_formula_ops_gpu.py).
Usage: python tools/formula_ulp.py [out.txt]"""
import ctypes as C
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import formula_cases as fc  # noqa: E402
import formula_reference as fr  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
capi, hs = pkg.capi, pkg.hipstore
INPUT = 1
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def device(op, arrays):
    stores = []
    for x in arrays:
        s = pkg.HipStore(x.size, "float64", math.nan)
        s.set_data_f64(x)
        stores.append(s)
    code = [INPUT, 0] + ([op] if len(arrays) == 1 else [])
    for k in range(1, len(arrays)):
        code += [INPUT, k, op]
    prog = hs._formula(code, [], stores)
    out = np.zeros(arrays[0].size, np.float64)
    capi.check(capi.lib().olap_store_eval_formula(*prog[:-1], (C.c_double * 1)(0.0), 0, out.ctypes.data_as(capi._pdbl)))
    return out


def report(name, got, exact, arrays):
    errs = np.array([fr.ulps(g, e) for g, e in zip(got.tolist(), exact)])
    wrong = int(np.isinf(errs).sum())  # another class or sign than the reference: the suite fails on these
    finite = np.where(np.isinf(errs), 0.0, errs)
    i = int(np.argmax(finite))
    at = ", ".join(repr(float(x[i])) for x in arrays)
    say("%-8s %6d %6d %10.3f %10.3f   %s" % (name, errs.size, wrong, finite[i], np.percentile(finite, 99.9), at))
    return finite[i]


say("# device results against the correctly rounded value; ulp = unit in the last place of that value")
say("%-8s %6s %6s %10s %10s   %s" % ("opcode", "cells", "wrong", "max ulp", "p99.9 ulp", "input of the maximum"))
worst = {}
for op in fr.UNARY_OPS + fr.BINARY_OPS:
    arrays = fc.sweep(op)
    worst[fr.NAMES[op]] = report(fr.NAMES[op], device(op, arrays), fc.sweep_exact(op), arrays)
arrays = fc.hypot3()
folded = [fr.hypot_fold(*xs) for xs in zip(*(x.tolist() for x in arrays))]
worst["HYPOT3"] = report("HYPOT3", device(fr.HYPOT, arrays), folded, arrays)
say("# the specials grid (tests/formula_cases.py SPECIALS, every pair for the two-argument opcodes)")
for op in fr.UNARY_OPS + fr.BINARY_OPS:
    arrays = fc.grid() if op in fr.BINARY_OPS else (np.array(fc.SPECIALS),)
    worst[fr.NAMES[op]] = max(worst[fr.NAMES[op]], report(fr.NAMES[op], device(op, arrays), fc.grid_exact(op), arrays))
over = sorted(k for k, v in worst.items() if v > 16)
say("# worse than 16 ulp somewhere: %s" % (", ".join(over) if over else "none"))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
