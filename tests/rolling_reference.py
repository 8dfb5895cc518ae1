"""Independent NumPy / Python restatement of Cube.rolling on typed cells (include/olap_hip.h, olap_store_rolling_multi).

The cell at item k of the rolled dimension holds what  dice(items j of k's group with k - before <= j <= k + after)
-> drillUp(rule)  leaves in its single item: the last position of the drillUp loop's state machine
(cumulate_reference.running_series: set members in ascending order, restart at the default, `average` divided once by
the count modulo 65 536) over the window's members, converted to the cell type once.  A window without members is
unset.  tests/test_rolling_reference.py pins it to the oracle."""
import numpy as np

from cumulate_reference import NP, input_set, running_series
from golden_util import is_default_typed
from oracle.oracle import to_typed


def window_members(k, K, before, after, g):
    lo, hi = max(k - before, 0), min(k + after, K - 1)
    return [j for j in range(lo, hi + 1) if g[j] == g[k]]


def rolling_reference(values, status, lens, axis, method, type_name, default_is_nan, before, after=0, groups=None):
    """values: the typed cells (flat, row-major over lens); status: Int32 mask or None.  groups: item -> group of
    dimension `axis` (None: one group).  Returns (typed values with the default in unset cells, Int32 mask)."""
    lens = [int(l) for l in lens]
    K = lens[axis]
    outer = int(np.prod(lens[:axis], dtype=np.int64)) if axis else 1
    inner = int(np.prod(lens[axis + 1:], dtype=np.int64)) if axis + 1 < len(lens) else 1
    typed = np.asarray(values, dtype=NP[type_name]).ravel()
    present = input_set(typed, status, type_name, default_is_nan).reshape(outer, K, inner)
    v64 = typed.astype(np.float64).reshape(outer, K, inner)
    g = np.zeros(K, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    out_v, out_h = np.zeros((outer, K, inner)), np.zeros((outer, K, inner), dtype=bool)
    for k in range(K):
        m = window_members(k, K, before, after, g)
        if not m:
            continue
        for o in range(outer):
            for i in range(inner):
                rv, rh = running_series(v64[o, m, i], present[o, m, i], method, default_is_nan)
                out_v[o, k, i], out_h[o, k, i] = rv[-1], rh[-1]
    t = to_typed(out_v.ravel(), type_name)
    has = out_h.ravel() & ~is_default_typed(t, type_name, default_is_nan)
    dflt = (np.nan if default_is_nan else 0.0) if type_name in ("float32", "float64") else 0
    t = np.where(has, t, np.asarray(dflt, dtype=t.dtype)).astype(NP[type_name])
    return t, np.where(has, 2, 0).astype(np.int32)
