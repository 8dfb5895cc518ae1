"""Independent NumPy / Python restatement of Cube.cumulate on typed cells (include/olap_hip.h, olap_store_cumulate_multi).

The cell at item k of the cumulated dimension holds what  dice(items of k's group at positions <= k) -> drillUp(rule)
leaves in its single item: per series and group a sequential float64 state machine over the SET cells in ascending item
order — the first contribution stores, later ones store rule(current, value), a running value equal to the default
drops the key (the next contribution starts over), contributions are counted modulo 65 536 for `average` — converted to
the cell type once per output cell.  tests/test_cumulate_reference.py pins it to the oracle."""
import math

import numpy as np

from golden_util import is_default_typed
from oracle.oracle import to_typed

NP = {"int32": np.int32, "uint32": np.uint32, "float32": np.float32, "float64": np.float64}
METHODS = ("sum", "average", "highest", "lowest", "first", "last", "product")


def js_max(a, b):
    if a != a or b != b:
        return math.nan
    if a == 0.0 and b == 0.0:
        return b if math.copysign(1.0, a) < 0 else a
    return a if a > b else b


def js_min(a, b):
    if a != a or b != b:
        return math.nan
    if a == 0.0 and b == 0.0:
        return a if math.copysign(1.0, a) < 0 else b
    return a if a < b else b


def _mul(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) * np.float64(b))  # (IEEE: inf and NaN instead of Python's OverflowError)


_RULE = {
    "sum": lambda a, b: a + b,
    "average": lambda a, b: a + b,
    "highest": js_max,
    "lowest": js_min,
    "first": lambda a, b: a,
    "last": lambda a, b: b,
    "product": _mul,
}


def input_set(values, status, type_name, default_is_nan):
    """which cells of a typed store are set: the mask bit (where there is a mask) and a value that is not the default"""
    values = np.asarray(values, dtype=NP[type_name]).ravel()
    present = ~is_default_typed(values, type_name, default_is_nan)
    if status is not None:
        present &= (np.asarray(status).ravel() & 2) != 0
    return present


def running_series(values, present, method, default_is_nan):
    """One series of one group, members in ascending order: float64 `values`, bool `present` ->
    (float64 running values, bool has) after each position."""
    rule = _RULE[method]
    default = math.nan if default_is_nan else 0.0

    def is_default(r):
        return r != r if default_is_nan else r == 0.0

    acc, has, count = 0.0, False, 0
    out_v, out_h = np.zeros(len(values)), np.zeros(len(values), dtype=bool)
    for k in range(len(values)):
        if present[k]:
            v = float(values[k])
            if not has:
                acc, has = v, True
            else:
                r = rule(acc, v)
                if is_default(r):
                    has = False
                else:
                    acc = r
            count += 1
        cur, cur_has = acc, has
        if method == "average":
            c16 = count & 0xFFFF
            if c16:
                cur = (acc if has else default) / c16
                cur_has = not is_default(cur)
        out_v[k], out_h[k] = (cur if cur_has else 0.0), cur_has
    return out_v, out_h


def cumulate_reference(values, status, lens, axis, method, type_name, default_is_nan, groups=None):
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
    members = [np.nonzero(g == gid)[0] for gid in np.unique(g)]
    out_v, out_h = np.zeros((outer, K, inner)), np.zeros((outer, K, inner), dtype=bool)
    for o in range(outer):
        for i in range(inner):
            for m in members:
                rv, rh = running_series(v64[o, m, i], present[o, m, i], method, default_is_nan)
                out_v[o, m, i], out_h[o, m, i] = rv, rh
    t = to_typed(out_v.ravel(), type_name)
    has = out_h.ravel() & ~is_default_typed(t, type_name, default_is_nan)
    if type_name in ("float32", "float64"):
        dflt = np.nan if default_is_nan else 0.0
    else:
        dflt = 0
    t = np.where(has, t, np.asarray(dflt, dtype=t.dtype)).astype(NP[type_name])
    return t, np.where(has, 2, 0).astype(np.int32)
