"""Independent NumPy / Python restatement of Cube.variance and Cube.stddev on typed cells (include/olap_hip.h,
olap_store_variance_multi; the definition is Cube._varianceHost).

One output cell (o, g, i) of the view [outer, K, inner] under a K -> G map:
  1. the members are the SET cells (o, k, i) with map[k] == g, in ascending item order, as float64 v[0..n)
  2. n - ddof <= 0: the cell is unset
  3. s = v[0]; s += v[k] for k = 1 .. n - 1
  4. mean = s / n
  5. m2 = 0; for each k: d = v[k] - mean; p = d * d; m2 += p
  6. r = m2 / (n - ddof); kind 1 (stddev): r = sqrt(r)
  7. every operation rounded on its own (Python floats do not fuse); a NaN result is the one quiet NaN (np.nan)
  8. converted to the cell type once (TypedArray conversion); a result equal to the default is unset."""
import math

import numpy as np

from golden_util import is_default_typed
from oracle.oracle import to_typed

NP = {"int32": np.int32, "uint32": np.uint32, "float32": np.float32, "float64": np.float64}
COMBOS = ((0, 0), (0, 1), (1, 0), (1, 1))  # (kind, ddof)


def moments_of(members):
    """steps 3 - 5 for the float64 members of one output cell (at least one), in the order given: (n, mean, m2)"""
    v = [float(x) for x in members]
    s = v[0]
    for x in v[1:]:
        s += x
    mean = s / len(v)
    m2 = 0.0
    for x in v:
        d = x - mean
        p = d * d
        m2 += p
    return len(v), mean, m2


def finish(n, m2, kind, ddof):
    """steps 2, 6 and 7: the float64 result, or None for an unset cell"""
    if n - ddof <= 0:
        return None
    r = m2 / (n - ddof)
    if kind:
        r = math.nan if r != r else math.sqrt(r)
    return math.nan if r != r else r


def variance_of(members, kind=0, ddof=0):
    """steps 2 - 7 for the float64 members of one output cell"""
    if not len(members):
        return None
    n, _, m2 = moments_of(members)
    return finish(n, m2, kind, ddof)


def input_set(values, status, type_name, default_is_nan):
    values = np.asarray(values, dtype=NP[type_name]).ravel()
    present = ~is_default_typed(values, type_name, default_is_nan)
    if status is not None:
        present &= (np.asarray(status).ravel() & 2) != 0
    return present


def variance_reference(values, status, lens, axis, kind, ddof, type_name, default_is_nan, groups=None, n_groups=None):
    """values: the typed cells (flat, row-major over lens); status: Int32 mask or None.  groups: item -> group of
    dimension `axis` (None: one group).  Returns (typed values [outer * G * inner] with the default in unset cells,
    Int32 mask)."""
    return variance_reference_all(values, status, lens, axis, type_name, default_is_nan, groups, n_groups, ((kind, ddof),))[(kind, ddof)]


def variance_reference_all(values, status, lens, axis, type_name, default_is_nan, groups=None, n_groups=None, combos=COMBOS):
    """{(kind, ddof): (typed values, mask)} for the combinations asked for; the members are folded once"""
    lens = [int(l) for l in lens]
    K = lens[axis]
    outer = int(np.prod(lens[:axis], dtype=np.int64)) if axis else 1
    inner = int(np.prod(lens[axis + 1:], dtype=np.int64)) if axis + 1 < len(lens) else 1
    typed = np.asarray(values, dtype=NP[type_name]).ravel()
    present = input_set(typed, status, type_name, default_is_nan).reshape(outer, K, inner)
    v64 = typed.astype(np.float64).reshape(outer, K, inner)
    g = np.zeros(K, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    G = 1 if groups is None else (int(n_groups) if n_groups is not None else int(g.max()) + 1)
    members = [np.nonzero(g == gid)[0] for gid in range(G)]  # ascending item order
    out_v = {c: np.zeros((outer, G, inner)) for c in combos}
    out_h = {c: np.zeros((outer, G, inner), dtype=bool) for c in combos}
    for o in range(outer):
        for gid, m in enumerate(members):
            if not len(m):
                continue
            vals, pres = v64[o, m, :], present[o, m, :]
            for i in range(inner):
                mine = vals[pres[:, i], i].tolist()
                if not mine:
                    continue
                n, _, m2 = moments_of(mine)
                for c in combos:
                    r = finish(n, m2, c[0], c[1])
                    if r is not None:
                        out_h[c][o, gid, i] = True
                        out_v[c][o, gid, i] = r
    results = {}
    dflt = (np.nan if default_is_nan else 0.0) if type_name in ("float32", "float64") else 0
    for c in combos:
        t = to_typed(out_v[c].ravel(), type_name)
        has = out_h[c].ravel() & ~is_default_typed(t, type_name, default_is_nan)
        t = np.where(has, t, np.asarray(dflt, dtype=t.dtype)).astype(NP[type_name])
        results[c] = (t, np.where(has, 2, 0).astype(np.int32))
    return results
