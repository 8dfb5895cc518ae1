"""Independent NumPy / Python restatement of Cube.quantile on typed cells (include/olap_hip.h, olap_store_quantile_multi;
the definition is Cube._quantileHost).

One output cell (o, g, i) of the view [outer, K, inner] under a K -> G map:
  1. the members are the SET cells (o, k, i) with map[k] == g, as float64; none: the cell is unset
  2. sorted ascending by the IEEE total order on values (-0 before +0), every NaN last whatever its sign — by an
     order-preserving integer key, never by np.sort (whose order of -0 / +0 is unspecified)
  3. h = q * (n - 1) (one float64 multiplication), lo = floor(h), frac = h - lo
  4. frac > 0: v[lo] + frac * (v[lo + 1] - v[lo]), one subtraction, one multiplication, one addition, each rounded on its
     own (Python floats do not fuse); otherwise v[lo].  A NaN result is the one quiet NaN (np.nan)
  5. converted to the cell type once (TypedArray conversion); a result equal to the default is unset."""
import math
import struct

import numpy as np

from golden_util import is_default_typed
from oracle.oracle import to_typed

NP = {"int32": np.int32, "uint32": np.uint32, "float32": np.float32, "float64": np.float64}
TOP = (1 << 64) - 1


def sort_key(x):
    """float64 -> unsigned 64-bit key, ascending in the stated order"""
    if x != x:
        return TOP
    (u,) = struct.unpack("<Q", struct.pack("<d", x))
    return u ^ TOP if u >> 63 else u | (1 << 63)


def quantile_of(members, q, is_sorted=False):
    """steps 2 - 4 for the float64 members of one output cell (at least one)"""
    v = members if is_sorted else sorted((float(x) for x in members), key=sort_key)
    h = q * (len(v) - 1)
    lo = math.floor(h)
    frac = h - lo
    r = v[lo]
    if frac > 0:
        with np.errstate(all="ignore"):
            d = np.float64(v[lo + 1]) - np.float64(r)  # (np.float64: inf - inf is NaN, not an exception)
            m = np.float64(frac) * d
            r = float(np.float64(r) + m)
    return math.nan if r != r else r


def input_set(values, status, type_name, default_is_nan):
    values = np.asarray(values, dtype=NP[type_name]).ravel()
    present = ~is_default_typed(values, type_name, default_is_nan)
    if status is not None:
        present &= (np.asarray(status).ravel() & 2) != 0
    return present


def quantile_reference(values, status, lens, axis, q, type_name, default_is_nan, groups=None, n_groups=None):
    """values: the typed cells (flat, row-major over lens); status: Int32 mask or None.  groups: item -> group of
    dimension `axis` (None: one group).  Returns (typed values [outer * G * inner] with the default in unset cells,
    Int32 mask); for a list of q (the members are sorted once) a list of such pairs."""
    if not np.isscalar(q):
        return _reference(values, status, lens, axis, list(q), type_name, default_is_nan, groups, n_groups)
    return _reference(values, status, lens, axis, [q], type_name, default_is_nan, groups, n_groups)[0]


def _reference(values, status, lens, axis, qs, type_name, default_is_nan, groups, n_groups):
    lens = [int(l) for l in lens]
    K = lens[axis]
    outer = int(np.prod(lens[:axis], dtype=np.int64)) if axis else 1
    inner = int(np.prod(lens[axis + 1:], dtype=np.int64)) if axis + 1 < len(lens) else 1
    typed = np.asarray(values, dtype=NP[type_name]).ravel()
    present = input_set(typed, status, type_name, default_is_nan).reshape(outer, K, inner)
    v64 = typed.astype(np.float64).reshape(outer, K, inner)
    g = np.zeros(K, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    G = 1 if groups is None else (int(n_groups) if n_groups is not None else int(g.max()) + 1)
    members = [np.nonzero(g == gid)[0] for gid in range(G)]
    out_v, out_h = np.zeros((len(qs), outer, G, inner)), np.zeros((outer, G, inner), dtype=bool)
    for o in range(outer):
        for gid, m in enumerate(members):
            if not len(m):
                continue
            vals, pres = v64[o, m, :], present[o, m, :]
            for i in range(inner):
                mine = sorted(vals[pres[:, i], i].tolist(), key=sort_key)
                if mine:
                    out_h[o, gid, i] = True
                    for n, q in enumerate(qs):
                        out_v[n, o, gid, i] = quantile_of(mine, q, True)
    results = []
    dflt = (np.nan if default_is_nan else 0.0) if type_name in ("float32", "float64") else 0
    for n in range(len(qs)):
        t = to_typed(out_v[n].ravel(), type_name)
        has = out_h.ravel() & ~is_default_typed(t, type_name, default_is_nan)
        t = np.where(has, t, np.asarray(dflt, dtype=t.dtype)).astype(NP[type_name])
        results.append((t, np.where(has, 2, 0).astype(np.int32)))
    return results
