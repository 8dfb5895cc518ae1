"""Python mirror of the reference's InMemoryStore (src/store/in-memory.js) over libolapgpu.

`HipStore` wraps a device-resident store handle; `Plan` wraps a reusable launch plan that runs on
raw device pointers (torch tensors' data_ptr(), or a HipStore's buffers).  Used by the parity
tests, bench.py and the sharded multi-GPU host.  Method names follow the reference's store.
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import DTYPES, DTYPE_NAMES, METHODS, OlapError, check

NP_DTYPES = {"int32": np.int32, "uint32": np.uint32, "float32": np.float32, "float64": np.float64}


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32).ravel())


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32).ravel())


def _tables(rows, np_dtype, c_type):
    """list of per-dimension arrays -> (keepalive list, C array of pointers)"""
    keep = [np.ascontiguousarray(np.asarray(r, dtype=np_dtype).ravel()) for r in rows]
    keep = [k if k.size else np.zeros(1, dtype=np_dtype) for k in keep]
    arr = (C.POINTER(c_type) * max(len(keep), 1))()
    for i, k in enumerate(keep):
        arr[i] = k.ctypes.data_as(C.POINTER(c_type))
    return keep, arr


def _levels(lens, levels):
    """(lens, axis array, n_sel array, keepalive, sel pointer table) of a selection given as [(axis, entries), ...]"""
    lv = _u32(lens)
    ax = (C.c_int * max(len(levels), 1))(*[int(a) for a, _ in levels])
    n = _u32([len(e) for _, e in levels])
    keep, arr = _tables([e for _, e in levels], np.int32, C.c_int32)
    return lv, ax, n, keep, arr


def _handles(stores):  # a None entry stays NULL: the C ABI refuses it by its index
    return (C.c_void_p * max(len(stores), 1))(*[s._h.value if s is not None else None for s in stores])


def _new_stores(n):  # (the array a call writes n new handles into, the int it writes its launch count into)
    return (C.c_void_p * max(n, 1))(), C.c_int(-1)


def _formula(code, consts, inputs):
    """(code, n_code, consts, n_consts, n_inputs, input table, keepalive) of a formula over stores"""
    c = np.ascontiguousarray(code, dtype=np.int32).reshape(-1)
    k = np.ascontiguousarray(consts if len(consts) else [0.0], dtype=np.float64).reshape(-1)
    table = _handles(inputs)
    return (c.ctypes.data_as(capi._pi32), len(c), k.ctypes.data_as(capi._pdbl), len(consts), len(inputs), table, (c, k))


def select_total_formula(code, consts, inputs, lens, levels):
    """getTotalForDimensionItems of a computed measure (olap_formula_select_total): the program evaluated over the stores
    `inputs` at every combination of the levels (see HipStore.select_total).  Returns (total, "device" | "sequential")."""
    prog = _formula(code, consts, inputs)
    lv, ax, n, keep, arr = _levels(lens, levels)
    total, path = C.c_double(), C.c_int()
    check(capi.lib().olap_formula_select_total(*prog[:-1], len(lv), lv.ctypes.data_as(capi._pu32), len(levels), ax, n.ctypes.data_as(capi._pu32),
                                                arr, C.byref(total), C.byref(path)))
    return total.value, ("device" if path.value else "sequential")


def formula_totals(code, consts, inputs, lens, methods):
    """getNestedObject(computed measure, withTotals) (olap_formula_totals): the program over the extended cubes of the
    stores `inputs`; `methods[i]` lists input i's rule per dimension.  Returns (float64 values of the extended cube,
    launches, bytes read)."""
    prog = _formula(code, consts, inputs)
    lv = _u32(lens)
    flat = [_method_code(m) for per_input in methods for m in per_input]
    if len(flat) != len(inputs) * len(lv):
        raise ValueError("formula_totals: one rule per input and dimension")
    m = (C.c_int * max(len(flat), 1))(*flat)
    n = int(np.prod([int(l) + 1 for l in lv])) if len(lv) else 1
    vals = np.zeros(n, np.float64)
    launches, nbytes = C.c_int(), C.c_uint64()
    check(capi.lib().olap_formula_totals(*prog[:-1], len(lv), lv.ctypes.data_as(capi._pu32), m, vals.ctypes.data_as(capi._pdbl), C.byref(launches),
                                          C.byref(nbytes)))
    return vals, launches.value, nbytes.value


def totals_report(inputs, lens, methods, outputs):
    """getNestedObjects(ids, withTotals) (olap_totals_report): the extended cubes of several measures in one call.
    `inputs` are the distinct stores, `methods[i]` lists input i's rule per dimension; an entry of `outputs` is either an
    int (the extended cube of that input) or (code, consts, input indices) — a formula whose INPUT operand j reads
    inputs[indices[j]].  Returns (float64 array [len(outputs), extended cells], launches, bytes read)."""
    lv = _u32(lens)
    flat = [_method_code(m) for per_input in methods for m in per_input]
    if len(flat) != len(inputs) * len(lv):
        raise ValueError("totals_report: one rule per input and dimension")
    m = (C.c_int * max(len(flat), 1))(*flat)
    table = _handles(inputs)
    stored, n_code, n_consts, n_in, code, consts, picks = [], [], [], [], [], [], []
    for out in outputs:
        if isinstance(out, (int, np.integer)):
            stored.append(int(out))
            n_code.append(0), n_consts.append(0), n_in.append(0)
            continue
        c, k, idx = out
        stored.append(-1)
        n_code.append(len(c)), n_consts.append(len(k)), n_in.append(len(idx))
        code.extend(int(x) for x in c), consts.extend(float(x) for x in k), picks.extend(int(x) for x in idx)
    ints = lambda a: (C.c_int * max(len(a), 1))(*a)
    code_a = np.ascontiguousarray(code if code else [0], dtype=np.int32)
    consts_a = np.ascontiguousarray(consts if consts else [0.0], dtype=np.float64)
    ext = int(np.prod([int(l) + 1 for l in lv])) if len(lv) else 1
    vals = np.zeros((len(outputs), ext), np.float64)
    launches, nbytes = C.c_int(), C.c_uint64()
    check(capi.lib().olap_totals_report(len(inputs), table, len(lv), lv.ctypes.data_as(capi._pu32), m, len(outputs), ints(stored), ints(n_code),
                                         code_a.ctypes.data_as(capi._pi32), ints(n_consts), consts_a.ctypes.data_as(capi._pdbl), ints(n_in),
                                         ints(picks), vals.ctypes.data_as(capi._pdbl), C.byref(launches), C.byref(nbytes)))
    return vals, launches.value, nbytes.value


def _entries(indexes, values):
    """(n, indexes, values, is_null or None) pointers of a set_values list (each keeps its array alive); None in `values`
    means unset"""
    idx = np.ascontiguousarray(indexes, dtype=np.uint64).reshape(-1)
    vals = list(values) if not isinstance(values, np.ndarray) else values
    if len(vals) != len(idx):
        raise ValueError("set_values: %d indexes, %d values" % (len(idx), len(vals)))
    if isinstance(vals, np.ndarray) and vals.dtype != object:
        v, nulls = np.ascontiguousarray(vals, dtype=np.float64).reshape(-1), None
    else:
        nulls = np.fromiter((x is None for x in vals), dtype=np.uint8, count=len(vals))
        v = np.fromiter((0.0 if x is None else float(x) for x in vals), dtype=np.float64, count=len(vals))
        if not nulls.any():
            nulls = None
    return (len(idx), idx.ctypes.data_as(capi._pu64), v.ctypes.data_as(capi._pdbl),
            nulls.ctypes.data_as(C.POINTER(C.c_uint8)) if nulls is not None else None)


def _default_kind(default):
    if isinstance(default, str):
        return capi.DEFAULT_NAN if default == "NaN" else capi.DEFAULT_ZERO
    if default != default:
        return capi.DEFAULT_NAN
    if default == 0:
        return capi.DEFAULT_ZERO
    raise OlapError(capi.ERR_INVALID_DEFAULT, "Invalid default value, only NaN and 0 are supported")


def _method_code(method):
    if method is None:
        return METHODS["sum"]
    if isinstance(method, int):
        return method
    return check_neg(capi.lib().olap_method_from_name(str(method).encode()))


def check_neg(rc):
    if rc < 0:
        raise OlapError(rc, capi.last_error())
    return rc


class Plan:
    """A reusable launch plan (olap_*_plan); run() takes raw device pointers."""

    def __init__(self, handle, keep=None):
        self._h = handle
        self._keep = keep

    @classmethod
    def drillup(cls, dtype, default, method, old_len, new_len, maps):
        L = capi.lib()
        ol, nl = _u32(old_len), _u32(new_len)
        keep, arr = _tables(maps, np.uint32, C.c_uint32)
        h = C.c_void_p()
        check(L.olap_drillup_plan(C.byref(h), DTYPES[dtype], _default_kind(default), _method_code(method), len(ol),
                                  ol.ctypes.data_as(capi._pu32), nl.ctypes.data_as(capi._pu32), arr))
        return cls(h)

    @classmethod
    def drilldown(cls, dtype, default, method, old_len, new_len, maps, distributions=None):
        L = capi.lib()
        ol, nl = _u32(old_len), _u32(new_len)
        keep, arr = _tables(maps, np.uint32, C.c_uint32)
        h = C.c_void_p()
        if distributions is not None:
            d = np.ascontiguousarray(np.asarray(distributions, dtype=np.float64))
            dp, dn = d.ctypes.data_as(capi._pdbl), d.size
        else:
            dp, dn = None, 0
        try:
            m = _method_code(method)
        except OlapError:
            m = METHODS["first"]  # any method other than 'sum' copies (in-memory.js:421-423)
        check(L.olap_drilldown_plan(C.byref(h), DTYPES[dtype], _default_kind(default), m, len(ol),
                                    ol.ctypes.data_as(capi._pu32), nl.ctypes.data_as(capi._pu32), arr, dp, dn))
        return cls(h)

    @classmethod
    def dice(cls, dtype, default, old_len, new_len, sel):
        L = capi.lib()
        ol, nl = _u32(old_len), _u32(new_len)
        keep, arr = _tables(sel, np.int32, C.c_int32)
        h = C.c_void_p()
        check(L.olap_dice_plan(C.byref(h), DTYPES[dtype], _default_kind(default), len(ol),
                               ol.ctypes.data_as(capi._pu32), nl.ctypes.data_as(capi._pu32), arr))
        return cls(h)

    @classmethod
    def dice_drillup(cls, dtype, default, method, old_len, mid_len, new_len, sel, maps):
        """Fused dice -> drillUp (one rolled-up dimension)."""
        L = capi.lib()
        ol, ml, nl = _u32(old_len), _u32(mid_len), _u32(new_len)
        keep_s, arr_s = _tables(sel, np.int32, C.c_int32)
        keep_m, arr_m = _tables(maps, np.uint32, C.c_uint32)
        h = C.c_void_p()
        check(L.olap_dice_drillup_plan(C.byref(h), DTYPES[dtype], _default_kind(default), _method_code(method), len(ol),
                                       ol.ctypes.data_as(capi._pu32), ml.ctypes.data_as(capi._pu32),
                                       nl.ctypes.data_as(capi._pu32), arr_s, arr_m))
        return cls(h)

    @classmethod
    def reorder(cls, dtype, default, old_len, perm):
        L = capi.lib()
        ol, p = _u32(old_len), _i32(perm)
        h = C.c_void_p()
        check(L.olap_reorder_plan(C.byref(h), DTYPES[dtype], _default_kind(default), len(ol),
                                  ol.ctypes.data_as(capi._pu32), p.ctypes.data_as(capi._pi32)))
        return cls(h)

    @classmethod
    def load(cls, dtype, my_default, his_default, my_len, his_len, his_to_mine):
        L = capi.lib()
        ml, hl = _u32(my_len), _u32(his_len)
        keep, arr = _tables(his_to_mine, np.int32, C.c_int32)
        h = C.c_void_p()
        check(L.olap_load_plan(C.byref(h), DTYPES[dtype], _default_kind(my_default), _default_kind(his_default),
                               len(ml), ml.ctypes.data_as(capi._pu32), hl.ctypes.data_as(capi._pu32), arr))
        return cls(h)

    @classmethod
    def load_typed(cls, my_dtype, his_dtype, my_default, his_default, my_len, his_len, his_to_mine):
        """load between stores whose cell types may differ (olap_load_plan_typed): `in` of run() holds his_dtype cells"""
        L = capi.lib()
        ml, hl = _u32(my_len), _u32(his_len)
        keep, arr = _tables(his_to_mine, np.int32, C.c_int32)
        h = C.c_void_p()
        check(L.olap_load_plan_typed(C.byref(h), DTYPES[my_dtype], DTYPES[his_dtype], _default_kind(my_default), _default_kind(his_default),
                                     len(ml), ml.ctypes.data_as(capi._pu32), hl.ctypes.data_as(capi._pu32), arr))
        return cls(h)

    @classmethod
    def compose(cls, dtype, default, my_len, his_len, his_to_mine):
        """the gather olap_store_compose_multi runs for stores of this cell type and default (olap_compose_plan)"""
        L = capi.lib()
        ml, hl = _u32(my_len), _u32(his_len)
        keep, arr = _tables(his_to_mine, np.int32, C.c_int32)
        h = C.c_void_p()
        check(L.olap_compose_plan(C.byref(h), DTYPES[dtype], _default_kind(default), len(ml), ml.ctypes.data_as(capi._pu32),
                                  hl.ctypes.data_as(capi._pu32), arr))
        return cls(h)

    @property
    def in_cells(self):
        return int(capi.lib().olap_plan_in_cells(self._h))

    @property
    def out_cells(self):
        return int(capi.lib().olap_plan_out_cells(self._h))

    @property
    def kernel_name(self):
        return capi.lib().olap_plan_kernel_name(self._h).decode()

    def describe(self):
        """The scalars the plan decided, one line of key=value pairs (olap_diag_plan_describe)."""
        buf = C.create_string_buffer(512)
        check(capi.lib().olap_diag_plan_describe(self._h, buf, len(buf)))
        return buf.value.decode()

    def run(self, in_values, in_status, out_values, out_status, stream=None):
        """All four are integer device addresses (0/None = absent); stream = hipStream_t address."""
        check(capi.lib().olap_plan_run(self._h, in_values or None, in_status or None, out_values or None,
                                       out_status or None, stream or None))

    def run_batch(self, in_values, in_status, out_values, out_status, stream=None):
        """The same plan over several buffer pairs in one call (one launch where the plan allows it): lists of device
        addresses; in_status / out_status may be None (no masks) or lists with 0 / None entries."""
        n = len(in_values)
        ptrs = lambda xs: None if xs is None else (C.c_void_p * n)(*[x or None for x in xs])
        check(capi.lib().olap_plan_run_batch(self._h, n, ptrs(in_values), ptrs(in_status), ptrs(out_values), ptrs(out_status),
                                             stream or None))

    def run_batch_rules(self, methods, in_values, in_status, out_values, out_status, stream=None):
        """A drillUp plan over several buffer pairs with a rule each (names or codes): one mixed-rule launch where the
        plan allows it (olap_plan_run_batch_rules)."""
        n = len(in_values)
        ptrs = lambda xs: None if xs is None else (C.c_void_p * n)(*[x or None for x in xs])
        codes = (C.c_int * n)(*[m if isinstance(m, int) else _method_code(m) for m in methods])
        check(capi.lib().olap_plan_run_batch_rules(self._h, n, codes, ptrs(in_values), ptrs(in_status), ptrs(out_values), ptrs(out_status),
                                                   stream or None))

    def status(self):
        check(capi.lib().olap_plan_status(self._h))

    def destroy(self):
        if self._h:
            capi.lib().olap_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class HipStore:
    """Device-resident store of one measure: the reference's InMemoryStore on an MI355X."""

    def __init__(self, size, type="float32", default=float("nan"), _handle=None):
        self._lib = capi.lib()
        if _handle is not None:
            self._h = _handle
            return
        kind = _default_kind(default)  # in-memory.js:56-57 is checked before :59-60
        if type not in DTYPES:
            raise OlapError(capi.ERR_INVALID_TYPE, "Invalid type")
        h = C.c_void_p()
        check(self._lib.olap_store_create(C.byref(h), int(size), DTYPES[type], kind))
        self._h = h

    def __del__(self):
        try:
            if self._h:
                self._lib.olap_store_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ---- properties (in-memory.js:8-28)
    @property
    def size(self):
        return int(self._lib.olap_store_size(self._h))

    @property
    def type(self):
        return DTYPE_NAMES[self._lib.olap_store_dtype(self._h)]

    @property
    def default_is_nan(self):
        return self._lib.olap_store_default(self._h) == capi.DEFAULT_NAN

    @property
    def byte_length(self):
        return int(self._lib.olap_store_byte_length(self._h))

    @property
    def values_ptr(self):
        return self._lib.olap_store_values_ptr(self._h)

    @property
    def status_ptr(self):
        return self._lib.olap_store_status_ptr(self._h)

    @property
    def total(self):
        t = C.c_double()
        check(self._lib.olap_store_total(self._h, C.byref(t)))
        return t.value

    def track_order(self, on=True):
        """olap_store_track_order: keep the reference Map's insertion order (first / last, keys(), serialize())."""
        check(self._lib.olap_store_track_order(self._h, 1 if on else 0))
        return self

    @property
    def order_tracked(self):
        return int(self._lib.olap_store_order_tracked(self._h))

    def count_set(self):
        n = C.c_uint64()
        check(self._lib.olap_store_count_set(self._h, C.byref(n)))
        return n.value

    # ---- data in / out
    def set_data(self, values):
        """`data` setter from a typed numpy array of the store's dtype."""
        v = np.ascontiguousarray(np.asarray(values, dtype=NP_DTYPES[self.type]).ravel())
        check(self._lib.olap_store_set_data(self._h, v.ctypes.data_as(C.c_void_p), v.size))

    def set_data_f64(self, values):
        """`data` setter from JS numbers (float64), converted like a TypedArray store."""
        v = np.ascontiguousarray(np.asarray(values, dtype=np.float64).ravel())
        check(self._lib.olap_store_set_data_f64(self._h, v.ctypes.data_as(capi._pdbl), v.size))

    def get_data(self):
        out = np.zeros(max(self.size, 1), dtype=NP_DTYPES[self.type])
        check(self._lib.olap_store_get_data(self._h, out.ctypes.data_as(C.c_void_p)))
        return out[: self.size]

    def get_data_f64(self):
        out = np.zeros(max(self.size, 1), dtype=np.float64)
        check(self._lib.olap_store_get_data_f64(self._h, out.ctypes.data_as(capi._pdbl)))
        return out[: self.size]

    def get_status(self):
        out = np.zeros(max(self.size, 1), dtype=np.int32)
        check(self._lib.olap_store_get_status(self._h, out.ctypes.data_as(capi._pi32)))
        return out[: self.size]

    def keys(self):
        n = C.c_uint64()
        check(self._lib.olap_store_get_keys(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.uint64)
        check(self._lib.olap_store_get_keys(self._h, out.ctypes.data_as(capi._pu64), n.value, C.byref(n)))
        return out[: n.value]

    def to_sparse(self):
        """(indexes uint32[n], values typed[n]) of the set cells, ascending: the reference's serialised form."""
        n = C.c_uint64()
        check(self._lib.olap_store_to_sparse(self._h, None, None, 0, C.byref(n)))
        idx = np.zeros(max(n.value, 1), dtype=np.uint32)
        vals = np.zeros(max(n.value, 1), dtype=NP_DTYPES[self.type])
        check(self._lib.olap_store_to_sparse(self._h, idx.ctypes.data_as(capi._pu32), vals.ctypes.data_as(C.c_void_p),
                                             n.value, C.byref(n)))
        return idx[: n.value], vals[: n.value]

    @classmethod
    def from_sparse(cls, size, type, default, indexes, values):
        L = capi.lib()
        idx = np.ascontiguousarray(np.asarray(indexes, dtype=np.uint32))
        vals = np.ascontiguousarray(np.asarray(values, dtype=NP_DTYPES[type]))
        h = C.c_void_p()
        check(L.olap_store_from_sparse(C.byref(h), int(size), DTYPES[type], _default_kind(default),
                                       idx.ctypes.data_as(capi._pu32), vals.ctypes.data_as(C.c_void_p), idx.size))
        return cls(0, _handle=h)

    def get_value(self, index):
        v, s = C.c_double(), C.c_int()
        check(self._lib.olap_store_get_value(self._h, int(index), C.byref(v), C.byref(s)))
        return v.value, bool(s.value)

    def set_value(self, index, value):
        if value is None:
            check(self._lib.olap_store_set_value(self._h, int(index), 0.0, 1))
        else:
            check(self._lib.olap_store_set_value(self._h, int(index), float(value), 0))

    def set_values(self, indexes, values):
        """olap_store_set_values: set_value(indexes[i], values[i]) for every i, in list order, in one call (None unsets)."""
        check(self._lib.olap_store_set_values(self._h, *_entries(indexes, values)))

    def fill(self, value):
        check(self._lib.olap_store_fill(self._h, float(value)))

    def clone(self):
        h = C.c_void_p()
        check(self._lib.olap_store_clone(self._h, C.byref(h)))
        return HipStore(0, _handle=h)

    def totals(self, lens, methods):
        """olap_store_totals: the extended cube of shape (len + 1) per dimension — every marginal of
        getNestedObject(measure, withTotals) — as (float64 values, Int32 mask, launches, bytes read)."""
        ol = _u32(lens)
        m = (C.c_int * max(len(ol), 1))(*[_method_code(x) for x in methods])
        n = int(np.prod([int(l) + 1 for l in ol])) if len(ol) else 1
        vals, stat = np.zeros(n, np.float64), np.zeros(n, np.int32)
        launches, nbytes = C.c_int(), C.c_uint64()
        check(self._lib.olap_store_totals(self._h, len(ol), ol.ctypes.data_as(capi._pu32), m, vals.ctypes.data_as(capi._pdbl),
                                          stat.ctypes.data_as(capi._pi32), C.byref(launches), C.byref(nbytes)))
        return vals, stat, launches.value, nbytes.value

    # ---- bulk operations (names follow in-memory.js)
    def drill_up(self, old_len, new_len, maps, method="sum"):
        ol, nl = _u32(old_len), _u32(new_len)
        keep, arr = _tables(maps, np.uint32, C.c_uint32)
        h = C.c_void_p()
        check(self._lib.olap_store_drillup(self._h, C.byref(h), len(ol), ol.ctypes.data_as(capi._pu32),
                                           nl.ctypes.data_as(capi._pu32), arr, _method_code(method)))
        return HipStore(0, _handle=h)

    @staticmethod
    def drill_up_batch(stores, old_len, new_len, maps, method="sum"):
        """drillUp of several measures of a cube by the same maps and rule: one launch when they share cell type,
        default and size (olap_store_drillup_batch); returns the new stores in order."""
        ol, nl = _u32(old_len), _u32(new_len)
        keep, arr = _tables(maps, np.uint32, C.c_uint32)
        n = len(stores)
        outs, _ = _new_stores(n)
        check(capi.lib().olap_store_drillup_batch(n, _handles(stores), outs, len(ol), ol.ctypes.data_as(capi._pu32), nl.ctypes.data_as(capi._pu32), arr,
                                                  _method_code(method)))
        return HipStore._multi_result(n, outs)

    @staticmethod
    def drill_up_multi(stores, methods, old_len, new_len, maps):
        """drillUp of the stored measures of a cube, each with its own rule (olap_store_drillup_multi): one mixed-rule
        launch where the roll-up allows it; returns the new stores in order."""
        ol, nl = _u32(old_len), _u32(new_len)
        keep, arr = _tables(maps, np.uint32, C.c_uint32)
        n = len(stores)
        codes = (C.c_int * max(n, 1))(*[_method_code(m) for m in methods])
        outs, _ = _new_stores(n)
        check(capi.lib().olap_store_drillup_multi(n, _handles(stores), codes, outs, len(ol), ol.ctypes.data_as(capi._pu32), nl.ctypes.data_as(capi._pu32), arr))
        return HipStore._multi_result(n, outs)

    def drill_down(self, old_len, new_len, maps, method="sum", distributions=None, integer_measure=False):
        """in-memory.js:336-430.  `integer_measure`: the measure is DECLARED int32 / uint32 but held in float64 cells (what
        the reference's Map does until serialize()): `sum` spreads the integer remainder (:343, :403-417) all the same."""
        ol, nl = _u32(old_len), _u32(new_len)
        keep, arr = _tables(maps, np.uint32, C.c_uint32)
        if distributions is not None:
            d = np.ascontiguousarray(np.asarray(distributions, dtype=np.float64))
            dp, dn = d.ctypes.data_as(capi._pdbl), d.size
        else:
            dp, dn = None, 0
        try:
            m = _method_code(method)
        except OlapError:
            m = METHODS["first"]
        if integer_measure:
            m |= capi.DRILLDOWN_INTEGER_MEASURE
        h = C.c_void_p()
        check(self._lib.olap_store_drilldown(self._h, C.byref(h), len(ol), ol.ctypes.data_as(capi._pu32),
                                             nl.ctypes.data_as(capi._pu32), arr, m, dp, dn))
        return HipStore(0, _handle=h)

    def dice(self, old_len, new_len, sel):
        ol, nl = _u32(old_len), _u32(new_len)
        keep, arr = _tables(sel, np.int32, C.c_int32)
        h = C.c_void_p()
        check(self._lib.olap_store_dice(self._h, C.byref(h), len(ol), ol.ctypes.data_as(capi._pu32),
                                        nl.ctypes.data_as(capi._pu32), arr))
        return HipStore(0, _handle=h)

    def dice_drillup(self, old_len, mid_len, new_len, sel, maps, method="sum"):
        ol, ml, nl = _u32(old_len), _u32(mid_len), _u32(new_len)
        keep_s, arr_s = _tables(sel, np.int32, C.c_int32)
        keep_m, arr_m = _tables(maps, np.uint32, C.c_uint32)
        h = C.c_void_p()
        check(self._lib.olap_store_dice_drillup(self._h, C.byref(h), len(ol), ol.ctypes.data_as(capi._pu32),
                                                ml.ctypes.data_as(capi._pu32), nl.ctypes.data_as(capi._pu32), arr_s, arr_m,
                                                _method_code(method)))
        return HipStore(0, _handle=h)

    # ---- all stored measures of a cube in one call (olap_store_*_multi): (new stores in order, kernel launches made)
    @staticmethod
    def _multi_result(n, outs, launches=None):
        stores = [HipStore(0, _handle=C.c_void_p(outs[i])) for i in range(n)]
        return stores if launches is None else (stores, launches.value)

    @staticmethod
    def dice_multi(stores, old_len, new_len, sel):
        ol, nl = _u32(old_len), _u32(new_len)
        keep, arr = _tables(sel, np.int32, C.c_int32)
        n = len(stores)
        hs, (outs, launches) = _handles(stores), _new_stores(n)
        check(capi.lib().olap_store_dice_multi(n, hs, outs, len(ol), ol.ctypes.data_as(capi._pu32), nl.ctypes.data_as(capi._pu32), arr,
                                               C.byref(launches)))
        return HipStore._multi_result(n, outs, launches)

    @staticmethod
    def dice_drillup_multi(stores, methods, old_len, mid_len, new_len, sel, maps):
        ol, ml, nl = _u32(old_len), _u32(mid_len), _u32(new_len)
        keep_s, arr_s = _tables(sel, np.int32, C.c_int32)
        keep_m, arr_m = _tables(maps, np.uint32, C.c_uint32)
        n = len(stores)
        hs, (outs, launches) = _handles(stores), _new_stores(n)
        codes = (C.c_int * max(n, 1))(*[_method_code(m) for m in methods])
        check(capi.lib().olap_store_dice_drillup_multi(n, hs, codes, outs, len(ol), ol.ctypes.data_as(capi._pu32), ml.ctypes.data_as(capi._pu32),
                                                       nl.ctypes.data_as(capi._pu32), arr_s, arr_m, C.byref(launches)))
        return HipStore._multi_result(n, outs, launches)

    @staticmethod
    def drill_down_multi(stores, methods, old_len, new_len, maps, integer_measures=None):
        """`integer_measures[i]`: as drill_down's integer_measure, for stores[i]"""
        ol, nl = _u32(old_len), _u32(new_len)
        keep, arr = _tables(maps, np.uint32, C.c_uint32)
        n = len(stores)
        hs, (outs, launches) = _handles(stores), _new_stores(n)
        flags = integer_measures or [False] * n
        codes = (C.c_int * max(n, 1))(*[_method_code(m) | (capi.DRILLDOWN_INTEGER_MEASURE if f else 0) for m, f in zip(methods, flags)])
        check(capi.lib().olap_store_drilldown_multi(n, hs, codes, outs, len(ol), ol.ctypes.data_as(capi._pu32), nl.ctypes.data_as(capi._pu32), arr,
                                                    C.byref(launches)))
        return HipStore._multi_result(n, outs, launches)

    def reorder(self, old_len, perm):
        ol, p = _u32(old_len), _i32(perm)
        h = C.c_void_p()
        check(self._lib.olap_store_reorder(self._h, C.byref(h), len(ol), ol.ctypes.data_as(capi._pu32),
                                           p.ctypes.data_as(capi._pi32)))
        return HipStore(0, _handle=h)

    # ---- filtered totals and copies (olap_store_select_total / olap_store_copy_select)
    def select_total(self, lens, levels):
        """getTotalForDimensionItems (src/cube.js:679-707) over a selection given as levels in nesting order:
        [(axis, entries), ...], axis = cube dimension or -1 (a free filter key), entries = item indices (-1 = a cell that
        does not exist).  Returns (total, path): path "device" (the certified order-free reduction) or "sequential"."""
        lv, ax, n, keep, arr = _levels(lens, levels)
        total, path = C.c_double(), C.c_int()
        check(self._lib.olap_store_select_total(self._h, len(lv), lv.ctypes.data_as(capi._pu32), len(levels), ax, n.ctypes.data_as(capi._pu32), arr,
                                                C.byref(total), C.byref(path)))
        return total.value, ("device" if path.value else "sequential")

    def copy_select(self, source, lens, levels):
        """copyMeasureData (src/cube.js:859-888): self.set_value(pos, source.get_value(pos)) over the selection."""
        lv, ax, n, keep, arr = _levels(lens, levels)
        check(self._lib.olap_store_copy_select(self._h, source._h, len(lv), lv.ctypes.data_as(capi._pu32), len(levels), ax,
                                               n.ctypes.data_as(capi._pu32), arr))
        return self

    def copy_select_formula(self, code, consts, inputs, lens, levels):
        """copyMeasureData from a computed measure (olap_store_copy_select_formula): self.set_value(pos, formula(pos))
        over the selection; `code` / `consts` as olap_eval_formula takes them, `inputs` the stores it reads."""
        prog = _formula(code, consts, inputs)
        lv, ax, n, keep, arr = _levels(lens, levels)
        check(self._lib.olap_store_copy_select_formula(self._h, *prog[:-1], len(lv), lv.ctypes.data_as(capi._pu32), len(levels), ax,
                                                       n.ctypes.data_as(capi._pu32), arr))
        return self

    def set_formula(self, code, consts, inputs, scalars=()):
        """olap_store_set_formula: self.set_data_f64(formula over `inputs`) in one launch, without the host.  `code` /
        `consts` as olap_eval_formula takes them, `inputs` the stores INPUT k reads, `scalars` the values SCALAR k reads."""
        prog = _formula(code, consts, inputs)
        sc = np.ascontiguousarray(scalars if len(scalars) else [0.0], dtype=np.float64).reshape(-1)
        check(self._lib.olap_store_set_formula(self._h, *prog[:-1], sc.ctypes.data_as(capi._pdbl), len(scalars)))
        return self

    def load(self, other, my_len, his_len, his_to_mine):
        ml, hl = _u32(my_len), _u32(his_len)
        keep, arr = _tables(his_to_mine, np.int32, C.c_int32)
        check(self._lib.olap_store_load(self._h, other._h, len(ml), ml.ctypes.data_as(capi._pu32),
                                        hl.ctypes.data_as(capi._pu32), arr))

    @staticmethod
    def load_many(targets, sources, my_len, his_len, his_to_mine):
        """targets[i].load(sources[i]) for every pair in one call (olap_store_load_multi); cell types may differ within a
        pair.  Returns the kernel launches made."""
        if len(targets) != len(sources):
            raise ValueError("load_many: %d targets, %d sources" % (len(targets), len(sources)))
        ml, hl = _u32(my_len), _u32(his_len)
        keep, arr = _tables(his_to_mine, np.int32, C.c_int32)
        n = len(targets)
        launches = C.c_int(-1)
        check(capi.lib().olap_store_load_multi(n, _handles(targets), _handles(sources), len(ml), ml.ctypes.data_as(capi._pu32), hl.ctypes.data_as(capi._pu32), arr,
                                               C.byref(launches)))
        return launches.value

    @staticmethod
    def reorder_many(stores, old_len, perm):
        """reorder of several measures of a cube in one call (olap_store_reorder_multi): (new stores in order, kernel
        launches made)"""
        ol, p = _u32(old_len), _i32(perm)
        n = len(stores)
        outs, launches = _new_stores(n)
        check(capi.lib().olap_store_reorder_multi(n, _handles(stores), outs, len(ol), ol.ctypes.data_as(capi._pu32), p.ctypes.data_as(capi._pi32),
                                                  C.byref(launches)))
        return HipStore._multi_result(n, outs, launches)

    @staticmethod
    def compose_many(sources, my_len, his_len, his_to_mine, fills=None):
        """The measures of one cube on the dimensions of a composed one (olap_store_compose_multi): new stores of
        prod(my_len) cells that end as create [+ fill(fills[i]) where fills[i] is not None] + load(sources[i]) leave them,
        in one pass per group of up to 8.  Returns (new stores in order, kernel launches made)."""
        ml, hl = _u32(my_len), _u32(his_len)
        keep, arr = _tables(his_to_mine, np.int32, C.c_int32)
        n = len(sources)
        outs, launches = _new_stores(n)
        values = has = None
        if fills is not None:
            if len(fills) != n:
                raise ValueError("compose_many: %d sources, %d fills" % (n, len(fills)))
            values = (C.c_double * max(n, 1))(*[0.0 if f is None else float(f) for f in fills])
            has = (C.c_uint8 * max(n, 1))(*[0 if f is None else 1 for f in fills])
        check(capi.lib().olap_store_compose_multi(n, _handles(sources), values, has, outs, len(ml), ml.ctypes.data_as(capi._pu32),
                                                  hl.ctypes.data_as(capi._pu32), arr, C.byref(launches)))
        return HipStore._multi_result(n, outs, launches)

    def cumulate(self, lens, axis, method="sum", groups=None, n_groups=None):
        """Running aggregate along dimension `axis` of the cube `lens` (olap_store_cumulate_multi with one store): the cell
        at item k holds dice(items of k's group up to k) -> drillUp(rule).  `groups`: item -> group (None: one group)."""
        return HipStore.cumulate_multi([self], [method], lens, axis, groups, n_groups)[0][0]

    @staticmethod
    def cumulate_multi(stores, methods, lens, axis, groups=None, n_groups=None):
        """Running aggregates of the stored measures of a cube, a rule each, in one call (olap_store_cumulate_multi):
        (new stores in order, kernel launches made).  `n_groups` defaults to max(groups) + 1."""
        lv = _u32(lens)
        n = len(stores)
        hs, (outs, launches) = _handles(stores), _new_stores(n)
        codes = (C.c_int * max(n, 1))(*[_method_code(m) for m in methods])
        g, gp, ng = _groups_arg(groups, n_groups)  # (g: the array behind gp, held until the call is over)
        check(capi.lib().olap_store_cumulate_multi(n, hs, codes, outs, len(lv), lv.ctypes.data_as(capi._pu32), int(axis), ng, gp, C.byref(launches)))
        return HipStore._multi_result(n, outs, launches)

    def rolling(self, lens, axis, method, before, after=0, groups=None, n_groups=None):
        """Rolling-window aggregate along dimension `axis` of the cube `lens` (olap_store_rolling_multi with one store): the
        cell at item k holds dice(items of k's group in [k - before, k + after]) -> drillUp(rule); unset where no item is left."""
        return HipStore.rolling_multi([self], [method], lens, axis, before, after, groups, n_groups)[0][0]

    @staticmethod
    def rolling_multi(stores, methods, lens, axis, before, after=0, groups=None, n_groups=None):
        """Rolling-window aggregates of the stored measures of a cube, a rule each, in one call (olap_store_rolling_multi):
        (new stores in order, kernel launches made).  `n_groups` defaults to max(groups) + 1."""
        lv = _u32(lens)
        n = len(stores)
        hs, (outs, launches) = _handles(stores), _new_stores(n)
        codes = (C.c_int * max(n, 1))(*[_method_code(m) for m in methods])
        g, gp, ng = _groups_arg(groups, n_groups)  # (g: the array behind gp, held until the call is over)
        check(capi.lib().olap_store_rolling_multi(n, hs, codes, outs, len(lv), lv.ctypes.data_as(capi._pu32), int(axis), int(before), int(after), ng, gp,
                                                  C.byref(launches)))
        return HipStore._multi_result(n, outs, launches)

    def quantile(self, lens, axis, q, groups=None, n_groups=None):
        """q-quantile along dimension `axis` of the cube `lens` (olap_store_quantile_multi with one store): a new store of
        outer * G * inner cells whose cell holds the quantile of the set cells of its group.  `groups`: item -> group
        (None: one group)."""
        return HipStore.quantile_multi([self], lens, axis, q, groups, n_groups)[0][0]

    @staticmethod
    def quantile_multi(stores, lens, axis, q, groups=None, n_groups=None):
        """q-quantiles of the stored measures of a cube in one call (olap_store_quantile_multi): (new stores in order,
        kernel launches made).  `n_groups` defaults to max(groups) + 1."""
        lv = _u32(lens)
        n = len(stores)
        hs, (outs, launches) = _handles(stores), _new_stores(n)
        g, gp, ng = _groups_arg(groups, n_groups)  # (g: the array behind gp, held until the call is over)
        check(capi.lib().olap_store_quantile_multi(n, hs, outs, len(lv), lv.ctypes.data_as(capi._pu32), int(axis), float(q), ng, gp, C.byref(launches)))
        return HipStore._multi_result(n, outs, launches)

    def variance(self, lens, axis, kind=0, ddof=0, groups=None, n_groups=None):
        """Variance (kind 0) or standard deviation (kind 1) along dimension `axis` of the cube `lens`
        (olap_store_variance_multi with one store): a new store of outer * G * inner cells whose cell holds the two-pass
        variance of the set cells of its group, divided by n - ddof.  `groups`: item -> group (None: one group)."""
        return HipStore.variance_multi([self], lens, axis, kind, ddof, groups, n_groups)[0][0]

    @staticmethod
    def variance_multi(stores, lens, axis, kind=0, ddof=0, groups=None, n_groups=None):
        """Variances of the stored measures of a cube in one call (olap_store_variance_multi): (new stores in order,
        kernel launches made).  `n_groups` defaults to max(groups) + 1."""
        lv = _u32(lens)
        n = len(stores)
        hs, (outs, launches) = _handles(stores), _new_stores(n)
        g, gp, ng = _groups_arg(groups, n_groups)  # (g: the array behind gp, held until the call is over)
        check(capi.lib().olap_store_variance_multi(n, hs, outs, len(lv), lv.ctypes.data_as(capi._pu32), int(axis), int(kind), int(ddof), ng, gp,
                                                   C.byref(launches)))
        return HipStore._multi_result(n, outs, launches)


def _groups_arg(groups, n_groups):
    """The K -> G map of the calls along a dimension as the C ABI takes it: (the uint32 array, its pointer, the number of
    groups), or (None, None, 1) without groups.  `n_groups` defaults to max(groups) + 1."""
    if groups is None:
        return None, None, 1
    g = np.ascontiguousarray(np.asarray(groups, dtype=np.uint32).ravel())
    return g, g.ctypes.data_as(capi._pu32), int(n_groups) if n_groups is not None else (int(g.max()) + 1 if g.size else 0)


def blocks_report(stores, lens, scanned):
    """Cube.scan / iterateOverDimension for several measures of one cube in one device pass (olap_store_blocks_report):
    `scanned` flags the scanned dimensions (one per dimension).  Returns ((n, C, B) float64 array, kernel launches made):
    [k, c] holds the cells combination c of the scanned dimensions' items receives of store k, as get_data_f64 reads them
    (the default in unset cells), row-major over the kept dimensions."""
    lv = _u32(lens)
    flags = np.ascontiguousarray(np.asarray(scanned, dtype=np.uint8).ravel())
    if len(flags) != len(lv):
        raise ValueError("blocks_report: one flag per dimension")
    n = len(stores)
    combos = int(np.prod([int(l) for l, f in zip(lv, flags) if f], dtype=np.uint64)) if len(lv) else 1
    kept = int(np.prod([int(l) for l, f in zip(lv, flags) if not f], dtype=np.uint64)) if len(lv) else 1
    out = np.zeros((n, combos, kept), np.float64)
    launches = C.c_int(-1)
    check(capi.lib().olap_store_blocks_report(n, _handles(stores), len(lv), lv.ctypes.data_as(capi._pu32), flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              out.ctypes.data_as(capi._pdbl), C.byref(launches)))
    return out, launches.value
