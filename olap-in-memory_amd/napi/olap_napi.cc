// olap_napi.cc — thin N-API binding of include/olap_hip.h for the Node.js host.
//
// Exposes one class, `Store`, wrapping an `olap_store*` (a device-resident measure, the
// replacement of the reference's InMemoryStore, /root/reference/src/store/in-memory.js), plus a few
// module functions.  No arithmetic happens here: every method forwards to the C ABI and turns a
// non-zero return into a JS Error carrying olap_last_error() (the reference's own messages).
// Handles are freed by the GC finalizer (the reference API has no explicit free).
#include <node_api.h>

#include <algorithm>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "olap_hip.h"

#define NAPI_OK(call)                                            \
  do {                                                           \
    if ((call) != napi_ok) {                                     \
      napi_throw_error(env, nullptr, "N-API call failed: " #call); \
      return nullptr;                                            \
    }                                                            \
  } while (0)

static napi_ref g_store_ctor = nullptr;

static napi_value throw_olap(napi_env env, int code) {
  char codebuf[16];
  snprintf(codebuf, sizeof codebuf, "OLAP%d", code);
  napi_throw_error(env, codebuf, olap_last_error());
  return nullptr;
}

// Device memory and the JS garbage collector.  Telling V8 about every result store
// (napi_adjust_external_memory) makes it run incremental mark-sweep steps for each 40 MB result: a
// drillUp then costs ~9 ms of GC around a 70 us kernel.  Telling it nothing would let dead stores
// pile up until the JS heap itself needs collecting.  So V8 is left alone while the stores held by
// live wrappers stay under a budget (OLAP_NAPI_GC_BYTES, default 16 GiB of the 288 GB; keep it
// below the pool's OLAP_POOL_BYTES so that what a collection frees is recycled, not hipFree'd).  When the
// budget is crossed, ONE large external-memory report makes V8 do a full collection right there
// (its hard limit for external memory is far below the amount reported), the report is taken back,
// and the wrappers found dead are swept (below).  The next such collection is not asked for before
// another quarter of the budget has been allocated, so live data above the budget does not thrash.
static int64_t g_held = 0;
static int64_t g_next_gc_at = 0;
static int64_t gc_budget() {
  static int64_t b = -1;
  if (b < 0) {
    const char *e = getenv("OLAP_NAPI_GC_BYTES");
    b = e ? (int64_t)strtoll(e, nullptr, 10) : ((int64_t)16 << 30);
  }
  return b;
}
static void sweep_boxes(napi_env env);
static void account(napi_env env, int64_t delta) {
  g_held += delta;
  if (delta > 0 && g_held > gc_budget() && g_held >= g_next_gc_at) {
    int64_t total;
    const int64_t nudge = (int64_t)8 << 30;
    napi_adjust_external_memory(env, nudge, &total);   // V8 collects synchronously in here
    napi_adjust_external_memory(env, -nudge, &total);
    sweep_boxes(env);
    g_next_gc_at = g_held + gc_budget() / 4;
  }
}

// Node runs N-API finalizers on a later event-loop turn, never inside a synchronous loop (even an
// explicit gc() does not run them), so a loop of 3 000 queries would hold 3 000 result stores.  Each
// wrapper therefore keeps its store in a small box next to a weak reference: once the budget is
// exceeded, creating a store first sweeps the boxes and frees the device memory of every wrapper the
// collector has already found dead (the weak reference is cleared during the GC itself); the late
// finalizer then finds an empty box.
struct StoreBox {
  olap_store *store;
  napi_ref ref;
  bool finalized;
};
static std::vector<StoreBox *> g_boxes;

static void release_box(napi_env env, StoreBox *box) {
  if (!box->store) return;
  account(env, -(int64_t)olap_store_byte_length(box->store));
  olap_store_destroy(box->store);
  box->store = nullptr;
}

static void finalize_store(napi_env env, void *data, void *) {
  StoreBox *box = (StoreBox *)data;
  release_box(env, box);
  if (box->ref) napi_delete_reference(env, box->ref);
  box->ref = nullptr;
  box->finalized = true;  // the box itself is deleted by the next sweep
}

static void sweep_boxes(napi_env env) {
  size_t keep = 0;
  for (size_t i = 0; i < g_boxes.size(); ++i) {
    StoreBox *box = g_boxes[i];
    if (box->finalized) {
      delete box;
      continue;
    }
    if (box->store && box->ref) {
      napi_value alive = nullptr;
      if (napi_get_reference_value(env, box->ref, &alive) == napi_ok && alive == nullptr) release_box(env, box);
    }
    g_boxes[keep++] = box;
  }
  g_boxes.resize(keep);
}

static olap_store *unwrap(napi_env env, napi_value v) {
  void *p = nullptr;
  if (napi_unwrap(env, v, &p) != napi_ok || !p || !((StoreBox *)p)->store) {
    napi_throw_type_error(env, nullptr, "not a Store");
    return nullptr;
  }
  return ((StoreBox *)p)->store;
}

static napi_value wrap_new_store(napi_env env, olap_store *s) {
  napi_value ctor, obj, ext;
  NAPI_OK(napi_get_reference_value(env, g_store_ctor, &ctor));
  NAPI_OK(napi_create_external(env, s, nullptr, nullptr, &ext));
  if (napi_new_instance(env, ctor, 1, &ext, &obj) != napi_ok) {
    olap_store_destroy(s);
    return nullptr;
  }
  return obj;
}

// new Store(size, dtypeCode, defaultKind)  |  new Store(external) [internal]
static napi_value StoreNew(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3], self;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, &self, nullptr));
  napi_valuetype t;
  NAPI_OK(napi_typeof(env, argv[0], &t));
  olap_store *s = nullptr;
  bool adopted = false;  // the handle came from wrap_new_store(), which destroys it itself when this constructor fails
  if (argc == 1 && t == napi_external) {
    void *p;
    NAPI_OK(napi_get_value_external(env, argv[0], &p));
    s = (olap_store *)p;
    adopted = true;
  } else {
    double size = 0;
    int32_t dtype = 0, def = 0;
    NAPI_OK(napi_get_value_double(env, argv[0], &size));
    NAPI_OK(napi_get_value_int32(env, argv[1], &dtype));
    NAPI_OK(napi_get_value_int32(env, argv[2], &def));
    int rc = olap_store_create(&s, (uint64_t)size, dtype, def);
    if (rc) return throw_olap(env, rc);
  }
  static unsigned since_sweep = 0;
  if (++since_sweep >= 1024) {  // housekeeping: drop the boxes of finalized wrappers
    sweep_boxes(env);
    since_sweep = 0;
  }
  StoreBox *box = new StoreBox{s, nullptr, false};
  if (napi_wrap(env, self, box, finalize_store, nullptr, &box->ref) != napi_ok) {
    if (!adopted) olap_store_destroy(s);
    delete box;
    napi_throw_error(env, nullptr, "napi_wrap failed");
    return nullptr;
  }
  g_boxes.push_back(box);
  account(env, (int64_t)olap_store_byte_length(s));
  return self;
}

#define STORE_METHOD_PROLOGUE(MAXARGS)                                     \
  size_t argc = MAXARGS;                                                   \
  napi_value argv[MAXARGS > 0 ? MAXARGS : 1], self;                        \
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, &self, nullptr));       \
  olap_store *s = unwrap(env, self);                                       \
  if (!s) return nullptr;

static napi_value num(napi_env env, double v) {
  napi_value r;
  napi_create_double(env, v, &r);
  return r;
}

static napi_value StoreSize(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(0)
  return num(env, (double)olap_store_size(s));
}
static napi_value StoreByteLength(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(0)
  return num(env, (double)olap_store_byte_length(s));
}
static napi_value StoreDtype(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(0)
  return num(env, olap_store_dtype(s));
}
static napi_value StoreDefault(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(0)
  return num(env, olap_store_default(s));
}

static napi_typedarray_type ta_of(int dtype) {
  switch (dtype) {
    case OLAP_INT32: return napi_int32_array;
    case OLAP_UINT32: return napi_uint32_array;
    case OLAP_FLOAT32: return napi_float32_array;
    default: return napi_float64_array;
  }
}

// setData(typedArray): Float64Array = JS numbers (converted on the device like a TypedArray
// store would); otherwise a typed array of the store's own element type
static napi_value StoreSetData(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(1)
  bool is_ta = false;
  NAPI_OK(napi_is_typedarray(env, argv[0], &is_ta));
  if (!is_ta) {
    napi_throw_type_error(env, nullptr, "setData expects a TypedArray");
    return nullptr;
  }
  napi_typedarray_type type;
  size_t len;
  void *data;
  NAPI_OK(napi_get_typedarray_info(env, argv[0], &type, &len, &data, nullptr, nullptr));
  int rc;
  if (type == napi_float64_array && olap_store_dtype(s) != OLAP_FLOAT64) rc = olap_store_set_data_f64(s, (const double *)data, len);
  else if (type == ta_of(olap_store_dtype(s))) rc = olap_store_set_data(s, data, len);
  else if (olap_store_dtype(s) == OLAP_FLOAT64 && (type == napi_int32_array || type == napi_uint32_array || type == napi_float32_array)) {
    // an integer (or Float32) typed array into Float64 cells — what the Node host keeps integer measures in: widened
    // here, in one pass, instead of element by element in JavaScript
    std::vector<double> wide(len);
    if (type == napi_int32_array) for (size_t i = 0; i < len; ++i) wide[i] = (double)((const int32_t *)data)[i];
    else if (type == napi_uint32_array) for (size_t i = 0; i < len; ++i) wide[i] = (double)((const uint32_t *)data)[i];
    else for (size_t i = 0; i < len; ++i) wide[i] = (double)((const float *)data)[i];
    rc = olap_store_set_data(s, wide.data(), len);
  } else {
    napi_throw_type_error(env, nullptr, "setData: typed array does not match the store's element type");
    return nullptr;
  }
  if (rc) return throw_olap(env, rc);
  return nullptr;
}

static napi_value make_ta(napi_env env, napi_typedarray_type type, size_t elem, size_t n, void **data) {
  napi_value ab, ta;
  NAPI_OK(napi_create_arraybuffer(env, n * elem, data, &ab));
  NAPI_OK(napi_create_typedarray(env, type, n, ab, 0, &ta));
  return ta;
}

static napi_value StoreGetData(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(0)
  void *data;
  const int dt = olap_store_dtype(s);
  napi_value ta = make_ta(env, ta_of(dt), olap_dtype_size(dt), olap_store_size(s), &data);
  if (!ta) return nullptr;
  int rc = olap_store_get_data(s, data);
  if (rc) return throw_olap(env, rc);
  return ta;
}

static napi_value StoreGetDataF64(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(0)
  void *data;
  napi_value ta = make_ta(env, napi_float64_array, 8, olap_store_size(s), &data);
  if (!ta) return nullptr;
  int rc = olap_store_get_data_f64(s, (double *)data);
  if (rc) return throw_olap(env, rc);
  return ta;
}

static napi_value StoreGetStatus(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(0)
  void *data;
  napi_value ta = make_ta(env, napi_int32_array, 4, olap_store_size(s), &data);
  if (!ta) return nullptr;
  int rc = olap_store_get_status(s, (int32_t *)data);
  if (rc) return throw_olap(env, rc);
  return ta;
}

// ascending indices of the set cells, as a Float64Array (indices < 2^53)
static napi_value StoreGetKeys(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(0)
  uint64_t n = 0;
  int rc = olap_store_get_keys(s, nullptr, 0, &n);
  if (rc) return throw_olap(env, rc);
  std::vector<uint64_t> keys(n ? n : 1);
  rc = olap_store_get_keys(s, keys.data(), n, &n);
  if (rc) return throw_olap(env, rc);
  void *data;
  napi_value ta = make_ta(env, napi_float64_array, 8, n, &data);
  if (!ta) return nullptr;
  for (uint64_t i = 0; i < n; ++i) ((double *)data)[i] = (double)keys[i];
  return ta;
}

static napi_value StoreCountSet(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(0)
  uint64_t n = 0;
  int rc = olap_store_count_set(s, &n);
  if (rc) return throw_olap(env, rc);
  return num(env, (double)n);
}

// getValue(i) -> number, or undefined when the cell is unset (Map.get of an absent key)
static napi_value StoreGetValue(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(1)
  double idx = 0;
  NAPI_OK(napi_get_value_double(env, argv[0], &idx));
  napi_value undef;
  napi_get_undefined(env, &undef);
  if (!(idx >= 0) || idx != std::floor(idx)) return undef;
  double v = 0;
  int is_set = 0;
  int rc = olap_store_get_value(s, (uint64_t)idx, &v, &is_set);
  if (rc) return throw_olap(env, rc);
  return is_set ? num(env, v) : undef;
}

// setValue(i, v): undefined / null unset the cell (in-memory.js:122-133)
static napi_value StoreSetValue(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(2)
  double idx = 0, v = 0;
  NAPI_OK(napi_get_value_double(env, argv[0], &idx));
  napi_valuetype t = napi_undefined;
  if (argc > 1) NAPI_OK(napi_typeof(env, argv[1], &t));
  int is_null = (t == napi_undefined || t == napi_null);
  if (!is_null) {
    napi_value coerced;
    NAPI_OK(napi_coerce_to_number(env, argv[1], &coerced));
    NAPI_OK(napi_get_value_double(env, coerced, &v));
  }
  int rc = olap_store_set_value(s, (uint64_t)idx, v, is_null);
  if (rc) return throw_olap(env, rc);
  return nullptr;
}

static napi_value bad_args(napi_env env, const char *what);

// setValues(indexes: Float64Array, values: Float64Array, nulls?: Uint8Array): setValue(indexes[i], values[i]) in list
// order (nulls[i] != 0: unset); every index must be an integer >= 0 (RangeError), checked before the store sees any
struct SetValuesArgs {
  std::vector<uint64_t> idx;
  const double *values = nullptr;
  const uint8_t *nulls = nullptr;

  bool decode(napi_env env, size_t argc, napi_value *argv) {
    napi_typedarray_type ti, tv, tn;
    size_t ni = 0, nv = 0, nn = 0;
    void *pi = nullptr, *pv = nullptr, *pn = nullptr;
    bool is_ta = false;
    if (argc < 2 || napi_is_typedarray(env, argv[0], &is_ta) != napi_ok || !is_ta ||
        napi_get_typedarray_info(env, argv[0], &ti, &ni, &pi, nullptr, nullptr) != napi_ok || ti != napi_float64_array ||
        napi_is_typedarray(env, argv[1], &is_ta) != napi_ok || !is_ta ||
        napi_get_typedarray_info(env, argv[1], &tv, &nv, &pv, nullptr, nullptr) != napi_ok || tv != napi_float64_array || ni != nv) {
      bad_args(env, "setValues(indexes: Float64Array, values: Float64Array, nulls?: Uint8Array) of one length");
      return false;
    }
    napi_valuetype t = napi_undefined;
    if (argc > 2 && napi_typeof(env, argv[2], &t) != napi_ok) t = napi_null;
    if (t != napi_undefined) {
      if (napi_is_typedarray(env, argv[2], &is_ta) != napi_ok || !is_ta ||
          napi_get_typedarray_info(env, argv[2], &tn, &nn, &pn, nullptr, nullptr) != napi_ok || tn != napi_uint8_array || nn != ni) {
        bad_args(env, "setValues: nulls must be undefined or a Uint8Array of the indexes' length");
        return false;
      }
      nulls = (const uint8_t *)pn;
    }
    values = (const double *)pv;
    idx.resize(ni);
    const double *d = (const double *)pi;
    for (size_t i = 0; i < ni; ++i) {
      if (!(d[i] >= 0) || d[i] != std::floor(d[i]) || d[i] >= 18446744073709551616.0) {
        char msg[96];
        snprintf(msg, sizeof msg, "setValues: index %zu is not an integer >= 0 (%g)", i, d[i]);
        napi_throw_range_error(env, nullptr, msg);
        return false;
      }
      idx[i] = (uint64_t)d[i];
    }
    return true;
  }
};

static napi_value StoreSetValues(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(3)
  SetValuesArgs a;
  if (!a.decode(env, argc, argv)) return nullptr;
  int rc = olap_store_set_values(s, a.idx.size(), a.idx.data(), a.values, a.nulls);
  if (rc) return throw_olap(env, rc);
  return nullptr;
}

static napi_value StoreFill(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(1)
  double v = 0;
  napi_value coerced;
  NAPI_OK(napi_coerce_to_number(env, argv[0], &coerced));
  NAPI_OK(napi_get_value_double(env, coerced, &v));
  int rc = olap_store_fill(s, v);
  if (rc) return throw_olap(env, rc);
  return nullptr;
}

static napi_value StoreTotal(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(0)
  double t = 0;
  int rc = olap_store_total(s, &t);
  if (rc) return throw_olap(env, rc);
  return num(env, t);
}

// trackOrder(on = true): keep the reference Map's insertion order (olap_store_track_order)
static napi_value StoreTrackOrder(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(1)
  bool on = true;
  if (argc > 0) {
    napi_valuetype t;
    NAPI_OK(napi_typeof(env, argv[0], &t));
    if (t == napi_boolean) NAPI_OK(napi_get_value_bool(env, argv[0], &on));
  }
  int rc = olap_store_track_order(s, on ? 1 : 0);
  if (rc) return throw_olap(env, rc);
  return nullptr;
}
// orderTracked: 0 = not tracked, 1 = tracked and still ascending, 2 = tracked with an explicit order
static napi_value StoreOrderTracked(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(0)
  return num(env, olap_store_order_tracked(s));
}

static napi_value StoreClone(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(0)
  olap_store *c = nullptr;
  int rc = olap_store_clone(s, &c);
  if (rc) return throw_olap(env, rc);
  return wrap_new_store(env, c);
}

// totals(lens: Uint32Array, methods: Int32Array, launchesOut?: Int32Array) -> Float64Array of the extended cube (olap_store_totals)
static bool get_u32_vec(napi_env env, napi_value v, std::vector<uint32_t> &out);
static void set_path(napi_env env, napi_value out, int path);
static napi_value StoreTotals(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(3)
  std::vector<uint32_t> lens, methods;
  if (argc < 2 || !get_u32_vec(env, argv[0], lens) || !get_u32_vec(env, argv[1], methods) || lens.size() != methods.size()) {
    napi_throw_type_error(env, nullptr, "totals(lens: Uint32Array, methods: Int32Array)");
    return nullptr;
  }
  double n = 1;
  for (uint32_t l : lens) n *= (double)l + 1;
  if (n > 4.0e9) {
    napi_throw_range_error(env, nullptr, "totals: extended cube too large");
    return nullptr;
  }
  void *data;
  napi_value ta = make_ta(env, napi_float64_array, 8, (size_t)n, &data);
  if (!ta) return nullptr;
  static const uint32_t none = 0;
  int launches = 0;
  int rc = olap_store_totals(s, (int)lens.size(), lens.empty() ? &none : lens.data(), lens.empty() ? (const int *)&none : (const int *)methods.data(),
                             (double *)data, nullptr, &launches, nullptr);
  if (rc) return throw_olap(env, rc);
  if (argc > 2) set_path(env, argv[2], launches);
  return ta;
}

// toSparse() -> { indexes: Uint32Array, values: TypedArray } of the set cells (ascending)
static napi_value StoreToSparse(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(0)
  uint64_t n = 0;
  int rc = olap_store_to_sparse(s, nullptr, nullptr, 0, &n);
  if (rc) return throw_olap(env, rc);
  void *idx, *vals;
  const int dt = olap_store_dtype(s);
  napi_value ta_idx = make_ta(env, napi_uint32_array, 4, n, &idx);
  napi_value ta_val = make_ta(env, ta_of(dt), olap_dtype_size(dt), n, &vals);
  if (!ta_idx || !ta_val) return nullptr;
  if (n) {
    rc = olap_store_to_sparse(s, (uint32_t *)idx, vals, n, &n);
    if (rc) return throw_olap(env, rc);
  }
  napi_value out;
  NAPI_OK(napi_create_object(env, &out));
  NAPI_OK(napi_set_named_property(env, out, "indexes", ta_idx));
  NAPI_OK(napi_set_named_property(env, out, "values", ta_val));
  return out;
}

// Store.fromSparse(size, dtypeCode, defaultKind, indexes: Uint32Array, values: TypedArray)
static napi_value StoreFromSparse(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (argc < 5) return nullptr;
  double size = 0;
  int32_t dtype = 0, def = 0;
  NAPI_OK(napi_get_value_double(env, argv[0], &size));
  NAPI_OK(napi_get_value_int32(env, argv[1], &dtype));
  NAPI_OK(napi_get_value_int32(env, argv[2], &def));
  napi_typedarray_type t_idx, t_val;
  size_t n_idx = 0, n_val = 0;
  void *idx = nullptr, *vals = nullptr;
  if (napi_get_typedarray_info(env, argv[3], &t_idx, &n_idx, &idx, nullptr, nullptr) != napi_ok || t_idx != napi_uint32_array ||
      napi_get_typedarray_info(env, argv[4], &t_val, &n_val, &vals, nullptr, nullptr) != napi_ok || n_idx != n_val ||
      t_val != ta_of(dtype)) {
    napi_throw_type_error(env, nullptr, "fromSparse(size, dtype, default, indexes: Uint32Array, values: TypedArray of the store type)");
    return nullptr;
  }
  olap_store *s = nullptr;
  static const uint32_t none = 0;
  int rc = olap_store_from_sparse(&s, (uint64_t)size, dtype, def, idx ? (const uint32_t *)idx : &none, vals ? vals : (const void *)&none, n_idx);
  if (rc) return throw_olap(env, rc);
  return wrap_new_store(env, s);
}

// ---- argument decoding for the bulk operations -----------------------------------------------
static bool get_u32_vec(napi_env env, napi_value v, std::vector<uint32_t> &out) {
  bool is_ta = false;
  if (napi_is_typedarray(env, v, &is_ta) != napi_ok || !is_ta) return false;
  napi_typedarray_type type;
  size_t len;
  void *data;
  if (napi_get_typedarray_info(env, v, &type, &len, &data, nullptr, nullptr) != napi_ok) return false;
  if (type != napi_uint32_array && type != napi_int32_array) return false;
  out.assign((uint32_t *)data, (uint32_t *)data + len);
  return true;
}

// array of Uint32Array / Int32Array, one per dimension
static bool get_tables(napi_env env, napi_value v, std::vector<std::vector<uint32_t>> &out) {
  bool is_arr = false;
  if (napi_is_array(env, v, &is_arr) != napi_ok || !is_arr) return false;
  uint32_t n = 0;
  napi_get_array_length(env, v, &n);
  out.resize(n);
  for (uint32_t i = 0; i < n; ++i) {
    napi_value e;
    if (napi_get_element(env, v, i, &e) != napi_ok || !get_u32_vec(env, e, out[i])) return false;
  }
  return true;
}

struct OpArgs {
  std::vector<uint32_t> a_len, b_len;
  std::vector<std::vector<uint32_t>> tables;
  std::vector<const uint32_t *> ptrs;
  static uint32_t dummy;
  bool decode(napi_env env, napi_value la, napi_value lb, napi_value tb) {
    if (!get_u32_vec(env, la, a_len) || !get_u32_vec(env, lb, b_len) || !get_tables(env, tb, tables)) return false;
    if (a_len.size() != b_len.size() || tables.size() != a_len.size()) return false;
    for (auto &t : tables) ptrs.push_back(t.empty() ? &dummy : t.data());
    return true;
  }
};
uint32_t OpArgs::dummy = 0;

static napi_value bad_args(napi_env env, const char *what) {
  napi_throw_type_error(env, nullptr, what);
  return nullptr;
}

// the caller's current view of the dimensions (oldLen) is applied to the handle first: Cube adds and drops
// one-item dimensions around store calls without touching the cells
static bool sharded_view(napi_env env, olap_sharded_store *s, napi_value old_len) {
  std::vector<uint32_t> lens;
  if (!get_u32_vec(env, old_len, lens)) {
    napi_throw_type_error(env, nullptr, "oldLen must be a Uint32Array");
    return false;
  }
  int rc = olap_sharded_store_reshape(s, (int)lens.size(), lens.data());
  if (rc) {
    throw_olap(env, rc);
    return false;
  }
  return true;
}

static bool decode_lens_tables(napi_env env, napi_value lens, napi_value tables, size_t ndim, std::vector<uint32_t> &len_out,
                               std::vector<std::vector<uint32_t>> &tab_out, std::vector<const uint32_t *> &ptrs) {
  if (!get_u32_vec(env, lens, len_out) || !get_tables(env, tables, tab_out)) return false;
  if (len_out.size() != ndim || tab_out.size() != ndim) return false;
  for (auto &t : tab_out) ptrs.push_back(t.empty() ? &OpArgs::dummy : t.data());
  return true;
}

// drillUp(oldLen, newLen, maps, methodCode)
static napi_value StoreDrillUp(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(4)
  OpArgs a;
  int32_t method = 0;
  if (argc < 4 || !a.decode(env, argv[0], argv[1], argv[2]) || napi_get_value_int32(env, argv[3], &method) != napi_ok)
    return bad_args(env, "drillUp(oldLen: Uint32Array, newLen: Uint32Array, maps: Uint32Array[], method: number)");
  olap_store *out = nullptr;
  int rc = olap_store_drillup(s, &out, (int)a.a_len.size(), a.a_len.data(), a.b_len.data(), a.ptrs.data(), method);
  if (rc) return throw_olap(env, rc);
  return wrap_new_store(env, out);
}

// drillDown(oldLen, newLen, maps, methodCode, distributions: Float64Array | null)
static napi_value StoreDrillDown(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(5)
  OpArgs a;
  int32_t method = 0;
  if (argc < 4 || !a.decode(env, argv[0], argv[1], argv[2]) || napi_get_value_int32(env, argv[3], &method) != napi_ok)
    return bad_args(env, "drillDown(oldLen, newLen, maps, method, distributions)");
  const double *dist = nullptr;
  size_t n_dist = 0;
  if (argc > 4) {
    bool is_ta = false;
    napi_is_typedarray(env, argv[4], &is_ta);
    if (is_ta) {
      napi_typedarray_type type;
      void *data;
      NAPI_OK(napi_get_typedarray_info(env, argv[4], &type, &n_dist, &data, nullptr, nullptr));
      if (type != napi_float64_array) return bad_args(env, "distributions must be a Float64Array");
      dist = (const double *)data;
      static const double none = 0;
      if (!dist) dist = &none;
    }
  }
  olap_store *out = nullptr;
  int rc = olap_store_drilldown(s, &out, (int)a.a_len.size(), a.a_len.data(), a.b_len.data(), a.ptrs.data(), method, dist, n_dist);
  if (rc) return throw_olap(env, rc);
  return wrap_new_store(env, out);
}

// dice(oldLen, newLen, sel: Int32Array[])
static napi_value StoreDice(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(3)
  OpArgs a;
  if (argc < 3 || !a.decode(env, argv[0], argv[1], argv[2])) return bad_args(env, "dice(oldLen, newLen, sel: Int32Array[])");
  olap_store *out = nullptr;
  int rc = olap_store_dice(s, &out, (int)a.a_len.size(), a.a_len.data(), a.b_len.data(), (const int32_t *const *)a.ptrs.data());
  if (rc) return throw_olap(env, rc);
  return wrap_new_store(env, out);
}

// diceDrillUp(oldLen, midLen, newLen, sel: Int32Array[], maps: Uint32Array[], methodCode)
static napi_value StoreDiceDrillUp(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(6)
  OpArgs a;
  std::vector<uint32_t> new_len;
  std::vector<std::vector<uint32_t>> maps;
  int32_t method = 0;
  if (argc < 6 || !a.decode(env, argv[0], argv[1], argv[3]) || !get_u32_vec(env, argv[2], new_len) || !get_tables(env, argv[4], maps) ||
      new_len.size() != a.a_len.size() || maps.size() != a.a_len.size() || napi_get_value_int32(env, argv[5], &method) != napi_ok)
    return bad_args(env, "diceDrillUp(oldLen, midLen, newLen, sel: Int32Array[], maps: Uint32Array[], method)");
  std::vector<const uint32_t *> map_ptrs;
  for (auto &m : maps) map_ptrs.push_back(m.empty() ? &OpArgs::dummy : m.data());
  olap_store *out = nullptr;
  int rc = olap_store_dice_drillup(s, &out, (int)a.a_len.size(), a.a_len.data(), a.b_len.data(), new_len.data(),
                                   (const int32_t *const *)a.ptrs.data(), map_ptrs.data(), method);
  if (rc) return throw_olap(env, rc);
  return wrap_new_store(env, out);
}

// reorder(oldLen, perm: Int32Array)
static napi_value StoreReorder(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(2)
  std::vector<uint32_t> len, perm;
  if (argc < 2 || !get_u32_vec(env, argv[0], len) || !get_u32_vec(env, argv[1], perm) || len.size() != perm.size())
    return bad_args(env, "reorder(oldLen: Uint32Array, perm: Int32Array)");
  olap_store *out = nullptr;
  int rc = olap_store_reorder(s, &out, (int)len.size(), len.data(), (const int32_t *)perm.data());
  if (rc) return throw_olap(env, rc);
  return wrap_new_store(env, out);
}

// load(other: Store, myLen, hisLen, hisToMine: Int32Array[])
static napi_value StoreLoad(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(4)
  if (argc < 4) return bad_args(env, "load(other, myLen, hisLen, hisToMine)");
  olap_store *other = unwrap(env, argv[0]);
  if (!other) return nullptr;
  OpArgs a;
  if (!a.decode(env, argv[1], argv[2], argv[3])) {
    // tables are indexed by HIS dimensions: decode() only checks equal counts
    return bad_args(env, "load(other: Store, myLen, hisLen, hisToMine: Int32Array[])");
  }
  int rc = olap_store_load(s, other, (int)a.a_len.size(), a.a_len.data(), a.b_len.data(), (const int32_t *const *)a.ptrs.data());
  if (rc) return throw_olap(env, rc);
  return nullptr;
}

// ---- filtered totals and copies (olap_store_select_total / olap_store_copy_select) ----------------------
// A selection: lens (Uint32Array, the cells' dimensions), axis (Int32Array: cube dimension or -1 per level, nesting
// order) and lists (Int32Array[] of item indices, -1 = a cell that does not exist).
struct SelectArgs {
  std::vector<uint32_t> lens, n_sel;
  std::vector<int32_t> axis;
  std::vector<std::vector<uint32_t>> lists;
  std::vector<const int32_t *> ptrs;
  bool decode(napi_env env, napi_value l, napi_value a, napi_value t) {
    std::vector<uint32_t> ax;
    if (!get_u32_vec(env, l, lens) || !get_u32_vec(env, a, ax) || !get_tables(env, t, lists) || lists.size() != ax.size()) return false;
    axis.assign(ax.begin(), ax.end());
    for (auto &v : lists) {
      n_sel.push_back((uint32_t)v.size());
      ptrs.push_back(v.empty() ? (const int32_t *)&OpArgs::dummy : (const int32_t *)v.data());
    }
    return true;
  }
};

static void set_path(napi_env env, napi_value out, int path) {
  bool is_ta = false;
  if (napi_is_typedarray(env, out, &is_ta) != napi_ok || !is_ta) return;
  napi_typedarray_type type;
  size_t len;
  void *data;
  if (napi_get_typedarray_info(env, out, &type, &len, &data, nullptr, nullptr) == napi_ok && type == napi_int32_array && len >= 1)
    ((int32_t *)data)[0] = path;
}

// selectTotal(lens, axis, lists, pathOut?: Int32Array) -> number; pathOut[0] = 1 (certified reduction) | 0 (sequential)
static napi_value StoreSelectTotal(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(4)
  SelectArgs a;
  if (argc < 3 || !a.decode(env, argv[0], argv[1], argv[2])) return bad_args(env, "selectTotal(lens: Uint32Array, axis: Int32Array, lists: Int32Array[])");
  double total = 0;
  int path = 1;
  int rc = olap_store_select_total(s, (int)a.lens.size(), a.lens.data(), (int)a.axis.size(), a.axis.data(), a.n_sel.data(), a.ptrs.data(), &total, &path);
  if (rc) return throw_olap(env, rc);
  if (argc > 3) set_path(env, argv[3], path);
  return num(env, total);
}

// copySelect(source: Store, lens, axis, lists): this.setValue(pos, source.getValue(pos)) over the selection
static napi_value StoreCopySelect(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(4)
  olap_store *src = argc > 0 ? unwrap(env, argv[0]) : nullptr;
  if (!src) return nullptr;
  SelectArgs a;
  if (argc < 4 || !a.decode(env, argv[1], argv[2], argv[3])) return bad_args(env, "copySelect(source: Store, lens: Uint32Array, axis: Int32Array, lists: Int32Array[])");
  int rc = olap_store_copy_select(s, src, (int)a.lens.size(), a.lens.data(), (int)a.axis.size(), a.axis.data(), a.n_sel.data(), a.ptrs.data());
  if (rc) return throw_olap(env, rc);
  return nullptr;
}

// The (code: Int32Array, consts: Float64Array, stores: Store[], scalars: Float64Array) of evalFormula and setFormula.
// An empty typed array may come without a buffer: the C ABI then gets the address of a zero instead of NULL.
struct ProgramArgs {
  size_t n_code = 0, n_consts = 0, n_scalars = 0;
  void *code_p = nullptr, *consts_p = nullptr, *scalars_p = nullptr;
  uint32_t n_inputs = 0;
  bool no_list = false;  // (after a failed decode_program) the typed arrays were fine, `stores` is no array
  std::vector<const olap_store *> stores;
  const int32_t *code() const { return (const int32_t *)code_p; }
  const double *consts() const { return consts_p ? (const double *)consts_p : &zero(); }
  const double *scalars() const { return scalars_p ? (const double *)scalars_p : &zero(); }
  static const double &zero() {
    static const double z = 0;
    return z;
  }
  // the three typed arrays and the length of the store list; false: the arguments have the wrong types
  bool decode_program(napi_env env, const napi_value *argv) {
    napi_typedarray_type t;
    if (napi_get_typedarray_info(env, argv[0], &t, &n_code, &code_p, nullptr, nullptr) != napi_ok || t != napi_int32_array ||
        napi_get_typedarray_info(env, argv[1], &t, &n_consts, &consts_p, nullptr, nullptr) != napi_ok || t != napi_float64_array ||
        napi_get_typedarray_info(env, argv[3], &t, &n_scalars, &scalars_p, nullptr, nullptr) != napi_ok || t != napi_float64_array)
      return false;
    bool is_arr = false;
    napi_is_array(env, argv[2], &is_arr);
    no_list = !is_arr;
    if (!is_arr) return false;
    napi_get_array_length(env, argv[2], &n_inputs);
    return true;
  }
  // the stores of a Store[]; false with an exception pending when an element is not a Store
  bool decode_stores(napi_env env, napi_value list) {
    stores.resize(n_inputs);
    for (uint32_t i = 0; i < n_inputs; ++i) {
      napi_value e;
      if (napi_get_element(env, list, i, &e) != napi_ok) return false;
      stores[i] = unwrap(env, e);
      if (!stores[i]) return false;
    }
    return true;
  }
};

// evalFormula(code: Int32Array, consts: Float64Array, stores: Store[], scalars: Float64Array) -> Float64Array
static napi_value EvalFormula(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (argc < 4) return bad_args(env, "evalFormula(code, consts, stores, scalars)");
  ProgramArgs a;
  if (!a.decode_program(env, argv))
    return bad_args(env, a.no_list ? "evalFormula: stores must be an array of Store" : "evalFormula(code: Int32Array, consts: Float64Array, stores: Store[], scalars: Float64Array)");
  if (!a.decode_stores(env, argv[2])) return nullptr;
  const uint64_t n = a.n_inputs ? olap_store_size(a.stores[0]) : 0;
  void *out;
  napi_value ta = make_ta(env, napi_float64_array, 8, n, &out);
  if (!ta) return nullptr;
  int rc = olap_store_eval_formula(a.code(), (int)a.n_code, a.consts(), (int)a.n_consts, (int)a.n_inputs, a.stores.data(), a.scalars(), (int)a.n_scalars,
                                   (double *)out);
  if (rc) return throw_olap(env, rc);
  return ta;
}

// store.setFormula(code, consts, stores: Store[], scalars): store.setData(evalFormula(...)) in one device call, without the host
static napi_value StoreSetFormula(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(4)
  ProgramArgs a;
  if (argc < 4 || !a.decode_program(env, argv)) return bad_args(env, "setFormula(code: Int32Array, consts: Float64Array, stores: Store[], scalars: Float64Array)");
  if (!a.decode_stores(env, argv[2])) return nullptr;
  int rc = olap_store_set_formula(s, a.code(), (int)a.n_code, a.consts(), (int)a.n_consts, (int)a.n_inputs, a.stores.data(), a.scalars(), (int)a.n_scalars);
  if (rc) return throw_olap(env, rc);
  return nullptr;
}

// A formula over a selection: code (Int32Array), consts (Float64Array) and stores (Store[], the inputs)
struct FormulaArgs {
  size_t n_code = 0, n_consts = 0;
  void *code = nullptr, *consts = nullptr;
  std::vector<const olap_store *> stores;
  // false with an exception pending when a store is not one
  bool decode(napi_env env, napi_value c, napi_value k, napi_value st, bool *bad) {
    napi_typedarray_type t;
    *bad = true;
    if (napi_get_typedarray_info(env, c, &t, &n_code, &code, nullptr, nullptr) != napi_ok || t != napi_int32_array ||
        napi_get_typedarray_info(env, k, &t, &n_consts, &consts, nullptr, nullptr) != napi_ok || t != napi_float64_array)
      return false;
    bool is_arr = false;
    napi_is_array(env, st, &is_arr);
    if (!is_arr) return false;
    *bad = false;
    uint32_t n = 0;
    napi_get_array_length(env, st, &n);
    stores.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
      napi_value e;
      if (napi_get_element(env, st, i, &e) != napi_ok) return false;
      stores[i] = unwrap(env, e);
      if (!stores[i]) return false;
    }
    return true;
  }
  const double *consts_ptr() const {
    static const double zero = 0;
    return consts ? (const double *)consts : &zero;
  }
};

// selectTotalFormula(code, consts, stores: Store[], lens, axis, lists, pathOut?: Int32Array) -> number (olap_formula_select_total)
static napi_value SelectTotalFormula(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const char *usage = "selectTotalFormula(code: Int32Array, consts: Float64Array, stores: Store[], lens: Uint32Array, axis: Int32Array, lists: Int32Array[])";
  if (argc < 6) return bad_args(env, usage);
  FormulaArgs f;
  bool bad;
  if (!f.decode(env, argv[0], argv[1], argv[2], &bad)) return bad ? bad_args(env, usage) : nullptr;
  SelectArgs a;
  if (!a.decode(env, argv[3], argv[4], argv[5])) return bad_args(env, usage);
  double total = 0;
  int path = 1;
  int rc = olap_formula_select_total((const int32_t *)f.code, (int)f.n_code, f.consts_ptr(), (int)f.n_consts, (int)f.stores.size(), f.stores.data(),
                                     (int)a.lens.size(), a.lens.data(), (int)a.axis.size(), a.axis.data(), a.n_sel.data(), a.ptrs.data(), &total, &path);
  if (rc) return throw_olap(env, rc);
  if (argc > 6) set_path(env, argv[6], path);
  return num(env, total);
}

// totalsFormula(code, consts, stores: Store[], lens: Uint32Array, methods: Int32Array /* stores.length * lens.length */,
//               launchesOut?: Int32Array) -> Float64Array of the formula's extended cube (olap_formula_totals)
static napi_value TotalsFormula(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const char *usage = "totalsFormula(code: Int32Array, consts: Float64Array, stores: Store[], lens: Uint32Array, methods: Int32Array)";
  if (argc < 5) return bad_args(env, usage);
  FormulaArgs f;
  bool bad;
  if (!f.decode(env, argv[0], argv[1], argv[2], &bad)) return bad ? bad_args(env, usage) : nullptr;
  std::vector<uint32_t> lens, methods;
  if (!get_u32_vec(env, argv[3], lens) || !get_u32_vec(env, argv[4], methods) || methods.size() != f.stores.size() * lens.size()) return bad_args(env, usage);
  double n = 1;
  for (uint32_t l : lens) n *= (double)l + 1;
  if (n > 4.0e9) {
    napi_throw_range_error(env, nullptr, "totals: extended cube too large");
    return nullptr;
  }
  void *data;
  napi_value ta = make_ta(env, napi_float64_array, 8, (size_t)n, &data);
  if (!ta) return nullptr;
  static const uint32_t none = 0;
  int launches = 0;
  int rc = olap_formula_totals((const int32_t *)f.code, (int)f.n_code, f.consts_ptr(), (int)f.n_consts, (int)f.stores.size(), f.stores.data(),
                               (int)lens.size(), lens.empty() ? &none : lens.data(), methods.empty() ? (const int *)&none : (const int *)methods.data(),
                               (double *)data, &launches, nullptr);
  if (rc) return throw_olap(env, rc);
  if (argc > 5) set_path(env, argv[5], launches);
  return ta;
}

// totalsReport(stores: Store[], lens: Uint32Array, methods: Int32Array /* stores.length * lens.length */, outStored: Int32Array,
//              nCode: Int32Array, code: Int32Array, nConsts: Int32Array, consts: Float64Array, nInputs: Int32Array,
//              formulaInputs: Int32Array, launchesOut?: Int32Array)
//   -> Float64Array of outStored.length extended cubes, one after the other (olap_totals_report; the flat arrays as there)
static napi_value TotalsReport(napi_env env, napi_callback_info info) {
  size_t argc = 11;
  napi_value argv[11];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const char *usage =
      "totalsReport(stores: Store[], lens: Uint32Array, methods: Int32Array, outStored: Int32Array, nCode: Int32Array, code: Int32Array, "
      "nConsts: Int32Array, consts: Float64Array, nInputs: Int32Array, formulaInputs: Int32Array)";
  if (argc < 10) return bad_args(env, usage);
  bool is_arr = false;
  napi_is_array(env, argv[0], &is_arr);
  if (!is_arr) return bad_args(env, usage);
  uint32_t n_stores = 0;
  napi_get_array_length(env, argv[0], &n_stores);
  std::vector<const olap_store *> stores(n_stores);
  for (uint32_t i = 0; i < n_stores; ++i) {
    napi_value e;
    NAPI_OK(napi_get_element(env, argv[0], i, &e));
    stores[i] = unwrap(env, e);
    if (!stores[i]) return nullptr;
  }
  std::vector<uint32_t> lens, methods, out_stored, n_code, code, n_consts, n_inputs, formula_inputs;
  napi_typedarray_type t;
  size_t consts_len = 0;
  void *consts = nullptr;
  if (!get_u32_vec(env, argv[1], lens) || !get_u32_vec(env, argv[2], methods) || !get_u32_vec(env, argv[3], out_stored) ||
      !get_u32_vec(env, argv[4], n_code) || !get_u32_vec(env, argv[5], code) || !get_u32_vec(env, argv[6], n_consts) ||
      napi_get_typedarray_info(env, argv[7], &t, &consts_len, &consts, nullptr, nullptr) != napi_ok || t != napi_float64_array ||
      !get_u32_vec(env, argv[8], n_inputs) || !get_u32_vec(env, argv[9], formula_inputs))
    return bad_args(env, usage);
  const size_t n_out = out_stored.size();
  if (methods.size() != stores.size() * lens.size() || n_code.size() != n_out || n_consts.size() != n_out || n_inputs.size() != n_out) return bad_args(env, usage);
  // the programs lie one after the other: the flat arrays must hold what the counts announce
  uint64_t words = 0, constants = 0, picks = 0;
  for (size_t k = 0; k < n_out; ++k) {
    if ((int32_t)n_code[k] < 0 || (int32_t)n_consts[k] < 0 || (int32_t)n_inputs[k] < 0) return bad_args(env, usage);
    words += n_code[k], constants += n_consts[k], picks += n_inputs[k];
  }
  if (words > code.size() || constants > consts_len || picks > formula_inputs.size()) return bad_args(env, usage);
  // the size limit of olap_totals_report, before the result is allocated: the outputs and the stores no output exports
  std::vector<bool> exported(stores.size(), false);
  for (uint32_t i : out_stored)
    if (i < stores.size()) exported[i] = true;
  size_t scratch = 0;
  for (bool x : exported) scratch += !x;
  double ext = 1;
  for (uint32_t l : lens) ext *= (double)l + 1;
  const double n = (double)n_out * ext;
  if ((double)(n_out + scratch) * ext > 4.0e9) {
    napi_throw_range_error(env, nullptr, "totals: extended cube too large");
    return nullptr;
  }
  void *data;
  napi_value ta = make_ta(env, napi_float64_array, 8, (size_t)n, &data);
  if (!ta) return nullptr;
  static const uint32_t none = 0;
  static const double zero = 0;
  int launches = 0;
  int rc = olap_totals_report((int)stores.size(), stores.data(), (int)lens.size(), lens.empty() ? &none : lens.data(),
                              methods.empty() ? (const int *)&none : (const int *)methods.data(), (int)n_out, (const int *)out_stored.data(),
                              (const int *)n_code.data(), code.empty() ? (const int32_t *)&none : (const int32_t *)code.data(), (const int *)n_consts.data(),
                              consts ? (const double *)consts : &zero, (const int *)n_inputs.data(),
                              formula_inputs.empty() ? (const int *)&none : (const int *)formula_inputs.data(), (double *)data, &launches, nullptr);
  if (rc) return throw_olap(env, rc);
  if (argc > 10) set_path(env, argv[10], launches);
  return ta;
}

// copySelectFormula(code, consts, stores: Store[], lens, axis, lists): this.setValue(pos, formula(pos)) over the selection
static napi_value StoreCopySelectFormula(napi_env env, napi_callback_info info) {
  STORE_METHOD_PROLOGUE(6)
  const char *usage = "copySelectFormula(code: Int32Array, consts: Float64Array, stores: Store[], lens: Uint32Array, axis: Int32Array, lists: Int32Array[])";
  if (argc < 6) return bad_args(env, usage);
  FormulaArgs f;
  bool bad;
  if (!f.decode(env, argv[0], argv[1], argv[2], &bad)) return bad ? bad_args(env, usage) : nullptr;
  SelectArgs a;
  if (!a.decode(env, argv[3], argv[4], argv[5])) return bad_args(env, usage);
  int rc = olap_store_copy_select_formula(s, (const int32_t *)f.code, (int)f.n_code, f.consts_ptr(), (int)f.n_consts, (int)f.stores.size(),
                                          f.stores.data(), (int)a.lens.size(), a.lens.data(), (int)a.axis.size(), a.axis.data(), a.n_sel.data(),
                                          a.ptrs.data());
  if (rc) return throw_olap(env, rc);
  return nullptr;
}

// ---- diceMulti / diceDrillUpMulti / drillDownMulti: ALL stored measures of a cube behind one call (olap_store_*_multi)
namespace {
// the Store[] and (where the operation has rules) the Int32Array with a rule per store
struct MultiArgs {
  std::vector<const olap_store *> stores;
  const int *methods = nullptr;
  bool miscounted = false;  // the rules are an Int32Array, but not one per store
  // false with an exception pending, or — *usage_error — arguments of the wrong shape
  bool decode(napi_env env, napi_value list, const napi_value *rules, bool *usage_error) {
    *usage_error = true;
    bool is_arr = false;
    if (napi_is_array(env, list, &is_arr) != napi_ok || !is_arr) return false;
    uint32_t n = 0;
    napi_get_array_length(env, list, &n);
    if (rules) {
      napi_typedarray_type mt;
      size_t n_methods = 0;
      void *mdata = nullptr;
      bool is_ta = false;
      if (napi_is_typedarray(env, *rules, &is_ta) != napi_ok || !is_ta || napi_get_typedarray_info(env, *rules, &mt, &n_methods, &mdata, nullptr, nullptr) != napi_ok ||
          mt != napi_int32_array)
        return false;
      if ((miscounted = n_methods != n)) return false;
      static const int none = 0;
      methods = n ? (const int *)mdata : &none;
    }
    *usage_error = false;
    stores.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
      napi_value e;
      if (napi_get_element(env, list, i, &e) != napi_ok) return false;
      stores[i] = unwrap(env, e);
      if (!stores[i]) return false;
    }
    return true;
  }
};
}  // namespace

static napi_value wrap_new_stores(napi_env env, std::vector<olap_store *> &outs) {
  const uint32_t n = (uint32_t)outs.size();
  napi_value arr;
  NAPI_OK(napi_create_array_with_length(env, n, &arr));
  for (uint32_t i = 0; i < n; ++i) {
    napi_value w = wrap_new_store(env, outs[i]);
    if (!w) {
      for (uint32_t j = i + 1; j < n; ++j) olap_store_destroy(outs[j]);
      return nullptr;
    }
    napi_set_element(env, arr, i, w);
  }
  return arr;
}

// The common end of the *Multi calls: the C ABI's refusal thrown, else the launch count into the optional Int32Array
// at argv[launches_at].  false: an exception is pending.
static bool multi_done(napi_env env, int rc, size_t argc, const napi_value *argv, size_t launches_at, int launches) {
  if (rc) {
    throw_olap(env, rc);
    return false;
  }
  if (argc > launches_at) set_path(env, argv[launches_at], launches);
  return true;
}

// drillUpMulti(stores: Store[], methods: Int32Array, oldLen, newLen, maps) -> Store[]
// Every stored measure of a cube with its own rule for the rolled-up dimension (olap_store_drillup_multi): one
// mixed-rule launch where the roll-up allows it, one launch per rule otherwise.
static napi_value DrillUpMulti(napi_env env, napi_callback_info info) {
  const char *usage = "drillUpMulti(stores: Store[], methods: Int32Array, oldLen: Uint32Array, newLen: Uint32Array, maps: Uint32Array[])";
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  OpArgs a;
  MultiArgs m;
  bool bad = true;
  if (argc < 5 || !a.decode(env, argv[2], argv[3], argv[4])) return bad_args(env, usage);
  if (!m.decode(env, argv[0], &argv[1], &bad)) return m.miscounted ? bad_args(env, "drillUpMulti: one method per store") : bad ? bad_args(env, usage) : nullptr;
  std::vector<olap_store *> outs(m.stores.size(), nullptr);
  int rc = olap_store_drillup_multi((int)m.stores.size(), m.stores.data(), m.methods, outs.data(), (int)a.a_len.size(), a.a_len.data(), a.b_len.data(),
                                    a.ptrs.data());
  return multi_done(env, rc, 0, nullptr, 0, 0) ? wrap_new_stores(env, outs) : nullptr;
}

// diceMulti(stores: Store[], oldLen, newLen, sel: Int32Array[], launchesOut?: Int32Array) -> Store[]
static napi_value DiceMulti(napi_env env, napi_callback_info info) {
  const char *usage = "diceMulti(stores: Store[], oldLen: Uint32Array, newLen: Uint32Array, sel: Int32Array[], launchesOut?: Int32Array)";
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  OpArgs a;
  MultiArgs m;
  bool bad = true;
  if (argc < 4 || !a.decode(env, argv[1], argv[2], argv[3])) return bad_args(env, usage);
  if (!m.decode(env, argv[0], nullptr, &bad)) return bad ? bad_args(env, usage) : nullptr;
  std::vector<olap_store *> outs(m.stores.size(), nullptr);
  int launches = 0;
  int rc = olap_store_dice_multi((int)m.stores.size(), m.stores.data(), outs.data(), (int)a.a_len.size(), a.a_len.data(), a.b_len.data(),
                                 (const int32_t *const *)a.ptrs.data(), &launches);
  return multi_done(env, rc, argc, argv, 4, launches) ? wrap_new_stores(env, outs) : nullptr;
}

// reorderMulti(stores: Store[], oldLen, perm: Int32Array, launchesOut?: Int32Array) -> Store[]
static napi_value ReorderMulti(napi_env env, napi_callback_info info) {
  const char *usage = "reorderMulti(stores: Store[], oldLen: Uint32Array, perm: Int32Array, launchesOut?: Int32Array)";
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  std::vector<uint32_t> len, perm;
  MultiArgs m;
  bool bad = true;
  if (argc < 3 || !get_u32_vec(env, argv[1], len) || !get_u32_vec(env, argv[2], perm) || len.size() != perm.size()) return bad_args(env, usage);
  if (!m.decode(env, argv[0], nullptr, &bad)) return bad ? bad_args(env, usage) : nullptr;
  std::vector<olap_store *> outs(m.stores.size(), nullptr);
  int launches = 0;
  int rc = olap_store_reorder_multi((int)m.stores.size(), m.stores.data(), outs.data(), (int)len.size(), len.data(), (const int32_t *)perm.data(), &launches);
  return multi_done(env, rc, argc, argv, 3, launches) ? wrap_new_stores(env, outs) : nullptr;
}

// loadMulti(targets: Store[], sources: Store[], myLen, hisLen, hisToMine: Int32Array[], launchesOut?: Int32Array): targets[i].load(sources[i])
static napi_value LoadMulti(napi_env env, napi_callback_info info) {
  const char *usage = "loadMulti(targets: Store[], sources: Store[], myLen: Uint32Array, hisLen: Uint32Array, hisToMine: Int32Array[], launchesOut?: Int32Array)";
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  OpArgs a;
  MultiArgs t, o;
  bool bad = true;
  if (argc < 5 || !a.decode(env, argv[2], argv[3], argv[4])) return bad_args(env, usage);
  if (!t.decode(env, argv[0], nullptr, &bad)) return bad ? bad_args(env, usage) : nullptr;
  if (!o.decode(env, argv[1], nullptr, &bad)) return bad ? bad_args(env, usage) : nullptr;
  if (t.stores.size() != o.stores.size()) return bad_args(env, usage);
  int launches = 0;
  int rc = olap_store_load_multi((int)t.stores.size(), (olap_store *const *)t.stores.data(), o.stores.data(), (int)a.a_len.size(), a.a_len.data(),
                                 a.b_len.data(), (const int32_t *const *)a.ptrs.data(), &launches);
  multi_done(env, rc, argc, argv, 5, launches);
  return nullptr;
}

// composeMulti(sources: Store[], myLen, hisLen, hisToMine: Int32Array[], fills: Float64Array, hasFill: Uint8Array, launchesOut?: Int32Array)
//   -> Store[]: new stores that end as create [+ fill(fills[i]) where hasFill[i]] + load(sources[i]) (olap_store_compose_multi)
static napi_value ComposeMulti(napi_env env, napi_callback_info info) {
  const char *usage =
      "composeMulti(sources: Store[], myLen: Uint32Array, hisLen: Uint32Array, hisToMine: Int32Array[], fills: Float64Array, hasFill: Uint8Array, "
      "launchesOut?: Int32Array)";
  size_t argc = 7;
  napi_value argv[7];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  OpArgs a;
  MultiArgs m;
  bool bad = true;
  if (argc < 6 || !a.decode(env, argv[1], argv[2], argv[3])) return bad_args(env, usage);
  for (size_t d = 0; d < a.tables.size(); ++d)
    if (a.tables[d].size() != a.b_len[d]) return bad_args(env, usage);  // one entry per item of his
  if (!m.decode(env, argv[0], nullptr, &bad)) return bad ? bad_args(env, usage) : nullptr;
  napi_typedarray_type vt, ft;
  size_t n_values = 0, n_flags = 0;
  void *values = nullptr, *flags = nullptr;
  if (napi_get_typedarray_info(env, argv[4], &vt, &n_values, &values, nullptr, nullptr) != napi_ok || vt != napi_float64_array ||
      napi_get_typedarray_info(env, argv[5], &ft, &n_flags, &flags, nullptr, nullptr) != napi_ok || ft != napi_uint8_array ||
      n_values != m.stores.size() || n_flags != m.stores.size())
    return bad_args(env, usage);
  std::vector<olap_store *> outs(m.stores.size(), nullptr);
  int launches = 0;
  int rc = olap_store_compose_multi((int)m.stores.size(), m.stores.data(), (const double *)values, (const uint8_t *)flags, outs.data(),
                                    (int)a.a_len.size(), a.a_len.data(), a.b_len.data(), (const int32_t *const *)a.ptrs.data(), &launches);
  return multi_done(env, rc, argc, argv, 6, launches) ? wrap_new_stores(env, outs) : nullptr;
}

// blocksReport(stores: Store[], lens: Uint32Array, scanned: Uint8Array, launchesOut?: Int32Array)
//   -> Float64Array of stores.length results, one after the other, each [scanned..., kept...] (olap_store_blocks_report)
static napi_value BlocksReport(napi_env env, napi_callback_info info) {
  const char *usage = "blocksReport(stores: Store[], lens: Uint32Array, scanned: Uint8Array, launchesOut?: Int32Array)";
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  std::vector<uint32_t> lens;
  MultiArgs m;
  bool bad = true;
  napi_typedarray_type ft;
  size_t n_flags = 0;
  void *flags = nullptr;
  if (argc < 3 || !get_u32_vec(env, argv[1], lens) || napi_get_typedarray_info(env, argv[2], &ft, &n_flags, &flags, nullptr, nullptr) != napi_ok ||
      ft != napi_uint8_array || n_flags != lens.size())
    return bad_args(env, usage);
  if (!m.decode(env, argv[0], nullptr, &bad)) return bad ? bad_args(env, usage) : nullptr;
  // the byte cap of olap_store_blocks_report, before the result is allocated
  double cells = 1;
  for (uint32_t l : lens) cells *= (double)l;
  double cap = (double)OLAP_BLOCKS_MAX_BYTES;
  if (const char *e = getenv("OLAP_BLOCKS_MAX_BYTES")) cap = std::min(cap, strtod(e, nullptr));
  if ((double)m.stores.size() * cells * 8.0 > cap) {
    napi_throw_range_error(env, nullptr, "blocks: the result is larger than one call may bring back");
    return nullptr;
  }
  void *data;
  napi_value ta = make_ta(env, napi_float64_array, 8, (size_t)((double)m.stores.size() * cells), &data);
  if (!ta) return nullptr;
  static const uint32_t none = 0;
  static const uint8_t no_flag = 0;
  static double no_cell = 0;
  int launches = 0;
  int rc = olap_store_blocks_report((int)m.stores.size(), m.stores.data(), (int)lens.size(), lens.empty() ? &none : lens.data(),
                                    flags ? (const uint8_t *)flags : &no_flag, data ? (double *)data : &no_cell, &launches);
  return multi_done(env, rc, argc, argv, 3, launches) ? ta : nullptr;
}

// diceDrillUpMulti(stores: Store[], methods: Int32Array, oldLen, midLen, newLen, sel: Int32Array[], maps: Uint32Array[], launchesOut?) -> Store[]
static napi_value DiceDrillUpMulti(napi_env env, napi_callback_info info) {
  const char *usage = "diceDrillUpMulti(stores: Store[], methods: Int32Array, oldLen, midLen, newLen, sel: Int32Array[], maps: Uint32Array[], launchesOut?: Int32Array)";
  size_t argc = 8;
  napi_value argv[8];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  OpArgs a;
  MultiArgs m;
  std::vector<uint32_t> new_len;
  std::vector<std::vector<uint32_t>> maps;
  bool bad = true;
  if (argc < 7 || !a.decode(env, argv[2], argv[3], argv[5]) || !get_u32_vec(env, argv[4], new_len) || !get_tables(env, argv[6], maps) ||
      new_len.size() != a.a_len.size() || maps.size() != a.a_len.size())
    return bad_args(env, usage);
  if (!m.decode(env, argv[0], &argv[1], &bad)) return bad ? bad_args(env, usage) : nullptr;
  std::vector<const uint32_t *> map_ptrs;
  for (auto &t : maps) map_ptrs.push_back(t.empty() ? &OpArgs::dummy : t.data());
  std::vector<olap_store *> outs(m.stores.size(), nullptr);
  int launches = 0;
  int rc = olap_store_dice_drillup_multi((int)m.stores.size(), m.stores.data(), m.methods, outs.data(), (int)a.a_len.size(), a.a_len.data(), a.b_len.data(),
                                         new_len.data(), (const int32_t *const *)a.ptrs.data(), map_ptrs.data(), &launches);
  return multi_done(env, rc, argc, argv, 7, launches) ? wrap_new_stores(env, outs) : nullptr;
}

// drillDownMulti(stores: Store[], methods: Int32Array, oldLen, newLen, maps: Uint32Array[], launchesOut?) -> Store[]
// methods[i]: the code Store.drillDown takes (0 = sum, else a copy; | 0x100: a measure declared int32 / uint32); no distributions
static napi_value DrillDownMulti(napi_env env, napi_callback_info info) {
  const char *usage = "drillDownMulti(stores: Store[], methods: Int32Array, oldLen: Uint32Array, newLen: Uint32Array, maps: Uint32Array[], launchesOut?: Int32Array)";
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  OpArgs a;
  MultiArgs m;
  bool bad = true;
  if (argc < 5 || !a.decode(env, argv[2], argv[3], argv[4])) return bad_args(env, usage);
  if (!m.decode(env, argv[0], &argv[1], &bad)) return bad ? bad_args(env, usage) : nullptr;
  std::vector<olap_store *> outs(m.stores.size(), nullptr);
  int launches = 0;
  int rc = olap_store_drilldown_multi((int)m.stores.size(), m.stores.data(), m.methods, outs.data(), (int)a.a_len.size(), a.a_len.data(), a.b_len.data(),
                                      a.ptrs.data(), &launches);
  return multi_done(env, rc, argc, argv, 5, launches) ? wrap_new_stores(env, outs) : nullptr;
}

// What the calls along one dimension share behind their own scalars: lens and axis at argv[lens_at] and the next,
// groups (null: one group) and nGroups at argv[groups_at] and the next.
struct AlongArgs {
  std::vector<uint32_t> lens, groups;
  int32_t axis = -1;
  uint32_t n_groups = 0;
  bool one_group = true;
  static bool refuse(napi_env env, const char *what) {
    bad_args(env, what);
    return false;
  }
  // false: refused (a TypeError is pending), with `usage` or with "<name>: one group per item of the dimension"
  bool decode(napi_env env, const napi_value *argv, size_t lens_at, size_t groups_at, const char *name, const char *usage) {
    napi_valuetype gt = napi_undefined;
    if (!get_u32_vec(env, argv[lens_at], lens) || napi_get_value_int32(env, argv[lens_at + 1], &axis) != napi_ok ||
        napi_typeof(env, argv[groups_at], &gt) != napi_ok || napi_get_value_uint32(env, argv[groups_at + 1], &n_groups) != napi_ok)
      return refuse(env, usage);
    one_group = gt == napi_null || gt == napi_undefined;
    if (!one_group && !get_u32_vec(env, argv[groups_at], groups)) return refuse(env, usage);
    // one entry per item of the dimension (the C ABI reads lens[axis] of them)
    if (!one_group && (axis < 0 || (size_t)axis >= lens.size() || groups.size() != lens[axis]))
      return refuse(env, (std::string(name) + ": one group per item of the dimension").c_str());
    return true;
  }
  int ndim() const { return (int)lens.size(); }
  const uint32_t *lens_data() const { return lens.empty() ? &OpArgs::dummy : lens.data(); }
  const uint32_t *map() const { return one_group ? nullptr : groups.empty() ? &OpArgs::dummy : groups.data(); }
};

// the end of a *Multi call that makes stores: multi_done, then the results as Store objects
static napi_value multi_stores(napi_env env, int rc, size_t argc, const napi_value *argv, size_t launches_at, int launches, std::vector<olap_store *> &outs) {
  return multi_done(env, rc, argc, argv, launches_at, launches) ? wrap_new_stores(env, outs) : nullptr;
}

// cumulateMulti(stores: Store[], methods: Int32Array, lens, axis: number, groups: Uint32Array | null, nGroups: number, launchesOut?) -> Store[]
// Running aggregates along dimension `axis` (olap_store_cumulate_multi): groups[k] < nGroups is the group of item k; null: one group.
static napi_value CumulateMulti(napi_env env, napi_callback_info info) {
  const char *usage =
      "cumulateMulti(stores: Store[], methods: Int32Array, lens: Uint32Array, axis: number, groups: Uint32Array | null, nGroups: number, launchesOut?: Int32Array)";
  size_t argc = 7;
  napi_value argv[7];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  AlongArgs a;
  MultiArgs m;
  bool bad = true;
  if (argc < 6) return bad_args(env, usage);
  if (!a.decode(env, argv, 2, 4, "cumulateMulti", usage)) return nullptr;
  if (!m.decode(env, argv[0], &argv[1], &bad)) return m.miscounted ? bad_args(env, "cumulateMulti: one method per store") : bad ? bad_args(env, usage) : nullptr;
  std::vector<olap_store *> outs(m.stores.size(), nullptr);
  int launches = 0;
  int rc = olap_store_cumulate_multi((int)m.stores.size(), m.stores.data(), m.methods, outs.data(), a.ndim(), a.lens_data(), a.axis, a.n_groups, a.map(), &launches);
  return multi_stores(env, rc, argc, argv, 6, launches, outs);
}

// rollingMulti(stores: Store[], methods: Int32Array, lens, axis: number, before: number, after: number, groups: Uint32Array | null, nGroups: number,
//              launchesOut?) -> Store[]
// Rolling-window aggregates along dimension `axis` (olap_store_rolling_multi): the window of item k is [k - before, k + after] within k's group.
static napi_value RollingMulti(napi_env env, napi_callback_info info) {
  const char *usage =
      "rollingMulti(stores: Store[], methods: Int32Array, lens: Uint32Array, axis: number, before: number, after: number, groups: Uint32Array | null, "
      "nGroups: number, launchesOut?: Int32Array)";
  size_t argc = 9;
  napi_value argv[9];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  AlongArgs a;
  MultiArgs m;
  bool bad = true;
  int32_t before = 0, after = 0;
  if (argc < 8 || napi_get_value_int32(env, argv[4], &before) != napi_ok || napi_get_value_int32(env, argv[5], &after) != napi_ok) return bad_args(env, usage);
  if (!a.decode(env, argv, 2, 6, "rollingMulti", usage)) return nullptr;
  if (!m.decode(env, argv[0], &argv[1], &bad)) return m.miscounted ? bad_args(env, "rollingMulti: one method per store") : bad ? bad_args(env, usage) : nullptr;
  std::vector<olap_store *> outs(m.stores.size(), nullptr);
  int launches = 0;
  int rc = olap_store_rolling_multi((int)m.stores.size(), m.stores.data(), m.methods, outs.data(), a.ndim(), a.lens_data(), a.axis, before, after, a.n_groups,
                                    a.map(), &launches);
  return multi_stores(env, rc, argc, argv, 8, launches, outs);
}

// quantileMulti(stores: Store[], lens, axis: number, q: number, groups: Uint32Array | null, nGroups: number, launchesOut?) -> Store[]
// Order statistics along dimension `axis` (olap_store_quantile_multi): new stores of outer * nGroups * inner cells (one group: outer * inner)
// holding the q-quantile of the set cells of each group; groups[k] < nGroups is the group of item k; null: one group.
static napi_value QuantileMulti(napi_env env, napi_callback_info info) {
  const char *usage = "quantileMulti(stores: Store[], lens: Uint32Array, axis: number, q: number, groups: Uint32Array | null, nGroups: number, launchesOut?: Int32Array)";
  size_t argc = 7;
  napi_value argv[7];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  AlongArgs a;
  MultiArgs m;
  bool bad = true;
  double q = 0;
  if (argc < 6 || napi_get_value_double(env, argv[3], &q) != napi_ok) return bad_args(env, usage);
  if (!a.decode(env, argv, 1, 4, "quantileMulti", usage)) return nullptr;
  if (!m.decode(env, argv[0], nullptr, &bad)) return bad ? bad_args(env, usage) : nullptr;
  std::vector<olap_store *> outs(m.stores.size(), nullptr);
  int launches = 0;
  int rc = olap_store_quantile_multi((int)m.stores.size(), m.stores.data(), outs.data(), a.ndim(), a.lens_data(), a.axis, q, a.n_groups, a.map(), &launches);
  return multi_stores(env, rc, argc, argv, 6, launches, outs);
}

// varianceMulti(stores: Store[], lens, axis: number, kind: number, ddof: number, groups: Uint32Array | null, nGroups: number, launchesOut?) -> Store[]
// Dispersion along dimension `axis` (olap_store_variance_multi): new stores of outer * nGroups * inner cells (one group: outer * inner)
// holding the variance (kind 0) or standard deviation (kind 1) of the set cells of each group, divided by n - ddof; groups[k] < nGroups is
// the group of item k; null: one group.
static napi_value VarianceMulti(napi_env env, napi_callback_info info) {
  const char *usage = "varianceMulti(stores: Store[], lens: Uint32Array, axis: number, kind: number, ddof: number, groups: Uint32Array | null, nGroups: number, launchesOut?: Int32Array)";
  size_t argc = 8;
  napi_value argv[8];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  AlongArgs a;
  MultiArgs m;
  bool bad = true;
  int32_t kind = -1, ddof = -1;
  if (argc < 7 || napi_get_value_int32(env, argv[3], &kind) != napi_ok || napi_get_value_int32(env, argv[4], &ddof) != napi_ok) return bad_args(env, usage);
  if (!a.decode(env, argv, 1, 5, "varianceMulti", usage)) return nullptr;
  if (!m.decode(env, argv[0], nullptr, &bad)) return bad ? bad_args(env, usage) : nullptr;
  std::vector<olap_store *> outs(m.stores.size(), nullptr);
  int launches = 0;
  int rc = olap_store_variance_multi((int)m.stores.size(), m.stores.data(), outs.data(), a.ndim(), a.lens_data(), a.axis, kind, ddof, a.n_groups, a.map(), &launches);
  return multi_stores(env, rc, argc, argv, 7, launches, outs);
}

// ---- ShardedStore: a measure split along dimension 0 over the devices of setDevices() -----------
// Wraps olap_sharded_store* (include/olap_hip.h, "Multi-GPU").  Method names and argument shapes are
// those of Store, so the JS HipStore drives either; what a sharded store cannot do in place throws an
// Error whose message starts with "sharded:" and the JS side gathers first.
struct CommRef {
  olap_comm *comm;
  int refs;      // live ShardedStore wrappers + 1 while it is the current communicator
};
static CommRef *g_comm = nullptr;
static napi_ref g_sharded_ctor = nullptr;

static void comm_release(CommRef *c) {
  if (c && --c->refs == 0) {
    olap_comm_destroy(c->comm);
    delete c;
  }
}

struct ShardedBox {
  olap_sharded_store *store;
  CommRef *comm;
  int64_t bytes;
};

static void finalize_sharded(napi_env env, void *data, void *) {
  ShardedBox *box = (ShardedBox *)data;
  if (box->store) {
    account(env, -box->bytes);
    olap_sharded_store_destroy(box->store);
  }
  comm_release(box->comm);
  delete box;
}

static ShardedBox *unwrap_sharded(napi_env env, napi_value v) {
  void *p = nullptr;
  if (napi_unwrap(env, v, &p) != napi_ok || !p || !((ShardedBox *)p)->store) {
    napi_throw_type_error(env, nullptr, "not a ShardedStore");
    return nullptr;
  }
  return (ShardedBox *)p;
}

struct ShardedInit {
  olap_sharded_store *store;
  CommRef *comm;
};

static int64_t sharded_bytes(const olap_sharded_store *s) {
  const olap_store *first = olap_sharded_store_shard(s, 0);
  return (int64_t)(olap_sharded_store_size(s) * olap_dtype_size(first ? olap_store_dtype(first) : OLAP_FLOAT32));
}

static napi_value wrap_new_sharded(napi_env env, olap_sharded_store *s, CommRef *comm) {
  napi_value ctor, obj, ext;
  ShardedInit init{s, comm};
  NAPI_OK(napi_get_reference_value(env, g_sharded_ctor, &ctor));
  NAPI_OK(napi_create_external(env, &init, nullptr, nullptr, &ext));
  if (napi_new_instance(env, ctor, 1, &ext, &obj) != napi_ok) {
    olap_sharded_store_destroy(s);
    return nullptr;
  }
  return obj;
}

// new ShardedStore(lens: Uint32Array, dtypeCode, defaultKind)  |  new ShardedStore(external) [internal]
static napi_value ShardedNew(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3], self;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, &self, nullptr));
  napi_valuetype t;
  NAPI_OK(napi_typeof(env, argv[0], &t));
  olap_sharded_store *s = nullptr;
  CommRef *comm = nullptr;
  bool adopted = false;  // the handle came from wrap_new_sharded(), which destroys it itself when this constructor fails
  if (argc == 1 && t == napi_external) {
    void *p;
    NAPI_OK(napi_get_value_external(env, argv[0], &p));
    s = ((ShardedInit *)p)->store;
    comm = ((ShardedInit *)p)->comm;
    adopted = true;
  } else {
    if (!g_comm) {
      napi_throw_error(env, nullptr, "sharded: no device list; call setDevices([...]) first");
      return nullptr;
    }
    std::vector<uint32_t> lens;
    int32_t dtype = 0, def = 0;
    if (argc < 3 || !get_u32_vec(env, argv[0], lens) || napi_get_value_int32(env, argv[1], &dtype) != napi_ok ||
        napi_get_value_int32(env, argv[2], &def) != napi_ok) {
      napi_throw_type_error(env, nullptr, "new ShardedStore(lens: Uint32Array, dtype: number, default: number)");
      return nullptr;
    }
    comm = g_comm;
    int rc = olap_sharded_store_create(&s, comm->comm, (int)lens.size(), lens.data(), dtype, def, nullptr);
    if (rc) return throw_olap(env, rc);
  }
  ShardedBox *box = new ShardedBox{s, comm, sharded_bytes(s)};
  comm->refs++;
  if (napi_wrap(env, self, box, finalize_sharded, nullptr, nullptr) != napi_ok) {
    if (!adopted) olap_sharded_store_destroy(s);
    comm_release(comm);
    delete box;
    napi_throw_error(env, nullptr, "napi_wrap failed");
    return nullptr;
  }
  account(env, box->bytes);
  return self;
}

#define SHARDED_PROLOGUE(MAXARGS)                                          \
  size_t argc = MAXARGS;                                                   \
  napi_value argv[MAXARGS > 0 ? MAXARGS : 1], self;                        \
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, &self, nullptr));       \
  ShardedBox *box = unwrap_sharded(env, self);                             \
  if (!box) return nullptr;                                                \
  olap_sharded_store *s = box->store;

static napi_value ShardedSize(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(0)
  return num(env, (double)olap_sharded_store_size(s));
}
static napi_value ShardedByteLength(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(0)
  return num(env, (double)box->bytes);
}
static napi_value ShardedDtype(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(0)
  return num(env, olap_store_dtype(olap_sharded_store_shard(s, 0)));
}
static napi_value ShardedDefault(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(0)
  return num(env, olap_store_default(olap_sharded_store_shard(s, 0)));
}
static napi_value ShardedIsSharded(napi_env env, napi_callback_info) {
  napi_value t;
  napi_get_boolean(env, true, &t);
  return t;
}
// rows of dimension 0 owned by each rank: bounds[r] .. bounds[r+1]
static napi_value ShardedBounds(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(0)
  const int world = olap_comm_world(olap_sharded_store_comm(s));
  void *data;
  napi_value ta = make_ta(env, napi_uint32_array, 4, (size_t)world + 1, &data);
  if (!ta) return nullptr;
  memcpy(data, olap_sharded_store_bounds(s), ((size_t)world + 1) * 4);
  return ta;
}

// setData(Float64Array): JS numbers, converted on the devices like a TypedArray store would
static napi_value ShardedSetData(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(1)
  napi_typedarray_type type;
  size_t len;
  void *data;
  bool is_ta = false;
  NAPI_OK(napi_is_typedarray(env, argv[0], &is_ta));
  if (!is_ta || napi_get_typedarray_info(env, argv[0], &type, &len, &data, nullptr, nullptr) != napi_ok || type != napi_float64_array) {
    napi_throw_type_error(env, nullptr, "ShardedStore.setData expects a Float64Array");
    return nullptr;
  }
  int rc = olap_sharded_store_set_data_f64(s, (const double *)data, len);
  if (rc) return throw_olap(env, rc);
  return nullptr;
}
static napi_value ShardedGetDataF64(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(0)
  void *data;
  napi_value ta = make_ta(env, napi_float64_array, 8, olap_sharded_store_size(s), &data);
  if (!ta) return nullptr;
  int rc = olap_sharded_store_get_data_f64(s, (double *)data);
  if (rc) return throw_olap(env, rc);
  return ta;
}
static napi_value ShardedGetStatus(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(0)
  void *data;
  napi_value ta = make_ta(env, napi_int32_array, 4, olap_sharded_store_size(s), &data);
  if (!ta) return nullptr;
  int rc = olap_sharded_store_get_status(s, (int32_t *)data);
  if (rc) return throw_olap(env, rc);
  return ta;
}
static napi_value ShardedGetValue(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(1)
  double idx = 0;
  NAPI_OK(napi_get_value_double(env, argv[0], &idx));
  napi_value undef;
  napi_get_undefined(env, &undef);
  if (!(idx >= 0) || idx != std::floor(idx)) return undef;
  double v = 0;
  int is_set = 0;
  int rc = olap_sharded_store_get_value(s, (uint64_t)idx, &v, &is_set);
  if (rc) return throw_olap(env, rc);
  return is_set ? num(env, v) : undef;
}
static napi_value ShardedSetValues(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(3)
  SetValuesArgs a;
  if (!a.decode(env, argc, argv)) return nullptr;
  int rc = olap_sharded_store_set_values(s, a.idx.size(), a.idx.data(), a.values, a.nulls);
  if (rc) return throw_olap(env, rc);
  return nullptr;
}
static napi_value ShardedSetValue(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(2)
  double idx = 0, v = 0;
  NAPI_OK(napi_get_value_double(env, argv[0], &idx));
  napi_valuetype t = napi_undefined;
  if (argc > 1) NAPI_OK(napi_typeof(env, argv[1], &t));
  int is_null = (t == napi_undefined || t == napi_null);
  if (!is_null) {
    napi_value coerced;
    NAPI_OK(napi_coerce_to_number(env, argv[1], &coerced));
    NAPI_OK(napi_get_value_double(env, coerced, &v));
  }
  int rc = olap_sharded_store_set_value(s, (uint64_t)idx, v, is_null);
  if (rc) return throw_olap(env, rc);
  return nullptr;
}
static napi_value ShardedFill(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(1)
  double v = 0;
  napi_value coerced;
  NAPI_OK(napi_coerce_to_number(env, argv[0], &coerced));
  NAPI_OK(napi_get_value_double(env, coerced, &v));
  int rc = olap_sharded_store_fill(s, v);
  if (rc) return throw_olap(env, rc);
  return nullptr;
}
static napi_value ShardedTotal(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(0)
  double t = 0;
  int rc = olap_sharded_store_total(s, &t);
  if (rc) return throw_olap(env, rc);
  return num(env, t);
}
static napi_value ShardedClone(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(0)
  olap_sharded_store *c = nullptr;
  int rc = olap_sharded_store_clone(s, &c);
  if (rc) return throw_olap(env, rc);
  return wrap_new_sharded(env, c, box->comm);
}
// gather() -> Store: the whole measure on the first device
static napi_value ShardedGather(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(0)
  olap_store *w = nullptr;
  int rc = olap_sharded_store_gather(s, &w);
  if (rc) return throw_olap(env, rc);
  return wrap_new_store(env, w);
}

// drillUp(oldLen, newLen, maps, method) -> ShardedStore (dimension 0 kept) | Store (dimension 0 rolled up: one collective)
static napi_value ShardedDrillUp(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(4)
  if (argc < 1 || !sharded_view(env, s, argv[0])) return nullptr;
  std::vector<uint32_t> new_len;
  std::vector<std::vector<uint32_t>> tables;
  std::vector<const uint32_t *> ptrs;
  int32_t method = 0;
  if (argc < 4 || !decode_lens_tables(env, argv[1], argv[2], (size_t)olap_sharded_store_ndim(s), new_len, tables, ptrs) ||
      napi_get_value_int32(env, argv[3], &method) != napi_ok)
    return bad_args(env, "drillUp(oldLen, newLen, maps, method)");
  olap_sharded_store *os = nullptr;
  olap_store *ow = nullptr;
  int rc = olap_sharded_store_drillup(s, &os, &ow, new_len.data(), ptrs.data(), method);
  if (rc) return throw_olap(env, rc);
  return os ? wrap_new_sharded(env, os, box->comm) : wrap_new_store(env, ow);
}
// dice(oldLen, newLen, sel)
static napi_value ShardedDice(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(3)
  if (argc < 1 || !sharded_view(env, s, argv[0])) return nullptr;
  std::vector<uint32_t> new_len;
  std::vector<std::vector<uint32_t>> tables;
  std::vector<const uint32_t *> ptrs;
  if (argc < 3 || !decode_lens_tables(env, argv[1], argv[2], (size_t)olap_sharded_store_ndim(s), new_len, tables, ptrs))
    return bad_args(env, "dice(oldLen, newLen, sel)");
  olap_sharded_store *os = nullptr;
  int rc = olap_sharded_store_dice(s, &os, new_len.data(), (const int32_t *const *)ptrs.data());
  if (rc) return throw_olap(env, rc);
  return wrap_new_sharded(env, os, box->comm);
}
// drillDown(oldLen, newLen, maps, method, distributions)
static napi_value ShardedDrillDown(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(5)
  if (argc < 1 || !sharded_view(env, s, argv[0])) return nullptr;
  std::vector<uint32_t> new_len;
  std::vector<std::vector<uint32_t>> tables;
  std::vector<const uint32_t *> ptrs;
  int32_t method = 0;
  if (argc < 4 || !decode_lens_tables(env, argv[1], argv[2], (size_t)olap_sharded_store_ndim(s), new_len, tables, ptrs) ||
      napi_get_value_int32(env, argv[3], &method) != napi_ok)
    return bad_args(env, "drillDown(oldLen, newLen, maps, method, distributions)");
  const double *dist = nullptr;
  size_t n_dist = 0;
  if (argc > 4) {
    bool is_ta = false;
    napi_is_typedarray(env, argv[4], &is_ta);
    if (is_ta) {
      napi_typedarray_type type;
      void *data;
      NAPI_OK(napi_get_typedarray_info(env, argv[4], &type, &n_dist, &data, nullptr, nullptr));
      static const double none = 0;
      dist = data ? (const double *)data : &none;
    }
  }
  olap_sharded_store *os = nullptr;
  int rc = olap_sharded_store_drilldown(s, &os, new_len.data(), ptrs.data(), method, dist, n_dist);
  if (rc) return throw_olap(env, rc);
  return wrap_new_sharded(env, os, box->comm);
}
// reorder(oldLen, perm)
static napi_value ShardedReorder(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(2)
  if (argc < 1 || !sharded_view(env, s, argv[0])) return nullptr;
  std::vector<uint32_t> perm;
  if (argc < 2 || !get_u32_vec(env, argv[1], perm) || perm.size() != (size_t)olap_sharded_store_ndim(s))
    return bad_args(env, "reorder(oldLen, perm)");
  olap_sharded_store *os = nullptr;
  int rc = olap_sharded_store_reorder(s, &os, (const int32_t *)perm.data());
  if (rc) return throw_olap(env, rc);
  return wrap_new_sharded(env, os, box->comm);
}

// selectTotal(lens, axis, lists, pathOut?) over the shards ("sharded: ..." when only the whole measure can answer)
static napi_value ShardedSelectTotal(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(4)
  if (argc < 1 || !sharded_view(env, s, argv[0])) return nullptr;
  SelectArgs a;
  if (argc < 3 || !a.decode(env, argv[0], argv[1], argv[2])) return bad_args(env, "selectTotal(lens, axis, lists)");
  double total = 0;
  int path = 1;
  int rc = olap_sharded_store_select_total(s, (int)a.axis.size(), a.axis.data(), a.n_sel.data(), a.ptrs.data(), &total, &path);
  if (rc) return throw_olap(env, rc);
  if (argc > 3) set_path(env, argv[3], path);
  return num(env, total);
}
// copySelect(source: ShardedStore, lens, axis, lists): per shard (both partitioned alike)
static napi_value ShardedCopySelect(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(4)
  ShardedBox *src = argc > 0 ? unwrap_sharded(env, argv[0]) : nullptr;
  if (!src) return nullptr;
  if (argc < 2 || !sharded_view(env, s, argv[1]) || !sharded_view(env, src->store, argv[1])) return nullptr;
  SelectArgs a;
  if (argc < 4 || !a.decode(env, argv[1], argv[2], argv[3])) return bad_args(env, "copySelect(source: ShardedStore, lens, axis, lists)");
  int rc = olap_sharded_store_copy_select(s, src->store, (int)a.axis.size(), a.axis.data(), a.n_sel.data(), a.ptrs.data());
  if (rc) return throw_olap(env, rc);
  return nullptr;
}

// shardStore(store: Store, lens: Uint32Array) -> ShardedStore (olap_sharded_store_scatter)
static napi_value ShardStore(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (!g_comm) {
    napi_throw_error(env, nullptr, "sharded: no device list; call setDevices([...]) first");
    return nullptr;
  }
  std::vector<uint32_t> lens;
  olap_store *whole = argc > 0 ? unwrap(env, argv[0]) : nullptr;
  if (!whole) return nullptr;
  if (argc < 2 || !get_u32_vec(env, argv[1], lens)) return bad_args(env, "shardStore(store, lens: Uint32Array)");
  olap_sharded_store *s = nullptr;
  int rc = olap_sharded_store_scatter(&s, g_comm->comm, whole, (int)lens.size(), lens.data());
  if (rc) return throw_olap(env, rc);
  return wrap_new_sharded(env, s, g_comm);
}

// the ShardedStore[] of evalFormulaSharded / setFormula; false with an exception pending when an element is not one
static bool decode_sharded_stores(napi_env env, napi_value list, uint32_t n, std::vector<const olap_sharded_store *> &stores) {
  stores.resize(n);
  for (uint32_t i = 0; i < n; ++i) {
    napi_value e;
    if (napi_get_element(env, list, i, &e) != napi_ok) return false;
    ShardedBox *box = unwrap_sharded(env, e);
    if (!box) return false;
    stores[i] = box->store;
  }
  return true;
}

// evalFormulaSharded(code, consts, stores: ShardedStore[], scalars) -> Float64Array: per shard, no gather
static napi_value EvalFormulaSharded(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (argc < 4) return bad_args(env, "evalFormulaSharded(code, consts, stores, scalars)");
  ProgramArgs a;
  if (!a.decode_program(env, argv) && !a.no_list)
    return bad_args(env, "evalFormulaSharded(code: Int32Array, consts: Float64Array, stores: ShardedStore[], scalars: Float64Array)");
  if (a.no_list || a.n_inputs == 0) return bad_args(env, "evalFormulaSharded: stores must be a non-empty array of ShardedStore");
  std::vector<const olap_sharded_store *> stores;
  if (!decode_sharded_stores(env, argv[2], a.n_inputs, stores)) return nullptr;
  void *out;
  napi_value ta = make_ta(env, napi_float64_array, 8, olap_sharded_store_size(stores[0]), &out);
  if (!ta) return nullptr;
  int rc = olap_sharded_store_eval_formula(a.code(), (int)a.n_code, a.consts(), (int)a.n_consts, (int)a.n_inputs, stores.data(), a.scalars(), (int)a.n_scalars,
                                           (double *)out);
  if (rc) return throw_olap(env, rc);
  return ta;
}

// sharded.setFormula(code, consts, stores: ShardedStore[], scalars): Store.setFormula per shard; "sharded: ..." when the
// stores are not partitioned like this one
static napi_value ShardedSetFormula(napi_env env, napi_callback_info info) {
  SHARDED_PROLOGUE(4)
  ProgramArgs a;
  if (argc < 4 || !a.decode_program(env, argv))
    return bad_args(env, "setFormula(code: Int32Array, consts: Float64Array, stores: ShardedStore[], scalars: Float64Array)");
  std::vector<const olap_sharded_store *> stores;
  if (!decode_sharded_stores(env, argv[2], a.n_inputs, stores)) return nullptr;
  int rc = olap_sharded_store_set_formula(s, a.code(), (int)a.n_code, a.consts(), (int)a.n_consts, (int)a.n_inputs, stores.data(), a.scalars(), (int)a.n_scalars);
  if (rc) return throw_olap(env, rc);
  return nullptr;
}

// setDevices(devices: number[] | null): the devices new sharded measures are split over
// (olap_comm_init_all: distinct devices talk over RCCL / xGMI; one device repeated exchanges directly)
static napi_value SetDevices(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  bool is_arr = false;
  if (argc) napi_is_array(env, argv[0], &is_arr);
  std::vector<int> devices;
  if (is_arr) {
    uint32_t n = 0;
    napi_get_array_length(env, argv[0], &n);
    for (uint32_t i = 0; i < n; ++i) {
      napi_value e;
      int32_t d = 0;
      NAPI_OK(napi_get_element(env, argv[0], i, &e));
      NAPI_OK(napi_get_value_int32(env, e, &d));
      devices.push_back(d);
    }
  }
  CommRef *next = nullptr;
  if (devices.size() > 1) {
    olap_comm *c = nullptr;
    int rc = olap_comm_init_all(&c, devices.data(), (int)devices.size());
    if (rc) return throw_olap(env, rc);
    next = new CommRef{c, 1};
  }
  comm_release(g_comm);
  g_comm = next;
  return num(env, next ? olap_comm_world(next->comm) : 0);
}
static napi_value ShardWorld(napi_env env, napi_callback_info) { return num(env, g_comm ? olap_comm_world(g_comm->comm) : 0); }
static napi_value ShardTransport(napi_env env, napi_callback_info) {
  napi_value v;
  napi_create_string_utf8(env, g_comm ? olap_comm_transport(g_comm->comm) : "none", NAPI_AUTO_LENGTH, &v);
  return v;
}

// ---- module functions -------------------------------------------------------------------------
static napi_value MethodFromName(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  napi_valuetype t = napi_undefined;
  if (argc) napi_typeof(env, argv[0], &t);
  int code;
  if (t == napi_undefined) {
    code = olap_method_from_name(nullptr);
  } else {
    napi_value str;
    NAPI_OK(napi_coerce_to_string(env, argv[0], &str));
    char buf[128];
    size_t n = 0;
    NAPI_OK(napi_get_value_string_utf8(env, str, buf, sizeof buf, &n));
    code = olap_method_from_name(buf);
  }
  if (code < 0) return throw_olap(env, code);
  return num(env, code);
}

static napi_value DeviceCount(napi_env env, napi_callback_info) { return num(env, olap_device_count()); }
// bytes of device memory currently owned by live Store objects (diagnostics)
static napi_value HeldBytes(napi_env env, napi_callback_info) { return num(env, (double)g_held); }
static napi_value AbiVersion(napi_env env, napi_callback_info) { return num(env, olap_abi_version()); }

static napi_value SetDevice(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  int32_t d = 0;
  NAPI_OK(napi_get_value_int32(env, argv[0], &d));
  int rc = olap_set_device(d);
  if (rc) return throw_olap(env, rc);
  return nullptr;
}

static napi_value Init(napi_env env, napi_value exports) {
  napi_property_descriptor props[] = {
      {"size", nullptr, nullptr, StoreSize, nullptr, nullptr, napi_default, nullptr},
      {"byteLength", nullptr, nullptr, StoreByteLength, nullptr, nullptr, napi_default, nullptr},
      {"dtype", nullptr, nullptr, StoreDtype, nullptr, nullptr, napi_default, nullptr},
      {"defaultKind", nullptr, nullptr, StoreDefault, nullptr, nullptr, napi_default, nullptr},
      {"setData", nullptr, StoreSetData, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"getData", nullptr, StoreGetData, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"getDataF64", nullptr, StoreGetDataF64, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"getStatus", nullptr, StoreGetStatus, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"getKeys", nullptr, StoreGetKeys, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"countSet", nullptr, StoreCountSet, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"getValue", nullptr, StoreGetValue, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"setValue", nullptr, StoreSetValue, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"setValues", nullptr, StoreSetValues, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"fill", nullptr, StoreFill, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"total", nullptr, StoreTotal, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"toSparse", nullptr, StoreToSparse, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"totals", nullptr, StoreTotals, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"trackOrder", nullptr, StoreTrackOrder, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"orderTracked", nullptr, nullptr, StoreOrderTracked, nullptr, nullptr, napi_default, nullptr},
      {"clone", nullptr, StoreClone, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"drillUp", nullptr, StoreDrillUp, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"drillDown", nullptr, StoreDrillDown, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"dice", nullptr, StoreDice, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"diceDrillUp", nullptr, StoreDiceDrillUp, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"reorder", nullptr, StoreReorder, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"load", nullptr, StoreLoad, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"selectTotal", nullptr, StoreSelectTotal, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"copySelect", nullptr, StoreCopySelect, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"copySelectFormula", nullptr, StoreCopySelectFormula, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"setFormula", nullptr, StoreSetFormula, nullptr, nullptr, nullptr, napi_default, nullptr},
  };
  napi_value ctor;
  if (napi_define_class(env, "Store", NAPI_AUTO_LENGTH, StoreNew, nullptr, sizeof(props) / sizeof(props[0]), props, &ctor) != napi_ok) return nullptr;
  napi_create_reference(env, ctor, 1, &g_store_ctor);
  napi_set_named_property(env, exports, "Store", ctor);
  napi_property_descriptor sprops[] = {
      {"size", nullptr, nullptr, ShardedSize, nullptr, nullptr, napi_default, nullptr},
      {"byteLength", nullptr, nullptr, ShardedByteLength, nullptr, nullptr, napi_default, nullptr},
      {"dtype", nullptr, nullptr, ShardedDtype, nullptr, nullptr, napi_default, nullptr},
      {"defaultKind", nullptr, nullptr, ShardedDefault, nullptr, nullptr, napi_default, nullptr},
      {"isSharded", nullptr, nullptr, ShardedIsSharded, nullptr, nullptr, napi_default, nullptr},
      {"bounds", nullptr, nullptr, ShardedBounds, nullptr, nullptr, napi_default, nullptr},
      {"setData", nullptr, ShardedSetData, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"getDataF64", nullptr, ShardedGetDataF64, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"getStatus", nullptr, ShardedGetStatus, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"getValue", nullptr, ShardedGetValue, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"setValue", nullptr, ShardedSetValue, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"setValues", nullptr, ShardedSetValues, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"setFormula", nullptr, ShardedSetFormula, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"fill", nullptr, ShardedFill, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"total", nullptr, ShardedTotal, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"clone", nullptr, ShardedClone, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"gather", nullptr, ShardedGather, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"drillUp", nullptr, ShardedDrillUp, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"drillDown", nullptr, ShardedDrillDown, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"dice", nullptr, ShardedDice, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"reorder", nullptr, ShardedReorder, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"selectTotal", nullptr, ShardedSelectTotal, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"copySelect", nullptr, ShardedCopySelect, nullptr, nullptr, nullptr, napi_default, nullptr},
  };
  napi_value sctor;
  if (napi_define_class(env, "ShardedStore", NAPI_AUTO_LENGTH, ShardedNew, nullptr, sizeof(sprops) / sizeof(sprops[0]), sprops, &sctor) != napi_ok) return nullptr;
  napi_create_reference(env, sctor, 1, &g_sharded_ctor);
  napi_set_named_property(env, exports, "ShardedStore", sctor);
  napi_property_descriptor fns[] = {
      {"setDevices", nullptr, SetDevices, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"shardWorld", nullptr, ShardWorld, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"shardTransport", nullptr, ShardTransport, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"shardStore", nullptr, ShardStore, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"evalFormulaSharded", nullptr, EvalFormulaSharded, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"evalFormula", nullptr, EvalFormula, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"selectTotalFormula", nullptr, SelectTotalFormula, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"totalsFormula", nullptr, TotalsFormula, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"totalsReport", nullptr, TotalsReport, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"drillUpMulti", nullptr, DrillUpMulti, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"diceMulti", nullptr, DiceMulti, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"reorderMulti", nullptr, ReorderMulti, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"loadMulti", nullptr, LoadMulti, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"composeMulti", nullptr, ComposeMulti, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"blocksReport", nullptr, BlocksReport, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"diceDrillUpMulti", nullptr, DiceDrillUpMulti, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"drillDownMulti", nullptr, DrillDownMulti, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"cumulateMulti", nullptr, CumulateMulti, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"quantileMulti", nullptr, QuantileMulti, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"varianceMulti", nullptr, VarianceMulti, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"rollingMulti", nullptr, RollingMulti, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"storeFromSparse", nullptr, StoreFromSparse, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"methodFromName", nullptr, MethodFromName, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"heldBytes", nullptr, HeldBytes, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"deviceCount", nullptr, DeviceCount, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"abiVersion", nullptr, AbiVersion, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"setDevice", nullptr, SetDevice, nullptr, nullptr, nullptr, napi_default, nullptr},
  };
  napi_define_properties(env, exports, sizeof(fns) / sizeof(fns[0]), fns);
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
