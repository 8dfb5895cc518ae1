// olap_select.hip — Cube.getTotalForDimensionItems / getDistribution / copyMeasureData on the device.
//
// The reference (the reference's src/cube.js:679-707, :665-673, :859-888, :19-32) enumerates the cartesian
// product of a filter (getCombinations) and calls getValue / setValue (src/store/in-memory.js:118-133) once per
// combination.  A selection is given here as LEVELS in nesting order (the first level outermost): level l is a
// cube dimension axis[l] with an index list sel[l] (repeats allowed; -1 = a cell that does not exist, read as the
// default: what a pending dice composes into), or a free filter key (axis -1) that only multiplies the count.
//
//   select_total   float64 sum, in nesting order, of getValue over the combinations: one reduction that streams
//                  the contiguous trailing runs with 16-byte loads and gathers the rest, with an exactness
//                  certificate; when the certificate fails, the values are gathered in nesting order and added
//                  on the host left to right (the reference's order, always).
//   copy_select    target.setValue(pos, source.getValue(pos)) for every combination, as one scatter.
//   set_values     a list of setValue calls (Cube.hydrateFromSparseNestedObject), duplicates allowed: the entries
//                  are sorted by cell, each cell's run is reduced to its last write and its place in the key order,
//                  and the distinct cells are written by the same per-cell code as copy_select.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cmath>
#include <cstring>
#include <vector>

#include "olap_device.hpp"
#include "olap_internal.hpp"
#include "olap_kernels.hpp"

using namespace olap;

namespace {

constexpr int kSelMaxLevels = 64;    // cube dimensions (OLAP_MAX_DIMS) + free filter keys
constexpr int kSelInline = 512;      // index entries that travel in the kernel arguments (no upload)
constexpr unsigned kSelBlocks = 2048;
constexpr uint32_t kFlagNaN = 1, kFlagPosInf = 2, kFlagNegInf = 4;

// Exactness certificate of a set of float64 terms (see select_total_kernel).
struct Cert {
  double sum;       // the finite terms, added in whatever order the reduction ran
  double abs_sum;   // A: sum of |x| over the finite terms
  int32_t min_exp;  // E: every non-zero finite term is an integer multiple of 2^E (INT_MAX: no such term)
  uint32_t flags;   // kFlagNaN | kFlagPosInf | kFlagNegInf
};

__device__ __forceinline__ int32_t low_bit_exponent(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  const int be = (int)((b >> 52) & 0x7ff);
  const unsigned long long man = b & ((1ull << 52) - 1);
  if (be == 0) return -1074 + __builtin_ctzll(man);  // subnormal (x != 0: man != 0)
  return be - 1075 + __builtin_ctzll(man | (1ull << 52));
}

__device__ __forceinline__ void cert_add(Cert &c, double x) {
  if (x != x) {
    c.flags |= kFlagNaN;
  } else if (__builtin_isinf(x)) {
    c.flags |= x > 0 ? kFlagPosInf : kFlagNegInf;
  } else if (x != 0.0) {
    c.sum += x;
    c.abs_sum += fabs(x);
    c.min_exp = min(c.min_exp, low_bit_exponent(x));
  }
}

__device__ __forceinline__ void cert_merge(Cert &a, const Cert &b) {
  a.sum += b.sum;
  a.abs_sum += b.abs_sum;
  a.min_exp = min(a.min_exp, b.min_exp);
  a.flags |= b.flags;
}

// getValue (in-memory.js:118-120) as a JS number: the cell, or the default when it is unset
template <typename T>
__device__ __forceinline__ double read_cell(const T *values, const int32_t *status, uint64_t i, bool def_nan) {
  const T v = values[i];
  return cell_is_set<T>(v, status ? status[i] : OLAP_STATUS_SET, status != nullptr, def_nan) ? Cell<T>::to_f64(v)
                                                                                               : (def_nan ? __builtin_nan("") : 0.0);
}

// Where a selection's values come from.  at(i): getValue of cell i as a JS number; missing(): the value of a cell that
// does not exist (a -1 entry); missing_row(c, n): cert_add of n such values by the workgroup (one lane or all).
template <typename T>
struct StoreSource {  // one stored measure
  const T *__restrict__ values;
  const int32_t *__restrict__ status;
  int def_nan_i;
  __device__ __forceinline__ double at(uint64_t i) const { return read_cell<T>(values, status, i, def_nan_i != 0); }
  __device__ __forceinline__ double missing() const { return def_nan_i != 0 ? __builtin_nan("") : 0.0; }
  __device__ __forceinline__ void missing_row(Cert &c, uint64_t) const {
    if (def_nan_i != 0 && threadIdx.x == 0) c.flags |= kFlagNaN;  // (the default 0 adds nothing)
  }
};

template <typename T>
StoreSource<T> store_source(const olap_store *s) {
  return StoreSource<T>{(const T *)s->values, mask_needed(s), s->default_kind == OLAP_DEFAULT_NAN};
}

struct FormulaSource {  // a computed measure: the program (in device memory) evaluated in registers at each cell
  const FormulaProgram *__restrict__ prog;
  __device__ __forceinline__ double at(uint64_t i) const { return formula_at<OLAP_FORMULA_MAX_STACK>(*prog, i); }
  __device__ __forceinline__ double missing() const { return formula_at_missing<OLAP_FORMULA_MAX_STACK>(*prog); }
  __device__ __forceinline__ void missing_row(Cert &c, uint64_t n) const {
    const double x = missing();
    for (uint64_t i = threadIdx.x; i < n; i += kBlock) cert_add(c, x);
  }
};

// The gathered part of a selection: `ngl` levels (cube order, outermost first) in front of a contiguous run of `run`
// cells that the trailing identity levels fold into.  Row g of the rows x run view starts at the cell
// sum_l idx[off[l] + digit_l(g)] * stride[l], or does not exist when one of those entries is -1.
struct GatherPlan {
  uint64_t rows, run;
  uint64_t chunk, chunks;  // ROW mode: a work unit is `chunk` cells of one row
  int ngl;
  int flat;                // FLAT mode (short runs): one lane per cell of the rows x run view
  uint32_t len[OLAP_MAX_DIMS];
  uint32_t off[OLAP_MAX_DIMS];
  uint64_t stride[OLAP_MAX_DIMS];
  const int32_t *idx;      // device copy of the lists, or nullptr: they are in `inl`
  int32_t inl[kSelInline];
};

__device__ __forceinline__ int64_t row_base(const GatherPlan &p, uint64_t g) {
  int64_t base = 0;
  bool ok = true;
  for (int l = p.ngl - 1; l >= 0; --l) {
    const uint64_t d = g % p.len[l];
    g /= p.len[l];
    const int32_t e = p.idx ? p.idx[p.off[l] + d] : p.inl[p.off[l] + d];
    if (e < 0) ok = false;
    else base += (int64_t)e * (int64_t)p.stride[l];
  }
  return ok ? base : -1;
}

// Every workgroup reduces its share of the selection into one Cert slot.
//
// Why the result can be exact whatever the order of the additions.  Let the selection hold the finite terms x_i
// (each taken m times: the free filter keys repeat the whole product), A = sum |x_i| and E the exponent of the lowest
// set mantissa bit over the non-zero x_i, so that every x_i is an integer multiple of 2^E.  When no NaN is present, A*m
// is finite and A*m <= 2^(52+E), every partial sum of the m-fold term list, in ANY order, is a multiple of 2^E of
// magnitude at most A*m < 2^(53+E) (the one bit of margin covers the rounding of the computed A itself: if the true A
// exceeded 2^(53+E) the computed one, a monotone rounding of increasing partial sums, would too), hence exactly
// representable: every addition is exact, the device's sum S of one copy of the terms equals the sequential one, and
// m*S is exact as well.  Non-finite terms: a NaN gives NaN in any order; +inf with -inf gives NaN in any order (once
// both have been added nothing finite can bring the sum back); a single-signed inf gives that inf, because under the
// condition the finite partial sums never overflow.  Otherwise (the condition fails) the host re-adds the values in
// nesting order (select_gather_kernel).
//
// VEC (a StoreSource<T> only): whole 16-byte groups of a row are read with one load each.
template <typename Src, typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void select_total_kernel(const Src src, GatherPlan p, Cert *__restrict__ partial) {
  Cert c{0.0, 0.0, INT_MAX, 0u};
  if (p.flat) {
    const uint64_t cells = p.rows * p.run;
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < cells; t += (uint64_t)gridDim.x * kBlock) {
      const uint64_t g = t / p.run, r = t - g * p.run;
      const int64_t base = row_base(p, g);
      cert_add(c, base < 0 ? src.missing() : src.at((uint64_t)base + r));
    }
  } else {
    const uint64_t units = p.rows * p.chunks;
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
      const uint64_t g = u / p.chunks, k = u - g * p.chunks;
      const int64_t base = row_base(p, g);
      const uint64_t lo = k * p.chunk, hi = lo + p.chunk < p.run ? lo + p.chunk : p.run;
      if (base < 0) {  // a row that does not exist: every cell reads the default
        src.missing_row(c, hi - lo);
        continue;
      }
      const uint64_t first = (uint64_t)base + lo, n = hi - lo;
      uint64_t done = 0;
      if constexpr (VEC) {
        constexpr int V = 16 / sizeof(T);
        const T *values = src.values;
        const int32_t *status = src.status;
        const bool def_nan = src.def_nan_i != 0;
        if ((first % V) == 0) {
          const uint64_t groups = n / V;
          for (uint64_t q = threadIdx.x; q < groups; q += kBlock) {
            const Vec<T, V> x = load_stream<T, V>(values + first + q * V);
            Vec<int32_t, V> sx;
            if (status) sx = load_stream<int32_t, V>(status + first + q * V);
#pragma unroll
            for (int e = 0; e < V; ++e) {
              const bool set = cell_is_set<T>(x.v[e], status ? sx.v[e] : OLAP_STATUS_SET, status != nullptr, def_nan);
              cert_add(c, set ? Cell<T>::to_f64(x.v[e]) : (def_nan ? __builtin_nan("") : 0.0));
            }
          }
          done = groups * V;
        }
      }
      for (uint64_t i = done + threadIdx.x; i < n; i += kBlock) cert_add(c, src.at(first + i));
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Cert o;
    o.sum = __shfl_down(c.sum, off, 64);
    o.abs_sum = __shfl_down(c.abs_sum, off, 64);
    o.min_exp = __shfl_down(c.min_exp, off, 64);
    o.flags = (uint32_t)__shfl_down((int)c.flags, off, 64);
    cert_merge(c, o);
  }
  __shared__ Cert s_c[kBlock / 64];
  if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    Cert a = s_c[0];
    for (int w = 1; w < kBlock / 64; ++w) cert_merge(a, s_c[w]);
    partial[blockIdx.x] = a;
  }
}

// folds the workgroup slots in a fixed order (one workgroup) and hands the result to the host
__global__ __launch_bounds__(kBlock) void select_finish_kernel(const Cert *__restrict__ partial, uint32_t n, Cert *out) {
  Cert c{0.0, 0.0, INT_MAX, 0u};
  for (uint32_t i = threadIdx.x; i < n; i += kBlock) cert_merge(c, partial[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Cert o;
    o.sum = __shfl_down(c.sum, off, 64);
    o.abs_sum = __shfl_down(c.abs_sum, off, 64);
    o.min_exp = __shfl_down(c.min_exp, off, 64);
    o.flags = (uint32_t)__shfl_down((int)c.flags, off, 64);
    cert_merge(c, o);
  }
  __shared__ Cert s_c[kBlock / 64];
  if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    Cert a = s_c[0];
    for (int w = 1; w < kBlock / 64; ++w) cert_merge(a, s_c[w]);
    *out = a;
  }
}

// Levels in nesting order (free levels included, stride 0 and no list), for the sequential fallback and the copy.
struct NestPlan {
  int nlev;
  uint32_t len[kSelMaxLevels];
  uint32_t off[kSelMaxLevels];
  uint64_t stride[kSelMaxLevels];
  uint32_t is_free[kSelMaxLevels];
  const int32_t *idx;
  int32_t inl[kSelInline / 2];
};

__device__ __forceinline__ int64_t nest_cell(const NestPlan &p, uint64_t rank) {
  int64_t cell = 0;
  bool ok = true;
  for (int l = p.nlev - 1; l >= 0; --l) {
    const uint64_t d = rank % p.len[l];
    rank /= p.len[l];
    if (p.is_free[l]) continue;
    const int32_t e = p.idx ? p.idx[p.off[l] + d] : p.inl[p.off[l] + d];
    if (e < 0) ok = false;
    else cell += (int64_t)e * (int64_t)p.stride[l];
  }
  return ok ? cell : -1;
}

// the value of every combination of ranks [first, first + n) in nesting order, as a JS number
template <typename Src>
__global__ __launch_bounds__(kBlock) void select_gather_kernel(const Src src, NestPlan p, uint64_t first, uint64_t n, double *__restrict__ out) {
  for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < n; t += (uint64_t)gridDim.x * kBlock) {
    const int64_t cell = nest_cell(p, first + t);
    out[t] = cell < 0 ? src.missing() : src.at((uint64_t)cell);
  }
}

// The last setValue (in-memory.js:122-133) a batch makes to one distinct cell: x, or an unset when !has.  Same
// conversion and delete-on-default as set_cell_kernel.  A tracked store (seq != nullptr) drops a cell that ends unset,
// leaves one that was set and keeps_place where it was, and appends any other set cell at `appended` (Map.set,
// in-memory.js:132).
template <typename T>
__device__ __forceinline__ void write_cell(T *dst, int32_t *dst_status, uint32_t *dst_seq, bool dst_nan, uint64_t cell, double x, bool has,
                                           bool keeps_place, uint32_t appended) {
  T ov;
  int32_t os;
  emit_cell<T>(x, has, dst_nan, ov, os);
  dst[cell] = ov;
  if (dst_status) dst_status[cell] = os;
  if (dst_seq) {
    const uint32_t old = dst_seq[cell];
    dst_seq[cell] = os ? (old && keeps_place ? old : appended) : 0u;
  }
}

// target.setValue(pos, source.getValue(pos)) (src/cube.js:859-888) for every combination; the levels are free of
// repeats, so every lane owns a distinct cell.  A tracked target appends a newly set cell at seq_base + its rank in
// nesting order.  The target may be one of a formula's inputs: each lane reads its own cell before it writes it.
template <typename Src, typename T>
__global__ __launch_bounds__(kBlock) void copy_select_kernel(const Src src, T *dst, int32_t *dst_status, uint32_t *dst_seq, uint32_t seq_base,
                                                             int dst_nan_i, NestPlan p, uint64_t n) {
  const bool dst_nan = dst_nan_i != 0;
  for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < n; t += (uint64_t)gridDim.x * kBlock) {
    const uint64_t cell = (uint64_t)nest_cell(p, t);
    const double x = src.at(cell);
    write_cell<T>(dst, dst_status, dst_seq, dst_nan, cell, x, !is_default_f64(x, dst_nan), true, seq_base + (uint32_t)t);
  }
}

// ---- set_values: n setValue calls as one scatter.  The entries are sorted by cell (stably: list order within a cell)
// into slots; a slot's entry "unsets" when setValue would leave its cell unset (null, the default, or a value whose
// conversion is the default).  run[j] = the first slot of j's cell after the last unsetting slot before j (or the
// cell's first slot): a max-scan of these markers.  The last slot of a cell decides its value; a cell that ends set
// and has no unsetting slot keeps its place, any other one is appended at the list position of slot run[last].

template <typename T>
__device__ __forceinline__ bool entry_unsets(double x, bool null, bool def_nan) {
  T ov;
  int32_t os;
  emit_cell<T>(x, !null && !is_default_f64(x, def_nan), def_nan, ov, os);
  return os == 0;
}

__global__ __launch_bounds__(kBlock) void iota_u32_kernel(uint32_t *out, uint64_t n) {
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBlock) out[j] = (uint32_t)j;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void set_values_mark_kernel(const uint64_t *__restrict__ cell, const uint32_t *__restrict__ pos,
                                                                 const double *__restrict__ values, const uint8_t *__restrict__ is_null, int def_nan_i,
                                                                 uint64_t n, uint32_t *__restrict__ marker) {
  const bool def_nan = def_nan_i != 0;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBlock) {
    bool starts = j == 0 || cell[j - 1] != cell[j];
    if (!starts) {
      const uint32_t q = pos[j - 1];
      starts = entry_unsets<T>(values[q], is_null && is_null[q], def_nan);
    }
    marker[j] = starts ? (uint32_t)j : 0u;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void set_values_write_kernel(const uint64_t *__restrict__ cell, const uint32_t *__restrict__ pos,
                                                                  const double *__restrict__ values, const uint8_t *__restrict__ is_null,
                                                                  const uint32_t *__restrict__ run, uint64_t n, T *dst, int32_t *dst_status,
                                                                  uint32_t *dst_seq, uint32_t seq_base, int dst_nan_i) {
  const bool dst_nan = dst_nan_i != 0;
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBlock) {
    if (j + 1 < n && cell[j + 1] == cell[j]) continue;  // not the cell's last slot
    const uint32_t q = pos[j], r = run[j];
    const double x = values[q];
    const bool has = !(is_null && is_null[q]) && !is_default_f64(x, dst_nan);
    const bool keeps_place = r == 0 || cell[r - 1] != cell[r];
    write_cell<T>(dst, dst_status, dst_seq, dst_nan, cell[j], x, has, keeps_place, seq_base + pos[r]);
  }
}

unsigned select_grid(uint64_t n) {
  const uint64_t want = (n + kBlock - 1) / kBlock;
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, kSelBlocks));
}

// index lists either inline (small) or uploaded; `dev` is freed by the caller
template <typename P>
int place_lists(P &p, int cap, const std::vector<int32_t> &all, int32_t **dev) {
  *dev = nullptr;
  p.idx = nullptr;
  if ((int)all.size() <= cap) {
    if (!all.empty()) memcpy(p.inl, all.data(), all.size() * sizeof(int32_t));
    return OLAP_OK;
  }
  HIP_TRY(dev_alloc((void **)dev, all.size() * sizeof(int32_t)));
  hipError_t e = hipMemcpy(*dev, all.data(), all.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    dev_free(*dev);
    *dev = nullptr;
    return hip_fail(e, "select lists");
  }
  p.idx = *dev;
  return OLAP_OK;
}

uint64_t product_of(const std::vector<uint32_t> &v) {
  uint64_t n = 1;
  for (uint32_t x : v) n *= x;
  return n;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------- host side

int select_validate(const olap_store *store, int ndim, const uint32_t *lens, int nlev, const int *axis, const uint32_t *n_sel,
                    const int32_t *const *sel, bool for_copy) {
  if (!store) return fail(OLAP_ERR_INVALID_ARGUMENT, "store is NULL");
  if (ndim < 1 || ndim > OLAP_MAX_DIMS || !lens) return fail(OLAP_ERR_INVALID_ARGUMENT, "a selection needs 1..%d dimensions", OLAP_MAX_DIMS);
  uint64_t size = 1;
  for (int d = 0; d < ndim; ++d) size *= lens[d];
  if (size != store->size) return fail(OLAP_ERR_LENGTH_MISMATCH, "dimension lengths give %llu cells, the store has %llu", (unsigned long long)size,
                                       (unsigned long long)store->size);
  if (nlev < ndim || nlev > kSelMaxLevels) return fail(OLAP_ERR_INVALID_ARGUMENT, "a selection has %d..%d levels, got %d", ndim, kSelMaxLevels, nlev);
  if (!axis || !n_sel || !sel) return fail(OLAP_ERR_INVALID_ARGUMENT, "axis/n_sel/sel is NULL");
  int seen[OLAP_MAX_DIMS] = {0};
  for (int l = 0; l < nlev; ++l) {
    const int d = axis[l];
    if (d < -1 || d >= ndim) return fail(OLAP_ERR_INVALID_ARGUMENT, "level %d names dimension %d of %d", l, d, ndim);
    if (d < 0) continue;
    if (seen[d]++) return fail(OLAP_ERR_INVALID_ARGUMENT, "dimension %d has two levels", d);
    if (n_sel[l] && !sel[l]) return fail(OLAP_ERR_INVALID_ARGUMENT, "sel[%d] is NULL", l);
    for (uint32_t j = 0; j < n_sel[l]; ++j) {
      const int32_t e = sel[l][j];
      if (e >= (int64_t)lens[d] || e < -1 || (for_copy && e < 0))
        return fail(OLAP_ERR_INDEX_RANGE, "selection entry %d of level %d is outside dimension %d", e, l, d);
    }
  }
  for (int d = 0; d < ndim; ++d)
    if (!seen[d]) return fail(OLAP_ERR_INVALID_ARGUMENT, "dimension %d has no level", d);
  return OLAP_OK;
}

// The order-free part of select_total: lists per cube dimension (cube order, repeats and -1 allowed).  Free levels are
// not seen here.  `launch(p, blocks, partial)` starts select_total_kernel for the value source; the certificate of one
// copy of the terms comes back.  Runs on the current device.
template <typename Launch>
static int cert_of(int ndim, const uint32_t *lens, const uint32_t *n_by_dim, const int32_t *const *sel_by_dim, Launch launch, double *sum,
                   double *abs_sum, int *min_exp, unsigned *flags) {
  *sum = 0.0;
  *abs_sum = 0.0;
  *min_exp = INT_MAX;
  *flags = 0;
  for (int d = 0; d < ndim; ++d)
    if (!n_by_dim[d]) return OLAP_OK;
  int rc = require_device();
  if (rc) return rc;
  // trailing dimensions selected whole and in order fold into one contiguous run
  int t = ndim;
  uint64_t run = 1;
  while (t > 0) {
    const int d = t - 1;
    bool ident = n_by_dim[d] == lens[d];
    for (uint32_t j = 0; ident && j < n_by_dim[d]; ++j) ident = sel_by_dim[d][j] == (int32_t)j;
    if (!ident) break;
    run *= lens[d];
    --t;
  }
  static thread_local GatherPlan p;  // (3 KB: off the host stack)
  memset(&p, 0, offsetof(GatherPlan, inl));
  p.ngl = t;
  p.run = run;
  p.rows = 1;
  std::vector<int32_t> all;
  uint64_t stride = run;
  for (int d = t - 1; d >= 0; --d) {
    p.len[d] = n_by_dim[d];
    p.stride[d] = stride;
    stride *= lens[d];
    p.rows *= n_by_dim[d];
  }
  for (int d = 0; d < t; ++d) {
    p.off[d] = (uint32_t)all.size();
    all.insert(all.end(), sel_by_dim[d], sel_by_dim[d] + n_by_dim[d]);
  }
  const uint64_t cells = p.rows * run;
  unsigned blocks;
  if (run < 1024) {
    p.flat = 1;
    blocks = select_grid(cells);
  } else {
    p.flat = 0;
    // about kSelBlocks units, each a contiguous piece of one row of at least 1024 cells (a multiple of 16 cells)
    const uint64_t want = std::max<uint64_t>(1, std::min<uint64_t>((kSelBlocks + p.rows - 1) / p.rows, run / 1024));
    p.chunk = ((run + want - 1) / want + 15) / 16 * 16;
    p.chunks = (run + p.chunk - 1) / p.chunk;
    blocks = (unsigned)std::min<uint64_t>(p.rows * p.chunks, kSelBlocks);
  }
  int32_t *dev_lists = nullptr;
  if ((rc = place_lists(p, kSelInline, all, &dev_lists))) return rc;
  static thread_local Cert *pinned = nullptr;
  static thread_local bool pinned_tried = false;
  if (!pinned_tried) {
    pinned_tried = true;
    void *q = nullptr;
    if (hipHostMalloc(&q, sizeof(Cert), hipHostMallocPortable | hipHostMallocMapped) == hipSuccess) pinned = (Cert *)q;
    else (void)hipGetLastError();
  }
  Cert *partial = nullptr;
  hipError_t e = dev_alloc((void **)&partial, (blocks + 1) * sizeof(Cert));
  if (e == hipSuccess) {
    launch(p, blocks, partial);
    e = hipGetLastError();
    if (e == hipSuccess) {
      hipLaunchKernelGGL(select_finish_kernel, 1, kBlock, 0, nullptr, partial, blocks, pinned ? pinned : partial + blocks);
      e = hipGetLastError();
    }
    Cert c{};
    if (e == hipSuccess) {
      if (pinned) {
        e = hipStreamSynchronize(nullptr);
        c = *pinned;
      } else {
        e = hipMemcpy(&c, partial + blocks, sizeof(Cert), hipMemcpyDeviceToHost);
      }
    }
    dev_free(partial);
    *sum = c.sum;
    *abs_sum = c.abs_sum;
    *min_exp = c.min_exp;
    *flags = c.flags;
  }
  if (dev_lists) dev_free(dev_lists);
  if (e != hipSuccess) return hip_fail(e, "select_total");
  return OLAP_OK;
}

// select_total's order-free part over ONE store
int select_cert(const olap_store *s, int ndim, const uint32_t *lens, const uint32_t *n_by_dim, const int32_t *const *sel_by_dim, double *sum,
                double *abs_sum, int *min_exp, unsigned *flags) {
  OnStoreDevice on_device__(s);
  const bool vec = (((uintptr_t)s->values | (uintptr_t)mask_needed(s)) & 15u) == 0;
  auto launch = [&](const GatherPlan &p, unsigned blocks, Cert *partial) {
    DISPATCH_DTYPE(s->dtype, T, {
      if (vec) hipLaunchKernelGGL((select_total_kernel<StoreSource<T>, T, true>), blocks, kBlock, 0, nullptr, store_source<T>(s), p, partial);
      else hipLaunchKernelGGL((select_total_kernel<StoreSource<T>, T, false>), blocks, kBlock, 0, nullptr, store_source<T>(s), p, partial);
    });
  };
  return cert_of(ndim, lens, n_by_dim, sel_by_dim, launch, sum, abs_sum, min_exp, flags);
}

// Applies the certificate.  Returns 1 and sets *total when the order-free result is the sequential one; 0 otherwise.
int select_certified_total(double sum, double abs_sum, int min_exp, unsigned flags, double m, double *total) {
  if ((flags & kFlagNaN) || ((flags & kFlagPosInf) && (flags & kFlagNegInf))) {
    *total = NAN;
    return 1;
  }
  if (min_exp == INT_MAX) {  // no non-zero finite term
    *total = (flags & kFlagPosInf) ? INFINITY : (flags & kFlagNegInf) ? -INFINITY : 0.0;
    return 1;
  }
  const double am = abs_sum * m;
  if (!std::isfinite(am)) return 0;
  if (min_exp + 52 <= 1023 && am > std::ldexp(1.0, min_exp + 52)) return 0;  // (above: every finite A*m is below the bound)
  *total = (flags & kFlagPosInf) ? INFINITY : (flags & kFlagNegInf) ? -INFINITY : sum * m + 0.0;  // (+0.0: never -0)
  return 1;
}

// lists of the selection in cube order (the dimension levels); m = product of the free levels' lengths
static void by_dimension(int ndim, int nlev, const int *axis, const uint32_t *n_sel, const int32_t *const *sel, std::vector<uint32_t> &n_by_dim,
                         std::vector<const int32_t *> &sel_by_dim, double *m, bool *empty) {
  n_by_dim.assign(ndim, 0);
  sel_by_dim.assign(ndim, nullptr);
  *m = 1.0;
  *empty = false;
  for (int l = 0; l < nlev; ++l) {
    if (!n_sel[l]) *empty = true;
    if (axis[l] < 0) {
      *m *= (double)n_sel[l];
    } else {
      n_by_dim[axis[l]] = n_sel[l];
      sel_by_dim[axis[l]] = sel[l];
    }
  }
}

// The reference's order, always: every combination's value in nesting order, added left to right from +0.
// `launch(p, first, k, out)` starts select_gather_kernel for the value source.  Runs on the current device.
template <typename Launch>
static int sequential_of(const uint32_t *lens, int ndim, int nlev, const int *axis, const uint32_t *n_sel, const int32_t *const *sel, Launch launch,
                         double *total) {
  static thread_local NestPlan p;
  memset(&p, 0, offsetof(NestPlan, inl));
  std::vector<uint64_t> stride(ndim);
  uint64_t st = 1;
  for (int d = ndim - 1; d >= 0; --d) {
    stride[d] = st;
    st *= lens[d];
  }
  std::vector<int32_t> all;
  uint64_t n = 1;
  p.nlev = nlev;
  for (int l = 0; l < nlev; ++l) {
    p.len[l] = n_sel[l];
    n *= n_sel[l];
    p.is_free[l] = axis[l] < 0;
    p.stride[l] = axis[l] < 0 ? 0 : stride[axis[l]];
    p.off[l] = (uint32_t)all.size();
    if (axis[l] >= 0) all.insert(all.end(), sel[l], sel[l] + n_sel[l]);
  }
  int32_t *dev_lists = nullptr;
  int rc = place_lists(p, kSelInline / 2, all, &dev_lists);
  if (rc) return rc;
  const uint64_t chunk = std::min<uint64_t>(n, 1ull << 23);  // 64 MB of float64 per round trip
  double *dev = nullptr;
  std::vector<double> host(chunk ? chunk : 1);
  hipError_t e = dev_alloc((void **)&dev, (chunk ? chunk : 1) * sizeof(double));
  double acc = 0.0;
  for (uint64_t first = 0; e == hipSuccess && first < n; first += chunk) {
    const uint64_t k = std::min(chunk, n - first);
    launch(p, first, k, dev);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(host.data(), dev, k * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess)
      for (uint64_t i = 0; i < k; ++i) acc += host[i];  // src/cube.js:705: `total += this.getSingleData(...)`
  }
  if (dev) dev_free(dev);
  if (dev_lists) dev_free(dev_lists);
  if (e != hipSuccess) return hip_fail(e, "select_total (sequential)");
  *total = acc;
  return OLAP_OK;
}

static int select_sequential(const olap_store *s, const uint32_t *lens, int ndim, int nlev, const int *axis, const uint32_t *n_sel,
                             const int32_t *const *sel, double *total) {
  OnStoreDevice on_device__(s);
  auto launch = [&](const NestPlan &p, uint64_t first, uint64_t k, double *out) {
    DISPATCH_DTYPE(s->dtype, T,
                 hipLaunchKernelGGL((select_gather_kernel<StoreSource<T>>), select_grid(k), kBlock, 0, nullptr, store_source<T>(s), p, first, k, out));
  };
  return sequential_of(lens, ndim, nlev, axis, n_sel, sel, launch, total);
}

extern "C" int olap_store_select_total(const olap_store *s, int ndim, const uint32_t *lens, int nlev, const int *axis, const uint32_t *n_sel,
                                       const int32_t *const *sel, double *total, int *exact_path) {
  int rc = select_validate(s, ndim, lens, nlev, axis, n_sel, sel, false);
  if (rc) return rc;
  if (!total) return fail(OLAP_ERR_INVALID_ARGUMENT, "total is NULL");
  std::vector<uint32_t> nd;
  std::vector<const int32_t *> sd;
  double m;
  bool empty;
  by_dimension(ndim, nlev, axis, n_sel, sel, nd, sd, &m, &empty);
  if (exact_path) *exact_path = 1;
  if (empty) {  // no combination: the reduce starts and ends at 0 (src/cube.js:704)
    *total = 0.0;
    return OLAP_OK;
  }
  double sum, abs_sum;
  int min_exp;
  unsigned flags;
  if ((rc = select_cert(s, ndim, lens, nd.data(), sd.data(), &sum, &abs_sum, &min_exp, &flags))) return rc;
  if (select_certified_total(sum, abs_sum, min_exp, flags, m, total)) return OLAP_OK;
  if (exact_path) *exact_path = 0;
  return select_sequential(s, lens, ndim, nlev, axis, n_sel, sel, total);
}

// The levels of a copy: every level without repeats (first occurrence kept), free levels dropped, so that each
// combination is a distinct cell and its rank among the distinct combinations is its place among the keys the copy
// creates.  *n = 0: no combination.
static void copy_plan(int ndim, const uint32_t *lens, int nlev, const int *axis, const uint32_t *n_sel, const int32_t *const *sel, NestPlan &p,
                      std::vector<int32_t> &all, uint64_t *n) {
  std::vector<uint64_t> stride(ndim);
  uint64_t st = 1;
  for (int d = ndim - 1; d >= 0; --d) {
    stride[d] = st;
    st *= lens[d];
  }
  memset(&p, 0, offsetof(NestPlan, inl));
  *n = 1;
  for (int l = 0; l < nlev; ++l) {
    if (!n_sel[l]) {  // no combination: nothing is written
      *n = 0;
      return;
    }
    if (axis[l] < 0) continue;
    const uint32_t at = (uint32_t)all.size();
    std::vector<char> seen(lens[axis[l]], 0);
    for (uint32_t j = 0; j < n_sel[l]; ++j)
      if (!seen[sel[l][j]]++) all.push_back(sel[l][j]);
    const int k = p.nlev++;
    p.len[k] = (uint32_t)all.size() - at;
    p.off[k] = at;
    p.stride[k] = stride[axis[l]];
    *n *= p.len[k];
  }
}

// Writes the copy into `t` on the current device: `launch(p, n, seq, seq_base)` starts copy_select_kernel.
template <typename Launch>
static int copy_into(olap_store *t, NestPlan &p, const std::vector<int32_t> &all, uint64_t n, Launch launch) {
  int rc = require_device();
  if (rc) return rc;
  uint32_t *seq = nullptr;
  uint32_t seq_base = 0;
  if ((rc = order_before_select_write(t, n, &seq, &seq_base))) return rc;
  int32_t *dev_lists = nullptr;
  if ((rc = place_lists(p, kSelInline / 2, all, &dev_lists))) return rc;
  launch(p, n, seq, seq_base);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (dev_lists) dev_free(dev_lists);
  if (e != hipSuccess) return hip_fail(e, "copy_select");
  order_after_select_write(t);
  return OLAP_OK;
}

// copy over ONE pair of stores on one device; levels already validated (entries >= 0)
int select_copy(olap_store *t, const olap_store *src, int ndim, const uint32_t *lens, int nlev, const int *axis, const uint32_t *n_sel,
                const int32_t *const *sel) {
  OnStoreDevice on_device__(t);
  if (t->device != src->device) return fail(OLAP_ERR_INVALID_ARGUMENT, "copy_select: source and target live on different devices");
  static thread_local NestPlan p;
  std::vector<int32_t> all;
  uint64_t n;
  copy_plan(ndim, lens, nlev, axis, n_sel, sel, p, all, &n);
  if (n == 0) return OLAP_OK;
  const int tn = t->default_kind == OLAP_DEFAULT_NAN;
  return copy_into(t, p, all, n, [&](const NestPlan &q, uint64_t k, uint32_t *seq, uint32_t seq_base) {
    DISPATCH_DTYPE(src->dtype, S, DISPATCH_DTYPE(t->dtype, T, hipLaunchKernelGGL((copy_select_kernel<StoreSource<S>, T>), select_grid(k), kBlock, 0, nullptr,
                                                                            store_source<S>(src), (T *)t->values, t->status, seq, seq_base, tn, q, k)));
  });
}

extern "C" int olap_store_copy_select(olap_store *target, const olap_store *source, int ndim, const uint32_t *lens, int nlev, const int *axis,
                                      const uint32_t *n_sel, const int32_t *const *sel) {
  int rc = select_validate(target, ndim, lens, nlev, axis, n_sel, sel, true);
  if (rc) return rc;
  if ((rc = select_validate(source, ndim, lens, nlev, axis, n_sel, sel, true))) return rc;
  return select_copy(target, source, ndim, lens, nlev, axis, n_sel, sel);
}

// ---- computed measures: the same reduction, gather and scatter with a formula as the value source ----------------

// the host checks of olap_formula_select_total / olap_store_copy_select_formula, before any device work
static int formula_select_validate(const int32_t *code, int n_code, const double *consts, int n_consts, int n_inputs,
                                   const olap_store *const *inputs, int ndim, const uint32_t *lens, int nlev, const int *axis, const uint32_t *n_sel,
                                   const int32_t *const *sel, bool for_copy) {
  if (n_inputs < 1 || n_inputs > OLAP_FORMULA_MAX_INPUTS)
    return fail(OLAP_ERR_INVALID_ARGUMENT, "a formula over a selection needs 1..%d stored measures, got %d", OLAP_FORMULA_MAX_INPUTS, n_inputs);
  if (code && n_code > 0 && n_code <= OLAP_FORMULA_MAX_CODE)
    for (int pc = 0; pc < n_code; ++pc) {
      if (code[pc] == F_SCALAR) return fail(OLAP_ERR_INVALID_ARGUMENT, "a formula over a selection cannot read a measure total (SCALAR)");
      if (code[pc] == F_CONST || code[pc] == F_INPUT) ++pc;
    }
  int rc = check_formula(code, n_code, n_consts, n_inputs, 0);
  if (rc) return rc;
  if (n_consts && !consts) return fail(OLAP_ERR_INVALID_ARGUMENT, "formula constants are NULL");
  if (!inputs) return fail(OLAP_ERR_INVALID_ARGUMENT, "formula inputs are NULL");
  for (int k = 0; k < n_inputs; ++k) {
    if (!inputs[k]) return fail(OLAP_ERR_INVALID_ARGUMENT, "formula input %d is NULL", k);
    if ((rc = select_validate(inputs[k], ndim, lens, nlev, axis, n_sel, sel, for_copy))) return rc;
    if (inputs[k]->device != inputs[0]->device) return fail(OLAP_ERR_INVALID_ARGUMENT, "formula inputs live on different devices");
  }
  return OLAP_OK;
}

// the program and its inputs in device memory of the current device (*dev is freed by the caller)
static int upload_formula(const int32_t *code, int n_code, const double *consts, int n_consts, int n_inputs, const olap_store *const *inputs,
                          FormulaProgram **dev) {
  *dev = nullptr;
  int rc = require_device();
  if (rc) return rc;
  static thread_local FormulaProgram h;
  memset(&h, 0, sizeof h);
  h.n_code = n_code;
  memcpy(h.code, code, n_code * sizeof(int32_t));
  if (n_consts) memcpy(h.consts, consts, n_consts * sizeof(double));
  h.n_inputs = n_inputs;
  for (int k = 0; k < n_inputs; ++k) {  // what olap_store_eval_formula hands its kernel
    h.in_values[k] = inputs[k]->values;
    h.in_status[k] = mask_needed(inputs[k]);
    h.in_dtype[k] = inputs[k]->dtype;
    h.in_def_nan[k] = inputs[k]->default_kind == OLAP_DEFAULT_NAN;
  }
  HIP_TRY(dev_alloc((void **)dev, sizeof h));
  const hipError_t e = hipMemcpy(*dev, &h, sizeof h, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    dev_free(*dev);
    *dev = nullptr;
    return hip_fail(e, "formula program");
  }
  return OLAP_OK;
}

extern "C" int olap_formula_select_total(const int32_t *code, int n_code, const double *consts, int n_consts, int n_inputs,
                                         const olap_store *const *inputs, int ndim, const uint32_t *lens, int nlev, const int *axis,
                                         const uint32_t *n_sel, const int32_t *const *sel, double *total, int *exact_path) {
  int rc = formula_select_validate(code, n_code, consts, n_consts, n_inputs, inputs, ndim, lens, nlev, axis, n_sel, sel, false);
  if (rc) return rc;
  if (!total) return fail(OLAP_ERR_INVALID_ARGUMENT, "total is NULL");
  std::vector<uint32_t> nd;
  std::vector<const int32_t *> sd;
  double m;
  bool empty;
  by_dimension(ndim, nlev, axis, n_sel, sel, nd, sd, &m, &empty);
  if (exact_path) *exact_path = 1;
  if (empty) {  // no combination: the reduce starts and ends at 0 (src/cube.js:704)
    *total = 0.0;
    return OLAP_OK;
  }
  OnStoreDevice on_device__(inputs[0]);
  FormulaProgram *prog = nullptr;
  if ((rc = upload_formula(code, n_code, consts, n_consts, n_inputs, inputs, &prog))) return rc;
  const FormulaSource src{prog};
  double sum, abs_sum;
  int min_exp;
  unsigned flags;
  rc = cert_of(
      ndim, lens, nd.data(), sd.data(),
      [&](const GatherPlan &p, unsigned blocks, Cert *partial) {
        hipLaunchKernelGGL((select_total_kernel<FormulaSource, double, false>), blocks, kBlock, 0, nullptr, src, p, partial);
      },
      &sum, &abs_sum, &min_exp, &flags);
  if (!rc && !select_certified_total(sum, abs_sum, min_exp, flags, m, total)) {
    if (exact_path) *exact_path = 0;
    rc = sequential_of(
        lens, ndim, nlev, axis, n_sel, sel,
        [&](const NestPlan &p, uint64_t first, uint64_t k, double *out) {
          hipLaunchKernelGGL((select_gather_kernel<FormulaSource>), select_grid(k), kBlock, 0, nullptr, src, p, first, k, out);
        },
        total);
  }
  dev_free(prog);
  return rc;
}

extern "C" int olap_store_copy_select_formula(olap_store *target, const int32_t *code, int n_code, const double *consts, int n_consts, int n_inputs,
                                              const olap_store *const *inputs, int ndim, const uint32_t *lens, int nlev, const int *axis,
                                              const uint32_t *n_sel, const int32_t *const *sel) {
  int rc = select_validate(target, ndim, lens, nlev, axis, n_sel, sel, true);
  if (rc) return rc;
  if ((rc = formula_select_validate(code, n_code, consts, n_consts, n_inputs, inputs, ndim, lens, nlev, axis, n_sel, sel, true))) return rc;
  if (target->device != inputs[0]->device) return fail(OLAP_ERR_INVALID_ARGUMENT, "copy_select: the formula's inputs and the target live on different devices");
  OnStoreDevice on_device__(target);
  static thread_local NestPlan p;
  std::vector<int32_t> all;
  uint64_t n;
  copy_plan(ndim, lens, nlev, axis, n_sel, sel, p, all, &n);
  if (n == 0) return OLAP_OK;
  FormulaProgram *prog = nullptr;
  if ((rc = upload_formula(code, n_code, consts, n_consts, n_inputs, inputs, &prog))) return rc;
  const FormulaSource src{prog};
  const int tn = target->default_kind == OLAP_DEFAULT_NAN;
  rc = copy_into(target, p, all, n, [&](const NestPlan &q, uint64_t k, uint32_t *seq, uint32_t seq_base) {
    DISPATCH_DTYPE(target->dtype, T,
                 hipLaunchKernelGGL((copy_select_kernel<FormulaSource, T>), select_grid(k), kBlock, 0, nullptr, src, (T *)target->values,
                                    target->status, seq, seq_base, tn, q, k));
  });
  dev_free(prog);
  return rc;
}

// ---- set_values ------------------------------------------------------------------------------------------------

int set_values_validate(const olap_store *s, uint64_t n, const uint64_t *indexes, const double *values) {
  if (!s) return fail(OLAP_ERR_INVALID_ARGUMENT, "store is NULL");
  if (n && (!indexes || !values)) return fail(OLAP_ERR_INVALID_ARGUMENT, "indexes/values is NULL");
  for (uint64_t i = 0; i < n; ++i)
    if (indexes[i] >= s->size)
      return fail(OLAP_ERR_INDEX_RANGE, "entry %llu: cell index %llu out of bounds [0, %llu[", (unsigned long long)i, (unsigned long long)indexes[i],
                  (unsigned long long)s->size);
  return OLAP_OK;
}

// one batch of validated entries (n >= 1, n < 2^32): one upload, the sort, the mark + scan, the write, one sync
static int set_values_batch(olap_store *s, uint64_t n, const uint64_t *indexes, const double *values, const uint8_t *is_null) {
  // a tracked store keeps its lazy order (ascending flat index) exactly when each setValue would have kept it
  // (order_before_set_value): every entry lies above all cells that may be set before it
  uint32_t *seq = nullptr;
  uint32_t seq_base = 0;
  int rc;
  if (s->track_order) {
    bool lazy = !s->seq && (!s->maybe_nonempty || indexes[0] > s->hi_index);
    for (uint64_t i = 1; i < n && lazy; ++i) lazy = indexes[i] > indexes[i - 1];
    if (!lazy && (rc = order_before_select_write(s, n, &seq, &seq_base))) return rc;
  }

  // entries in one buffer: cells (8n) | values (8n) | nulls (n)
  const size_t nb = is_null ? n : 0;
  std::vector<unsigned char> host(16 * n + nb);
  memcpy(host.data(), indexes, 8 * n);
  memcpy(host.data() + 8 * n, values, 8 * n);
  if (nb) memcpy(host.data() + 16 * n, is_null, nb);
  int cell_bits = 1;
  while (cell_bits < 64 && ((s->size - 1) >> cell_bits)) ++cell_bits;
  unsigned char *entries = nullptr;
  uint64_t *cell_sorted = nullptr;
  uint32_t *pos_in = nullptr, *pos_sorted = nullptr;
  void *tmp = nullptr;
  size_t sort_bytes = 0, scan_bytes = 0;
  hipError_t e = dev_alloc((void **)&entries, host.size());
  if (e == hipSuccess) e = dev_alloc((void **)&cell_sorted, 8 * n);
  if (e == hipSuccess) e = dev_alloc((void **)&pos_in, 4 * n);
  if (e == hipSuccess) e = dev_alloc((void **)&pos_sorted, 4 * n);
  uint64_t *cell_in = (uint64_t *)entries;
  const double *dv = (const double *)(entries + 8 * n);
  const uint8_t *dn = nb ? entries + 16 * n : nullptr;
  uint32_t *marker = pos_in, *run = (uint32_t *)cell_in;  // (both free once the sort has read them)
  if (e == hipSuccess)
    e = hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint64_t *)cell_in, cell_sorted, (const uint32_t *)pos_in, pos_sorted,
                                           (unsigned int)n, 0, cell_bits, (hipStream_t) nullptr);
  if (e == hipSuccess) e = hipcub::DeviceScan::InclusiveScan(nullptr, scan_bytes, (const uint32_t *)marker, run, hipcub::Max(), (unsigned int)n,
                                                             (hipStream_t) nullptr);
  if (e == hipSuccess) e = dev_alloc(&tmp, std::max<size_t>(std::max(sort_bytes, scan_bytes), 16));
  if (e == hipSuccess) e = hipMemcpy(entries, host.data(), host.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(iota_u32_kernel, select_grid(n), kBlock, 0, nullptr, pos_in, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess)
    e = hipcub::DeviceRadixSort::SortPairs(tmp, sort_bytes, (const uint64_t *)cell_in, cell_sorted, (const uint32_t *)pos_in, pos_sorted,
                                           (unsigned int)n, 0, cell_bits, (hipStream_t) nullptr);
  const int def_nan = s->default_kind == OLAP_DEFAULT_NAN;
  if (e == hipSuccess) {
    DISPATCH_DTYPE(s->dtype, T, hipLaunchKernelGGL((set_values_mark_kernel<T>), select_grid(n), kBlock, 0, nullptr, (const uint64_t *)cell_sorted,
                                                 (const uint32_t *)pos_sorted, dv, dn, def_nan, n, marker));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipcub::DeviceScan::InclusiveScan(tmp, scan_bytes, (const uint32_t *)marker, run, hipcub::Max(), (unsigned int)n,
                                                             (hipStream_t) nullptr);
  if (e == hipSuccess) {
    DISPATCH_DTYPE(s->dtype, T, hipLaunchKernelGGL((set_values_write_kernel<T>), select_grid(n), kBlock, 0, nullptr, (const uint64_t *)cell_sorted,
                                                 (const uint32_t *)pos_sorted, dv, dn, (const uint32_t *)run, n, (T *)s->values, s->status, seq,
                                                 seq_base, def_nan));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  for (void *q : {(void *)entries, (void *)cell_sorted, (void *)pos_in, (void *)pos_sorted, tmp})
    if (q) dev_free(q);
  if (e != hipSuccess) return hip_fail(e, "set_values");
  if (seq) {
    order_after_select_write(s);
  } else {  // what order_after_set_value leaves without seq
    s->maybe_nonempty = true;
    s->hi_index = std::max(s->hi_index, *std::max_element(indexes, indexes + n));
  }
  return OLAP_OK;
}

int set_values(olap_store *s, uint64_t n, const uint64_t *indexes, const double *values, const uint8_t *is_null) {
  OnStoreDevice on_device__(s);
  int rc = set_values_validate(s, n, indexes, values);
  if (rc || n == 0) return rc;
  if ((rc = require_device())) return rc;
  // sequential setValue calls compose: a long list is written as consecutive batches (positions stay 32-bit)
  constexpr uint64_t kBatch = 1ull << 26;
  for (uint64_t first = 0; first < n; first += kBatch) {
    const uint64_t k = std::min(kBatch, n - first);
    if ((rc = set_values_batch(s, k, indexes + first, values + first, is_null ? is_null + first : nullptr))) return rc;
  }
  return OLAP_OK;
}

extern "C" int olap_store_set_values(olap_store *store, uint64_t n, const uint64_t *indexes, const double *values, const uint8_t *is_null) {
  return set_values(store, n, indexes, values, is_null);
}
