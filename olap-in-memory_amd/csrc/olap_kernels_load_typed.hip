// load between stores of different cell types: the twelve (his type, my type) pairs, in a translation unit of their own
// so that they are compiled once and not into every per-cell-type object.
#include "olap_kernels.hpp"

namespace olap {

// up to kMaxBatch (his, mine) pairs of one launch; blockIdx.y picks the pair (a single load is a batch of one)
template <typename S, typename T>
struct LoadPairs {
  const S *his[kMaxBatch];
  const int32_t *his_st[kMaxBatch];
  T *mine[kMaxBatch];
  int32_t *mine_st[kMaxBatch];
};

// One cell of HIS store (cells of type S, his default) as MY store (cells of type T, my default) holds it after
// load(): what the two existing kernels leave when they run one after the other, without the cube in between.
//   1. from_f64_kernel over his float64 values (olap_store_get_data_f64: an unset cell reads as his default, also an
//      unset integer cell under a NaN default) into T cells under HIS default: setValue on the JS number
//      (is_default_f64), then emit_cell<T> (TypedArray conversion, and a converted value that IS his default is unset);
//   2. load_scatter_kernel of that store into mine: a set cell keeps its value unless it is MY default; an unset one
//      hands out HIS default, which my setValue keeps unless it is MY default (the "his default against mine" branch).
template <typename S, typename T, bool HAS_STATUS>
__device__ __forceinline__ void load_convert_cell(S x, int32_t st, bool his_nan, bool def_nan, T &ov, int32_t &os) {
  const bool his_set = cell_is_set<S>(x, HAS_STATUS ? st : OLAP_STATUS_SET, HAS_STATUS, his_nan);
  const double d = Cell<S>::to_f64(x);
  // step 1
  T tv;
  int32_t ts;
  emit_cell<T>(d, his_set && !is_default_f64(d, his_nan), his_nan, tv, ts);
  // step 2
  bool set;
  T v;
  if (ts) {
    v = tv;
    set = !Cell<T>::is_default(v, def_nan);
  } else {
    v = Cell<T>::default_value(his_nan);
    set = his_nan ? (IsFloatCell<T>::value && !def_nan) : def_nan;
  }
  ov = set ? v : Cell<T>::default_value(def_nan);
  os = set ? OLAP_STATUS_SET : 0;
}

// Trailing dimensions left alone (the innermost merged run is contiguous in both stores and a whole number of lanes).
// A lane owns 16 bytes of HIS — the side every cell of which is read exactly once, with one 16-byte streaming load —
// and writes the V = 16 / sizeof(S) converted cells where they sit in mine: 8 bytes (two float64 cells into 4-byte
// ones), 16 bytes or 32 bytes (four 4-byte cells into float64 ones, two 16-byte stores).  Taking 16 bytes of MINE per
// lane instead would read 4-byte cells 8 bytes at a time for a float64 target.  The index is decoded once per lane.
template <typename S, typename T, bool HAS_STATUS, typename IDX>
__global__ __launch_bounds__(kBlock) void load_convert_lanes_kernel(const LoadPairs<S, T> b, const Remap r) {
  constexpr int V = 16 / sizeof(S);
  const uint32_t pair = blockIdx.y;
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= r.total) return;
  const bool def_nan = r.def_nan != 0, his_nan = r.src_def_nan != 0;
  IDX c = (IDX)(t * V);
  uint64_t dst = 0;
  bool ok = true;
#pragma unroll
  for (int d = kMaxDims - 1; d >= 0; --d) {
    if (d < r.nd) {
      const IDX q = c / (IDX)r.len[d];
      const uint32_t digit = (uint32_t)(c - q * (IDX)r.len[d]);
      c = q;
      if (r.tab_off[d] < 0) {
        dst += (uint64_t)digit * r.stride[d];
      } else {
        const int64_t o = r.tab[r.tab_off[d] + digit];
        if (o < 0) ok = false;
        else dst += (uint64_t)o;
      }
    }
  }
  if (!ok) return;  // an item this store does not have: its cells are not loaded
  const Vec<S, V> x = load_stream<S, V>(b.his[pair] + t * V);
  Vec<int32_t, V> xs{};
  if constexpr (HAS_STATUS) xs = load_stream<int32_t, V>(b.his_st[pair] + t * V);
  Vec<T, V> ov;
  Vec<int32_t, V> os;
#pragma unroll
  for (int e = 0; e < V; ++e) load_convert_cell<S, T, HAS_STATUS>(x.v[e], xs.v[e], his_nan, def_nan, ov.v[e], os.v[e]);
  store_stream<T, V>(b.mine[pair] + dst, ov);
  int32_t *mine_st = b.mine_st[pair];
  if (mine_st) store_stream<int32_t, V>(mine_st + dst, os);
}

// The innermost dimension remapped, or rows that are not whole lanes: as load_scatter_run_kernel, a lane still reads
// 16 consecutive bytes of his with one streaming load (`vector_loads`: every his buffer is on the 16-byte grid) and
// decodes its index once; the cells that follow in the same innermost row only add their own innermost offset, a cell
// past the row's end is decoded afresh, and every cell is stored on its own.
template <typename S, typename T, bool HAS_STATUS, typename IDX>
__global__ __launch_bounds__(kBlock) void load_convert_run_kernel(const LoadPairs<S, T> b, const Remap r, const uint64_t n_cells,
                                                                  const int vector_loads) {
  constexpr int R = 16 / sizeof(S);
  const uint32_t pair = blockIdx.y;
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t * R >= n_cells) return;
  const S *__restrict__ his = b.his[pair];
  const int32_t *__restrict__ his_st = b.his_st[pair];
  T *__restrict__ mine = b.mine[pair];
  int32_t *__restrict__ mine_st = b.mine_st[pair];
  const bool def_nan = r.def_nan != 0, his_nan = r.src_def_nan != 0;
  const int last = r.nd - 1;  // (the plan keeps at least one dimension)
  auto inner_off = [&](uint32_t dg) -> int64_t { return r.tab_off[last] < 0 ? (int64_t)((uint64_t)dg * r.stride[last]) : r.tab[r.tab_off[last] + dg]; };
  auto decode = [&](IDX c, uint32_t *digit0) -> int64_t {
    uint64_t dst = 0;
    bool ok = true;
    const IDX q0 = c / (IDX)r.len[last];
    *digit0 = (uint32_t)(c - q0 * (IDX)r.len[last]);
    c = q0;
#pragma unroll
    for (int d = kMaxDims - 2; d >= 0; --d) {
      if (d < last) {
        const IDX q = c / (IDX)r.len[d];
        const uint32_t digit = (uint32_t)(c - q * (IDX)r.len[d]);
        c = q;
        if (r.tab_off[d] < 0) {
          dst += (uint64_t)digit * r.stride[d];
        } else {
          const int64_t o = r.tab[r.tab_off[d] + digit];
          if (o < 0) ok = false;
          else dst += (uint64_t)o;
        }
      }
    }
    return ok ? (int64_t)dst : -1;
  };
  const uint64_t c0 = t * R;
  Vec<S, R> x;
  Vec<int32_t, R> xs{};
  if (vector_loads && c0 + R <= n_cells) {
    x = load_stream<S, R>(his + c0);
    if constexpr (HAS_STATUS) xs = load_stream<int32_t, R>(his_st + c0);
  } else {
#pragma unroll
    for (int e = 0; e < R; ++e) {
      x.v[e] = c0 + e < n_cells ? his[c0 + e] : S(0);
      if constexpr (HAS_STATUS) xs.v[e] = c0 + e < n_cells ? his_st[c0 + e] : 0;
    }
  }
  uint32_t digit0 = 0;
  int64_t outer = decode((IDX)c0, &digit0);
#pragma unroll
  for (int e = 0; e < R; ++e) {
    if (c0 + e >= n_cells) break;
    if (e > 0 && ++digit0 >= r.len[last]) outer = decode((IDX)(c0 + e), &digit0);  // the next innermost row
    const int64_t in = inner_off(digit0);
    if (outer < 0 || in < 0) continue;  // an item this store does not have: its cells are not loaded
    const uint64_t dst = (uint64_t)outer + (uint64_t)in;
    T ov;
    int32_t os;
    load_convert_cell<S, T, HAS_STATUS>(x.v[e], xs.v[e], his_nan, def_nan, ov, os);
    mine[dst] = ov;
    if (mine_st) mine_st[dst] = os;
  }
}

template <typename S, typename T>
static hipError_t launch_pair(bool has_status, int vec, const void *const *his, const int32_t *const *his_st, void *const *mine,
                              int32_t *const *mine_st, unsigned nb, const Remap &r, hipStream_t stream) {
  constexpr int V = 16 / (int)sizeof(S);
  LoadPairs<S, T> b{};
  bool his_aligned = true;
  for (unsigned i = 0; i < nb; ++i) {
    b.his[i] = (const S *)his[i];
    b.his_st[i] = has_status && his_st ? his_st[i] : nullptr;
    b.mine[i] = (T *)mine[i];
    b.mine_st[i] = mine_st ? mine_st[i] : nullptr;
    his_aligned = his_aligned && (((uintptr_t)b.his[i] | (uintptr_t)b.his_st[i]) & 15u) == 0;
  }
  const uint64_t cells = r.total * (uint64_t)vec;
  const bool idx32 = cells < 0xFFFFFFFFull;
  const uint64_t lanes = vec > 1 ? r.total : (cells + V - 1) / V;
  const uint64_t blocks = (lanes + kBlock - 1) / kBlock;
  if (blocks >= 0x7FFFFFFFull) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks, nb);
#define OLAP_LC(HS, IDX)                                                                                                  \
  do {                                                                                                                    \
    if (vec > 1) hipLaunchKernelGGL((load_convert_lanes_kernel<S, T, HS, IDX>), grid, kBlock, 0, stream, b, r);           \
    else hipLaunchKernelGGL((load_convert_run_kernel<S, T, HS, IDX>), grid, kBlock, 0, stream, b, r, cells, his_aligned ? 1 : 0); \
  } while (0)
  if (has_status) {
    if (idx32) OLAP_LC(true, uint32_t); else OLAP_LC(true, uint64_t);
  } else {
    if (idx32) OLAP_LC(false, uint32_t); else OLAP_LC(false, uint64_t);
  }
#undef OLAP_LC
  return hipGetLastError();
}

template <typename S>
static hipError_t launch_from(int my_dtype, bool has_status, int vec, const void *const *his, const int32_t *const *his_st, void *const *mine,
                              int32_t *const *mine_st, unsigned nb, const Remap &r, hipStream_t stream) {
  // (S == T never comes here: the same-type kernels of olap_kernels.hpp run it; the branch below keeps it out of this object)
#define OLAP_TO(T)                                                                                    \
  if constexpr (!std::is_same<S, T>::value) return launch_pair<S, T>(has_status, vec, his, his_st, mine, mine_st, nb, r, stream); \
  else return hipErrorInvalidValue
  switch (my_dtype) {
    case OLAP_INT32: OLAP_TO(int32_t);
    case OLAP_UINT32: OLAP_TO(uint32_t);
    case OLAP_FLOAT32: OLAP_TO(float);
    default: OLAP_TO(double);
  }
#undef OLAP_TO
}

hipError_t launch_load_convert(int his_dtype, int my_dtype, bool has_status, int vec, const void *const *his, const int32_t *const *his_st,
                               void *const *mine, int32_t *const *mine_st, unsigned nb, const Remap &r, hipStream_t stream) {
  if (r.total == 0 || nb == 0) return hipSuccess;
  if (nb > (unsigned)kMaxBatch || r.nd < 1) return hipErrorInvalidValue;
  switch (his_dtype) {
    case OLAP_INT32: return launch_from<int32_t>(my_dtype, has_status, vec, his, his_st, mine, mine_st, nb, r, stream);
    case OLAP_UINT32: return launch_from<uint32_t>(my_dtype, has_status, vec, his, his_st, mine, mine_st, nb, r, stream);
    case OLAP_FLOAT32: return launch_from<float>(my_dtype, has_status, vec, his, his_st, mine, mine_st, nb, r, stream);
    default: return launch_from<double>(my_dtype, has_status, vec, his, his_st, mine, mine_st, nb, r, stream);
  }
}

}  // namespace olap
