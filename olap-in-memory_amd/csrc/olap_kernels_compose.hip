// compose (K12): the measures of one source cube brought onto the dimensions of a composed cube — what
// olap_store_create [+ olap_store_fill] + olap_store_load leave, as ONE gather indexed by the TARGET.  A target cell
// takes the source cell that maps onto it (the host inverts the item maps, the last of several items winning as the
// last write of a load wins), or the fill value, or stays unset: every target cell is written exactly once, nothing is
// cleared or filled first, and no cell of the source is read twice.  Both stores have the source's cell type and
// default, so a loaded cell keeps its value and its state (load_scatter_kernel's "his default against mine" never
// arises).  In a translation unit of its own so that the four cell types are compiled once.
#include "olap_kernels.hpp"

namespace olap {

// up to kMaxBatch (his, mine) pairs of one launch; blockIdx.y picks the pair.  The fill travels as a converted cell and
// its mask (fill_set == 0: no fill, or one that olap_store_fill would drop: the cell stays unset).
template <typename T>
struct ComposePairs {
  const T *his[kMaxBatch];
  const int32_t *his_st[kMaxBatch];
  T *mine[kMaxBatch];
  int32_t *mine_st[kMaxBatch];
  T fill[kMaxBatch];
  int32_t fill_set[kMaxBatch];
};

// one source cell as the target holds it
template <typename T, bool HAS_STATUS>
__device__ __forceinline__ void compose_cell(T x, int32_t st, bool def_nan, T &ov, int32_t &os) {
  const bool set = cell_is_set<T>(x, HAS_STATUS ? st : OLAP_STATUS_SET, HAS_STATUS, def_nan);
  ov = set ? x : Cell<T>::default_value(def_nan);
  os = set ? OLAP_STATUS_SET : 0;
}

// The innermost merged run left alone by the maps and a whole number of 16-byte lanes (so it is one in both stores): a
// lane owns 16 bytes of MINE, decodes its index once, reads the 16 bytes of his that land there with one streaming
// load — or nothing at all where no item of his maps onto the lane's items — and writes one 16-byte streaming store.
template <typename T, bool HAS_STATUS, typename IDX>
__global__ __launch_bounds__(kBlock) void compose_lanes_kernel(const ComposePairs<T> b, const Remap r, const int any_fill) {
  constexpr int V = 16 / sizeof(T);
  const uint32_t pair = blockIdx.y;
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= r.total) return;
  const bool def_nan = r.def_nan != 0;
  uint64_t src;
  const bool ok = gather_source<V, IDX>(t, r, src);
  Vec<T, V> ov;
  Vec<int32_t, V> os;
  if (ok) {
    const Vec<T, V> x = load_stream<T, V>(b.his[pair] + src);
    Vec<int32_t, V> xs{};
    if constexpr (HAS_STATUS) xs = load_stream<int32_t, V>(b.his_st[pair] + src);
#pragma unroll
    for (int e = 0; e < V; ++e) compose_cell<T, HAS_STATUS>(x.v[e], xs.v[e], def_nan, ov.v[e], os.v[e]);
  } else {
    const bool filled = any_fill && b.fill_set[pair] != 0;
    const T v = filled ? b.fill[pair] : Cell<T>::default_value(def_nan);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      ov.v[e] = v;
      os.v[e] = filled ? OLAP_STATUS_SET : 0;
    }
  }
  store_stream<T, V>(b.mine[pair] + t * V, ov);
  if (b.mine_st[pair]) store_stream<int32_t, V>(b.mine_st[pair] + t * V, os);
}

// offset in his of the outer digits of my cell c (-1: an item his store has no counterpart of) and c's innermost digit
template <typename IDX>
__device__ __forceinline__ int64_t compose_outer(const Remap &r, IDX c, uint32_t *digit0) {
  const int last = r.nd - 1;
  uint64_t src = 0;
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
        src += (uint64_t)digit * r.stride[d];
      } else {
        const int64_t o = r.tab[r.tab_off[d] + digit];
        if (o < 0) ok = false;
        else src += (uint64_t)o;
      }
    }
  }
  return ok ? (int64_t)src : -1;
}

// Everything else — the innermost dimension remapped, rows that are not whole lanes: a lane still owns V = 16 / sizeof(T)
// consecutive cells of MINE and leaves them as one 16-byte streaming store (cell by cell in the ragged last lane, and
// when my buffer is off the 16-byte grid), so the stores stay coalesced; his cells are read one by one, all V loads
// issued before the first is used.  The index is decoded once per lane; the cells that follow in the same innermost
// row only add their own innermost offset, and a cell past the row's end is decoded afresh.
template <typename T, bool HAS_STATUS, typename IDX>
__global__ __launch_bounds__(kBlock) void compose_cells_kernel(const ComposePairs<T> b, const Remap r, const uint64_t n_cells, const int any_fill,
                                                               const int mine_aligned) {
  constexpr int V = 16 / sizeof(T);
  const uint32_t pair = blockIdx.y;
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t c0 = t * V;
  if (c0 >= n_cells) return;
  const bool def_nan = r.def_nan != 0;
  const int last = r.nd - 1;
  const T *__restrict__ his = b.his[pair];
  const int32_t *__restrict__ his_st = b.his_st[pair];
  T *__restrict__ mine = b.mine[pair];
  int32_t *__restrict__ mine_st = b.mine_st[pair];
  int64_t src[V];
  uint32_t digit0 = 0;
  int64_t outer = compose_outer<IDX>(r, (IDX)c0, &digit0);
#pragma unroll
  for (int e = 0; e < V; ++e) {
    src[e] = -1;
    if (c0 + e < n_cells) {
      if (e > 0 && ++digit0 >= r.len[last]) outer = compose_outer<IDX>(r, (IDX)(c0 + e), &digit0);  // the next innermost row
      const int64_t in = r.tab_off[last] < 0 ? (int64_t)((uint64_t)digit0 * r.stride[last]) : r.tab[r.tab_off[last] + digit0];
      if (outer >= 0 && in >= 0) src[e] = outer + in;
    }
  }
  T x[V];
  int32_t xs[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    x[e] = src[e] >= 0 ? his[src[e]] : T(0);
    xs[e] = 0;
    if constexpr (HAS_STATUS) xs[e] = src[e] >= 0 ? his_st[src[e]] : 0;
  }
  const bool filled = any_fill && b.fill_set[pair] != 0;
  const T fv = filled ? b.fill[pair] : Cell<T>::default_value(def_nan);
  Vec<T, V> ov;
  Vec<int32_t, V> os;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    if (src[e] >= 0) {
      compose_cell<T, HAS_STATUS>(x[e], xs[e], def_nan, ov.v[e], os.v[e]);
    } else {
      ov.v[e] = fv;
      os.v[e] = filled ? OLAP_STATUS_SET : 0;
    }
  }
  if (mine_aligned && c0 + V <= n_cells) {
    store_stream<T, V>(mine + c0, ov);
    if (mine_st) store_stream<int32_t, V>(mine_st + c0, os);
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if (c0 + e < n_cells) {
        mine[c0 + e] = ov.v[e];
        if (mine_st) mine_st[c0 + e] = os.v[e];
      }
    }
  }
}

template <typename T>
static hipError_t launch_compose_typed(bool has_status, int vec, const void *const *his, const int32_t *const *his_st, void *const *mine,
                                       int32_t *const *mine_st, const double *fill_cells, const int32_t *fill_set, unsigned nb, const Remap &r,
                                       hipStream_t stream) {
  constexpr int V = 16 / (int)sizeof(T);
  ComposePairs<T> b{};
  bool mine_aligned = true;
  int any_fill = 0;
  for (unsigned i = 0; i < nb; ++i) {
    b.his[i] = (const T *)his[i];
    b.his_st[i] = has_status && his_st ? his_st[i] : nullptr;
    b.mine[i] = (T *)mine[i];
    b.mine_st[i] = mine_st ? mine_st[i] : nullptr;
    // the fill arrives as the float64 image of the converted cell: exact for every cell type
    b.fill[i] = fill_cells && fill_set && fill_set[i] ? (T)fill_cells[i] : T(0);
    b.fill_set[i] = fill_set ? fill_set[i] : 0;
    any_fill |= b.fill_set[i];
    mine_aligned = mine_aligned && (((uintptr_t)b.mine[i] | (uintptr_t)b.mine_st[i]) & 15u) == 0;
  }
  const uint64_t cells = r.total * (uint64_t)vec;
  const bool idx32 = cells < 0xFFFFFFFFull;
  const uint64_t lanes = vec > 1 ? r.total : (cells + V - 1) / V;
  const uint64_t blocks = (lanes + kBlock - 1) / kBlock;
  if (blocks >= 0x7FFFFFFFull) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks, nb);
#define OLAP_CP(HS, IDX)                                                                                                        \
  do {                                                                                                                          \
    if (vec > 1) hipLaunchKernelGGL((compose_lanes_kernel<T, HS, IDX>), grid, kBlock, 0, stream, b, r, any_fill);               \
    else hipLaunchKernelGGL((compose_cells_kernel<T, HS, IDX>), grid, kBlock, 0, stream, b, r, cells, any_fill, mine_aligned ? 1 : 0); \
  } while (0)
  if (has_status) {
    if (idx32) OLAP_CP(true, uint32_t); else OLAP_CP(true, uint64_t);
  } else {
    if (idx32) OLAP_CP(false, uint32_t); else OLAP_CP(false, uint64_t);
  }
#undef OLAP_CP
  return hipGetLastError();
}

hipError_t launch_compose(int dtype, bool has_status, int vec, const void *const *his, const int32_t *const *his_st, void *const *mine,
                          int32_t *const *mine_st, const double *fill_cells, const int32_t *fill_set, unsigned nb, const Remap &r,
                          hipStream_t stream) {
  if (r.total == 0 || nb == 0) return hipSuccess;
  if (nb > (unsigned)kMaxBatch || r.nd < 1 || (vec != 1 && vec != 16 / (int)olap_dtype_size(dtype))) return hipErrorInvalidValue;
  switch (dtype) {
    case OLAP_INT32: return launch_compose_typed<int32_t>(has_status, vec, his, his_st, mine, mine_st, fill_cells, fill_set, nb, r, stream);
    case OLAP_UINT32: return launch_compose_typed<uint32_t>(has_status, vec, his, his_st, mine, mine_st, fill_cells, fill_set, nb, r, stream);
    case OLAP_FLOAT32: return launch_compose_typed<float>(has_status, vec, his, his_st, mine, mine_st, fill_cells, fill_set, nb, r, stream);
    default: return launch_compose_typed<double>(has_status, vec, his, his_st, mine, mine_st, fill_cells, fill_set, nb, r, stream);
  }
}

}  // namespace olap
