// olap_blocks.hip — Cube.scan / Cube.iterateOverDimension in one device pass (olap_store_blocks_report).
//
// Every combination of the scanned dimensions' items receives cells that are already on the device: each stored measure
// is regrouped to [scanned..., kept...] so that a combination's cells are contiguous, converted to float64 with the
// store's default in unset cells (what olap_store_get_data_f64 hands out) and brought back in one copy.  Two kernels:
//   blocks_rows_kernel       the innermost cube dimension is kept: rows stay contiguous on both sides, a row gather
//   blocks_transpose_kernel  the innermost cube dimension is scanned: the destination's fastest axis is strided in the
//                            source, so tiles go through LDS (padded) and both sides stay coalesced
// No atomics, no state across workgroups, every output cell written exactly once.
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "olap_internal.hpp"
#include "olap_kernels.hpp"

namespace olap {

// where the float64 cells of the pairs of one launch go (the inputs travel in Batch<T>::in / st_in)
struct BlockSlots {
  double *out[kMaxBatch];
};

// The cube's dimensions after runs that stay adjacent on both sides were merged and one-item dimensions dropped,
// outermost first.  The row kernel decodes all of them; the transpose decodes the ones outside its two tile axes.
struct BlockDims {
  int nd;
  int by_result;  // rows: the lanes walk the RESULT (a gather: writes in address order) instead of the store (a scatter)
  uint32_t len[OLAP_MAX_DIMS];
  uint64_t dst_stride[OLAP_MAX_DIMS];  // in cells of the result
  uint64_t src_stride[OLAP_MAX_DIMS];  // in cells of the store
};

template <typename T, bool HAS_STATUS>
__device__ __forceinline__ double block_cell(T x, int32_t st, bool def_nan) {
  // (a mask travels only where it is primary: integer cells under a NaN default, whose unset cells read as NaN)
  if constexpr (HAS_STATUS) return (st & OLAP_STATUS_SET) ? Cell<T>::to_f64(x) : (def_nan ? __builtin_nan("") : 0.0);
  else return Cell<T>::to_f64(x);
}

// A lane owns V consecutive cells of a row (V = 16 bytes of the store where the row length and the alignment allow, 1
// otherwise), decodes its index on the side the lanes walk once and finds the row on the other side.  `total` = cells / V.
template <typename T, bool HAS_STATUS, int V>
__global__ __launch_bounds__(kBlock) void blocks_rows_kernel(const Batch<T> b, const BlockSlots o, const BlockDims m, const uint32_t total,
                                                             const int def_nan) {
  const uint32_t pair = blockIdx.y;
  const uint64_t t64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t64 >= total) return;
  const uint32_t cell = (uint32_t)t64 * V;  // (the byte cap of the call keeps a store below 2^27 cells)
  uint32_t c = cell;
  uint64_t other = 0;
  for (int d = m.nd - 1; d >= 0; --d) {
    const uint32_t q = c / m.len[d];
    other += (uint64_t)(c - q * m.len[d]) * (m.by_result ? m.src_stride[d] : m.dst_stride[d]);
    c = q;
  }
  const uint64_t src = m.by_result ? other : cell, dst = m.by_result ? cell : other;
  const Vec<T, V> x = load_stream<T, V>(b.in[pair] + src);
  Vec<int32_t, V> xs{};
  if constexpr (HAS_STATUS) xs = load_stream<int32_t, V>(b.st_in[pair] + src);
  Vec<double, V> r;
#pragma unroll
  for (int e = 0; e < V; ++e) r.v[e] = block_cell<T, HAS_STATUS>(x.v[e], xs.v[e], def_nan != 0);
  store_stream<double, V>(o.out[pair] + dst, r);
}

// The transposing form.  X = the innermost (scanned) dimension, contiguous in the store; Y = the last kept dimension,
// contiguous in the result.  A workgroup moves one tx x ty tile (powers of two up to kBlockTile) of one coordinate of
// the other dimensions: rows of X are read into LDS, columns are read back with lanes along Y, converted and written.
constexpr int kBlockTile = 64;
struct BlockTiles {
  uint32_t lx, ly;          // extents of X and Y
  uint32_t tx, ty;          // tile extents (cells), powers of two, 1..kBlockTile
  uint32_t tiles_x, tiles_y;
  uint64_t src_y, dst_x;    // stride of Y in the store, of X in the result (X in the store and Y in the result: 1)
};

template <typename T, bool HAS_STATUS>
__global__ __launch_bounds__(kBlock) void blocks_transpose_kernel(const Batch<T> b, const BlockSlots o, const BlockDims m, const BlockTiles t,
                                                                  const int def_nan) {
  // pitch tx + 1: a column read (lanes along y) walks the banks with an odd stride
  __shared__ T tile[kBlockTile * (kBlockTile + 1)];
  __shared__ int32_t tile_st[HAS_STATUS ? kBlockTile * (kBlockTile + 1) : 1];
  const uint32_t pair = blockIdx.y;
  uint32_t w = blockIdx.x;
  const uint32_t bx = w % t.tiles_x;
  w /= t.tiles_x;
  const uint32_t by = w % t.tiles_y;
  w /= t.tiles_y;
  uint64_t src = 0, dst = 0;  // the other dimensions' coordinate (uniform over the workgroup)
  for (int d = m.nd - 1; d >= 0; --d) {
    const uint32_t q = w / m.len[d];
    const uint32_t digit = w - q * m.len[d];
    src += (uint64_t)digit * m.src_stride[d];
    dst += (uint64_t)digit * m.dst_stride[d];
    w = q;
  }
  const uint32_t x0 = bx * t.tx, y0 = by * t.ty;
  const uint32_t pitch = t.tx + 1;
  const T *__restrict__ in = b.in[pair] + src;
  const int32_t *__restrict__ st = HAS_STATUS ? b.st_in[pair] + src : nullptr;
  {
    const uint32_t x = threadIdx.x % t.tx;
    for (uint32_t y = threadIdx.x / t.tx; y < t.ty; y += kBlock / t.tx) {
      if (x0 + x < t.lx && y0 + y < t.ly) {
        const uint64_t at = (uint64_t)(y0 + y) * t.src_y + (x0 + x);
        tile[y * pitch + x] = in[at];
        if constexpr (HAS_STATUS) tile_st[y * pitch + x] = st[at];
      }
    }
  }
  __syncthreads();
  {
    double *__restrict__ out = o.out[pair] + dst;
    const uint32_t y = threadIdx.x % t.ty;
    for (uint32_t x = threadIdx.x / t.ty; x < t.tx; x += kBlock / t.ty) {
      if (x0 + x < t.lx && y0 + y < t.ly) {
        int32_t s = 0;
        if constexpr (HAS_STATUS) s = tile_st[y * pitch + x];
        out[(uint64_t)(x0 + x) * t.dst_x + (y0 + y)] = block_cell<T, HAS_STATUS>(tile[y * pitch + x], s, def_nan != 0);
      }
    }
  }
}

}  // namespace olap

using namespace olap;

namespace {

// what the host decides from the lengths and the flags alone
struct BlocksPlan {
  bool transpose = false;
  BlockDims dims{};    // rows: every merged dimension; transpose: the ones outside X and Y
  BlockTiles tiles{};
  uint32_t row = 1;    // rows: cells of the innermost merged dimension (contiguous on both sides)
};

uint32_t pow2_up_to_tile(uint32_t n) {
  uint32_t p = 1;
  while (p < n && p < (uint32_t)kBlockTile) p *= 2;
  return p;
}

BlocksPlan plan_blocks(int ndim, const uint32_t *lens, const uint8_t *scanned, uint64_t kept_cells) {
  // strides of every cube dimension in the store and in the result [scanned..., kept...]
  std::vector<uint64_t> src(ndim), dst(ndim);
  uint64_t s = 1, k = 1, c = kept_cells;
  for (int d = ndim - 1; d >= 0; --d) {
    src[d] = s;
    s *= lens[d];
    if (scanned[d]) dst[d] = c, c *= lens[d];
    else dst[d] = k, k *= lens[d];
  }
  // one-item dimensions dropped, neighbours of one kind merged (they are neighbours in the result too)
  BlockDims m{};
  int last_kind = -1;
  for (int d = 0; d < ndim; ++d) {
    if (lens[d] == 1) continue;
    const int kind = scanned[d] ? 1 : 0;
    if (m.nd > 0 && kind == last_kind) {
      m.len[m.nd - 1] *= lens[d];
      m.dst_stride[m.nd - 1] = dst[d];
      m.src_stride[m.nd - 1] = src[d];
    } else {
      m.len[m.nd] = lens[d];
      m.dst_stride[m.nd] = dst[d];
      m.src_stride[m.nd] = src[d];
      ++m.nd;
    }
    last_kind = kind;
  }
  BlocksPlan p;
  if (m.nd == 0) {  // one cell
    m.nd = 1, m.len[0] = 1, m.dst_stride[0] = 1, m.src_stride[0] = 1;
  }
  if (m.dst_stride[m.nd - 1] == 1) {  // the innermost dimension is kept (or everything is scanned: the identity)
    p.row = m.len[m.nd - 1];
    if (m.nd == 1 || getenv("OLAP_BLOCKS_BY_STORE")) {  // (developer knob: lanes in the order of the store, A/B against the default)
      p.dims = m;
      return p;
    }
    // lanes in the order of the result: the scanned merged dimensions, then the kept ones (kinds alternate, the last is kept)
    BlockDims &r = p.dims;
    r.by_result = 1;
    for (int kept_pass = 0; kept_pass < 2; ++kept_pass)
      for (int d = 0; d < m.nd; ++d)
        if (((m.nd - 1 - d) % 2 == 0) == (kept_pass == 1)) {
          r.len[r.nd] = m.len[d], r.dst_stride[r.nd] = m.dst_stride[d], r.src_stride[r.nd] = m.src_stride[d];
          ++r.nd;
        }
    return p;
  }
  // innermost scanned: X = the last merged dimension, Y = the kept one before it (kinds alternate, so it is there)
  p.transpose = true;
  BlockTiles &t = p.tiles;
  t.lx = m.len[m.nd - 1], t.ly = m.len[m.nd - 2];
  t.src_y = m.src_stride[m.nd - 2], t.dst_x = m.dst_stride[m.nd - 1];
  t.tx = pow2_up_to_tile(t.lx), t.ty = pow2_up_to_tile(t.ly);
  t.tiles_x = (t.lx + t.tx - 1) / t.tx, t.tiles_y = (t.ly + t.ty - 1) / t.ty;
  p.dims.nd = m.nd - 2;
  for (int d = 0; d < m.nd - 2; ++d) p.dims.len[d] = m.len[d], p.dims.dst_stride[d] = m.dst_stride[d], p.dims.src_stride[d] = m.src_stride[d];
  return p;
}

template <typename T>
hipError_t launch_blocks(const BlocksPlan &p, bool has_status, const Batch<T> &b, const BlockSlots &o, unsigned nb, uint64_t size, bool aligned16,
                         int def_nan) {
  if (p.transpose) {
    uint64_t groups = (uint64_t)p.tiles.tiles_x * p.tiles.tiles_y;
    for (int d = 0; d < p.dims.nd; ++d) groups *= p.dims.len[d];
    if (groups >= 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)groups, nb);
    if (has_status) hipLaunchKernelGGL((blocks_transpose_kernel<T, true>), grid, kBlock, 0, nullptr, b, o, p.dims, p.tiles, def_nan);
    else hipLaunchKernelGGL((blocks_transpose_kernel<T, false>), grid, kBlock, 0, nullptr, b, o, p.dims, p.tiles, def_nan);
    return hipGetLastError();
  }
  constexpr int V = 16 / (int)sizeof(T);
  const bool lanes = aligned16 && p.row % V == 0;
  const uint64_t total = lanes ? size / V : size;
  const dim3 grid((unsigned)((total + kBlock - 1) / kBlock), nb);
#define OLAP_ROWS(HS)                                                                                                                 \
  do {                                                                                                                                \
    if (lanes) hipLaunchKernelGGL((blocks_rows_kernel<T, HS, V>), grid, kBlock, 0, nullptr, b, o, p.dims, (uint32_t)total, def_nan);    \
    else hipLaunchKernelGGL((blocks_rows_kernel<T, HS, 1>), grid, kBlock, 0, nullptr, b, o, p.dims, (uint32_t)total, def_nan);          \
  } while (0)
  if (has_status) OLAP_ROWS(true);
  else OLAP_ROWS(false);
#undef OLAP_ROWS
  return hipGetLastError();
}

// prod(lens) over the dimensions `pick` selects (0 / 1 per dimension, nullptr: all); saturates instead of wrapping
uint64_t product_of(int ndim, const uint32_t *lens, const uint8_t *flags, bool want) {
  uint64_t n = 1;
  for (int d = 0; d < ndim; ++d) {
    if (flags && (flags[d] != 0) != want) continue;
    if (lens[d] != 0 && n > UINT64_MAX / lens[d]) return UINT64_MAX;
    n *= lens[d];
  }
  return n;
}

uint64_t blocks_byte_cap() {
  uint64_t cap = OLAP_BLOCKS_MAX_BYTES;
  if (const char *e = getenv("OLAP_BLOCKS_MAX_BYTES")) cap = std::min<uint64_t>(cap, strtoull(e, nullptr, 10));  // lowered only: the kernels index in 32 bits
  return cap;
}

// The arguments, refused on the host before any device work, in the order the header lists them.
int check_blocks(int n, const olap_store *const *stores, int ndim, const uint32_t *lens, const uint8_t *scanned, const double *host_values,
                 uint64_t *size, uint64_t *kept_cells) {
  int rc = check_list(n, stores && host_values, "store list is NULL");
  if (!rc) rc = check_entries(n, stores);
  if (rc) return rc;
  if (ndim < 0 || ndim > OLAP_MAX_DIMS) return fail(OLAP_ERR_INVALID_ARGUMENT, "ndim %d out of range [0, %d]", ndim, OLAP_MAX_DIMS);
  if (ndim > 0 && !lens) return fail(OLAP_ERR_INVALID_ARGUMENT, "dimension length vectors must not be NULL");
  if (ndim > 0 && !scanned) return fail(OLAP_ERR_INVALID_ARGUMENT, "scanned flags are NULL");
  bool any = false;
  for (int d = 0; d < ndim; ++d) any = any || scanned[d] != 0;
  if (!any) return fail(OLAP_ERR_INVALID_ARGUMENT, "blocks: no dimension is scanned");
  const uint64_t combos = product_of(ndim, lens, scanned, true), kept = product_of(ndim, lens, scanned, false);
  if (combos == 0 || kept == 0) return fail(OLAP_ERR_INVALID_ARGUMENT, "blocks: a dimension has no items");
  const uint64_t cells = product_of(ndim, lens, nullptr, true);
  if ((rc = check_cells(n, stores, cells))) return rc;
  for (int i = 1; i < n; ++i)
    if (stores[i]->device != stores[0]->device)
      return fail(OLAP_ERR_INVALID_ARGUMENT, "blocks: the stores live on different devices (%d and %d)", stores[0]->device, stores[i]->device);
  if ((rc = check_untracked(n, stores, "use the single-store call"))) return rc;
  const uint64_t cap = blocks_byte_cap();
  if (n > 0 && cells > cap / 8 / (uint64_t)n)
    return fail(OLAP_ERR_INVALID_ARGUMENT, "blocks: %d stores of %llu cells are more than the %llu bytes of one call", n, (unsigned long long)cells,
                (unsigned long long)cap);
  *size = cells;
  *kept_cells = kept;
  return OLAP_OK;
}

// one group (cell type T, one default, mask or none) in launches of up to kMaxBatch
template <typename T>
int run_group(const BlocksPlan &p, const olap_store *const *stores, const std::vector<int> &members, double *slab, uint64_t size, int *made) {
  const olap_store *s0 = stores[members[0]];
  const bool has_status = mask_is_primary(s0);
  const int def_nan = s0->default_kind == OLAP_DEFAULT_NAN;
  for (size_t first = 0; first < members.size(); first += kMaxBatch) {
    const unsigned nb = (unsigned)std::min<size_t>(members.size() - first, (size_t)kMaxBatch);
    Batch<T> b{};
    BlockSlots o{};
    const bool aligned16 = fill_chunk((int)nb, b.in, b.st_in, o.out, (int32_t **)nullptr, [&](int i) {
      const olap_store *s = stores[members[first + i]];
      return PairBuffers{s->values, has_status ? s->status : nullptr, slab + (uint64_t)members[first + i] * size, nullptr};
    });
    const hipError_t e = launch_blocks<T>(p, has_status, b, o, nb, size, aligned16, def_nan);
    if (e != hipSuccess) return hip_fail(e, "blocks_report");
    ++*made;
  }
  return OLAP_OK;
}

}  // namespace

extern "C" int olap_store_blocks_report(int n, const olap_store *const *stores, int ndim, const uint32_t *lens, const uint8_t *scanned,
                                        double *host_values, int *launches) {
  if (launches) *launches = 0;
  uint64_t size = 0, kept = 0;
  int rc = check_blocks(n, stores, ndim, lens, scanned, host_values, &size, &kept);
  if (rc) return rc;
  if (n == 0) return OLAP_OK;
  if ((rc = require_device())) return rc;
  OnStoreDevice on_device__(stores[0]);
  const BlocksPlan plan = plan_blocks(ndim, lens, scanned, kept);
  double *slab = nullptr;
  HIP_TRY(dev_alloc((void **)&slab, (uint64_t)n * size * sizeof(double)));
  int made = 0;
  rc = for_each_group(  // cell type and default decide whether a store keeps a mask
      n, [&](int i, int j) { return same_cells(stores[j], stores[i]); },
      [&](const std::vector<int> &members) {
        DISPATCH_DTYPE(stores[members[0]]->dtype, T, return run_group<T>(plan, stores, members, slab, size, &made));
      });
  hipError_t e = hipSuccess;
  if (!rc) e = hipMemcpy(host_values, slab, (uint64_t)n * size * sizeof(double), hipMemcpyDeviceToHost);  // the call's only wait
  else (void)hipStreamSynchronize(nullptr);  // launches already made still write the slab
  dev_free(slab);
  if (rc) return rc;
  if (e != hipSuccess) return hip_fail(e, "blocks_report");
  if (launches) *launches = made;
  return OLAP_OK;
}
