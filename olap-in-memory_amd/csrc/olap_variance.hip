// olap_variance.hip — K16: dispersion along one dimension (Cube.variance, Cube.stddev).
//
// View [outer, K, inner] with one K -> G map; the result is [outer, G, inner].  An output cell holds the variance (kind
// 1: its square root) of the SET cells of its group, two passes, Cube._varianceHost is the definition:
//   s = v[0]; s += v[k];  mean = s / n;  m2 += (v[k] - mean) * (v[k] - mean);  r = m2 / (n - ddof)
// in float64, the members in ascending item order, every operation rounded on its own (nothing fuses: JS has no FMA).
// Never E[x^2] - E[x]^2.
//
//   column form    inner of four slots or more (or a narrower one whose series is beyond a tile): a workgroup stages the
//                  rows of a run of whole groups for a slice of `inner` into LDS once (tile_move; tile row j is member j
//                  of the CSR, so interleaved groups lie together in the tile, in item order) and one lane per output
//                  cell (group, column) folds twice out of LDS.  Lanes of a wave hold neighbouring columns: staging,
//                  LDS reads and the result's stores are all coalesced.
//   row form       inner below four slots: a workgroup stages whole series (K * inner contiguous cells each, odd pitch
//                  between two series), one lane per (series, group, i).
//   direct, lanes  a group larger than a tile: a lane per output cell walks its group twice straight from device memory,
//                  neighbouring lanes neighbouring cells of inner (coalesced where inner allows; the second walk is
//                  served by L2 / the Infinity Cache where the group's rows fit).
//   direct, block  few output cells with long groups: a workgroup per output cell.  Lane t folds the members j0 + t,
//                  j0 + t + 256, ... in ascending order, the 256 partial sums are added by a tree of FIXED shape (xor
//                  butterfly within a wave, then the four waves in order), first for the sum, then for m2.
//                  This is the one RE-ASSOCIATED form (as K1r is for drillUp): its float64 additions are grouped
//                  differently from the definition's, so its result may differ from the definition's in the last bits
//                  (within the two-pass bound, header); the shape of the tree depends on the plan alone, never on
//                  timing, so a second run gives the same bytes.  The three one-lane forms equal the definition bit
//                  for bit.
//
// No atomics, no state across workgroups; every output cell is written exactly once and the inputs are only read.
// kind and ddof are launch arguments: plans do not depend on them.
#include <cstring>

#include "olap_series.hpp"

using namespace olap;

namespace {

// ---------------------------------------------------------------- the members of one output cell
// Member j in [j0, j1) lies at base + (order ? order[j] : j) * stride of v (and of s, the mask, where it is primary).
// BLOCK: the 256 lanes of a workgroup share both walks; every lane of the workgroup must then come here, and every lane
// gets the answer.
template <typename T, bool HS, typename IDX, bool BLOCK>
struct Walk {
  const T *v;
  const int32_t *s;
  const uint32_t *order;
  IDX base, stride;
  uint32_t j0, j1;
  bool def_nan;

  __device__ __forceinline__ bool get(uint64_t j, double &x) const {
    const IDX at = base + (IDX)(order ? order[j] : (uint32_t)j) * stride;
    const T c = v[at];
    const int32_t st = HS ? s[at] : OLAP_STATUS_SET;
    x = Cell<T>::to_f64(c);
    return cell_is_set<T>(c, st, HS, def_nan);
  }
  // f(x) for every set member this lane looks at, in ascending item order
  template <typename F>
  __device__ __forceinline__ void each(F f) const {
#pragma unroll 4
    for (uint64_t j = (uint64_t)j0 + (BLOCK ? threadIdx.x : 0u); j < j1; j += (BLOCK ? kBlock : 1u)) {
      double x;
      if (get(j, x)) f(x);
    }
  }
  // BLOCK: the workgroup's sum of the lanes' partial sums and member counts, by a tree of fixed shape — the butterfly
  // gives every lane of a wave the same bits (a + b == b + a), the waves are added in order.  A lane without a member
  // holds +0 and count 0; it takes part like any other (x + 0 == x but for -0 + 0 == +0, which the folds do not tell apart)
  __device__ __forceinline__ void across(double &x, uint32_t &c) const {
    if constexpr (BLOCK) {
      __shared__ double part[kBlock / 64];
      __shared__ uint32_t count[kBlock / 64];
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        x = x + __shfl_xor(x, d, 64);
        c += __shfl_xor(c, d, 64);
      }
      if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x, count[threadIdx.x >> 6] = c;
      __syncthreads();
      x = part[0], c = count[0];
#pragma unroll
      for (int w = 1; w < kBlock / 64; ++w) x = x + part[w], c += count[w];
      __syncthreads();  // the next fold writes part[] again
    }
  }
};

// One output cell.  The arithmetic is Cube._varianceHost's, operation by operation.
template <typename T, typename W>
__device__ __forceinline__ void variance_cell(const W &w, int kind, int ddof, bool def_nan, T &ov, int32_t &os) {
#pragma clang fp contract(off)
  uint32_t n = 0;
  double s = 0.0;
  w.each([&](double x) {
    s = n ? s + x : x;
    ++n;
  });
  w.across(s, n);
  if (n <= (uint32_t)ddof) {
    emit_cell<T>(0.0, false, def_nan, ov, os);
    return;
  }
  const double mean = s / (double)n;
  double m2 = 0.0;
  uint32_t seen = 0;
  w.each([&](double x) {
    const double d = x - mean;
    const double p = d * d;
    m2 = m2 + p;
  });
  w.across(m2, seen);
  double r = m2 / (double)(n - (uint32_t)ddof);
  if (kind) r = sqrt(r);
  if (r != r) r = __builtin_nan("");  // one NaN, whatever the arithmetic made of its operands' payloads
  emit_cell<T>(r, true, def_nan, ov, os);
}

template <typename T, bool HS>
struct Tile {
  static constexpr uint32_t kCells = kVarianceTileBytes / (uint32_t)(sizeof(T) + (HS ? 4 : 0));
  static constexpr uint32_t kAlloc = kCells + 256;  // + one pad cell per series of the row form (at most 256 series per tile)
};

// ---------------------------------------------------------------- column form
template <typename T, bool HS>
__global__ __launch_bounds__(kBlock) void variance_column_kernel(const Batch<T> b, const VarianceView v, const int kind, const int ddof,
                                                                 const uint64_t n_work) {
  constexpr int VEC = 16 / (int)sizeof(T);
  __shared__ T tv[Tile<T, HS>::kAlloc];
  __shared__ int32_t ts[HS ? Tile<T, HS>::kAlloc : 1];
  const uint32_t p = blockIdx.y;
  const T *__restrict__ in = b.in[p];
  const int32_t *__restrict__ st_in = b.st_in[p];
  T *__restrict__ out = b.out[p];
  int32_t *__restrict__ st_out = b.st_out[p];
  const bool def_nan = v.def_nan != 0;
  const uint64_t slices = (v.inner + v.cols - 1) / v.cols;
  for (uint64_t work = blockIdx.x; work < n_work; work += gridDim.x) {
    const uint64_t slice = work % slices, t = (work / slices) % v.n_gtile, o = work / (slices * v.n_gtile);
    const uint32_t g0 = v.gtile[t], g1 = v.gtile[t + 1];
    const uint32_t ja = v.gstart[g0], rows = v.gstart[g1] - ja;  // rows * cols <= v.tile <= kCells (group_tiles, olap_plan_along.hip)
    const uint64_t c0 = slice * v.cols;
    const uint32_t nc = (uint32_t)(v.inner - c0 < v.cols ? v.inner - c0 : v.cols);
    const uint64_t first = o * v.K * v.inner + c0 + (v.order ? 0 : (uint64_t)ja * v.inner);
    const uint32_t *piece = v.order ? v.order + ja : nullptr;
    tile_move<T, VEC, true>(tv, in, nullptr, first, v.inner, rows, nc, v.cols, piece);
    if constexpr (HS) tile_move<int32_t, 4, true>(ts, st_in, nullptr, first, v.inner, rows, nc, v.cols, piece);
    __syncthreads();
    const uint32_t cells = (g1 - g0) * nc;
    for (uint32_t it = threadIdx.x; it < cells; it += kBlock) {
      const uint32_t c = it % nc, g = g0 + it / nc;
      const Walk<T, HS, uint32_t, false> w{tv, ts, nullptr, c, v.cols, v.gstart[g] - ja, v.gstart[g + 1] - ja, def_nan};
      T ov;
      int32_t os;
      variance_cell<T>(w, kind, ddof, def_nan, ov, os);
      const uint64_t at = (o * v.G + g) * v.inner + c0 + c;
      out[at] = ov;
      if constexpr (HS) st_out[at] = os;
    }
    __syncthreads();  // the next tile overwrites what is being read
  }
}

// ---------------------------------------------------------------- row form
template <typename T, bool HS>
__global__ __launch_bounds__(kBlock) void variance_rows_kernel(const Batch<T> b, const VarianceView v, const int kind, const int ddof,
                                                               const uint64_t n_tiles) {
  constexpr int VEC = 16 / (int)sizeof(T);
  __shared__ T tv[Tile<T, HS>::kAlloc];
  __shared__ int32_t ts[HS ? Tile<T, HS>::kAlloc : 1];
  const uint32_t p = blockIdx.y;
  const T *__restrict__ in = b.in[p];
  const int32_t *__restrict__ st_in = b.st_in[p];
  T *__restrict__ out = b.out[p];
  int32_t *__restrict__ st_out = b.st_out[p];
  const bool def_nan = v.def_nan != 0;
  const uint32_t inner = (uint32_t)v.inner, G = (uint32_t)v.G;
  const uint32_t series_cells = (uint32_t)(v.K * v.inner);  // <= v.tile
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t s0 = tile * v.series;
    const uint32_t ns = (uint32_t)(v.outer - s0 < v.series ? v.outer - s0 : v.series);  // ns * pitch <= v.tile + 256 <= kAlloc
    tile_move<T, VEC, true>(tv, in, nullptr, s0 * series_cells, series_cells, ns, series_cells, v.pitch);
    if constexpr (HS) tile_move<int32_t, 4, true>(ts, st_in, nullptr, s0 * series_cells, series_cells, ns, series_cells, v.pitch);
    __syncthreads();
    const uint64_t cells = (uint64_t)ns * G * inner;  // (G may exceed K: group ids nobody maps to)
    for (uint64_t it = threadIdx.x; it < cells; it += kBlock) {
      const uint32_t i = (uint32_t)(it % inner), g = (uint32_t)((it / inner) % G), s = (uint32_t)(it / ((uint64_t)inner * G));
      const Walk<T, HS, uint32_t, false> w{tv, ts, v.order, s * v.pitch + i, inner, v.gstart[g], v.gstart[g + 1], def_nan};
      T ov;
      int32_t os;
      variance_cell<T>(w, kind, ddof, def_nan, ov, os);
      const uint64_t at = s0 * G * inner + it;
      out[at] = ov;
      if constexpr (HS) st_out[at] = os;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- direct forms
template <typename T, bool HS, bool BLOCK>
__global__ __launch_bounds__(kBlock) void variance_direct_kernel(const Batch<T> b, const VarianceView v, const int kind, const int ddof,
                                                                 const uint64_t cells) {
  const uint32_t p = blockIdx.y;
  const T *in = b.in[p];
  const int32_t *st_in = b.st_in[p];
  T *__restrict__ out = b.out[p];
  int32_t *__restrict__ st_out = b.st_out[p];
  const bool def_nan = v.def_nan != 0;
  const uint64_t first = BLOCK ? blockIdx.x : (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t step = BLOCK ? gridDim.x : (uint64_t)gridDim.x * kBlock;
  for (uint64_t it = first; it < cells; it += step) {  // (BLOCK: `it` is the workgroup's, the loop uniform)
    const uint64_t i = it % v.inner, g = (it / v.inner) % v.G, o = it / (v.inner * v.G);
    const Walk<T, HS, uint64_t, BLOCK> w{in, st_in, v.order, o * v.K * v.inner + i, v.inner, v.gstart[g], v.gstart[g + 1], def_nan};
    T ov;
    int32_t os;
    variance_cell<T>(w, kind, ddof, def_nan, ov, os);
    if (!BLOCK || threadIdx.x == 0) {
      out[it] = ov;
      if constexpr (HS) st_out[it] = os;
    }
  }
}

template <typename T, bool HS>
hipError_t launch_typed(int nb, const void *const *in, const int32_t *const *st_in, void *const *out, int32_t *const *st_out, const VarianceView &v,
                        int kind, int ddof, hipStream_t stream) {
  if (v.tile > Tile<T, HS>::kCells) return hipErrorInvalidValue;  // the tile the cuts were made for does not fit this kernel's
  Batch<T> b{};
  for (int k = 0; k < nb; ++k) {
    b.in[k] = (const T *)in[k], b.st_in[k] = HS ? st_in[k] : nullptr;
    b.out[k] = (T *)out[k], b.st_out[k] = HS ? st_out[k] : nullptr;
  }
  const uint64_t cells = v.outer * v.G * v.inner;
  auto grid = [&](uint64_t want) { return dim3((unsigned)(want < series_max_grid("OLAP_VARIANCE_GRID", 1u << 20) ? want : series_max_grid("OLAP_VARIANCE_GRID", 1u << 20)), (unsigned)nb); };
  switch (v.form) {
    case VARIANCE_COLUMN: {
      const uint64_t n_work = v.outer * v.n_gtile * ((v.inner + v.cols - 1) / v.cols);
      variance_column_kernel<T, HS><<<grid(n_work), kBlock, 0, stream>>>(b, v, kind, ddof, n_work);
      break;
    }
    case VARIANCE_ROW: {
      const uint64_t n_tiles = (v.outer + v.series - 1) / v.series;
      variance_rows_kernel<T, HS><<<grid(n_tiles), kBlock, 0, stream>>>(b, v, kind, ddof, n_tiles);
      break;
    }
    case VARIANCE_DIRECT_LANES:
      variance_direct_kernel<T, HS, false><<<grid((cells + kBlock - 1) / kBlock), kBlock, 0, stream>>>(b, v, kind, ddof, cells);
      break;
    default:
      variance_direct_kernel<T, HS, true><<<grid(cells), kBlock, 0, stream>>>(b, v, kind, ddof, cells);
      break;
  }
  return hipGetLastError();
}

}  // namespace

uint32_t variance_tile_cells(int cell_bytes, bool has_mask) {
  const uint32_t most = kVarianceTileBytes / (uint32_t)(cell_bytes + (has_mask ? 4 : 0));
  const unsigned long n = env_number("OLAP_VARIANCE_TILE");
  return n >= 1 && n < most ? (uint32_t)n : most;
}

// OLAP_VARIANCE_BLOCK=members[,cells] (a developer knob, NOTEBOOK) moves the cut of the workgroup form
uint32_t variance_block_members() {
  const unsigned long n = env_number("OLAP_VARIANCE_BLOCK");
  return n >= 1 && n <= 0xFFFFFFFFul ? (uint32_t)n : kVarianceBlockMembers;
}

uint32_t variance_block_cells() {
  const char *e = getenv("OLAP_VARIANCE_BLOCK");
  const char *comma = e ? strchr(e, ',') : nullptr;
  const unsigned long n = comma ? strtoul(comma + 1, nullptr, 10) : 0;
  return n >= 1 && n <= 0xFFFFFFFFul ? (uint32_t)n : kVarianceBlockCells;
}

void variance_choose(VarianceView &v, int cell_bytes) {
  const uint32_t slot = 16u / (uint32_t)cell_bytes;
  v.series = v.pitch = v.cols = v.rows = v.n_gtile = 0;
  const uint64_t cells = v.outer * v.G * v.inner;
  // Few output cells with long groups: a lane per output cell leaves the device idle while each lane walks its whole
  // group alone, whether out of a tile or not; a workgroup per output cell shares the walk (the re-associated form;
  // the crossover: DESIGN K16).  Every other shape takes a one-lane form and equals the definition bit for bit.
  if (cells <= v.block_cells && v.longest >= v.block_members) {
    v.form = VARIANCE_DIRECT_BLOCK;
    return;
  }
  const uint64_t series_cells = v.K * v.inner;
  if (v.inner < 4 * slot && series_cells <= v.tile) {
    // rows of fewer than four slots, as cumulate's row form: whole series, as many as fit
    v.form = VARIANCE_ROW;
    const uint64_t fit = v.tile / (series_cells ? series_cells : 1);
    v.series = (uint32_t)(fit < 256 ? fit : 256);
    v.pitch = (uint32_t)series_cells | 1u;
    return;
  }
  // a tile must hold the largest group one slot wide (the whole row, where that is narrower)
  const uint64_t least = v.inner < slot ? v.inner : slot;
  if ((uint64_t)v.longest * least > v.tile) {
    v.form = VARIANCE_DIRECT_LANES;  // (groups this long with few output cells left above)
    return;
  }
  // Column form.  Rows of fewer than four slots whose series is beyond a tile come here too, the whole row a slice:
  // with contiguous groups the rows of a tile are one run of device memory
  v.form = VARIANCE_COLUMN;
  const uint64_t fit = v.tile / (v.longest ? v.longest : 1);  // >= least
  uint64_t cols = v.inner < 256 ? v.inner : 256;
  if (cols > fit) cols = fit;
  // slices start on whole slots of the row (a tile below one slot — the knob, and a dimension without items — keeps its cells)
  if (cols < v.inner && cols >= slot) cols -= cols % slot;
  v.cols = (uint32_t)cols;
  v.rows = v.tile / v.cols;  // >= longest
}

hipError_t launch_variance(int dtype, bool has_status, int nb, const void *const *in, const int32_t *const *st_in, void *const *out,
                           int32_t *const *st_out, const VarianceView &v, int kind, int ddof, hipStream_t stream) {
  if (nb < 1 || nb > kMaxBatch) return hipErrorInvalidValue;
  if (v.outer == 0 || v.G == 0 || v.inner == 0) return hipSuccess;
  return series_cell_type(dtype, has_status, [&](auto cell, auto hs) {
    return launch_typed<decltype(cell), decltype(hs)::value>(nb, in, st_in, out, st_out, v, kind, ddof, stream);
  });
}
