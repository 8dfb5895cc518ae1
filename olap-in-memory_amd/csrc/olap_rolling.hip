// olap_rolling.hip — K14: rolling-window aggregates along one dimension (Cube.rolling, Cube.shift).
//
// View [outer, K, inner] with one K -> G map (or none: one group).  The cell at item k holds what the reference's
// drillUp loop (in-memory.js:298-331) leaves after the members of k's window: items j in [k - before, k + after],
// clipped to [0, K), of k's group, in ascending order — Agg<METHOD> (olap_device.hpp) started afresh per window,
// finished (average) and converted to the cell type (emit_cell) once per output cell.  A window without members gives
// an unset cell.  No value leaves a window by subtraction and nothing re-associates: every window is folded from its
// first member.  Windows are independent, so there is one lane per output CELL; neighbouring windows share all but one
// row, so a workgroup stages the rows of its windows in LDS once.  Every output cell is written exactly once; there are
// no atomics and no state across workgroups.
//
//   tiled forms   a workgroup owns series x rows x cols output cells and stages input rows
//                 [k0 - before, k0 + rows - 1 + after] ∩ [0, K) of them with coalesced 16-byte loads (cell-aligned, the
//                 ragged last slot cell by cell), the mask too where it is primary.  Lanes take the tile's output cells
//                 with the innermost index fastest, fold their windows out of LDS into a second, output tile, and that
//                 leaves as 16-byte stores.
//     series      inner below four slots (e.g. the dimension is innermost): the tile is `series` series wide, a series'
//                 staged rows are one contiguous piece.  Lanes in step read consecutive tile cells within a series; the
//                 pitch between two series is congruent to the output piece modulo 32 cells, so the run continues on
//                 the next bank across a series border.
//     columns     wider rows: one series, `cols` cells of inner per tile row, pitch = cols: lanes in step read
//                 consecutive cells.
//   direct form   windows whose rows do not fit a tile: a lane folds its window straight from global memory, O(W)
//                 global reads per cell.  Correct and slow (include/olap_hip.h states the cliff).
//
// rolling_choose keeps rows >= the halo (before + after), so a tile stages at most twice its output rows: an input
// cell is read from global memory at most (rows + W - 1) / rows <= 2 times, and at most 1.25 times in the columns form
// wherever a tile width allows it.  The rule is read per pair (Batch<T>::method), uniformly for a workgroup.
#include <algorithm>

#include "olap_series.hpp"

using namespace olap;

namespace {

// The window of item k: members in ascending order through read(j, x, st) (st is preset to "set" for stores without a
// primary mask), folded as the drillUp loop folds them.
template <typename T, bool HS, int METHOD, typename Read>
__device__ __forceinline__ void fold_window(const RollingView &v, int64_t k, Read read, T &ov, int32_t &os) {
  const bool def_nan = v.def_nan != 0;
  const int64_t lo = k - v.before > 0 ? k - v.before : 0;
  const int64_t hi = k + v.after < (int64_t)v.K - 1 ? k + v.after : (int64_t)v.K - 1;
  const uint32_t *map = v.map;
  const uint32_t g = map ? map[k] : 0;
  // sum over a zero default without a mask: an unset cell holds 0, and the restart at 0 is invisible for addition, so
  // the plain float64 sum is the state and the cell is set iff it does not convert to 0 (as K13's running_step)
  constexpr bool kPlainSum = METHOD == OLAP_SUM && !HS;
  Agg<METHOD> a;
  a.init();
  for (int64_t j = lo; j <= hi; ++j) {
    if (map && map[j] != g) continue;
    T x;
    int32_t st = OLAP_STATUS_SET;
    read(j, x, st);
    if (kPlainSum && !def_nan) a.acc += Cell<T>::to_f64(x);
    else if (cell_is_set<T>(x, st, HS, def_nan)) a.add(Cell<T>::to_f64(x), def_nan);
  }
  if (kPlainSum && !def_nan) a.has = true;  // (emit_cell drops a sum that converts to 0)
  a.finish(def_nan);
  emit_cell<T>(a.acc, a.has, def_nan, ov, os);
}

// ---------------------------------------------------------------- tiled forms
template <typename T, bool HS, int METHOD>
__device__ __forceinline__ void tiles_walk(T *tin, int32_t *sin, T *tout, int32_t *sout, const T *__restrict__ in, const int32_t *__restrict__ st_in,
                                           T *__restrict__ out, int32_t *__restrict__ st_out, const RollingView &v, const uint64_t n_tiles) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const bool columns = v.form == ROLLING_COLUMNS;
  const uint32_t inner = (uint32_t)v.inner;
  const uint64_t series_cells = v.K * v.inner;
  const uint64_t tiles_c = (v.inner + v.cols - 1) / v.cols, tiles_k = (v.K + v.rows - 1) / v.rows;
  // a tile cell (series s, row r, column c) lies at s * p_s + r * p_r + c
  const uint32_t in_s = columns ? 0 : v.pitch, in_r = columns ? v.pitch : inner;
  const uint32_t out_s = columns ? 0 : v.rows * inner, out_r = columns ? v.cols : inner;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t s0 = (tile / (tiles_c * tiles_k)) * v.series, k0 = ((tile / tiles_c) % tiles_k) * v.rows, c0 = (tile % tiles_c) * v.cols;
    const uint32_t ns = (uint32_t)(v.outer - s0 < v.series ? v.outer - s0 : v.series);
    const uint32_t nr = (uint32_t)(v.K - k0 < v.rows ? v.K - k0 : v.rows);
    const uint32_t nc = (uint32_t)(v.inner - c0 < v.cols ? v.inner - c0 : v.cols);
    // input rows [klo, khi] of the tile's windows; none when the windows lie off the dimension altogether
    const int64_t klo = (int64_t)k0 - v.before > 0 ? (int64_t)k0 - v.before : 0;
    const int64_t khi = (int64_t)(k0 + nr) - 1 + v.after < (int64_t)v.K - 1 ? (int64_t)(k0 + nr) - 1 + v.after : (int64_t)v.K - 1;
    if (khi >= klo) {
      const uint32_t nri = (uint32_t)(khi - klo + 1);
      const uint64_t first = s0 * series_cells + (uint64_t)klo * inner + c0;
      const uint32_t pieces = columns ? nri : ns, seg = columns ? nc : nri * inner;
      const uint64_t stride = columns ? v.inner : series_cells;
      tile_move<T, VEC, true>(tin, in, nullptr, first, stride, pieces, seg, v.pitch);
      if constexpr (HS) tile_move<int32_t, 4, true>(sin, st_in, nullptr, first, stride, pieces, seg, v.pitch);
    }
    __syncthreads();
    for (uint32_t it = threadIdx.x; it < ns * nr * nc; it += kBlock) {
      const uint32_t c = it % nc, r = (it / nc) % nr, s = it / (nc * nr);
      const T *col = tin + s * in_s + c;
      const int32_t *scol = sin + s * in_s + c;
      const uint32_t at = s * out_s + r * out_r + c;
      T ov;
      int32_t os;
      fold_window<T, HS, METHOD>(
          v, (int64_t)(k0 + r),
          [&](int64_t j, T &x, int32_t &st) {
            const uint32_t row = (uint32_t)(j - klo) * in_r;
            x = col[row];
            if constexpr (HS) st = scol[row];
          },
          ov, os);
      tout[at] = ov;
      if constexpr (HS) sout[at] = os;
    }
    __syncthreads();
    {
      const uint64_t first = s0 * series_cells + k0 * inner + c0;
      const uint32_t pieces = columns ? nr : ns, seg = columns ? nc : nr * inner;
      const uint64_t stride = columns ? v.inner : series_cells;
      const uint32_t pitch = columns ? v.cols : v.rows * inner;
      tile_move<T, VEC, false>(tout, nullptr, out, first, stride, pieces, seg, pitch);
      if constexpr (HS) tile_move<int32_t, 4, false>(sout, nullptr, st_out, first, stride, pieces, seg, pitch);
    }
    __syncthreads();  // the next tile overwrites what is being stored
  }
}

template <typename T, bool HS>
__global__ __launch_bounds__(kBlock) void rolling_tiled_kernel(const Batch<T> b, const RollingView v, const uint64_t n_tiles) {
  __shared__ T tin[kRollingInBytes / sizeof(T)];
  __shared__ T tout[kRollingOutBytes / sizeof(T)];
  __shared__ int32_t sin[HS ? kRollingInBytes / sizeof(T) : 1];
  __shared__ int32_t sout[HS ? kRollingOutBytes / sizeof(T) : 1];
  const uint32_t p = blockIdx.y;
  SERIES_RULE(b.method[p], (tiles_walk<T, HS, M>(tin, sin, tout, sout, b.in[p], b.st_in[p], b.out[p], b.st_out[p], v, n_tiles)));
}

// ---------------------------------------------------------------- direct form
template <typename T, bool HS, int METHOD>
__device__ __forceinline__ void direct_walk(const T *__restrict__ in, const int32_t *__restrict__ st_in, T *__restrict__ out,
                                            int32_t *__restrict__ st_out, const RollingView &v, const uint64_t cells) {
  for (uint64_t cell = (uint64_t)blockIdx.x * kBlock + threadIdx.x; cell < cells; cell += (uint64_t)gridDim.x * kBlock) {
    const uint64_t i = cell % v.inner, k = (cell / v.inner) % v.K, o = cell / (v.inner * v.K);
    const uint64_t base = o * v.K * v.inner + i;
    T ov;
    int32_t os;
    fold_window<T, HS, METHOD>(
        v, (int64_t)k,
        [&](int64_t j, T &x, int32_t &st) {
          x = in[base + (uint64_t)j * v.inner];
          if constexpr (HS) st = st_in[base + (uint64_t)j * v.inner];
        },
        ov, os);
    out[cell] = ov;
    if constexpr (HS) st_out[cell] = os;
  }
}

template <typename T, bool HS>
__global__ __launch_bounds__(kBlock) void rolling_direct_kernel(const Batch<T> b, const RollingView v, const uint64_t cells) {
  const uint32_t p = blockIdx.y;
  SERIES_RULE(b.method[p], (direct_walk<T, HS, M>(b.in[p], b.st_in[p], b.out[p], b.st_out[p], v, cells)));
}

template <typename T, bool HS>
hipError_t launch_typed(int nb, const int *methods, const void *const *in, const int32_t *const *st_in, void *const *out, int32_t *const *st_out,
                        const RollingView &v, hipStream_t stream) {
  Batch<T> b{};
  for (int k = 0; k < nb; ++k) {
    b.in[k] = (const T *)in[k], b.st_in[k] = HS ? st_in[k] : nullptr;
    b.out[k] = (T *)out[k], b.st_out[k] = HS ? st_out[k] : nullptr;
    b.method[k] = methods[k];
  }
  if (v.form == ROLLING_DIRECT) {
    const uint64_t cells = v.outer * v.K * v.inner;
    const uint64_t blocks = (cells + kBlock - 1) / kBlock;
    const dim3 grid((unsigned)std::min<uint64_t>(blocks, series_max_grid("OLAP_ROLLING_GRID", 1u << 22)), (unsigned)nb);
    rolling_direct_kernel<T, HS><<<grid, kBlock, 0, stream>>>(b, v, cells);
  } else {
    const uint64_t n_tiles = ((v.outer + v.series - 1) / v.series) * ((v.K + v.rows - 1) / v.rows) * ((v.inner + v.cols - 1) / v.cols);
    const dim3 grid((unsigned)std::min<uint64_t>(n_tiles, series_max_grid("OLAP_ROLLING_GRID", 1u << 20)), (unsigned)nb);
    rolling_tiled_kernel<T, HS><<<grid, kBlock, 0, stream>>>(b, v, n_tiles);
  }
  return hipGetLastError();
}

}  // namespace

void rolling_choose(RollingView &v, int cell_bytes) {
  const uint64_t in_cells = kRollingInBytes / (uint32_t)cell_bytes, out_cells = kRollingOutBytes / (uint32_t)cell_bytes;
  const uint64_t slot = 16u / (uint32_t)cell_bytes;
  const uint64_t halo = (uint64_t)(v.before + v.after);  // W - 1: the input rows a tile stages beyond its output rows
  v.form = ROLLING_DIRECT;
  v.series = v.rows = v.cols = v.pitch = 0;
  if (v.outer == 0 || v.K == 0 || v.inner == 0) return;
  const auto staged = [&](uint64_t rows) { return std::min(rows + halo, v.K); };
  const auto take = [&](int form, uint64_t series, uint64_t rows, uint64_t cols, uint64_t pitch) {
    v.form = form;
    v.series = (uint32_t)series, v.rows = (uint32_t)rows, v.cols = (uint32_t)cols, v.pitch = (uint32_t)pitch;
  };
  if (v.inner >= 4 * slot) {
    // columns: the widest tile row (at most 1 KiB) whose rows keep the halo below a quarter of them; failing that the
    // narrowest one (four slots) if its rows are at least the halo
    for (uint64_t cols = std::min(v.inner, 64 * slot);; cols = std::max(cols / 2, 4 * slot)) {
      const bool narrowest = cols == 4 * slot;
      uint64_t rows = std::min(v.K, out_cells / cols);
      if (staged(rows) * cols > in_cells) rows = in_cells / cols > halo ? in_cells / cols - halo : 0;
      if (rows >= 1 && (staged(rows) * 4 <= rows * 5 || (narrowest && staged(rows) <= 2 * rows))) return take(ROLLING_COLUMNS, 1, rows, cols, cols);
      if (narrowest) return;
    }
  }
  const uint64_t row = v.inner;
  if (v.K * row <= out_cells) {  // whole series: nothing is staged twice
    return take(ROLLING_SERIES, std::min(out_cells / (v.K * row), v.outer), v.K, row, v.K * row);
  }
  // chunks of series: pieces of at least 256 output cells per series where there are that many series, else one series
  for (const uint64_t series : {std::min(v.outer, out_cells / 256), (uint64_t)1}) {
    const uint64_t room = in_cells / series;  // cells of the input tile per series, the pad (below 32) included
    uint64_t rows = std::min(v.K, out_cells / (series * row));
    const uint64_t most = (room - 31) / row;  // staged rows that fit whatever the pad
    if (staged(rows) > most) rows = most > halo ? most - halo : 0;
    if (rows < 1 || staged(rows) > 2 * rows) continue;
    // lanes in step read consecutive cells of a series, rows * row of them: the next series starts where that run ends, modulo 32 banks
    const uint64_t least = staged(rows) * row;
    return take(ROLLING_SERIES, series, rows, row, least + (rows * row % 32 + 32 - least % 32) % 32);
  }
}

hipError_t launch_rolling(int dtype, bool has_status, int nb, const int *methods, const void *const *in, const int32_t *const *st_in,
                          void *const *out, int32_t *const *st_out, const RollingView &v, hipStream_t stream) {
  if (nb < 1 || nb > kMaxBatch) return hipErrorInvalidValue;
  if (v.outer == 0 || v.K == 0 || v.inner == 0) return hipSuccess;
  return series_cell_type(dtype, has_status, [&](auto cell, auto hs) {
    return launch_typed<decltype(cell), decltype(hs)::value>(nb, methods, in, st_in, out, st_out, v, stream);
  });
}
