// olap_cumulate.hip — K13: running aggregates along one dimension (Cube.cumulate).
//
// View [outer, K, inner] with one K -> G map.  The cell at item k holds the state of the reference's drillUp loop
// (in-memory.js:298-331) over the members of k's group at positions <= k: Agg<METHOD> (olap_device.hpp) after each
// contribution instead of only after the last one, finished (average) and converted to the cell type (emit_cell) on a
// COPY of the state, once per output cell.  Every series-and-group is walked sequentially, ascending, by ONE lane:
// float64 addition does not re-associate, so there is no parallel prefix scan here, no atomics and no state that
// crosses workgroups.  Parallelism comes from outer x G x inner and from independent row loads in flight ahead of the
// dependent fold.  Every output cell is written exactly once.
//
//   column form   a lane owns one 16-byte slot of `inner` for one (outer, group), walks the group's rows ascending
//                 with one state per cell of the slot and writes each row's running cells as it goes; lanes of a wave
//                 hold neighbouring slots, so loads and stores are coalesced streams.  Rows need not be whole slots:
//                 accesses are cell-aligned and the last slot of a ragged row goes cell by cell.  With one-cell slots
//                 it is also the (uncoalesced) form of long series with interleaved groups.
//   row form      inner below four slots (e.g. the dimension is innermost): a series is K * inner contiguous cells.  A
//                 workgroup stages `series` series into LDS with coalesced 16-byte loads, one lane per
//                 (series, group, i) walks its members in LDS and writes the running cells back in place, and the
//                 tile leaves as coalesced 16-byte stores.  The pitch between two series is odd, so lanes that walk
//                 different series in step hit different banks.  A series longer than one tile (contiguous groups or
//                 one group only) is cut into chunks of `rows` rows; lane (series, i) walks all groups in turn and
//                 carries its state in registers from chunk to chunk.
//
// All rules use Agg<> in float64: for highest / lowest / first / last the round trip through float64 is exact for
// every cell type and emit_cell keeps such a value as it is, so the result equals Pick<>'s.  The rule is read per
// pair (Batch<T>::method), uniformly for a workgroup: measures with different rules share a launch.
#include "olap_series.hpp"

using namespace olap;

namespace {

constexpr int kRowsAhead = 8;  // row form: cells a lane reads from the tile ahead of the dependent fold
constexpr uint32_t kTileAlloc = kCumulateTileCells + 256;  // + one pad cell per series (at most 256 series per tile)

// One position of a series: the input cell (x, s) contributes if it is set; (x, s) leave as the running cell.
template <typename T, int METHOD, bool HS>
__device__ __forceinline__ void running_step(Agg<METHOD> &a, T &x, int32_t &s, bool def_nan) {
  if constexpr (METHOD == OLAP_SUM && !HS) {
    if (!def_nan) {
      // sum over a zero default without a mask, as K1's FAST lanes: an unset cell holds 0 and adding it changes nothing, and
      // "restart when the running sum hits 0" is invisible for addition (the sum since the restart IS the sum), so the plain
      // float64 running sum is the state and the cell is set iff it does not convert to 0.  A step is a handful of
      // instructions instead of the state machine's few dozen, which is what the row form's time is made of (NOTEBOOK).
      a.acc += Cell<T>::to_f64(x);
      const T tv = Cell<T>::from_f64(a.acc);
      const bool set = !Cell<T>::is_default(tv, false);
      x = set ? tv : Cell<T>::default_value(false);
      s = set ? OLAP_STATUS_SET : 0;
      return;
    }
  }
  if (cell_is_set<T>(x, s, HS, def_nan)) a.add(Cell<T>::to_f64(x), def_nan);
  Agg<METHOD> f = a;  // average divides a copy: the running sum itself is never rounded or divided
  f.finish(def_nan);
  emit_cell<T>(f.acc, f.has, def_nan, x, s);
}

// ---------------------------------------------------------------- column form
template <typename T, bool HS, int VEC, int METHOD>
__device__ __forceinline__ void column_walk(const T *__restrict__ in, const int32_t *__restrict__ st_in, T *__restrict__ out,
                                            int32_t *__restrict__ st_out, const CumulateView &v, const uint64_t items) {
  constexpr int U = 4;  // rows in flight per lane ahead of the dependent fold
  const bool def_nan = v.def_nan != 0;
  const uint64_t n_slots = (v.inner + VEC - 1) / VEC;
  for (uint64_t item = (uint64_t)blockIdx.x * kBlock + threadIdx.x; item < items; item += (uint64_t)gridDim.x * kBlock) {
    const uint64_t slot = item % n_slots, t = item / n_slots;
    const uint64_t g = t % v.G, o = t / v.G;
    const uint64_t c0 = slot * VEC;
    const int n = (int)(v.inner - c0 < (uint64_t)VEC ? v.inner - c0 : (uint64_t)VEC);
    const uint64_t base = o * v.K * v.inner + c0;
    const uint32_t j1 = v.gstart[g + 1];
    Agg<METHOD> a[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) a[e].init();
    for (uint32_t j = v.gstart[g]; j < j1; j += U) {
      Vec<T, VEC> x[U];
      Vec<int32_t, VEC> s[U];
      uint64_t at[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (j + u < j1) {
          const uint64_t k = v.order ? v.order[j + u] : j + u;
          at[u] = base + k * v.inner;
          x[u] = load_slot<T, VEC>(in + at[u], n);
          if constexpr (HS) s[u] = load_slot<int32_t, VEC>(st_in + at[u], n);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (j + u < j1) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            if constexpr (!HS) s[u].v[e] = OLAP_STATUS_SET;
            running_step<T, METHOD, HS>(a[e], x[u].v[e], s[u].v[e], def_nan);
          }
          store_slot<T, VEC>(out + at[u], x[u], n);
          if constexpr (HS) store_slot<int32_t, VEC>(st_out + at[u], s[u], n);
        }
      }
    }
  }
}

template <typename T, bool HS, int VEC>
__global__ __launch_bounds__(kBlock) void cumulate_column_kernel(const Batch<T> b, const CumulateView v, const uint64_t items) {
  const uint32_t p = blockIdx.y;
  SERIES_RULE(b.method[p], (column_walk<T, HS, VEC, M>(b.in[p], b.st_in[p], b.out[p], b.st_out[p], v, items)));
}

// ---------------------------------------------------------------- row form
// (tile_move, olap_series.hpp, moves rows [k0, k0 + rows) of `ns` series between global memory and the tile: a series'
// piece is rows * inner contiguous cells)

// whole series in the tile: one lane per (series, group, i) walks the group's members
template <typename T, bool HS, int METHOD>
__device__ __forceinline__ void rows_walk_whole(T *tv, int32_t *ts, const CumulateView &v, uint32_t ns) {
  const bool def_nan = v.def_nan != 0;
  const uint32_t inner = (uint32_t)v.inner, G = (uint32_t)v.G;
  const uint64_t items = (uint64_t)ns * G * inner;  // (G may exceed K: group ids nobody maps to)
  for (uint64_t it = threadIdx.x; it < items; it += kBlock) {
    const uint32_t i = (uint32_t)(it % inner), g = (uint32_t)((it / inner) % G), s = (uint32_t)(it / ((uint64_t)inner * G));
    const uint32_t j1 = v.gstart[g + 1];
    Agg<METHOD> a;
    a.init();
    const uint32_t base = s * v.pitch + i;
    for (uint32_t j = v.gstart[g]; j < j1; j += kRowsAhead) {
      // the reads of kRowsAhead members first: behind a write to the tile the compiler would wait for each in turn
      T x[kRowsAhead];
      int32_t st[kRowsAhead];
      uint32_t at[kRowsAhead];
#pragma unroll
      for (int u = 0; u < kRowsAhead; ++u) {
        if (j + u < j1) {
          at[u] = base + (v.order ? v.order[j + u] : j + u) * inner;
          x[u] = tv[at[u]];
          st[u] = HS ? ts[at[u]] : OLAP_STATUS_SET;
        }
      }
#pragma unroll
      for (int u = 0; u < kRowsAhead; ++u) {
        if (j + u < j1) {
          running_step<T, METHOD, HS>(a, x[u], st[u], def_nan);
          tv[at[u]] = x[u];
          if constexpr (HS) ts[at[u]] = st[u];
        }
      }
    }
  }
}

// state of lane (series, i) of the chunked form between two chunks
template <int METHOD>
struct Carried {
  Agg<METHOD> a;
  uint32_t g, gnext;  // the group the lane is in and the first row of the next one
};

template <typename T, bool HS, int METHOD>
__device__ __forceinline__ void rows_walk_chunk(T *tv, int32_t *ts, const CumulateView &v, uint32_t ns, uint32_t k0, uint32_t rows, Carried<METHOD> &c) {
  const bool def_nan = v.def_nan != 0;
  const uint32_t inner = (uint32_t)v.inner;
  if (threadIdx.x >= ns * inner) return;
  const uint32_t s = threadIdx.x / inner, i = threadIdx.x % inner;
  const uint32_t base = s * v.pitch + i;
  for (uint32_t r0 = 0; r0 < rows; r0 += kRowsAhead) {
    T x[kRowsAhead];
    int32_t st[kRowsAhead];
#pragma unroll
    for (int u = 0; u < kRowsAhead; ++u) {
      if (r0 + u < rows) {
        x[u] = tv[base + (r0 + u) * inner];
        st[u] = HS ? ts[base + (r0 + u) * inner] : OLAP_STATUS_SET;
      }
    }
#pragma unroll
    for (int u = 0; u < kRowsAhead; ++u) {
      if (r0 + u < rows) {
        const uint32_t k = k0 + r0 + u;
        while (k == c.gnext) {  // (a loop: groups without members)  k < K = gstart[G], so g + 1 stays <= G
          c.a.init();
          ++c.g;
          c.gnext = v.gstart[c.g + 1];
        }
        running_step<T, METHOD, HS>(c.a, x[u], st[u], def_nan);
        tv[base + (r0 + u) * inner] = x[u];
        if constexpr (HS) ts[base + (r0 + u) * inner] = st[u];
      }
    }
  }
}

template <typename T, bool HS, int METHOD>
__device__ __forceinline__ void rows_tiles(T *tv, int32_t *ts, const T *__restrict__ in, const int32_t *__restrict__ st_in, T *__restrict__ out,
                                           int32_t *__restrict__ st_out, const CumulateView &v, const uint64_t n_tiles) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const uint64_t series_cells = v.K * v.inner;
  const uint32_t K = (uint32_t)v.K, inner = (uint32_t)v.inner;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t s0 = tile * v.series;
    const uint32_t ns = (uint32_t)(v.outer - s0 < v.series ? v.outer - s0 : v.series);
    Carried<METHOD> c;
    c.a.init();
    c.g = 0;
    c.gnext = v.gstart[1];
    for (uint32_t k0 = 0; k0 < K; k0 += v.rows) {
      const uint32_t rows = K - k0 < v.rows ? K - k0 : v.rows;
      const uint64_t first = s0 * series_cells + (uint64_t)k0 * inner;
      tile_move<T, VEC, true>(tv, in, nullptr, first, series_cells, ns, rows * inner, v.pitch);
      if constexpr (HS) tile_move<int32_t, 4, true>(ts, st_in, nullptr, first, series_cells, ns, rows * inner, v.pitch);
      __syncthreads();
      if (v.form == CUMULATE_ROW_WHOLE) rows_walk_whole<T, HS, METHOD>(tv, ts, v, ns);
      else rows_walk_chunk<T, HS, METHOD>(tv, ts, v, ns, k0, rows, c);
      __syncthreads();
      tile_move<T, VEC, false>(tv, nullptr, out, first, series_cells, ns, rows * inner, v.pitch);
      if constexpr (HS) tile_move<int32_t, 4, false>(ts, nullptr, st_out, first, series_cells, ns, rows * inner, v.pitch);
      __syncthreads();  // the next chunk or tile overwrites what is being stored
    }
  }
}

template <typename T, bool HS>
__global__ __launch_bounds__(kBlock) void cumulate_rows_kernel(const Batch<T> b, const CumulateView v, const uint64_t n_tiles) {
  __shared__ T tv[kTileAlloc];
  __shared__ int32_t ts[HS ? kTileAlloc : 1];
  const uint32_t p = blockIdx.y;
  SERIES_RULE(b.method[p], (rows_tiles<T, HS, M>(tv, ts, b.in[p], b.st_in[p], b.out[p], b.st_out[p], v, n_tiles)));
}

template <typename T, bool HS>
hipError_t launch_typed(int nb, const int *methods, const void *const *in, const int32_t *const *st_in, void *const *out, int32_t *const *st_out,
                        const CumulateView &v, hipStream_t stream) {
  Batch<T> b{};
  for (int k = 0; k < nb; ++k) {
    b.in[k] = (const T *)in[k], b.st_in[k] = HS ? st_in[k] : nullptr;
    b.out[k] = (T *)out[k], b.st_out[k] = HS ? st_out[k] : nullptr;
    b.method[k] = methods[k];
  }
  if (v.form == CUMULATE_COLUMN) {
    const uint64_t items = v.outer * v.G * ((v.inner + v.vec - 1) / v.vec);
    const uint64_t blocks = (items + kBlock - 1) / kBlock;
    const dim3 grid((unsigned)(blocks < series_max_grid("OLAP_CUMULATE_GRID", 1u << 22) ? blocks : series_max_grid("OLAP_CUMULATE_GRID", 1u << 22)), (unsigned)nb);
    if (v.vec == 1) cumulate_column_kernel<T, HS, 1><<<grid, kBlock, 0, stream>>>(b, v, items);
    else cumulate_column_kernel<T, HS, 16 / (int)sizeof(T)><<<grid, kBlock, 0, stream>>>(b, v, items);
  } else {
    const uint64_t n_tiles = (v.outer + v.series - 1) / v.series;
    const dim3 grid((unsigned)(n_tiles < series_max_grid("OLAP_CUMULATE_GRID", 1u << 20) ? n_tiles : series_max_grid("OLAP_CUMULATE_GRID", 1u << 20)), (unsigned)nb);
    cumulate_rows_kernel<T, HS><<<grid, kBlock, 0, stream>>>(b, v, n_tiles);
  }
  return hipGetLastError();
}

}  // namespace

void cumulate_choose(CumulateView &v, int cell_bytes, bool contiguous) {
  const uint32_t slot = 16u / (uint32_t)cell_bytes;
  v.form = CUMULATE_COLUMN;
  v.vec = slot;
  v.series = v.rows = v.pitch = 0;
  // Rows of fewer than four slots take the row form: a lane of the column form then reads 16 bytes out of every
  // K * inner-cell series and little coalesces.  Measured at 10^8 Float32 cells, K = 100, one group, in times of the
  // copy: column form 12.5 at one slot, 4.7 at two, 4.1 at three, 1.7 at four; row form 3.4 whatever the row
  // (NOTEBOOK, cumulate)
  if (v.inner >= 4 * slot) return;
  const uint64_t series_cells = v.K * v.inner;
  if (series_cells <= kCumulateTileCells) {
    v.form = CUMULATE_ROW_WHOLE;
    const uint64_t fit = kCumulateTileCells / (series_cells ? series_cells : 1);
    v.series = (uint32_t)(fit < 256 ? fit : 256);
    v.rows = (uint32_t)v.K;
    v.pitch = (uint32_t)series_cells | 1u;
  } else if (contiguous) {
    v.form = CUMULATE_ROW_CHUNKED;
    // series * inner <= 256 lanes carry a state each.  A workgroup walks its series from end to end, so the series
    // are dealt out thinly — about 1024 workgroups where there are that many series — before the tiles get wider
    const uint32_t most = 128u / (uint32_t)v.inner;
    uint64_t series = v.outer / 1024;
    if (series < 8) series = 8;
    if (series > most) series = most;
    if (series > v.outer) series = v.outer;
    v.series = (uint32_t)series;
    v.rows = kCumulateTileCells / (v.series * (uint32_t)v.inner);
    v.pitch = (v.rows * (uint32_t)v.inner) | 1u;
  } else {
    if (v.inner < slot) v.vec = 1;  // long series with interleaved groups: one-cell slots, correct but uncoalesced
  }
}

hipError_t launch_cumulate(int dtype, bool has_status, int nb, const int *methods, const void *const *in, const int32_t *const *st_in,
                           void *const *out, int32_t *const *st_out, const CumulateView &v, hipStream_t stream) {
  if (nb < 1 || nb > kMaxBatch) return hipErrorInvalidValue;
  if (v.outer == 0 || v.K == 0 || v.inner == 0) return hipSuccess;
  return series_cell_type(dtype, has_status, [&](auto cell, auto hs) {
    return launch_typed<decltype(cell), decltype(hs)::value>(nb, methods, in, st_in, out, st_out, v, stream);
  });
}
