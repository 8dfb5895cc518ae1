// olap_series.hpp — what the kernels that walk series along one dimension share (olap_cumulate.hip, K13;
// olap_rolling.hip, K14; olap_quantile.hip, K15; olap_variance.hip, K16).  On the device: the per-pair rule dispatch
// (SERIES_RULE), 16-byte slots at cell-aligned addresses (load_slot, store_slot) and the move of contiguous pieces
// between global memory and an LDS tile (tile_move).  On the host, for the launch functions at the units' ends: the
// dispatch on cell type and mask (series_cell_type), the developer knobs' numbers (env_number) and the grid cap with its
// knob (series_max_grid).
#pragma once

#include <cstdlib>
#include <type_traits>

#include "olap_internal.hpp"
#include "olap_kernels.hpp"

namespace olap {

// runs CALL with M naming the rule `method` (one of the seven; checked on the host)
#define SERIES_RULE(method, CALL)                                        \
  switch (method) {                                                      \
    case OLAP_SUM: { constexpr int M = OLAP_SUM; CALL; break; }          \
    case OLAP_AVERAGE: { constexpr int M = OLAP_AVERAGE; CALL; break; }  \
    case OLAP_HIGHEST: { constexpr int M = OLAP_HIGHEST; CALL; break; }  \
    case OLAP_LOWEST: { constexpr int M = OLAP_LOWEST; CALL; break; }    \
    case OLAP_FIRST: { constexpr int M = OLAP_FIRST; CALL; break; }      \
    case OLAP_LAST: { constexpr int M = OLAP_LAST; CALL; break; }        \
    default: { constexpr int M = OLAP_PRODUCT; CALL; break; }            \
  }

// The cell type and mask of a launch, on the host: launch(T{}, HS{}) with T the cell type of `dtype` and HS
// std::true_type where the pairs carry masks.  Float cells never hold a mask of their own (mask_is_primary).
template <typename Launch>
hipError_t series_cell_type(int dtype, bool has_status, Launch launch) {
  switch (dtype) {
    case OLAP_INT32:
      return has_status ? launch(int32_t{}, std::true_type{}) : launch(int32_t{}, std::false_type{});
    case OLAP_UINT32:
      return has_status ? launch(uint32_t{}, std::true_type{}) : launch(uint32_t{}, std::false_type{});
    case OLAP_FLOAT32:
      return has_status ? hipErrorInvalidValue : launch(float{}, std::false_type{});
    default:
      return has_status ? hipErrorInvalidValue : launch(double{}, std::false_type{});
  }
}

// the number in a developer knob; 0 where it is not set
inline unsigned long env_number(const char *name) {
  const char *e = getenv(name);
  return e ? strtoul(e, nullptr, 10) : 0;
}

// Workgroups of a launch along x: beyond `most` a workgroup takes several tiles, a lane several cells.  The knob
// (OLAP_CUMULATE_GRID=n and its like; developer knobs, NOTEBOOK) lowers it, so that the tests reach those loops with
// small cubes.  Read at every launch.
inline uint64_t series_max_grid(const char *knob, uint32_t most) {
  const unsigned long n = env_number(knob);
  return n >= 1 && n < most ? n : most;
}

// n <= VEC cells from a cell-aligned address: one 16-byte access for a whole slot, cell by cell otherwise
template <typename T, int VEC>
__device__ __forceinline__ Vec<T, VEC> load_slot(const T *p, int n) {
  Vec<T, VEC> r;
  if constexpr (VEC == 1) {
    r.v[0] = __builtin_nontemporal_load(p);
  } else {
    if (n == VEC) {
      r = load_stream_cell_aligned<T, VEC>(p);
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) r.v[e] = e < n ? __builtin_nontemporal_load(p + e) : T(0);
    }
  }
  return r;
}
template <typename T, int VEC>
__device__ __forceinline__ void store_slot(T *p, const Vec<T, VEC> &x, int n) {
  if constexpr (VEC == 1) {
    __builtin_nontemporal_store(x.v[0], p);
  } else {
    if (n == VEC) {
      store_stream_cell_aligned<T, VEC>(p, x);
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        if (e < n) __builtin_nontemporal_store(x.v[e], p + e);
    }
  }
}

// Moves `ns` pieces of `seg` contiguous cells between global memory and an LDS tile: piece s starts at cell
// first_cell + s * piece_stride in global memory (`piece` given: first_cell + piece[s] * piece_stride) and at s * pitch
// in the tile.  Read and written in 16-byte slots (the last slot of a piece cell by cell).
template <typename T, int VEC, bool LOAD>
__device__ __forceinline__ void tile_move(T *tile, const T *src, T *dst, uint64_t first_cell, uint64_t piece_stride, uint32_t ns, uint32_t seg,
                                          uint32_t pitch, const uint32_t *piece = nullptr) {
  const uint32_t slots = (seg + VEC - 1) / VEC;
  for (uint32_t c = threadIdx.x; c < ns * slots; c += kBlock) {
    const uint32_t s = c / slots, r = (c % slots) * VEC;
    const int n = (int)(seg - r < (uint32_t)VEC ? seg - r : (uint32_t)VEC);
    const uint64_t at = first_cell + (uint64_t)(piece ? piece[s] : s) * piece_stride + r;
    T *cell = tile + s * pitch + r;
    if constexpr (LOAD) {
      const Vec<T, VEC> x = load_slot<T, VEC>(src + at, n);
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        if (e < n) cell[e] = x.v[e];
    } else {
      Vec<T, VEC> x;
#pragma unroll
      for (int e = 0; e < VEC; ++e) x.v[e] = e < n ? cell[e] : T(0);
      store_slot<T, VEC>(dst + at, x, n);
    }
  }
}

}  // namespace olap
