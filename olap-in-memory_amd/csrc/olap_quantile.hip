// olap_quantile.hip — K15: order statistics along one dimension (Cube.quantile, Cube.median).
//
// View [outer, K, inner] with one K -> G map; the result is [outer, G, inner].  An output cell holds the q-quantile
// (linear interpolation between the two neighbouring order statistics, Cube._quantileHost is the definition) of the SET
// cells of its group.  Nothing is sorted and nothing is accumulated: selection runs on an order-preserving unsigned key
// of the cell (QKey) and finds the key of rank r by bisection on the key's bits — for each bit from the top, "how many
// members lie below prefix | bit" — so ties are counted like anything else, and the two order statistics are DECODED
// from keys.  A group of a few members counts ranks instead (by_ranks): n * n reads against bits * n.
//
//   column form    inner of four slots or more (or a narrower one whose series is beyond a tile): a workgroup stages the rows of a run of whole groups for a slice of
//                  `inner` into LDS once (tile_move; tile row j is member j of the CSR, so interleaved groups lie
//                  together in the tile) and one lane per output cell (group, column) selects out of LDS.  Lanes of a
//                  wave hold neighbouring columns: staging, LDS reads and the result's stores are all coalesced.
//   row form       inner below four slots: a workgroup stages whole series (K * inner contiguous cells each, odd pitch
//                  between two series), one lane per (series, group, i).
//   direct forms   a group larger than a tile (or a series, in the row form's place): the same selection straight from
//                  device memory, the group's cells re-read once per pass and held by L2 / the Infinity Cache where the
//                  series fits, no per-group storage.  `lanes`: a lane per output cell, neighbouring lanes neighbouring
//                  cells of inner (coalesced passes; needs a wide inner and enough outputs to fill the device).
//                  `block`: a workgroup per output cell, its 256 lanes share every pass and add their counts up.
//
// No atomics, no state across workgroups; every output cell is written exactly once and the inputs are only read.
// q is a launch argument: plans do not depend on it.
#include <type_traits>

#include "olap_series.hpp"

using namespace olap;

namespace {

constexpr uint32_t kRankMax = 24;  // groups of at most this many members count ranks (NOTEBOOK: quantile); OLAP_QUANTILE_RANK

// ---------------------------------------------------------------- order-preserving keys
// key(a) < key(b) <=> a sorts before b in the IEEE total order on values (-0 before +0), every NaN at the top key.
template <typename T> struct QKey;
template <> struct QKey<float> {
  typedef uint32_t K;
  static constexpr int bits = 32;
  static __device__ __forceinline__ K of(float v) {
    const uint32_t u = __float_as_uint(v);
    return v != v ? ~0u : u ^ ((u >> 31) ? ~0u : 0x80000000u);
  }
  static __device__ __forceinline__ double value(K k) {
    if (k == ~0u) return __builtin_nan("");
    return (double)__uint_as_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k);
  }
};
template <> struct QKey<double> {
  typedef uint64_t K;
  static constexpr int bits = 64;
  static __device__ __forceinline__ K of(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    return v != v ? ~0ull : u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull);
  }
  static __device__ __forceinline__ double value(K k) {
    if (k == ~0ull) return __builtin_nan("");
    return __longlong_as_double((long long)((k & 0x8000000000000000ull) ? k ^ 0x8000000000000000ull : ~k));
  }
};
template <> struct QKey<int32_t> {
  typedef uint32_t K;
  static constexpr int bits = 32;
  static __device__ __forceinline__ K of(int32_t v) { return (uint32_t)v ^ 0x80000000u; }
  static __device__ __forceinline__ double value(K k) { return (double)(int32_t)(k ^ 0x80000000u); }
};
template <> struct QKey<uint32_t> {
  typedef uint32_t K;
  static constexpr int bits = 32;
  static __device__ __forceinline__ K of(uint32_t v) { return v; }
  static __device__ __forceinline__ double value(K k) { return (double)k; }
};

// ---------------------------------------------------------------- the members of one output cell
// Member j in [j0, j1) lies at base + (order ? order[j] : j) * stride of v (and of s, the mask, where it is primary).
// BLOCK: the 256 lanes of a workgroup share every pass (lane t takes members j0 + t, j0 + t + 256, ...) and add their
// counts up; every lane of the workgroup must then come here, and every lane gets the answer.  Otherwise a team of
// 1, 2, 4 ... neighbouring lanes of a wave does the same with shuffles: where a tile holds few output cells (one long
// group) the other lanes of the workgroup would idle.
template <typename T, bool HS, typename IDX, bool BLOCK, bool TEAMS = false>
struct Scan {
  typedef typename QKey<T>::K Key;
  static constexpr bool kBlockWide = BLOCK;
  const T *v;
  const int32_t *s;
  const uint32_t *order;
  IDX base, stride;
  uint32_t j0, j1;
  bool def_nan;
  uint32_t team, sub;  // (TEAMS) `team` neighbouring lanes of a wave, a power of two, share the walk; this is lane `sub` of them

  __device__ __forceinline__ uint32_t members() const { return j1 - j0; }
  __device__ __forceinline__ bool get(uint64_t j, Key &k) const {
    const IDX at = base + (IDX)(order ? order[j] : (uint32_t)j) * stride;
    const T x = v[at];
    const int32_t st = HS ? s[at] : OLAP_STATUS_SET;
    k = QKey<T>::of(x);
    return cell_is_set<T>(x, st, HS, def_nan);
  }
  // f(set, key) for every member this lane looks at
  template <typename F>
  __device__ __forceinline__ void each(F f) const {
#pragma unroll 4
    for (uint64_t j = (uint64_t)j0 + (BLOCK ? threadIdx.x : TEAMS ? sub : 0u); j < j1; j += (BLOCK ? kBlock : TEAMS ? team : 1u)) {
      Key k;
      const bool set = get(j, k);
      f(set, k);
    }
  }
  // the workgroup's sum / least of the lanes' values (BLOCK), or the lane's own
  enum { SUM, LEAST };
  template <int OP>
  static __device__ __forceinline__ unsigned long long fold(unsigned long long a, unsigned long long b) {
    if constexpr (OP == SUM) return a + b;
    else return b < a ? b : a;
  }
  template <int OP>
  __device__ __forceinline__ unsigned long long across(unsigned long long x) const {
    if constexpr (!BLOCK) {
      if constexpr (TEAMS)
        for (uint32_t d = team >> 1; d >= 1; d >>= 1) x = fold<OP>(x, __shfl_xor(x, (int)d, 64));
    } else {
      __shared__ unsigned long long part[kBlock / 64];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) x = fold<OP>(x, __shfl_xor(x, d, 64));
      if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x;
      __syncthreads();
      x = part[0];
#pragma unroll
      for (int w = 1; w < kBlock / 64; ++w) x = fold<OP>(x, part[w]);
      __syncthreads();  // the next pass writes part[] again
    }
    return x;
  }
  __device__ __forceinline__ uint32_t count_set() const {
    uint32_t c = 0;
    each([&](bool set, Key) { c += set; });
    return (uint32_t)across<SUM>(c);
  }
  __device__ __forceinline__ uint32_t count_below(Key t) const {
    uint32_t c = 0;
    each([&](bool set, Key k) { c += set && k < t; });
    return (uint32_t)across<SUM>(c);
  }
  // members <= x, and the least key above x (the top key when there is none)
  __device__ __forceinline__ void upto_and_next(Key x, uint32_t &upto, Key &next) const {
    uint32_t c = 0;
    Key nx = ~(Key)0;
    each([&](bool set, Key k) {
      c += set && k <= x;
      nx = (set && k > x && k < nx) ? k : nx;
    });
    upto = (uint32_t)across<SUM>(c);
    next = (Key)across<LEAST>(nx);
  }
  // the keys of rank lo and lo + 1 (the latter only where there is one) by counting, for every set member, the
  // members below it and up to it: a key holds the ranks [below, upto)
  __device__ __forceinline__ void by_ranks(uint32_t lo, Key &klo, Key &khi) const {
    static_assert(!BLOCK, "rank counting is a lane's (or a team's) walk");
    for (uint32_t i = j0; i < j1; ++i) {
      Key ki;
      if (!get(i, ki)) continue;
      uint32_t below = 0, upto = 0;
      each([&](bool set, Key k) {
        below += set && k < ki;
        upto += set && k <= ki;
      });
      below = (uint32_t)across<SUM>(below), upto = (uint32_t)across<SUM>(upto);
      if (below <= lo && lo < upto) klo = ki;
      if (below <= lo + 1 && lo + 1 < upto) khi = ki;
    }
  }
};

// One output cell.  The arithmetic is Cube._quantileHost's, operation by operation; nothing may fuse (JS has no FMA).
template <typename T, typename S>
__device__ __forceinline__ void select_cell(const S &sc, double q, bool def_nan, uint32_t rank_max, T &ov, int32_t &os) {
#pragma clang fp contract(off)
  typedef typename QKey<T>::K Key;
  const uint32_t n = sc.count_set();
  if (n == 0) {
    emit_cell<T>(0.0, false, def_nan, ov, os);
    return;
  }
  const double h = q * (double)(n - 1);
  const double fl = floor(h);
  const double frac = h - fl;
  const uint32_t lo = (uint32_t)fl;  // <= n - 1; frac > 0 => lo + 1 <= n - 1
  Key klo = 0, khi = 0;
  bool ranked = false;
  if constexpr (!S::kBlockWide) {
    if (sc.members() <= rank_max) {
      sc.by_ranks(lo, klo, khi);
      ranked = true;
    }
  }
  if (!ranked) {
    // the largest x with fewer than lo + 1 members below it is the key of rank lo (with lo < n such a member exists),
    // built from the top bit down
    Key x = 0;
    for (int b = QKey<T>::bits - 1; b >= 0; --b) {
      const Key t = x | ((Key)1 << b);
      if (sc.count_below(t) <= lo) x = t;
    }
    klo = khi = x;
    if (frac > 0) {
      uint32_t upto;
      Key next;
      sc.upto_and_next(x, upto, next);
      if (upto <= lo + 1) khi = next;  // rank lo + 1 is no longer x
    }
  }
  double r = QKey<T>::value(klo);
  if (frac > 0) {
    const double d = QKey<T>::value(khi) - r;
    const double m = frac * d;
    r = r + m;
  }
  if (r != r) r = __builtin_nan("");  // one NaN, whatever the arithmetic made of its operands' payloads
  emit_cell<T>(r, true, def_nan, ov, os);
}

template <typename T, bool HS>
struct Tile {
  static constexpr uint32_t kCells = kQuantileTileBytes / (uint32_t)(sizeof(T) + (HS ? 4 : 0));
  static constexpr uint32_t kAlloc = kCells + 256;  // + one pad cell per series of the row form (at most 256 series per tile)
};

// ---------------------------------------------------------------- column form
template <typename T, bool HS>
__global__ __launch_bounds__(kBlock) void quantile_column_kernel(const Batch<T> b, const QuantileView v, const double q, const uint32_t rank_max,
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
    // (teams of one are the common case and keep a loop without the team's arithmetic)
    auto select_cells = [&](auto teams) {
      constexpr bool TEAMS = decltype(teams)::value;
      const uint32_t team = TEAMS ? v.team : 1u;
      for (uint32_t it = threadIdx.x / team; it < cells; it += kBlock / team) {
        const uint32_t c = it % nc, g = g0 + it / nc;
        const Scan<T, HS, uint32_t, false, TEAMS> sc{tv, ts, nullptr, c, v.cols, v.gstart[g] - ja, v.gstart[g + 1] - ja, def_nan, team, TEAMS ? threadIdx.x % team : 0u};
        T ov;
        int32_t os;
        select_cell<T>(sc, q, def_nan, rank_max, ov, os);
        if (sc.sub != 0) continue;
        const uint64_t at = (o * v.G + g) * v.inner + c0 + c;
        out[at] = ov;
        if constexpr (HS) st_out[at] = os;
      }
    };
    if (v.team == 1) select_cells(std::false_type{});
    else select_cells(std::true_type{});
    __syncthreads();  // the next tile overwrites what is being read
  }
}

// ---------------------------------------------------------------- row form
template <typename T, bool HS>
__global__ __launch_bounds__(kBlock) void quantile_rows_kernel(const Batch<T> b, const QuantileView v, const double q, const uint32_t rank_max,
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
    auto select_cells = [&](auto teams) {
      constexpr bool TEAMS = decltype(teams)::value;
      const uint32_t team = TEAMS ? v.team : 1u;
      for (uint64_t it = threadIdx.x / team; it < cells; it += kBlock / team) {
        const uint32_t i = (uint32_t)(it % inner), g = (uint32_t)((it / inner) % G), s = (uint32_t)(it / ((uint64_t)inner * G));
        const Scan<T, HS, uint32_t, false, TEAMS> sc{tv, ts, v.order, s * v.pitch + i, inner, v.gstart[g], v.gstart[g + 1], def_nan, team, TEAMS ? threadIdx.x % team : 0u};
        T ov;
        int32_t os;
        select_cell<T>(sc, q, def_nan, rank_max, ov, os);
        if (sc.sub != 0) continue;
        const uint64_t at = s0 * G * inner + it;
        out[at] = ov;
        if constexpr (HS) st_out[at] = os;
      }
    };
    if (v.team == 1) select_cells(std::false_type{});
    else select_cells(std::true_type{});
    __syncthreads();
  }
}

// ---------------------------------------------------------------- direct forms
template <typename T, bool HS, bool BLOCK>
__global__ __launch_bounds__(kBlock) void quantile_direct_kernel(const Batch<T> b, const QuantileView v, const double q, const uint32_t rank_max,
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
    const Scan<T, HS, uint64_t, BLOCK> sc{in, st_in, v.order, o * v.K * v.inner + i, v.inner, v.gstart[g], v.gstart[g + 1], def_nan, 1, 0};
    T ov;
    int32_t os;
    select_cell<T>(sc, q, def_nan, rank_max, ov, os);
    if (!BLOCK || threadIdx.x == 0) {
      out[it] = ov;
      if constexpr (HS) st_out[it] = os;
    }
  }
}

template <typename T, bool HS>
hipError_t launch_typed(int nb, const void *const *in, const int32_t *const *st_in, void *const *out, int32_t *const *st_out, const QuantileView &v,
                        double q, hipStream_t stream) {
  if (v.tile > Tile<T, HS>::kCells) return hipErrorInvalidValue;  // the tile the cuts were made for does not fit this kernel's
  Batch<T> b{};
  for (int k = 0; k < nb; ++k) {
    b.in[k] = (const T *)in[k], b.st_in[k] = HS ? st_in[k] : nullptr;
    b.out[k] = (T *)out[k], b.st_out[k] = HS ? st_out[k] : nullptr;
  }
  uint32_t rank_max = kRankMax;
  if (getenv("OLAP_QUANTILE_RANK")) rank_max = (uint32_t)env_number("OLAP_QUANTILE_RANK");
  const uint64_t cells = v.outer * v.G * v.inner;
  auto grid = [&](uint64_t want) { return dim3((unsigned)(want < series_max_grid("OLAP_QUANTILE_GRID", 1u << 20) ? want : series_max_grid("OLAP_QUANTILE_GRID", 1u << 20)), (unsigned)nb); };
  switch (v.form) {
    case QUANTILE_COLUMN: {
      const uint64_t n_work = v.outer * v.n_gtile * ((v.inner + v.cols - 1) / v.cols);
      quantile_column_kernel<T, HS><<<grid(n_work), kBlock, 0, stream>>>(b, v, q, rank_max, n_work);
      break;
    }
    case QUANTILE_ROW: {
      const uint64_t n_tiles = (v.outer + v.series - 1) / v.series;
      quantile_rows_kernel<T, HS><<<grid(n_tiles), kBlock, 0, stream>>>(b, v, q, rank_max, n_tiles);
      break;
    }
    case QUANTILE_DIRECT_LANES:
      quantile_direct_kernel<T, HS, false><<<grid((cells + kBlock - 1) / kBlock), kBlock, 0, stream>>>(b, v, q, rank_max, cells);
      break;
    default:
      quantile_direct_kernel<T, HS, true><<<grid(cells), kBlock, 0, stream>>>(b, v, q, 0, cells);
      break;
  }
  return hipGetLastError();
}

}  // namespace

uint32_t quantile_tile_cells(int cell_bytes, bool has_mask) {
  const uint32_t most = kQuantileTileBytes / (uint32_t)(cell_bytes + (has_mask ? 4 : 0));
  const unsigned long n = env_number("OLAP_QUANTILE_TILE");
  return n >= 1 && n < most ? (uint32_t)n : most;
}

// Lanes that share one output cell's walk: as many as leave no lane of the workgroup idle when a tile holds `cells`
// output cells, at most 32, and no more than half the members of the largest group.
static uint32_t quantile_team(uint64_t cells, uint32_t longest) {
  uint32_t team = 1;
  while (team < 32 && (uint64_t)team * 2 * cells <= (uint64_t)kBlock && team * 4 <= longest) team *= 2;
  return team;
}

void quantile_choose(QuantileView &v, int cell_bytes) {
  const uint32_t slot = 16u / (uint32_t)cell_bytes;
  v.series = v.pitch = v.cols = v.rows = v.n_gtile = 0;
  v.team = 1;
  const uint64_t cells = v.outer * v.G * v.inner;
  // a lane per output cell reads coalesced only across a wide inner and fills the device only with enough cells;
  // otherwise a workgroup per output cell (a choice from the shapes' arithmetic, not a sweep: NOTEBOOK)
  const int direct = v.inner >= 64 && cells >= 4096 ? QUANTILE_DIRECT_LANES : QUANTILE_DIRECT_BLOCK;
  const uint64_t series_cells = v.K * v.inner;
  if (v.inner < 4 * slot && series_cells <= v.tile) {
    // rows of fewer than four slots, as cumulate's row form: whole series, as many as fit
    v.form = QUANTILE_ROW;
    const uint64_t fit = v.tile / (series_cells ? series_cells : 1);
    v.series = (uint32_t)(fit < 256 ? fit : 256);
    v.pitch = (uint32_t)series_cells | 1u;
    v.team = quantile_team((v.outer < v.series ? v.outer : v.series) * v.G * v.inner, v.longest);
    return;
  }
  // a tile must hold the largest group one slot wide (the whole row, where that is narrower)
  const uint64_t least = v.inner < slot ? v.inner : slot;
  if ((uint64_t)v.longest * least > v.tile) {
    v.form = direct;
    return;
  }
  // Column form.  Rows of fewer than four slots whose series is beyond a tile come here too, the whole row a slice:
  // with contiguous groups the rows of a tile are one run of device memory
  v.form = QUANTILE_COLUMN;
  const uint64_t fit = v.tile / (v.longest ? v.longest : 1);  // >= least
  uint64_t cols = v.inner < 256 ? v.inner : 256;
  if (cols > fit) cols = fit;
  if (cols < v.inner) cols -= cols % slot;  // slices start on whole slots of the row
  v.cols = (uint32_t)cols;
  v.rows = v.tile / v.cols;  // >= longest
  // (a tile holds about rows / longest of the largest groups; tiles of smaller groups hold more cells and could do with less)
  v.team = quantile_team((uint64_t)v.cols * (v.rows / (v.longest ? v.longest : 1)), v.longest);
}

hipError_t launch_quantile(int dtype, bool has_status, int nb, const void *const *in, const int32_t *const *st_in, void *const *out,
                           int32_t *const *st_out, const QuantileView &v, double q, hipStream_t stream) {
  if (nb < 1 || nb > kMaxBatch) return hipErrorInvalidValue;
  if (v.outer == 0 || v.G == 0 || v.inner == 0) return hipSuccess;
  return series_cell_type(dtype, has_status, [&](auto cell, auto hs) {
    return launch_typed<decltype(cell), decltype(hs)::value>(nb, in, st_in, out, st_out, v, q, stream);
  });
}
