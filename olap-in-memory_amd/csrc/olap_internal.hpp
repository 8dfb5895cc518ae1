// olap_internal.hpp — what the translation units of libolapgpu share besides the C ABI: error
// reporting, the device memory pool and the layout of a store handle.  Nothing here is exported.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/olap_hip.h"

#define OLAP_INTERNAL __attribute__((visibility("hidden")))

// sets the calling thread's olap_last_error() and returns `code`
OLAP_INTERNAL int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
OLAP_INTERNAL int hip_fail(hipError_t e, const char *what);

#define HIP_TRY(expr)                                  \
  do {                                                 \
    hipError_t e__ = (expr);                           \
    if (e__ != hipSuccess) return hip_fail(e__, #expr); \
  } while (0)

// Runs CALL with T naming the cell type of `dtype` (an OLAP_* dtype that passed check_dtype).  The one cell-type
// dispatch of the library; the type's name is a parameter so that two dispatches can nest.
#define DISPATCH_DTYPE(dtype, T, CALL)                     \
  switch (dtype) {                                         \
    case OLAP_INT32: { using T = int32_t; CALL; break; }   \
    case OLAP_UINT32: { using T = uint32_t; CALL; break; } \
    case OLAP_FLOAT32: { using T = float; CALL; break; }   \
    default: { using T = double; CALL; break; }            \
  }

// remembers the calling thread's device and puts it back
struct DeviceGuard {
  int saved = -1;
  DeviceGuard() { (void)hipGetDevice(&saved); }
  ~DeviceGuard() {
    if (saved >= 0) (void)hipSetDevice(saved);
  }
};

// pooled device memory of the CURRENT device (olap_capi.hip: DevicePool)
OLAP_INTERNAL hipError_t dev_alloc(void **out, size_t bytes);
OLAP_INTERNAL void dev_free(void *p);

OLAP_INTERNAL int check_dtype(int dtype);
OLAP_INTERNAL int check_default(int kind);
OLAP_INTERNAL int require_device();

// One measure's cells on one device (in-memory.js:7-64).  values are always resident; the Int32
// mask is materialised lazily except where it is primary (integer cells over a NaN default).
struct olap_store {
  uint64_t size;
  int dtype;
  int default_kind;
  int device;               // the HIP device the buffers live on
  void *values;
  mutable int32_t *status;  // nullptr until needed
  // Insertion order of the reference's Map (in-memory.js:298 iterates it), kept only on request
  // (olap_store_track_order) and only once it differs from ascending flat index: seq[i] > 0 <=> cell i is set,
  // and set cells compare by seq as the reference's Map entries compare by age.  olap_order.hip.
  bool track_order = false;
  mutable uint32_t *seq = nullptr;   // nullptr: the order is the ascending flat index
  mutable uint64_t next_seq = 1;     // next value to hand out
  bool maybe_nonempty = false;       // some cell may be set (false only for a store nothing was written to)
  uint64_t hi_index = 0;             // no set cell lies above this index (valid while seq == nullptr)
};

// tests/test_set_formula_host.py restates the fields up to `status` (a ctypes stand-in for refusals decided without a
// device): a change of their order or types must be made there too
static_assert(offsetof(olap_store, size) == 0 && offsetof(olap_store, dtype) == 8 && offsetof(olap_store, default_kind) == 12 &&
                  offsetof(olap_store, device) == 16 && offsetof(olap_store, values) == 24 && offsetof(olap_store, status) == 32,
              "struct olap_store moved: update FakeStore in tests/test_set_formula_host.py");

// The handle layer runs every operation on the device its store lives on, whatever device the
// calling thread had current (one process may drive several GPUs: the sharded stores hand whole
// results back as plain stores on their first device), and puts the caller's device back on exit.
struct OnStoreDevice : DeviceGuard {
  explicit OnStoreDevice(const olap_store *s) {
    if (s && saved >= 0 && s->device != saved) (void)hipSetDevice(s->device);
  }
};

OLAP_INTERNAL bool mask_is_primary(const olap_store *s);
OLAP_INTERNAL const int32_t *mask_needed(const olap_store *s);
OLAP_INTERNAL int store_alloc(olap_store **out, uint64_t size, int dtype, int default_kind);
OLAP_INTERNAL int ensure_status(const olap_store *s);
OLAP_INTERNAL void drop_lazy_status(olap_store *s);

// ---- lists of stores: what the entry points over several stores share (olap_capi.hip, olap_blocks.hip) -------------
// The refusals, each written once; an entry point composes them in the order it reports them, with its own wording
// (`what`, `advice`) where entry points differ.
OLAP_INTERNAL int check_list(int n, bool there, const char *what);  // n < 0, or a list that is not `there`
OLAP_INTERNAL int check_entry(const olap_store *s, int i);          // entry i of a list is NULL
OLAP_INTERNAL int check_entries(int n, const olap_store *const *stores);
OLAP_INTERNAL int check_untracked(int n, const olap_store *const *stores, const char *advice);  // no member tracks its order
// every member holds `cells` cells (`what`: instead of the message that names the two counts)
OLAP_INTERNAL int check_cells(int n, const olap_store *const *stores, uint64_t cells, const char *what = nullptr);

inline bool same_cells(const olap_store *a, const olap_store *b) { return a->dtype == b->dtype && a->default_kind == b->default_kind; }

// Partitions 0..n-1 (nothing for n <= 0) by same(i, j), i the group's first member.  Groups come in the order of their
// first member, members ascending: launch counts and "the first error wins" follow from this.  fn(members) -> rc; the
// first non-zero rc ends the walk and is returned.
template <typename Same, typename Fn>
int for_each_group(int n, Same same, Fn fn) {
  if (n <= 0) return 0;
  std::vector<char> done(n, 0);
  std::vector<int> members;
  for (int i = 0; i < n; ++i) {
    if (done[i]) continue;
    members.clear();
    for (int j = i; j < n; ++j)
      if (!done[j] && same(i, j)) {
        members.push_back(j);
        done[j] = 1;
      }
    const int rc = fn(members);
    if (rc) return rc;
  }
  return 0;
}

// every buffer of a launch starts on a 16-byte boundary (a buffer the launch does not have is passed as nullptr)
inline bool all_aligned16(const void *in, const void *in_s, const void *out, const void *out_s) {
  return (((uintptr_t)in | (uintptr_t)in_s | (uintptr_t)out | (uintptr_t)out_s) & 15u) == 0;
}

// Fills the pointer slots of one chunk of nb <= kMaxBatch pairs as a kernel takes them (st_out == nullptr: it takes no
// result masks) from pair(k), the buffers of the chunk's k-th member.  Returns all_aligned16 of the whole chunk.
struct PairBuffers {
  const void *in;
  const int32_t *st_in;
  void *out;
  int32_t *st_out;
};
template <typename In, typename Out, typename Pair>
bool fill_chunk(int nb, const In **in, const int32_t **st_in, Out **out, int32_t **st_out, Pair pair) {
  bool aligned = true;
  for (int k = 0; k < nb; ++k) {
    const PairBuffers p = pair(k);
    in[k] = (const In *)p.in, st_in[k] = p.st_in, out[k] = (Out *)p.out;
    if (st_out) st_out[k] = p.st_out;
    aligned = aligned && all_aligned16(p.in, p.st_in, p.out, p.st_out);
  }
  return aligned;
}

// ---- reorder of 4-byte cells as a two-axis LDS transpose (olap_transpose.hip) ---------------------
constexpr int kTransposeMaxAxis = 4;    // dimensions merged into the X (source-contiguous) or Y (destination-contiguous) axis
constexpr int kTransposeMaxBatch = 12;  // remaining dimensions: one coordinate per workgroup
struct TransposeXY {
  int nx, ny, nb;
  uint32_t len_x[kTransposeMaxAxis];         // X chain, fastest source dimension first
  uint64_t out_stride_x[kTransposeMaxAxis];  // their strides in the destination
  uint32_t len_y[kTransposeMaxAxis];         // Y chain, fastest destination dimension first
  uint64_t in_stride_y[kTransposeMaxAxis];   // their strides in the source
  uint32_t len_b[kTransposeMaxBatch];
  uint64_t in_stride_b[kTransposeMaxBatch], out_stride_b[kTransposeMaxBatch];
  uint64_t lx, ly;                           // merged axis lengths
  uint64_t tiles_x, tiles_y, batch;
  int tx, ty;                                // tile extents (cells)
  int super;                                 // tiles are walked in super x super blocks
  int y_first;                               // tile order: Y fastest (write locality) instead of X fastest (read locality)
  int cached_stores;                         // OLAP_XY_CACHED_STORES=1: plain instead of streaming stores (L2 may merge neighbouring tiles' pieces)
  int vec_in, vec_out;                       // every tile row starts 16-byte aligned on that side
  int default_test;                          // how a generated mask tells the default: 0 int/0, 1 float/0, 2 float/NaN, 3 never
};
OLAP_INTERNAL hipError_t launch_transpose_xy(const TransposeXY &t, int cell_bytes, const void *in, void *out, int32_t *st_out, bool aligned16,
                                              hipStream_t stream);

// ---- running aggregates along one axis (olap_cumulate.hip, K13) -----------------------------------
// View [outer, K, inner] with one K -> G map as the CSR of the drillUp plans: members of group g are
// order[gstart[g] .. gstart[g + 1]) ascending (order == nullptr: the groups are the contiguous runs themselves).
constexpr uint32_t kCumulateTileCells = 4096;  // cells of one row-form tile in LDS (NOTEBOOK: cumulate)
enum CumulateForm { CUMULATE_COLUMN = 0, CUMULATE_ROW_WHOLE = 1, CUMULATE_ROW_CHUNKED = 2 };
struct CumulateView {
  uint64_t outer, K, inner, G;
  const uint32_t *gstart;  // device, [G + 1]
  const uint32_t *order;   // device, [K], or nullptr
  int def_nan;
  int form;                // CumulateForm
  uint32_t vec;            // column form: cells per slot (16 bytes' worth, or 1: the uncoalesced form of long interleaved series)
  uint32_t series;         // row forms: series per tile
  uint32_t rows;           // chunked row form: rows of K per chunk
  uint32_t pitch;          // row forms: cells between two series of a tile (odd)
};
// chooses form, slot width and tile cuts from the shape alone (cell_bytes: 4 or 8); `contiguous`: order == nullptr
OLAP_INTERNAL void cumulate_choose(CumulateView &v, int cell_bytes, bool contiguous);
// nb <= 8 pairs of one cell type and default, a rule each (methods[k]); masks on all pairs or on none
OLAP_INTERNAL hipError_t launch_cumulate(int dtype, bool has_status, int nb, const int *methods, const void *const *in, const int32_t *const *st_in,
                                         void *const *out, int32_t *const *st_out, const CumulateView &v, hipStream_t stream);

// ---- rolling-window aggregates along one axis (olap_rolling.hip, K14) ------------------------------
// View [outer, K, inner]; the window of item k is [k - before, k + after] clipped to [0, K) and to k's group under the
// K -> G map, which the device gets as it is (map == nullptr: one group).
constexpr uint32_t kRollingInBytes = 16384;  // LDS of a tile's input rows (output rows + halo), and of its mask where primary
constexpr uint32_t kRollingOutBytes = 8192;  // LDS of a tile's output rows (a choice, not a measurement)
enum RollingForm { ROLLING_SERIES = 0, ROLLING_COLUMNS = 1, ROLLING_DIRECT = 2 };
struct RollingView {
  uint64_t outer, K, inner;
  const uint32_t *map;    // device, [K], or nullptr
  int64_t before, after;  // within [-K, K]; before + after >= 0
  int def_nan;
  int form;               // RollingForm
  uint32_t series;        // tiled forms: series per tile (ROLLING_COLUMNS: 1)
  uint32_t rows;          // output rows of K per tile
  uint32_t cols;          // cells of `inner` per tile row (ROLLING_SERIES: inner)
  uint32_t pitch;         // LDS cells between two series (ROLLING_SERIES) or two rows (ROLLING_COLUMNS) of the input tile
};
// chooses form and tile cuts from shape and window alone (cell_bytes: 4 or 8); before / after already within [-K, K]
OLAP_INTERNAL void rolling_choose(RollingView &v, int cell_bytes);
// nb <= 8 pairs of one cell type and default, a rule each (methods[k]); masks on all pairs or on none
OLAP_INTERNAL hipError_t launch_rolling(int dtype, bool has_status, int nb, const int *methods, const void *const *in, const int32_t *const *st_in,
                                        void *const *out, int32_t *const *st_out, const RollingView &v, hipStream_t stream);

// ---- order statistics along one axis (olap_quantile.hip, K15) --------------------------------------
// View [outer, K, inner] with one K -> G map as the CSR of CumulateView; the result is [outer, G, inner].
constexpr uint32_t kQuantileTileBytes = 32768;  // LDS of one tile: cells, and their mask where it is primary
enum QuantileForm { QUANTILE_COLUMN = 0, QUANTILE_ROW = 1, QUANTILE_DIRECT_LANES = 2, QUANTILE_DIRECT_BLOCK = 3 };
struct QuantileView {
  uint64_t outer, K, inner, G;
  const uint32_t *gstart;  // device, [G + 1]
  const uint32_t *order;   // device, [K], or nullptr
  const uint32_t *gtile;   // device, [n_gtile + 1]: column form, tile t holds the groups [gtile[t], gtile[t + 1])
  int def_nan;
  int form;                // QuantileForm
  uint32_t tile;           // cells a tile may hold (kQuantileTileBytes' worth, or OLAP_QUANTILE_TILE)
  uint32_t longest;        // members of the largest group
  uint32_t series;         // row form: series per tile
  uint32_t pitch;          // row form: cells between two series of a tile (odd)
  uint32_t cols;           // column form: cells of `inner` per tile row
  uint32_t rows;           // column form: rows a tile may hold
  uint32_t n_gtile;        // column form: tiles of groups per (outer, slice of inner)
  uint32_t team;           // tiled forms: neighbouring lanes of a wave that share one output cell's walk (a power of two)
};
// cells of one tile for cells of cell_bytes (4 or 8), with a mask tile beside them or not; OLAP_QUANTILE_TILE lowers it
OLAP_INTERNAL uint32_t quantile_tile_cells(int cell_bytes, bool has_mask);
// chooses form and tile cuts from the shape, the tile and the largest group alone; fills everything but the tables
OLAP_INTERNAL void quantile_choose(QuantileView &v, int cell_bytes);
// nb <= 8 pairs of one cell type and default; masks on all pairs or on none
OLAP_INTERNAL hipError_t launch_quantile(int dtype, bool has_status, int nb, const void *const *in, const int32_t *const *st_in, void *const *out,
                                         int32_t *const *st_out, const QuantileView &v, double q, hipStream_t stream);

// ---- dispersion along one axis (olap_variance.hip, K16) --------------------------------------------
// View [outer, K, inner] with one K -> G map as the CSR of CumulateView; the result is [outer, G, inner].
constexpr uint32_t kVarianceTileBytes = 32768;    // LDS of one tile: cells, and their mask where it is primary
constexpr uint32_t kVarianceBlockCells = 65536;   // at most this many output cells ...
constexpr uint32_t kVarianceBlockMembers = 1024;  // ... of groups at least this long go to a workgroup each (DESIGN K16; OLAP_VARIANCE_BLOCK)
// VARIANCE_DIRECT_BLOCK is the one RE-ASSOCIATED form: a workgroup adds a group's members up by a tree of fixed shape
enum VarianceForm { VARIANCE_COLUMN = 0, VARIANCE_ROW = 1, VARIANCE_DIRECT_LANES = 2, VARIANCE_DIRECT_BLOCK = 3 };
struct VarianceView {
  uint64_t outer, K, inner, G;
  const uint32_t *gstart;  // device, [G + 1]
  const uint32_t *order;   // device, [K], or nullptr
  const uint32_t *gtile;   // device, [n_gtile + 1]: column form, tile t holds the groups [gtile[t], gtile[t + 1])
  int def_nan;
  int form;                // VarianceForm
  uint32_t tile;           // cells a tile may hold (kVarianceTileBytes' worth, or OLAP_VARIANCE_TILE)
  uint32_t block_members;  // members of the largest group from which few output cells take a workgroup each
  uint32_t block_cells;    // ... and how many output cells are few
  uint32_t longest;        // members of the largest group
  uint32_t series;         // row form: series per tile
  uint32_t pitch;          // row form: cells between two series of a tile (odd)
  uint32_t cols;           // column form: cells of `inner` per tile row
  uint32_t rows;           // column form: rows a tile may hold
  uint32_t n_gtile;        // column form: tiles of groups per (outer, slice of inner)
};
// cells of one tile for cells of cell_bytes (4 or 8), with a mask tile beside them or not; OLAP_VARIANCE_TILE lowers it
OLAP_INTERNAL uint32_t variance_tile_cells(int cell_bytes, bool has_mask);
// kVarianceBlockMembers and kVarianceBlockCells, or OLAP_VARIANCE_BLOCK=members[,cells]
OLAP_INTERNAL uint32_t variance_block_members();
OLAP_INTERNAL uint32_t variance_block_cells();
// chooses form and tile cuts from the shape, the tile and the largest group alone; fills everything but the tables
OLAP_INTERNAL void variance_choose(VarianceView &v, int cell_bytes);
// nb <= 8 pairs of one cell type and default; masks on all pairs or on none.  kind: 0 variance, 1 stddev; ddof: 0 or 1
OLAP_INTERNAL hipError_t launch_variance(int dtype, bool has_status, int nb, const void *const *in, const int32_t *const *st_in, void *const *out,
                                         int32_t *const *st_out, const VarianceView &v, int kind, int ddof, hipStream_t stream);

// ---- insertion order of tracked stores (olap_order.hip) --------------------------------------------
OLAP_INTERNAL void order_free(olap_store *s);
OLAP_INTERNAL int order_clone(const olap_store *from, olap_store *to);
OLAP_INTERNAL int order_before_bulk_write(olap_store *s);
OLAP_INTERNAL int order_after_bulk_write(olap_store *s);
OLAP_INTERNAL int order_before_set_value(olap_store *s, uint64_t index);
OLAP_INTERNAL int order_after_set_value(olap_store *s, uint64_t index);
OLAP_INTERNAL int order_after_from_sparse(olap_store *s, const uint32_t *host_indexes, uint64_t n);
OLAP_INTERNAL int order_drillup(const olap_store *s, olap_store **out, int ndim, const uint32_t *old_len, const uint32_t *new_len,
                                const uint32_t *const *maps, int method);
OLAP_INTERNAL int order_after_dice(const olap_store *s, olap_store *out, int ndim, const uint32_t *old_len, const uint32_t *new_len,
                                   const int32_t *const *sel);
OLAP_INTERNAL int order_after_reorder(const olap_store *s, olap_store *out, int ndim, const uint32_t *old_len, const int32_t *perm);
OLAP_INTERNAL int order_after_drilldown(const olap_store *s, olap_store *out);
OLAP_INTERNAL int order_before_load(olap_store *mine);
OLAP_INTERNAL int order_after_load(olap_store *mine, const olap_store *his, int ndim, const uint32_t *my_len, const uint32_t *his_len,
                                   const int32_t *const *his_to_mine);
// a copy_select (olap_select.hip) is about to write n distinct cells of a tracked store: the order is made explicit and
// *seq / *seq_base say where the newly set cells go (nullptr: the store keeps no order)
OLAP_INTERNAL int order_before_select_write(olap_store *s, uint64_t n, uint32_t **seq, uint32_t *seq_base);
OLAP_INTERNAL void order_after_select_write(olap_store *s);
// host copy of the set cells' indices in insertion order (ascending when the store has no seq)
OLAP_INTERNAL int order_sorted_keys(const olap_store *s, std::vector<uint64_t> &keys);
// the untracked operations of olap_capi.hip (what the public entry points do for a store that is not tracked)
OLAP_INTERNAL int store_drillup_plain(const olap_store *s, olap_store **out, int ndim, const uint32_t *old_len, const uint32_t *new_len,
                                      const uint32_t *const *maps, int method);

// ---- filtered totals and copies (olap_select.hip) --------------------------------------------------
OLAP_INTERNAL int select_validate(const olap_store *store, int ndim, const uint32_t *lens, int nlev, const int *axis, const uint32_t *n_sel,
                                  const int32_t *const *sel, bool for_copy);
// order-free sum of one copy of the selected terms with its exactness certificate (lists per cube dimension)
OLAP_INTERNAL int select_cert(const olap_store *s, int ndim, const uint32_t *lens, const uint32_t *n_by_dim, const int32_t *const *sel_by_dim,
                              double *sum, double *abs_sum, int *min_exp, unsigned *flags);
// 1 and *total when the certificate proves the order-free sum (times m) equal to the sequential one
OLAP_INTERNAL int select_certified_total(double sum, double abs_sum, int min_exp, unsigned flags, double m, double *total);
// the program checks of olap_eval_formula (olap_capi.hip): length, operands, stack; *max_depth: the deepest the stack gets
OLAP_INTERNAL int check_formula(const int32_t *code, int n_code, int n_consts, int n_inputs, int n_scalars, int *max_depth = nullptr);
OLAP_INTERNAL int select_copy(olap_store *target, const olap_store *source, int ndim, const uint32_t *lens, int nlev, const int *axis,
                              const uint32_t *n_sel, const int32_t *const *sel);

// ---- batched setValue (olap_select.hip) ------------------------------------------------------------------------------
// the host checks of olap_store_set_values (NULL arguments, every index < size), before any device work
OLAP_INTERNAL int set_values_validate(const olap_store *store, uint64_t n, const uint64_t *indexes, const double *values);
OLAP_INTERNAL int set_values(olap_store *store, uint64_t n, const uint64_t *indexes, const double *values, const uint8_t *is_null);
