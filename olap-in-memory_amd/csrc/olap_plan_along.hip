// olap_plan_along.hip — the plans of the calls that run along one dimension: cumulate (kernels: olap_cumulate.hip, K13),
// rolling (olap_rolling.hip, K14), quantile (olap_quantile.hip, K15) and variance (olap_variance.hip, K16).  A dimension
// under its K -> G map becomes the view [outer, K, inner] with the map's CSR; what the four plans share is built once
// here (the description of the dimension, the table on the device, the start of a plan), and each builder adds what is
// its own: its view, its *_choose and its kernel name.  The olap_diag_*_choice entry points ask the same *_choose
// without a plan.  Host code only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "olap_plan.hpp"

namespace {

// One dimension of a cube under a K -> G map (map == nullptr: the whole dimension is one group).
struct AxisGroups {
  uint64_t outer, K, inner, G;
  std::vector<uint32_t> gstart, order;  // the CSR: members of group g are order[gstart[g] .. gstart[g + 1]) ascending
  bool contiguous = true;               // order is the identity: the groups are runs of the dimension
  uint32_t longest = 0;                 // members of the largest group

  AxisGroups(int ndim, const uint32_t *lens, int axis, uint32_t n_groups, const uint32_t *map)
      : outer(product(lens, axis)), K(lens[axis]), inner(product(lens + axis + 1, ndim - axis - 1)), G(map ? n_groups : 1) {
    if (map) {
      build_csr(map, lens[axis], n_groups, gstart, order);
      for (size_t j = 0; j < order.size(); ++j) contiguous = contiguous && order[j] == j;
    } else {
      gstart = {0, lens[axis]};
    }
    for (size_t g = 0; g + 1 < gstart.size(); ++g) longest = std::max(longest, gstart[g + 1] - gstart[g]);
  }
};

// The table of a plan on the device: gstart, then — interleaved groups only — order, then gtile where there is one.
// The three pointers are the view's (gtile_dev: nullptr for a view without group tiles).
int upload_groups(olap_plan *p, const AxisGroups &a, const std::vector<uint32_t> &gtile, const uint32_t *&gstart, const uint32_t *&order,
                  const uint32_t **gtile_dev) {
  std::vector<uint32_t> tab(a.gstart);
  const size_t order_off = tab.size();
  if (!a.contiguous) tab.insert(tab.end(), a.order.begin(), a.order.end());
  const size_t gtile_off = tab.size();
  tab.insert(tab.end(), gtile.begin(), gtile.end());
  if (const int rc = upload(&p->dev_tab, tab.data(), tab.size() * sizeof(uint32_t))) return rc;
  gstart = (const uint32_t *)p->dev_tab;
  order = a.contiguous ? nullptr : (const uint32_t *)p->dev_tab + order_off;
  if (gtile_dev) *gtile_dev = gtile.empty() ? nullptr : (const uint32_t *)p->dev_tab + gtile_off;
  return OLAP_OK;
}

// How every plan here starts.  `owner` destroys the plan on every return but the one that releases it into *out.
int begin_plan(olap_plan **out, PlanOwner &owner, PlanKind kind, int dtype, int default_kind, uint64_t in_cells, uint64_t out_cells) {
  *out = nullptr;
  if (const int rc = require_device()) return rc;
  owner.reset(new (std::nothrow) olap_plan());
  olap_plan *const p = owner.get();
  if (!p) return fail(OLAP_ERR_OUT_OF_MEMORY, "out of host memory");
  p->kind = kind;
  p->dtype = dtype;
  p->def_nan = default_kind == OLAP_DEFAULT_NAN;
  p->method = OLAP_SUM;
  p->in_cells = in_cells;
  p->out_cells = out_cells;
  return OLAP_OK;
}

// what every view holds of the dimension and the plan
template <typename View>
void view_shape(View &v, const AxisGroups &a, const olap_plan *p) {
  v.outer = a.outer, v.K = a.K, v.inner = a.inner;
  v.def_nan = p->def_nan;
}

// the tile of quantile and variance holds a mask beside the cells where the mask is primary (integer cells under a NaN default)
bool mask_tile(const olap_plan *p) { return p->def_nan && (p->dtype == OLAP_INT32 || p->dtype == OLAP_UINT32); }

// The column form's cut of the G groups into tiles of at most `rows` rows (host CSR; needs rows >= the largest group):
// tile t holds the groups [gtile[t], gtile[t + 1]).
std::vector<uint32_t> group_tiles(uint64_t G, uint32_t rows, const uint32_t *gstart) {
  std::vector<uint32_t> gtile{0};
  uint32_t g0 = 0;
  for (uint32_t g = 0; g < G; ++g) {
    if (g > g0 && gstart[g + 1] - gstart[g0] > rows) {  // group g no longer fits beside [g0, g): it opens the next tile
      gtile.push_back(g);
      g0 = g;
    }
  }
  gtile.push_back((uint32_t)G);
  return gtile;
}

// quantile's and variance's table, their *_choose done: the group tiles of the column form go behind the CSR
template <typename View>
int upload_grouped(olap_plan *p, const AxisGroups &a, View &v, bool column) {
  std::vector<uint32_t> gtile;
  if (column) {
    gtile = group_tiles(v.G, v.rows, a.gstart.data());
    v.n_gtile = (uint32_t)gtile.size() - 1;
  }
  return upload_groups(p, a, gtile, v.gstart, v.order, &v.gtile);
}

const char *quantile_kernel_name(int form) {
  return form == QUANTILE_COLUMN ? "quantile_column_kernel" : form == QUANTILE_ROW ? "quantile_rows_kernel"
         : form == QUANTILE_DIRECT_LANES ? "quantile_direct_kernel<lanes>" : "quantile_direct_kernel<block>";
}

const char *variance_kernel_name(int form) {
  return form == VARIANCE_COLUMN ? "variance_column_kernel" : form == VARIANCE_ROW ? "variance_rows_kernel"
         : form == VARIANCE_DIRECT_LANES ? "variance_direct_kernel<lanes>" : "variance_direct_kernel<block>";
}

// the argument checks of the olap_diag_*_choice entry points (longest: quantile's and variance's)
int check_choice(const char *what, int cell_bytes, const uint32_t *choice, uint64_t K, uint32_t longest = 0) {
  if (cell_bytes != 4 && cell_bytes != 8) return fail(OLAP_ERR_INVALID_ARGUMENT, "%s choice: cells of %d bytes", what, cell_bytes);
  if (!choice) return fail(OLAP_ERR_INVALID_ARGUMENT, "%s choice: NULL result", what);
  if (K > 0xFFFFFFFFull) return fail(OLAP_ERR_INVALID_ARGUMENT, "%s choice: a dimension of more than 2^32 - 1 items", what);
  if (longest > K) return fail(OLAP_ERR_INVALID_ARGUMENT, "%s choice: a group of %u of the dimension's %llu items", what, longest, (unsigned long long)K);
  return OLAP_OK;
}

// what olap_diag_quantile_choice and olap_diag_variance_choice report of a chosen view
template <typename View>
void report_choice(const View &v, uint32_t choice[6]) {
  choice[0] = (uint32_t)v.form, choice[1] = v.tile, choice[2] = v.series, choice[3] = v.pitch, choice[4] = v.cols, choice[5] = v.rows;
}

}  // namespace

int cumulate_plan(olap_plan **out, int dtype, int default_kind, int ndim, const uint32_t *lens, int axis, uint32_t n_groups, const uint32_t *map) {
  PlanOwner owner;
  const AxisGroups a(ndim, lens, axis, n_groups, map);
  const uint64_t cells = product(lens, ndim);  // a running cell per cell
  if (const int rc = begin_plan(out, owner, PLAN_CUMULATE, dtype, default_kind, cells, cells)) return rc;
  olap_plan *const p = owner.get();
  CumulateView &v = p->cum;
  view_shape(v, a, p);
  v.G = a.G;
  if (const int rc = upload_groups(p, a, {}, v.gstart, v.order, nullptr)) return rc;
  cumulate_choose(v, (int)olap_dtype_size(dtype), a.contiguous);
  p->kernel_name = v.form == CUMULATE_COLUMN ? (v.vec == 1 ? "cumulate_column_kernel<cell>" : "cumulate_column_kernel")
                   : v.form == CUMULATE_ROW_WHOLE ? "cumulate_rows_kernel" : "cumulate_rows_kernel<chunked>";
  *out = owner.release();
  return OLAP_OK;
}

int rolling_plan(olap_plan **out, int dtype, int default_kind, int ndim, const uint32_t *lens, int axis, int32_t before, int32_t after,
                 const uint32_t *map) {
  PlanOwner owner;
  const AxisGroups a(ndim, lens, axis, 1, nullptr);  // the shape only: the device gets the map as it is, not its CSR
  const uint64_t cells = product(lens, ndim);        // a window's cell per cell
  if (const int rc = begin_plan(out, owner, PLAN_ROLLING, dtype, default_kind, cells, cells)) return rc;
  olap_plan *const p = owner.get();
  RollingView &v = p->roll;
  view_shape(v, a, p);
  v.before = window_side(before, lens[axis]);
  v.after = window_side(after, lens[axis]);
  if (map)
    if (const int rc = upload(&p->dev_tab, map, (size_t)lens[axis] * sizeof(uint32_t))) return rc;
  v.map = (const uint32_t *)p->dev_tab;
  rolling_choose(v, (int)olap_dtype_size(dtype));
  p->kernel_name = v.form == ROLLING_DIRECT ? "rolling_direct_kernel" : v.form == ROLLING_COLUMNS ? "rolling_tiled_kernel<columns>" : "rolling_tiled_kernel<series>";
  *out = owner.release();
  return OLAP_OK;
}

int quantile_plan(olap_plan **out, int dtype, int default_kind, int ndim, const uint32_t *lens, int axis, uint32_t n_groups, const uint32_t *map) {
  PlanOwner owner;
  const AxisGroups a(ndim, lens, axis, n_groups, map);
  if (const int rc = begin_plan(out, owner, PLAN_QUANTILE, dtype, default_kind, product(lens, ndim), a.outer * a.G * a.inner)) return rc;
  olap_plan *const p = owner.get();
  QuantileView &v = p->quant;
  view_shape(v, a, p);
  v.G = a.G;
  v.tile = quantile_tile_cells((int)olap_dtype_size(dtype), mask_tile(p));
  v.longest = a.longest;
  quantile_choose(v, (int)olap_dtype_size(dtype));
  if (const int rc = upload_grouped(p, a, v, v.form == QUANTILE_COLUMN)) return rc;
  p->kernel_name = quantile_kernel_name(v.form);
  *out = owner.release();
  return OLAP_OK;
}

int variance_plan(olap_plan **out, int dtype, int default_kind, int ndim, const uint32_t *lens, int axis, uint32_t n_groups, const uint32_t *map) {
  PlanOwner owner;
  const AxisGroups a(ndim, lens, axis, n_groups, map);
  if (const int rc = begin_plan(out, owner, PLAN_VARIANCE, dtype, default_kind, product(lens, ndim), a.outer * a.G * a.inner)) return rc;
  olap_plan *const p = owner.get();
  VarianceView &v = p->var;
  view_shape(v, a, p);
  v.G = a.G;
  v.tile = variance_tile_cells((int)olap_dtype_size(dtype), mask_tile(p));
  v.block_members = variance_block_members(), v.block_cells = variance_block_cells();
  v.longest = a.longest;
  variance_choose(v, (int)olap_dtype_size(dtype));
  if (const int rc = upload_grouped(p, a, v, v.form == VARIANCE_COLUMN)) return rc;
  p->kernel_name = variance_kernel_name(v.form);
  *out = owner.release();
  return OLAP_OK;
}

extern "C" int olap_diag_rolling_choice(int cell_bytes, uint64_t outer, uint64_t K, uint64_t inner, int32_t before, int32_t after, int has_map,
                                        uint32_t choice[4]) {
  if (const int rc = check_choice("rolling", cell_bytes, choice, K)) return rc;
  if ((int64_t)before + after < 0) return fail(OLAP_ERR_INVALID_ARGUMENT, "rolling: empty window (before %d, after %d)", before, after);
  (void)has_map;  // the map travels as it is: it does not change the cuts
  RollingView v{};
  v.outer = outer, v.K = K, v.inner = inner;
  v.before = window_side(before, (uint32_t)K), v.after = window_side(after, (uint32_t)K);
  rolling_choose(v, cell_bytes);
  choice[0] = (uint32_t)v.form, choice[1] = v.series, choice[2] = v.rows, choice[3] = v.cols;
  return OLAP_OK;
}

extern "C" int olap_diag_quantile_choice(int cell_bytes, int has_mask, uint64_t outer, uint64_t K, uint64_t inner, uint32_t n_groups,
                                         uint32_t longest, int contiguous, uint32_t choice[6]) {
  if (const int rc = check_choice("quantile", cell_bytes, choice, K, longest)) return rc;
  (void)contiguous;  // interleaved groups are staged member by member: the cuts are the same
  QuantileView v{};
  v.outer = outer, v.K = K, v.inner = inner, v.G = n_groups;
  v.tile = quantile_tile_cells(cell_bytes, has_mask != 0);
  v.longest = longest;
  quantile_choose(v, cell_bytes);
  report_choice(v, choice);
  return OLAP_OK;
}

extern "C" int olap_diag_variance_choice(int cell_bytes, int has_mask, uint64_t outer, uint64_t K, uint64_t inner, uint32_t n_groups,
                                         uint32_t longest, int contiguous, uint32_t choice[6]) {
  if (const int rc = check_choice("variance", cell_bytes, choice, K, longest)) return rc;
  (void)contiguous;  // interleaved groups are staged member by member: the cuts are the same
  VarianceView v{};
  v.outer = outer, v.K = K, v.inner = inner, v.G = n_groups;
  v.tile = variance_tile_cells(cell_bytes, has_mask != 0);
  v.block_members = variance_block_members(), v.block_cells = variance_block_cells();
  v.longest = longest;
  variance_choose(v, cell_bytes);
  report_choice(v, choice);
  return OLAP_OK;
}
