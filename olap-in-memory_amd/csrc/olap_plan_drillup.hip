// olap_plan_drillup.hip — olap_drillup_plan: the drillUp of the reference (InMemoryStore.drillUp, in-memory.js:265-334)
// folded into kernel views.  One changed dimension becomes the view [outer, K, inner] with the CSR of its K -> G map, and
// one step each prepares what a regime of the one-axis roll-up needs (tile permutation, group tiles, the cooperative
// reduce, segmented rows); WHICH regime a launch then runs in is drillup_form's decision (olap_kernels.hpp), here only
// asked for the plan's kernel name.  Several changed dimensions take the generic kernel.  Host code only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <new>
#include <vector>

#include "olap_plan.hpp"

using namespace olap;

namespace {

// The changed axis' groups: their CSR and what the steps below ask of it.
struct Groups {
  std::vector<uint32_t> gstart, order;
  uint32_t longest = 0, shortest = ~0u;  // members of the longest / shortest group
  bool contiguous = true;                // order is the identity: the groups are runs of the axis
};

// the statistics of a CSR
void group_statistics(Groups &g) {
  for (size_t j = 0; j < g.order.size(); ++j)
    if (g.order[j] != j) g.contiguous = false;
  for (size_t gi = 0; gi + 1 < g.gstart.size(); ++gi) {
    g.longest = std::max(g.longest, g.gstart[gi + 1] - g.gstart[gi]);
    g.shortest = std::min(g.shortest, g.gstart[gi + 1] - g.gstart[gi]);
  }
}

// CUs of the current device (dry planning: the MI355X's 256)
int device_cus() {
  int dev = 0, n = 0;
  const bool known = !plan_dry() && hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0;
  return known ? n : 256;
}

// How many pieces of `each` give every CU the same number of workgroups: k per CU for the smallest k in 2..8 that the
// pieces fill to >= 94 % (`per_k`: what one workgroup per CU holds, in the unit of `each`); 0 when no k does.
uint64_t balanced_per_cu(uint64_t per_k, uint64_t each) {
  for (uint64_t k = 2; k <= 8; ++k) {
    const uint64_t total = per_k * k, s_k = total / each;
    if (s_k >= 1 && each * s_k * 100 >= total * 94) return s_k;
  }
  return 0;
}

// The checks of olap_drillup_plan in the order they report; ident[d]: dimension d keeps its items.
int validate(olap_plan **out, int dtype, int default_kind, int method, int ndim, const uint32_t *old_len, const uint32_t *new_len,
             const uint32_t *const *maps, std::vector<bool> &ident) {
  if (!out) return fail(OLAP_ERR_INVALID_ARGUMENT, "plan out-pointer is NULL");
  *out = nullptr;
  int rc;
  if ((rc = check_dtype(dtype)) || (rc = check_default(default_kind))) return rc;
  if (method < OLAP_SUM || method > OLAP_PARTIAL_AVERAGE)
    return fail(OLAP_ERR_UNSUPPORTED_METHOD, "Unsupported aggregation method: %d", method);
  if ((rc = check_dims(ndim, old_len, new_len))) return rc;
  if (ndim > 0 && !maps) return fail(OLAP_ERR_INVALID_ARGUMENT, "maps is NULL");
  ident.assign(ndim, false);
  for (int d = 0; d < ndim; ++d) {
    if (old_len[d] && !maps[d]) return fail(OLAP_ERR_INVALID_ARGUMENT, "maps[%d] is NULL", d);
    for (uint32_t k = 0; k < old_len[d]; ++k)
      if (maps[d][k] >= new_len[d])
        return fail(OLAP_ERR_INDEX_RANGE, "drillUp map of dimension %d: entry %u = %u is outside the new dimension (%u items)", d, k, maps[d][k], new_len[d]);
    ident[d] = is_identity_u32(maps[d], old_len[d], new_len[d]);
  }
  return require_device();
}

// the CSR on the device: gstart, then — interleaved groups only — order
int plan_csr(olap_plan *p, const Groups &g) {
  DrillUpAxis &a = p->axis;
  std::vector<uint32_t> tab(g.gstart);
  const size_t order_off = tab.size();
  if (!g.contiguous) tab.insert(tab.end(), g.order.begin(), g.order.end());
  if (const int rc = upload(&p->dev_tab, tab.data(), tab.size() * sizeof(uint32_t))) return rc;
  a.gstart = (const uint32_t *)p->dev_tab;
  a.order = g.contiguous ? nullptr : (const uint32_t *)p->dev_tab + order_off;
  return OLAP_OK;
}

// row-tile regime with interleaved groups (drillup_tile_kernel MODE 3): where every cell of a row goes in
// the permuted tile
int plan_tile_perm(olap_plan *p, const Groups &g) {
  DrillUpAxis &a = p->axis;
  a.perm_cell = a.perm_grp = nullptr;
  a.perm_pitch = 0;
  const uint64_t budget = kTileBytes / olap_dtype_size(p->dtype);
  if (g.contiguous || a.inner == 0 || a.inner >= 4096 || a.K * a.inner > budget) return OLAP_OK;
  TilePerm tp;
  tile_perm_build(g.gstart.data(), g.order.data(), (uint32_t)a.K, (uint32_t)a.G, (uint32_t)a.inner, budget, 16 / olap_dtype_size(p->dtype), &tp);
  std::vector<uint32_t> both(tp.cell);
  both.insert(both.end(), tp.grp.begin(), tp.grp.end());
  void *dev_perm = nullptr;
  if (const int rc = upload(&dev_perm, both.data(), both.size() * sizeof(uint32_t))) return rc;
  p->owned.push_back(dev_perm);
  a.perm_cell = (const uint32_t *)dev_perm;
  a.perm_grp = (const uint32_t *)dev_perm + tp.cell.size();
  a.perm_pitch = tp.pitch;
  return OLAP_OK;
}

// group-tile regime (drillup_gtile_kernel): contiguous groups, short row pieces, rows too long for
// the row-tile regime; the group list is cut into tiles of whole groups that fit kTileBytes
int plan_gtile(olap_plan *p, const Groups &g) {
  DrillUpAxis &a = p->axis;
  a.gtile = nullptr;
  a.n_gtile = 0;
  const uint64_t budget = kTileBytes / olap_dtype_size(p->dtype);
  const uint64_t vcells = 16 / olap_dtype_size(p->dtype);
  uint64_t gtile_max_slots = 128;
  if (const char *e = getenv("OLAP_GTILE_MAX_SLOTS")) gtile_max_slots = (uint64_t)atoll(e);  // developer knob
  if (!(g.contiguous && a.G > 1 && a.inner > 0 && a.inner / (uint64_t)p->vec < gtile_max_slots && a.K * a.inner > budget && !getenv("OLAP_NO_GTILE")))
    return OLAP_OK;
  std::vector<uint32_t> cut{0};
  uint64_t cells = 0;
  uint32_t groups = 0;
  bool fits = true;
  for (uint32_t gi = 0; gi < a.G && fits; ++gi) {
    const uint64_t c = (uint64_t)(g.gstart[gi + 1] - g.gstart[gi]) * a.inner;
    if (c > budget - vcells) fits = false;
    if (cells + c > budget - vcells || groups == kGroupTileMaxGroups) {
      cut.push_back(gi);
      cells = 0;
      groups = 0;
    }
    cells += c;
    ++groups;
  }
  cut.push_back((uint32_t)a.G);
  // a tile reduces groups-in-tile x inner output cells, one lane each: with a long group or two
  // per tile most of the workgroup idles and the flat form is faster ([3001,3333,10] -> 11 groups
  // of 303 members: 145 us here, 89 us flat) — unless every group is long enough for several lanes to share an
  // output cell (>= 256 members: the kernel's cooperative form)
  const bool coop = g.shortest >= 256 && !getenv("OLAP_GTILE_NO_COOP");  // (whatever the rule: a plan's tables do not depend on it)
  // (short groups too: a lane's work is its group's members, so a tile with few output cells is cheap when those are
  // few — day -> month over 8-byte cells with the day innermost: 67 months per tile, 31 LDS reads each; 320 us flat)
  const bool enough_lanes = a.G * a.inner >= 64 * (cut.size() - 1) || coop || g.longest <= 64;
  if (!(fits && enough_lanes && a.outer * (cut.size() - 1) < 0x7FFFFFFFull)) return OLAP_OK;
  void *dev_cut = nullptr;
  if (const int rc = upload(&dev_cut, cut.data(), cut.size() * sizeof(uint32_t))) return rc;
  p->owned.push_back(dev_cut);
  a.gtile = (const uint32_t *)dev_cut;
  a.n_gtile = (uint32_t)(cut.size() - 1);
  a.min_group = coop ? g.shortest : 0;
  return OLAP_OK;
}

// few output cells and long groups: cooperative reduction of S segments per group (workspace
// in the plan), see DrillUpReduce.  Sizes p->reduce but for its workspace; 0: the roll-up is not of that kind.
uint64_t size_reduce(olap_plan *p, const Groups &g) {
  const DrillUpAxis &a = p->axis;
  const uint32_t longest = g.longest;
  const size_t cell = olap_dtype_size(p->dtype);
  const uint64_t cells = a.outer * a.G * a.inner;
  // (a wavefront per 271-cell row was tried for more outputs than this: 260 us against the tile's 103)
  uint64_t reduce_max_cells = 131072;
  if (const char *e = getenv("OLAP_REDUCE_MAX_CELLS")) reduce_max_cells = (uint64_t)atoll(e);  // developer / test knob: who takes small outputs
  if (!(cells > 0 && cells < reduce_max_cells && longest >= 256)) return 0;
  DrillUpReduce &rd = p->reduce;
  uint64_t S;
  // (rows of up to 1 024 four-byte cells too when the 16-byte form below applies — one contiguous '-> all' group
  // whose steps are whole 16-byte groups: a unit then streams its segment as ONE contiguous range, 1-7 rows per
  // step, where the lane-per-cell split form reads 4 KB pieces a row apart: [4e5,250] -> [1,250] 88 us -> see DESIGN K1r)
  // (V = cells per 16 bytes; the smallest whole number of rows that is whole 16-byte groups must fit a unit's lanes)
  const uint64_t V16 = 16 / cell;
  uint64_t rows_min = 1;
  while ((rows_min * a.inner) % V16 != 0) rows_min *= 2;
  const bool wide16 = a.inner > 128 && rows_min * a.inner <= (uint64_t)kBlock * V16 && g.contiguous && a.G == 1 && (a.K * a.inner) % V16 == 0 &&
                      !getenv("OLAP_REDUCE_NO_WIDE");
  if (a.inner <= 128 || wide16) {
    const uint64_t groups = a.outer * a.G;
    // Segments per group.  More, shorter segments lose to the per-unit epilogue and to the partials they write
    // and the merge reads back ([1e6,100] -> [1,100] with 4 096 units: 81 us; with 512: 65 us); fewer leave CUs
    // idle.  Workgroup-sized units are few enough to be resident all at once, so what matters is that every CU gets
    // the same number: k per CU for the smallest k in 2..8 that the groups fill to >= 94 % (1 per CU is slower:
    // 84-100 us); with more groups than that the dispatcher balances ~4 K units by itself (tools/reduce_units.py).
    uint64_t by_grid = (4096 + groups - 1) / groups;
    if (const char *e = getenv("OLAP_REDUCE_UNITS")) by_grid = std::max<uint64_t>(1, (uint64_t)atoll(e) / groups);
    else if (const uint64_t s_k = balanced_per_cu((uint64_t)device_cus(), groups)) by_grid = s_k;
    const uint64_t by_work = std::max<uint64_t>(1, (uint64_t)longest * a.inner / 8192);  // >= 8 K cells each
    S = std::max<uint64_t>(1, std::min(by_grid, by_work));
    // short segments: a wavefront per segment; long ones: the whole workgroup
    const uint64_t seg_cells = ((uint64_t)longest + S - 1) / S * a.inner;
    rd.unit = (seg_cells <= 16384 && a.inner <= 64) ? 64 : kBlock;
    uint32_t rows = 1;
    while (rows * 2 * a.inner <= (uint64_t)rd.unit) rows *= 2;
    rd.rows = rows;
    // 16 B form: one contiguous '-> all' group, whole rows and segments in multiples of 4 cells
    uint64_t seg_len = ((uint64_t)longest + S - 1) / S;
    seg_len = (seg_len + 3) & ~3ull;
    // rows per step: a power of two whose cells are whole 16-byte groups (4-byte cells: 1 for rows of a multiple of 4
    // cells, 2 for even rows, 4 otherwise; 8-byte cells: 1 for even rows, 2 otherwise), doubled while the unit's lanes hold them
    uint32_t rows4 = (uint32_t)rows_min;
    while ((uint64_t)rows4 * 2 * a.inner <= (uint64_t)rd.unit * V16) rows4 *= 2;
    if (rows4 < V16 && a.inner <= 128) rows4 = (uint32_t)V16;  // (narrow rows: as before)
    if (g.contiguous && a.G == 1 && (a.K * a.inner) % V16 == 0 && (uint64_t)rows4 * a.inner <= (uint64_t)rd.unit * V16) {
      // as many rows per step as the unit's lanes hold (whole 16-byte groups): 10 rows of 100 cells fill 250 of 256
      // lanes where the power of two below fills 200; the rows are then merged through LDS instead of lane to lane
      uint64_t rows_any = (uint64_t)rd.unit * V16 / a.inner;
      while (rows_any > rows4 && (rows_any * a.inner) % V16 != 0) --rows_any;
      if (a.inner * 2 > V16 && rows_any * 10 >= (uint64_t)rows4 * 11 && !getenv("OLAP_REDUCE_POW2_ROWS")) rows4 = (uint32_t)rows_any;
      rd.vec4 = 1;
      rd.rows = rows4;
      rd.seg_len = (uint32_t)seg_len;
    } else if (g.contiguous && a.G == 1 && a.inner == 1) {
      // rows at any cell offset: aligned 16-byte groups with masked ends (every lane of the unit busy)
      rd.vec4 = 1;
      rd.edge = 1;
      rd.rows = rd.unit * (uint32_t)V16;
      rd.seg_len = (uint32_t)seg_len;
    }
  } else {
    rd.rows = 0;
    rd.unit = kBlock;
    S = std::max<uint64_t>(1, std::min<uint64_t>((524288 + cells - 1) / cells, longest / 32));
    // 16-byte lanes (drillup_split4_kernel): four output cells per lane; as many segments as give every CU the same
    // number of workgroups (k per CU, smallest k in 2..8 filled to >= 94 %), each of at least 32 members
    if (cell == 4 && a.inner % 4 == 0 && !getenv("OLAP_NO_SPLIT4")) {
      rd.vec4 = 1;
      const uint64_t cus = (uint64_t)device_cus();
      const uint64_t lanes_per_seg = cells / 4;
      uint64_t s_bal = balanced_per_cu(cus * kBlock, lanes_per_seg);
      if (!s_bal) s_bal = std::max<uint64_t>(1, cus * 8 * kBlock / lanes_per_seg);
      if (const char *e = getenv("OLAP_SPLIT_K")) s_bal = std::max<uint64_t>(1, cus * (uint64_t)atoll(e) * kBlock / lanes_per_seg);  // developer knob: workgroups per CU
      S = std::max<uint64_t>(1, std::min<uint64_t>(s_bal, longest / 32));
    }
  }
  rd.S = (uint32_t)S;
  if (!rd.vec4 || rd.rows == 0) rd.seg_len = (uint32_t)((longest + S - 1) / S);
  return S;
}

// Wide rows of the reduce regime (beyond the cooperative forms): the row kernel over SEGMENTS of the groups + a fold (see
// SegmentedRows) — as many segments as give the chip ~8 workgroups per CU, at least 16 members each.  Never when
// planning dry.
int plan_segments(olap_plan *p, const Groups &g) {
  const DrillUpAxis &a = p->axis;
  if (!(p->reduce.rows == 0 && !plan_dry() && !getenv("OLAP_NO_SEGMENTED_ROWS") && a.inner / (uint64_t)p->vec >= 128 &&
        a.inner * olap_dtype_size(p->dtype) >= 2048))
    return OLAP_OK;
  const uint64_t cus = (uint64_t)device_cus();
  const uint64_t n_vec = a.inner / (uint64_t)p->vec, bpr = (n_vec + kBlock - 1) / kBlock;
  // (two workgroups per CU with four rows in flight per lane: [1e4,1e4] -> [1,1e4] 62.9 us; eight per CU with one
  // row in flight, as the plain row regime runs: 75-77 us — four times the partials to write and to fold)
  uint64_t per_cu = 2;
  if (const char *e = getenv("OLAP_SEG_WG_PER_CU")) per_cu = std::max<uint64_t>(1, (uint64_t)atoll(e));  // developer knob
  const uint64_t want = std::max<uint64_t>(1, cus * per_cu / std::max<uint64_t>(1, a.outer * bpr));
  const uint64_t seg_len = std::max<uint64_t>(16, (a.K + want - 1) / want);
  std::vector<uint32_t> sg_gstart{0}, sg_first{0};
  for (uint64_t gi = 0; gi < a.G; ++gi) {
    for (uint64_t j = g.gstart[gi]; j < g.gstart[gi + 1]; j += seg_len) sg_gstart.push_back((uint32_t)std::min<uint64_t>(j + seg_len, g.gstart[gi + 1]));
    sg_first.push_back((uint32_t)sg_gstart.size() - 1);
  }
  const uint64_t s_tot = sg_gstart.size() - 1;
  void *d_g = nullptr, *d_f = nullptr, *d_p = nullptr, *d_a = nullptr;
  int rc = OLAP_OK;
  if (s_tot > a.G && a.outer * s_tot * bpr < 0x7FFFFFFFull && !(rc = upload(&d_g, sg_gstart.data(), sg_gstart.size() * 4)) &&
      !(rc = upload(&d_f, sg_first.data(), sg_first.size() * 4))) {
    hipError_t e1 = dev_alloc(&d_p, a.outer * s_tot * a.inner * sizeof(double));
    if (e1 == hipSuccess) e1 = dev_alloc(&d_a, a.outer * s_tot * a.inner * sizeof(int32_t));
    if (e1 == hipSuccess) {
      p->seg.S_tot = (uint32_t)s_tot;
      p->seg.gstart = (const uint32_t *)d_g;
      p->seg.seg_start = (const uint32_t *)d_f;
      p->seg.partial = d_p;
      p->seg.aux = (int32_t *)d_a;
    } else {
      (void)hipGetLastError();  // no room for the partials: the split forms need less
    }
  }
  for (void *q : {d_g, d_f, d_p, d_a})
    if (q) p->owned.push_back(q);
  return rc;
}

// the reduce regime's partials: one per output cell and segment
int plan_reduce_workspace(olap_plan *p, uint64_t S) {
  const hipError_t e = dev_alloc(&p->dev_tmp, p->axis.outer * p->axis.G * p->axis.inner * S * sizeof(Partial));
  if (e != hipSuccess) return hip_fail(e, "hipMalloc(drillUp reduce workspace)");
  p->reduce.part = (Partial *)p->dev_tmp;
  return OLAP_OK;
}

// One changed axis (or none: then the whole cube is a single untouched "axis" of length 1).
int plan_axis(olap_plan *p, int ndim, const uint32_t *old_len, const uint32_t *new_len, const uint32_t *const *maps, int changed) {
  p->kind = PLAN_DRILLUP_AXIS;
  DrillUpAxis &a = p->axis;
  Groups g;
  if (changed >= 0) {
    a.outer = product(old_len, changed);
    a.K = old_len[changed];
    a.G = new_len[changed];
    a.inner = product(old_len + changed + 1, ndim - changed - 1);
    build_csr(maps[changed], old_len[changed], new_len[changed], g.gstart, g.order);  // (a dimension without items may come with a NULL map)
  } else {
    a.outer = a.K = a.G = 1;
    a.inner = p->in_cells;
    g.gstart = {0, 1}, g.order = {0};
  }
  group_statistics(g);
  p->longest_group = g.longest;
  p->vec = vec_for(p->dtype, a.inner);
  a.def_nan = p->def_nan;
  a.min_group = a.depth = 0;
  int rc;
  if ((rc = plan_csr(p, g)) || (rc = plan_tile_perm(p, g)) || (rc = plan_gtile(p, g))) return rc;
  if (const uint64_t S = size_reduce(p, g))
    if ((rc = plan_segments(p, g)) || (rc = plan_reduce_workspace(p, S))) return rc;
  p->kernel_name = drillup_form_kernels(plan_drillup_form(p, p->method));
  return OLAP_OK;
}

// Several changed dimensions: drillup_generic_kernel over the merged dimensions.
int plan_generic(olap_plan *p, int ndim, const uint32_t *old_len, const uint32_t *new_len, const uint32_t *const *maps,
                 const std::vector<bool> &ident) {
  int rc;
  p->kind = PLAN_DRILLUP_GENERIC;
  DrillUpGeneric &g = p->gen;
  std::vector<uint32_t> tab;
  std::vector<uint64_t> old_stride(ndim);
  {
    uint64_t s = 1;
    for (int d = ndim - 1; d >= 0; --d) {
      old_stride[d] = s;
      s *= old_len[d];
    }
  }
  int nd = 0;
  for (int d = 0; d < ndim; ++d) {
    if (ident[d] && nd > 0 && g.csr[nd - 1] < 0 && ident[d - 1]) {
      // merge with the previous identity dim
      g.new_len[nd - 1] *= new_len[d];
      g.old_stride[nd - 1] = old_stride[d];
      continue;
    }
    if (nd == kMaxDims) return fail(OLAP_ERR_INVALID_ARGUMENT, "drillUp: more than %d non-mergeable dimensions", kMaxDims);
    g.new_len[nd] = new_len[d];
    g.old_stride[nd] = old_stride[d];
    if (ident[d]) {
      g.csr[nd] = -1;
      g.ord[nd] = -1;
    } else {
      std::vector<uint32_t> gstart, order;
      build_csr(maps[d], old_len[d], new_len[d], gstart, order);
      const uint32_t ord_base = (uint32_t)(tab.size() + gstart.size());
      g.csr[nd] = (int32_t)tab.size();
      g.ord[nd] = 0;  // gstart entries index straight into `tab` (absolute)
      for (auto &x : gstart) x += ord_base;
      tab.insert(tab.end(), gstart.begin(), gstart.end());
      tab.insert(tab.end(), order.begin(), order.end());
    }
    ++nd;
  }
  g.nd = nd;
  g.total = p->out_cells;
  g.def_nan = p->def_nan;
  if ((rc = upload(&p->dev_tab, tab.data(), tab.size() * sizeof(uint32_t)))) return rc;
  g.tab = (const uint32_t *)p->dev_tab;
  p->kernel_name = drillup_form_kernels(DrillUpChoice{FORM_GENERIC});
  return OLAP_OK;
}

}  // namespace

extern "C" int olap_drillup_plan(olap_plan **out, int dtype, int default_kind, int method, int ndim,
                                 const uint32_t *old_len, const uint32_t *new_len,
                                 const uint32_t *const *maps) {
  std::vector<bool> ident;
  int rc;
  if ((rc = validate(out, dtype, default_kind, method, ndim, old_len, new_len, maps, ident))) return rc;
  int n_changed = 0, changed = -1;
  for (int d = 0; d < ndim; ++d)
    if (!ident[d]) ++n_changed, changed = d;
  PlanOwner owner(new (std::nothrow) olap_plan());  // destroyed on every return but the one that releases it into *out
  olap_plan *const p = owner.get();
  if (!p) return fail(OLAP_ERR_OUT_OF_MEMORY, "out of host memory");
  p->dtype = dtype;
  p->def_nan = default_kind == OLAP_DEFAULT_NAN;
  p->method = method;
  p->in_cells = product(old_len, ndim);
  p->out_cells = product(new_len, ndim);
  if ((rc = n_changed <= 1 ? plan_axis(p, ndim, old_len, new_len, maps, changed) : plan_generic(p, ndim, old_len, new_len, maps, ident))) return rc;
  *out = owner.release();
  return OLAP_OK;
}
