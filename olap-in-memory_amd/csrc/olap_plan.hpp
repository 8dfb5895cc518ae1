// olap_plan.hpp — what a plan is and what its builders share (olap_capi.hip, olap_plan_drillup.hip, olap_plan_along.hip).
// Nothing here is exported.
#pragma once

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "olap_internal.hpp"
#include "olap_kernels.hpp"

enum PlanKind { PLAN_DRILLUP_AXIS, PLAN_DRILLUP_GENERIC, PLAN_GATHER, PLAN_LOAD, PLAN_DRILLDOWN, PLAN_BRICK, PLAN_GATHER_REDUCE, PLAN_COMPOSE, PLAN_CUMULATE, PLAN_ROLLING, PLAN_QUANTILE, PLAN_VARIANCE };

struct olap_plan {
  PlanKind kind;
  int dtype = 0, def_nan = 0, his_def_nan = 0, method = 0;
  int his_dtype = -1;                      // load between cell types: the other store's (>= 0 and != dtype: load_convert kernels)
  uint64_t in_cells = 0, out_cells = 0;
  int vec = 1;
  olap::DrillUpAxis axis{};
  olap::DrillUpGeneric gen{};
  olap::Remap remap{};
  olap::DrillDown dd{};
  olap::DrillDownScale dds{};
  olap::Brick brick{};
  uint64_t n_bricks = 0;
  olap::GatherReduce gr{};
  CumulateView cum{};                      // PLAN_CUMULATE (olap_cumulate.hip)
  RollingView roll{};                      // PLAN_ROLLING (olap_rolling.hip)
  QuantileView quant{};                    // PLAN_QUANTILE (olap_quantile.hip)
  VarianceView var{};                      // PLAN_VARIANCE (olap_variance.hip)
  bool xy_ok = false;                      // reorder without a mask: two-axis LDS transpose (olap_transpose.hip; 4- and 8-byte cells)
  TransposeXY xy{};
  olap::DrillUpReduce reduce{};            // S > 0: reduce regime of the one-axis drillUp
  olap::LoadPermute lperm{};               // lperm.perm != nullptr: load whose innermost items are permuted, nothing else (load_permute_rows_kernel)
  uint32_t longest_group = 0;              // one-axis drillUp: members of the longest group (olap_diag_plan_describe)
  olap::SegmentedRows seg{};               // S_tot > 0: wide rows of that regime run as the row kernel over segments + a fold (all rules but product)
  bool dd_two_pass = false;                // float cells, no distributions: scale + broadcast
  bool dice_direct = false;                // dice of one dimension, rows not whole 16-byte groups: dice_direct_kernel
  olap::DiceRows dice_rows{};
  bool dd_rows = false;                    // one refined axis, wide rows: drilldown_rows_kernel (uses `axis`)
  uint32_t dd_longest = 0;                 // children of the largest parent
  void *dev_tab2 = nullptr;                // second table set (two-pass drillDown)
  void *dev_tmp = nullptr;                 // quotients of the two-pass drillDown (old cells)
  std::vector<void *> owned;               // further device allocations freed with the plan
  void *dev_tab = nullptr;                 // index tables
  double *dev_dist = nullptr;              // drillDown distributions
  unsigned long long *dev_err = nullptr;   // drillDown deferred error word
  std::string kernel_name;
  hipStream_t last_stream = nullptr;
  bool ran = false;
  int device = 0;                          // the device the tables and scratch live on (current at creation)
  olap_plan() { (void)hipGetDevice(&device); }
  int cache_refs = 0;                      // handle-layer LRU: users between find() and release() (guarded by the cache lock)
  bool cache_evicted = false;              // evicted while in use: the last release() destroys it
};

// A plan under construction: destroyed with everything it owns on every return but the one that release()s it into *out.
struct PlanDestroy {
  void operator()(olap_plan *p) const { olap_plan_destroy(p); }
};
using PlanOwner = std::unique_ptr<olap_plan, PlanDestroy>;

// What a launch over p->axis runs with (olap_capi.hip, run section): buffers off the 16-byte grid take one cell per lane.
OLAP_INTERNAL olap::DrillUpAxis axis_for_launch(const olap_plan *p, bool aligned, int *vec);
// The form a PLAN_DRILLUP_AXIS plan runs in under `method` when every buffer is on the 16-byte grid and carries no mask:
// what olap_plan_kernel_name and olap_diag_plan_describe report.
inline olap::DrillUpChoice plan_drillup_form(const olap_plan *p, int method) {
  int vec;
  const olap::DrillUpAxis a = axis_for_launch(p, true, &vec);
  return olap::drillup_form(a, vec, olap_dtype_size(p->dtype), false, method, p->reduce, p->seg);
}

// OLAP_PLAN_DRY=1: plans are validated and BUILT without a device (see olap_capi.hip)
OLAP_INTERNAL bool plan_dry();
OLAP_INTERNAL uint64_t product(const uint32_t *v, int n);
OLAP_INTERNAL int check_dims(int ndim, const uint32_t *a, const uint32_t *b);
// pooled device memory holding `bytes` bytes of `host` (nullptr: uninitialised)
OLAP_INTERNAL int upload(void **dev, const void *host, size_t bytes);
// cells per 16-byte lane that divide `contiguous`
OLAP_INTERNAL int vec_for(int dtype, uint64_t contiguous);
OLAP_INTERNAL bool is_identity_u32(const uint32_t *m, uint32_t old_len, uint32_t new_len);
// CSR of a K->G map: members of each group in ascending order (counting sort, stable)
OLAP_INTERNAL void build_csr(const uint32_t *m, uint32_t K, uint32_t G, std::vector<uint32_t> &gstart, std::vector<uint32_t> &order);

// ---- plans of the calls along one dimension (olap_plan_along.hip) ----------------------------------------------------
// The arguments passed the checks of the call's entry point (olap_capi.hip); map == nullptr: the dimension is one group.
// Rules, q, kind and ddof are not part of a plan: they travel with the launch.
OLAP_INTERNAL int cumulate_plan(olap_plan **out, int dtype, int default_kind, int ndim, const uint32_t *lens, int axis, uint32_t n_groups,
                                const uint32_t *map);
OLAP_INTERNAL int rolling_plan(olap_plan **out, int dtype, int default_kind, int ndim, const uint32_t *lens, int axis, int32_t before, int32_t after,
                               const uint32_t *map);
OLAP_INTERNAL int quantile_plan(olap_plan **out, int dtype, int default_kind, int ndim, const uint32_t *lens, int axis, uint32_t n_groups,
                                const uint32_t *map);
OLAP_INTERNAL int variance_plan(olap_plan **out, int dtype, int default_kind, int ndim, const uint32_t *lens, int axis, uint32_t n_groups,
                                const uint32_t *map);
// rolling's before / after as the plan (and its cache key) holds them: beyond +-K they act as +-K
inline int64_t window_side(int32_t side, uint32_t K) { return std::max<int64_t>(-(int64_t)K, std::min<int64_t>(side, K)); }
