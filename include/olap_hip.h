/*
 * olap_hip.h — C ABI of libolapgpu, the MI355X (gfx950) implementation of the
 * olap-in-memory cube aggregation path.
 *
 * The reference (Growblocks/olap-in-memory @ 2024_08_07) has no FFI: its seam for this path
 * is the `InMemoryStore` class, src/store/in-memory.js, which `Cube` constructs at
 * src/cube.js:172-176 / :198-202 and calls at :1013 (drillUp), :938 / :979 (drillDown),
 * :628 / :826 / :851 (dice), :778 (reorder), :741 (load).  Every entry point below cites the
 * reference method it replaces.  The Node.js host (olap-in-memory_amd/js) binds these through
 * the N-API addon (olap-in-memory_amd/napi); Python hosts (bench.py, tests) bind them with
 * ctypes.  See INTEGRATION.md for the reference-side binding.
 *
 * Data model (dense restatement of the reference's Map<flatIndex, number>):
 *   values : one element per cell, row-major over the cube's dimensions, last dimension
 *            fastest (src/cube.js:709-728), element type = the measure's declared type;
 *   status : Int32 per cell, bit OLAP_STATUS_SET (0x2) <=> the reference Map holds the key.
 *   A cell is "set" iff (status == NULL || status[i] & 0x2) and values[i] is not the
 *   measure's default (setValue deletes default-valued keys, in-memory.js:122-133; for an
 *   integer type with NaN default no value is the default, so status alone decides).
 *   Outputs always hold the default in unset cells (0 for integer types) and an exact mask.
 *
 * All pointers named `*_values`, `*_status`, `workspace` are DEVICE pointers; everything
 * else is host memory.  Functions return OLAP_OK or a negative olap_error; the message of
 * the last failure on the calling thread is olap_last_error().  Arguments are validated
 * before the device is touched, so argument errors are identical with and without a GPU.
 * Nothing here falls back to the CPU: without a usable device the calls fail with
 * OLAP_ERR_NO_DEVICE.
 */
#ifndef OLAP_HIP_H
#define OLAP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OLAP_ABI_VERSION 2
#define OLAP_MAX_DIMS 32
#define OLAP_STATUS_SET 0x2 /* README.md:714-716: the only status bit the reference code implements */

/* in-memory.js:59 — ['int32','uint32','float32','float64'] */
typedef enum { OLAP_INT32 = 0, OLAP_UINT32 = 1, OLAP_FLOAT32 = 2, OLAP_FLOAT64 = 3 } olap_dtype;
/* in-memory.js:56-57 — only NaN and 0 are legal defaults */
typedef enum { OLAP_DEFAULT_ZERO = 0, OLAP_DEFAULT_NAN = 1 } olap_default;
/* in-memory.js:282-290 */
typedef enum {
  OLAP_SUM = 0,
  OLAP_AVERAGE = 1,
  OLAP_HIGHEST = 2,
  OLAP_LOWEST = 3,
  OLAP_FIRST = 4,
  OLAP_LAST = 5,
  OLAP_PRODUCT = 6,
  /* Not a reference method.  The shard-local half of `sum` / `average` for a cube partitioned across GPUs
   * (drillUp plans only).  out_values is a FLOAT64 buffer whatever the cell type: it receives the float64
   * accumulator itself — the undivided, unrounded sum of the set cells, 0 where nothing contributed (never
   * NaN) — because the reference adds all contributions of a cell in float64 and rounds never
   * (in-memory.js:282-290); out_status (optional) receives the NUMBER of contributions, not a mask.  Ranks add
   * both; the sums are rounded to the cell type once, after the division for `average`
   * (olap_shard_recipe: OLAP_FINISH_ROUND / OLAP_FINISH_AVERAGE). */
  OLAP_PARTIAL_AVERAGE = 7
} olap_method;

typedef enum {
  OLAP_OK = 0,
  OLAP_ERR_INVALID_ARGUMENT = -1,
  OLAP_ERR_INVALID_TYPE = -2,        /* 'Invalid type'                                 in-memory.js:60 */
  OLAP_ERR_INVALID_DEFAULT = -3,     /* 'Invalid default value, only NaN and 0 ...'    in-memory.js:57 */
  OLAP_ERR_UNSUPPORTED_METHOD = -4,  /* 'Unsupported aggregation method: <m>'          in-memory.js:295 */
  OLAP_ERR_LENGTH_MISMATCH = -5,     /* 'value length is invalid: a !== b'             in-memory.js:41-43 */
  OLAP_ERR_DISTRIBUTION_MISSING = -6,/* 'distribution missing for index <i>'           in-memory.js:398 */
  OLAP_ERR_NO_DEVICE = -7,
  OLAP_ERR_HIP = -8,
  OLAP_ERR_OUT_OF_MEMORY = -9,
  OLAP_ERR_INDEX_RANGE = -10
} olap_error;

const char *olap_last_error(void);
int olap_abi_version(void);
/* 'sum' | 'average' | 'highest' | 'lowest' | 'first' | 'last' | 'product' -> olap_method, or
 * OLAP_ERR_UNSUPPORTED_METHOD (message = the reference's).  NULL means the default, 'sum'. */
int olap_method_from_name(const char *name);
/* 'int32' | 'uint32' | 'float32' | 'float64' -> olap_dtype, or OLAP_ERR_INVALID_TYPE */
int olap_dtype_from_name(const char *name);
size_t olap_dtype_size(int dtype);

/* Number of HIP devices visible (0 when none / no driver); selects the device used by the
 * calling thread's subsequent calls (hipSetDevice). */
int olap_device_count(void);
int olap_set_device(int device);
int olap_device_synchronize(void);

/* ------------------------------------------------------------------------------------------
 * Plans: an op's small host-side tables (per-dimension index maps) are validated, folded into
 * a launch plan and uploaded once; olap_plan_run() is then pure kernel launches on `stream`
 * (a hipStream_t, NULL = the null stream) and may be captured into a hipGraph.  A plan may be
 * run any number of times on buffers of the planned sizes.  It belongs to the device that was
 * current when it was built (its tables and scratch live there; running it with another device
 * current fails with OLAP_ERR_INVALID_ARGUMENT), it is not thread-safe, and because the reduce
 * regimes keep their scratch in the plan it must not run on two streams at once.
 * ---------------------------------------------------------------------------------------- */
typedef struct olap_plan olap_plan;

/* InMemoryStore.drillUp(oldDimensions, newDimensions, method) — in-memory.js:265-334.
 * maps[d] has old_len[d] entries: old root index -> new index (< new_len[d]); this is
 * oldDimensions[d].getGroupIndexFromRootIndexMap(newDimensions[d].rootAttribute) (:270-274).
 * Semantics kept from the reference: only set cells contribute; float64 accumulation in
 * ascending flat-index order; `average` divides by the number of contributions modulo 65536
 * (Uint16Array, :278/:320) and leaves the sum when that is 0; a cell whose running value equals
 * the default is dropped and restarts (:126-131); Math.max/Math.min NaN propagation. */
int olap_drillup_plan(olap_plan **plan, int dtype, int default_kind, int method, int ndim,
                      const uint32_t *old_len, const uint32_t *new_len,
                      const uint32_t *const *maps);

/* InMemoryStore.drillDown(oldDimensions, newDimensions, method, distributions) — :336-430.
 * maps[d] has new_len[d] entries: new root index -> old index (< old_len[d]) (:349-353).
 * distributions: NULL or n_dist float64 weights (NaN entry = JS null/undefined => the run
 * fails with OLAP_ERR_DISTRIBUTION_MISSING if a contributing cell needs it, :397-398).
 * method: OLAP_SUM splits the parent between its children, anything else copies it (:421-423).
 * The reference decides "integers: spread the remainder one by one" by the measure's DECLARED type
 * (:343), while its cells are float64 numbers until serialize() (:77-92).  A host that wants exactly
 * that — int32 / uint32 measures whose intermediate values keep fractions and never wrap — holds them
 * in OLAP_FLOAT64 cells and ORs OLAP_DRILLDOWN_INTEGER_MEASURE into `method`; the remainder rule
 * (:403-417) then runs on the float64 cells.  Int32 / Uint32 cells always use it. */
#define OLAP_DRILLDOWN_INTEGER_MEASURE 0x100
int olap_drilldown_plan(olap_plan **plan, int dtype, int default_kind, int method, int ndim,
                        const uint32_t *old_len, const uint32_t *new_len,
                        const uint32_t *const *maps, const double *distributions,
                        uint64_t n_dist);

/* InMemoryStore.dice(oldDimensions, newDimensions) — :213-263.
 * sel[d] has new_len[d] entries: new index -> old index, or -1 when the new item does not exist
 * in the old dimension (:219-224; such rows stay unset). */
int olap_dice_plan(olap_plan **plan, int dtype, int default_kind, int ndim,
                   const uint32_t *old_len, const uint32_t *new_len, const int32_t *const *sel);

/* Fused dice -> drillUp (the slice / dice / drillUp chains of src/cube.js:799-857 + :995-1023):
 * equivalent to olap_dice_plan(old_len -> mid_len, sel) followed by olap_drillup_plan(mid_len ->
 * new_len, maps, method) with ONE rolled-up dimension, but the selection tables are folded into the
 * reduction's address computation, so only the surviving cells are read, once, and the diced
 * intermediate cube is never written.  More than one non-identity map: OLAP_ERR_INVALID_ARGUMENT
 * (run the two plans instead). */
int olap_dice_drillup_plan(olap_plan **plan, int dtype, int default_kind, int method, int ndim,
                           const uint32_t *old_len, const uint32_t *mid_len, const uint32_t *new_len,
                           const int32_t *const *sel, const uint32_t *const *maps);

/* InMemoryStore.reorder(oldDimensions, newDimensions) — :178-211.  New axis i is old axis perm[i]. */
int olap_reorder_plan(olap_plan **plan, int dtype, int default_kind, int ndim,
                      const uint32_t *old_len, const int32_t *perm);

/* InMemoryStore.load(otherStore, myDimensions, hisDimensions) — :139-176.  his_to_mine[d] has
 * his_len[d] entries: his index -> my index (or -1: skipped).  `in` of olap_plan_run is the
 * other store (his default kind given here), `out` is this store and is updated in place. */
int olap_load_plan(olap_plan **plan, int dtype, int my_default_kind, int his_default_kind,
                   int ndim, const uint32_t *my_len, const uint32_t *his_len,
                   const int32_t *const *his_to_mine);
/* The same between stores whose cell types may differ: `in` holds cells of his_dtype, `out` cells of my_dtype.  The
 * result is, cell for cell and mask for mask, what olap_convert_from_f64 of the other store's float64 values into
 * my_dtype cells under HIS default, followed by a same-type load, leaves — in one pass, without a cube in between
 * ("load between cell types").  his_dtype == my_dtype is olap_load_plan.  Between cell types a load with
 * only the last dimension permuted runs the remapped-innermost form (olap_plan_kernel_name says so). */
int olap_load_plan_typed(olap_plan **plan, int my_dtype, int his_dtype, int my_default_kind, int his_default_kind,
                         int ndim, const uint32_t *my_len, const uint32_t *his_len,
                         const int32_t *const *his_to_mine);
/* The plan olap_store_compose_multi runs for stores of this cell type and default (below): a gather over MY cells with
 * the item maps inverted on the host.  `in` of olap_plan_run is the other store, `out` a store of my_len cells of which
 * EVERY cell is written (no fill: cells without a cell of his end unset).  olap_plan_kernel_name tells the form:
 * "compose_gather (16-byte lanes)" or "compose_gather (16-byte runs of this store)". */
int olap_compose_plan(olap_plan **plan, int dtype, int default_kind, int ndim, const uint32_t *my_len,
                      const uint32_t *his_len, const int32_t *const *his_to_mine);

uint64_t olap_plan_in_cells(const olap_plan *plan);
uint64_t olap_plan_out_cells(const olap_plan *plan);
/* name of the kernel variant the plan selected (diagnostics / profiles) */
const char *olap_plan_kernel_name(const olap_plan *plan);

/* in_status may be NULL (every cell whose value is not the default is set).  out_status may be
 * NULL when the caller does not need the mask.  Buffers must not alias.  Asynchronous: returns
 * once the work is enqueued on `stream`. */
int olap_plan_run(olap_plan *plan, const void *in_values, const int32_t *in_status,
                  void *out_values, int32_t *out_status, void *stream);
/* The same plan over n independent (input, output) buffer pairs — the stored measures of a cube that share cell
 * type, default and rule: Cube.drillUp calls the store once per measure (src/cube.js:1012-1020), and on cubes of a
 * few MB a launch costs more than the bytes it moves.  drillUp plans of one dimension outside the few-outputs reduce
 * regime run up to 8 pairs per LAUNCH (the grid's second dimension picks the pair; pairs must all carry masks or
 * none).  So do the gather family (a dice without masks as a lane loop over the pairs instead): dice plans (and a
 * reorder that runs as a gather or through bricks), fused dice -> drillUp plans and
 * the row forms of drillDown and every form of load (`in` the other stores, `out` the stores updated in place; between
 * cell types too), when every buffer of the eight starts on a 16-byte boundary.  Pair by pair behind this
 * one call: pairs with mixed masks, buffers off the 16-byte grid, the two-pass drillDown, drillDown with distributions
 * and its per-cell form, the two-axis transpose of a reorder and the other drillUp regimes.  in_status / out_status may be
 * NULL (no masks) or lists whose entries may be NULL.  Same results as n olap_plan_run calls. */
int olap_plan_run_batch(olap_plan *plan, int n, const void *const *in_values, const int32_t *const *in_status,
                        void *const *out_values, int32_t *const *out_status, void *stream);
/* A drillUp plan over n pairs with a rule EACH (methods[i], one of the seven reference methods; the rule the plan
 * was built with is ignored — a drillUp plan's tables do not depend on it).  ONE launch when the roll-up runs in the
 * row regime with full 16-byte lanes and the pairs all carry masks or none (drillup_rows_mixed_kernel: the rule is a
 * workgroup-uniform switch); pair by pair otherwise.  Same results as n runs of n plans. */
int olap_plan_run_batch_rules(olap_plan *plan, int n, const int *methods, const void *const *in_values,
                              const int32_t *const *in_status, void *const *out_values, int32_t *const *out_status, void *stream);
/* After the stream has been synchronised: OLAP_OK, or the deferred data-dependent error of the
 * last run (OLAP_ERR_DISTRIBUTION_MISSING, message as in-memory.js:398). */
int olap_plan_status(olap_plan *plan);
void olap_plan_destroy(olap_plan *plan);

/* ------------------------------------------------------------------------------------------
 * Element-wise helpers on raw device buffers.
 * ---------------------------------------------------------------------------------------- */
/* Applies setValue (in-memory.js:122-133) to every cell: status[i] = set ? 0x2 : 0 and unset
 * cells get the canonical default.  If `status_in_place` already holds a mask it is AND-ed in
 * when `use_existing_status` != 0.  This is the `data` setter (:39-46) for a typed array. */
int olap_canonicalize(void *values, int32_t *status, uint64_t n, int dtype, int default_kind,
                      int use_existing_status, void *stream);
/* JS numbers (float64) -> typed cells with TypedArray conversion, then setValue semantics;
 * NaN in `nulls` positions is not needed: a JS null/undefined is passed as the default. */
int olap_convert_from_f64(const double *src_f64, void *values, int32_t *status, uint64_t n,
                          int dtype, int default_kind, void *stream);
int olap_convert_to_f64(const void *values, double *dst_f64, uint64_t n, int dtype, void *stream);
/* SURVEY §8(d) synthetic measure generated on the device: cell i gets fround(0.5 + u(2i)),
 * kept iff u(2i+1) < frac, u = mulberry32 stream of `seed` (identical to the golden
 * generator); `first_cell` lets a shard generate its own slab. */
int olap_fill_seeded(void *values, int32_t *status, uint64_t n, uint64_t first_cell, int dtype,
                     uint32_t seed, double frac, void *stream);
/* Completes a sharded `average` (in-memory.js:323-331): values[i] = counts[i] mod 65536 ?
 * values[i] / (counts[i] mod 65536) : values[i]; out_status (optional) gets the mask. */
int olap_average_finish(void *values, const int32_t *counts, int32_t *out_status, uint64_t n,
                        int dtype, int default_kind, void *stream);
/* Computed measures (src/cube.js:326-363: one formula evaluated per cell over the stored measures'
 * getValue(i)), as an element-wise interpreter on the device.  `code` is a postfix program
 * (opcodes: olap-in-memory_amd/js/formula.js OP / csrc FormulaOp; CONST k, INPUT i and SCALAR j
 * carry one operand word), at most OLAP_FORMULA_MAX_CODE words, OLAP_FORMULA_MAX_CONSTS constants,
 * OLAP_FORMULA_MAX_INPUTS input measures (device buffers of n cells each; status may be NULL per
 * input) and as many scalars (`<measure>__total` parameters).  out_f64: n float64 results. */
#define OLAP_FORMULA_MAX_CODE 96
#define OLAP_FORMULA_MAX_CONSTS 24
#define OLAP_FORMULA_MAX_INPUTS 8
#define OLAP_FORMULA_MAX_STACK 16
int olap_eval_formula(const int32_t *code, int n_code, const double *consts, int n_consts, int n_inputs,
                      const void *const *in_values, const int32_t *const *in_status, const int *in_dtypes,
                      const int *in_defaults, const double *scalars, int n_scalars, double *out_f64,
                      uint64_t n, void *stream);
/* Plain copies between host memory and device buffers of the raw-pointer API, for hosts without a
 * HIP binding of their own (blocking). */
int olap_memcpy_to_host(void *host, const void *device, uint64_t bytes);
int olap_memcpy_to_device(void *device, const void *host, uint64_t bytes);
/* Diagnostic: a plain 16-byte streaming read of `bytes` bytes that computes (and drops) one float sum per
 * lane (the achievable read ceiling of the box, measured in the same run as the kernels
 * it is compared with).  `scratch` needs 4 * 2048 bytes.  Asynchronous on `stream`. */
int olap_diag_read_ceiling(const void *device, uint64_t bytes, void *scratch, void *stream);
/* Diagnostic: the write-side counterpart — `bytes` bytes of `device` overwritten with 16-byte streaming stores (the box's
 * write ceiling; HBM is half-duplex, so a kernel that reads R and writes W bytes is bounded by R / read ceiling +
 * W / write ceiling, not by (R + W) / peak).  The buffer's contents are lost.  Asynchronous on `stream`. */
int olap_diag_write_ceiling(void *device, uint64_t bytes, void *stream);
/* Diagnostic, host-only (no device): where the cells of one row of the view [outer, K, inner] go in the LDS tile of the
 * row-tile drillUp regime when groups interleave (DESIGN.md K1', MODE 3) — cell_pos[K * inner] (LDS cell of every cell
 * of a row), group_bounds[2 G] (first and one-past-last member position of every group's run) and *pitch (members
 * between two rows of the tile).  `map` is a drillUp map as in olap_drillup_plan.  For tests of the planning code. */
int olap_diag_tile_placement(int dtype, uint32_t K, uint32_t G, uint32_t inner, const uint32_t *map, uint32_t *cell_pos,
                             uint32_t *group_bounds, uint32_t *pitch);
/* Diagnostic, host-only: what a plan decided, as one line of key=value pairs (no pointers), at most cap - 1 characters.
 * A one-axis drillUp plan tells its kind, the form it runs in over 16-byte-aligned buffers (rows, rows_ragged, tile,
 * gtile, flat, segments, reduce4, reduce, split4, split), vec, outer K G inner, contiguous, perm_pitch, n_gtile, min_group,
 * longest_group, the reduce regime's S (and, where it is not 0, unit rows seg_len vec4 edge), the segmented rows' S_tot
 * and, for the tile form, its mode, rows per tile and LDS bytes.  Every other plan tells its kind and kernel name. */
int olap_diag_plan_describe(const olap_plan *plan, char *buf, size_t cap);
/* Diagnostic, host-only: the number of plans the plan cache of the store-level calls holds now (at most 128).  A call
 * whose key is in the cache leaves it unchanged: for tests of what a plan-cache key holds and what it does not. */
int olap_diag_plan_cache_count(void);
/* `total` getter (in-memory.js:22-28): float64 sum of the set cells, and their count.
 * Synchronises `stream`. */
int olap_total(const void *values, const int32_t *status, uint64_t n, int dtype, int default_kind,
               double *total, uint64_t *n_set, void *stream);

/* ------------------------------------------------------------------------------------------
 * Store handles: device-resident cells owned by the library, for hosts that cannot hold device
 * pointers (the Node.js addon).  One handle = one measure's InMemoryStore (in-memory.js:7-64).
 * Bulk operations are enqueued on the library's (null) stream and return at once; they are ordered
 * behind each other, and every call that hands data to the host (get_*, total, to_sparse, ...) is
 * a blocking copy on that stream, so the API behaves synchronously like the reference's.  Plans
 * built for handles are cached (LRU) and device buffers come from a pool.
 * ---------------------------------------------------------------------------------------- */
typedef struct olap_store olap_store;

/* new InMemoryStore(size, type, defaultValue) — :48-64; every cell unset */
int olap_store_create(olap_store **store, uint64_t size, int dtype, int default_kind);
void olap_store_destroy(olap_store *store);
int olap_store_clone(const olap_store *store, olap_store **out); /* :66-73 */
uint64_t olap_store_size(const olap_store *store);
int olap_store_dtype(const olap_store *store);
int olap_store_default(const olap_store *store);
uint64_t olap_store_byte_length(const olap_store *store); /* :8-16 */
void *olap_store_values_ptr(const olap_store *store);       /* device pointer */
int32_t *olap_store_status_ptr(const olap_store *store);    /* device pointer */

/* Insertion order of the reference's Map (in-memory.js:298 iterates it; `first` / `last`, keys() and serialize()
 * depend on it).  A dense buffer has none: by default cells are ordered by flat index, which is the reference's
 * order for a store filled ascending (`data=`, `fill`) and rolled up while dense.  A TRACKED store keeps the order
 * exactly — through setValue, data=, fill, drillUp (an output cell sits where its first contributing cell sat),
 * dice, reorder, drillDown and load — at the price of one more uint32 per cell once the order stops being the flat
 * index, and of a second pass per operation; results of operations on a tracked store are tracked.
 * olap_store_from_sparse turns tracking on by itself when its index list is not ascending.
 * sum / average / product depend on the order of their contributions (float64 addition is not associative, and a running
 * value that hits the default drops the key, which re-enters at the end): over an order that is not the flat index the
 * set cells are sorted by (output cell, insertion sequence) and every output cell is replayed in that order — the
 * reference's values and key order exactly, at the price of a radix sort; so are `first` / `last` over several
 * rolled-up dimensions at once.
 * Limits: stores below 2^31 cells; olap_store_totals refuses a tracked store ("ordered: ..."): run the chain of drillUps.
 * olap_store_order_tracked: 0 = not tracked, 1 = tracked and still ascending, 2 = tracked with an explicit order. */
int olap_store_track_order(olap_store *store, int on);
int olap_store_order_tracked(const olap_store *store);

/* `data` setter (:39-46) from a host typed array of the store's dtype (n must equal size,
 * else OLAP_ERR_LENGTH_MISMATCH) or from JS numbers */
int olap_store_set_data(olap_store *store, const void *host_values, uint64_t n);
int olap_store_set_data_f64(olap_store *store, const double *host_values, uint64_t n);
/* `data` getter (:30-37) into a host typed array / float64 array; status mask / key list */
int olap_store_get_data(const olap_store *store, void *host_values);
int olap_store_get_data_f64(const olap_store *store, double *host_values);
int olap_store_get_status(const olap_store *store, int32_t *host_status);
int olap_store_count_set(const olap_store *store, uint64_t *n_set);
/* indices of the set cells in the reference's _dataMap.keys() order: ascending, or the tracked insertion order
 * (olap_store_track_order); `cap` entries available, *n_keys receives the full count */
int olap_store_get_keys(const olap_store *store, uint64_t *host_keys, uint64_t cap, uint64_t *n_keys);
int olap_store_get_value(const olap_store *store, uint64_t index, double *value, int *is_set); /* :118-120 */
int olap_store_set_value(olap_store *store, uint64_t index, double value, int is_null);       /* :122-133 */
/* n sequential setValue calls (in-memory.js:122-133) in one call: entry i writes values[i] to cell indexes[i], or unsets
 * it when is_null (may be NULL) has is_null[i] != 0.  The store ends bit for bit as n olap_store_set_value calls in list
 * order leave it (values, mask, conversions, delete-on-default, a tracked store's key order).  Duplicates allowed: the
 * last write decides.  Every index is checked on the host first: one >= size gives OLAP_ERR_INDEX_RANGE and nothing is
 * written.  n == 0 does nothing.  DESIGN.md §3 K9. */
int olap_store_set_values(olap_store *store, uint64_t n, const uint64_t *indexes, const double *values,
                          const uint8_t *is_null);
int olap_store_fill(olap_store *store, double value);                                         /* :135-137 */
int olap_store_total(const olap_store *store, double *total);                                 /* :22-28 */

/* The sparse form the reference serialises (in-memory.js:94-100: `indexes` = Map keys as Uint32,
 * `dataBuffer` = the values as the store's TypedArray): device-side stream compaction of the set
 * cells in ascending index order, and its inverse.  olap_store_sparse_count() sizes the host
 * arrays; indices are 32-bit like the reference's (stores above 2^32 cells are refused). */
int olap_store_to_sparse(const olap_store *store, uint32_t *host_indexes, void *host_values,
                         uint64_t cap, uint64_t *n_set);
/* new store with the given cells set (deserialize, in-memory.js:103-116).  Values are stored as
 * given (TypedArray of the store's dtype); setValue semantics apply (a default value unsets). */
int olap_store_from_sparse(olap_store **store, uint64_t size, int dtype, int default_kind,
                           const uint32_t *host_indexes, const void *host_values, uint64_t n);

/* getNestedObject(measure, withTotals = true) (src/cube.js:421-440): every marginal of the measure in ONE
 * call.  The reference runs, for each of the 2^D subsets of dimensions, the chain drillUp(dim, 'all') over
 * the subset's dimensions in ascending order; all 2^D results are the cells of one extended cube of shape
 * (lens[0] + 1) x ... x (lens[D-1] + 1), row-major, index lens[d] of dimension d meaning 'all'.
 * methods[d] is the measure's rule for dimension d (src/cube.js:1013).  host_values receives that extended
 * cube as float64 (the default in unset cells), host_status (optional) its mask.  Same operations, order
 * and per-stage rounding as the chain of olap_store_drillup calls, hence the same values.
 * When the extended cube fits in LDS (<= 12288 cells) this is one launch that reads the cube from HBM
 * once; otherwise D + 2 launches instead of 2^D - 1.  *launches / *bytes_read (optional) report what ran. */
int olap_store_totals(const olap_store *store, int ndim, const uint32_t *lens, const int *methods, double *host_values,
                      int32_t *host_status, int *launches, uint64_t *bytes_read);
/* getNestedObject(computed measure, withTotals = true): the extended cube of a formula over stored measures in one
 * call.  Marginal s of a stored measure is the sub-lattice s of its extended cube E (olap_store_totals), and a computed
 * measure on marginal s is the formula applied cell by cell to its inputs there — so the result is the program
 * (olap_eval_formula's code and constants, no SCALAR operand) evaluated at every cell e of the extended cube on
 * (E_0[e], ..., E_{n-1}[e]), E_i being what olap_store_totals(inputs[i], ..., methods + i * ndim) exports: the default
 * where unset, NaN for an integer cell unset under a NaN default.  Same values as evaluating the formula on each of
 * the 2^D marginal cubes.  inputs: 1..OLAP_FORMULA_MAX_INPUTS stores of any cell types and defaults, each of the
 * product of lens cells, on one device, none tracked ("ordered: ..."); methods[i * ndim + d] is input i's own rule for
 * dimension d.  host_values receives prod(lens[d] + 1) float64.  The E_i never leave the device: when the extended cube
 * fits in LDS one launch per distinct cell type builds them (a workgroup per input) and one more evaluates the
 * program; otherwise each input runs olap_store_totals' passes and one launch evaluates.  One copy to the host, one
 * synchronisation.  *launches / *bytes_read (optional) report what ran (bytes: every pass's reads plus the n_inputs
 * extended cubes the evaluation reads).  Arguments are checked on the host before any device work.  DESIGN.md §3 K6. */
int olap_formula_totals(const int32_t *code, int n_code, const double *consts, int n_consts, int n_inputs,
                        const olap_store *const *inputs, int ndim, const uint32_t *lens, const int *methods,
                        double *host_values, int *launches, uint64_t *bytes_read);
/* getNestedObjects(ids, withTotals = true): the extended cubes of SEVERAL measures of one cube — stored and computed —
 * in one call.  `inputs` are the n_inputs (1..OLAP_REPORT_MAX_INPUTS) distinct stores the outputs draw on, input i with
 * its own rules methods[i * ndim + d]; every input's extended cube E_i is built ONCE, whatever number of outputs reads it.
 * The n_outputs (1..OLAP_REPORT_MAX_OUTPUTS) outputs are described by flat arrays of n_outputs entries:
 *   out_stored[k] >= 0    output k is E of input out_stored[k]: the bits olap_store_totals(inputs[i], ...) puts in its
 *                         host_values; out_n_code[k], out_n_consts[k] and out_n_inputs[k] must be 0;
 *   out_stored[k] == -1   output k is a formula: its program is the next out_n_code[k] words of `code` and the next
 *                         out_n_consts[k] entries of `consts` (the programs of the formula outputs lie one after the other
 *                         in output order), exactly what olap_formula_totals accepts, no SCALAR operand; the next
 *                         out_n_inputs[k] (1..OLAP_FORMULA_MAX_INPUTS) entries of `formula_inputs` name the report input
 *                         its INPUT operand j reads (each input at most once per formula).  The bits are those of
 *                         olap_formula_totals over these inputs.
 * Refused on the host, before any device work, with messages that name the output ("output k: ..."): what
 * olap_formula_totals refuses in a formula; an input index out of range; an input named twice by one formula; a stored
 * input named by two outputs (the caller de-duplicates ids); an input no output uses; a tracked input ("ordered: ...");
 * size, device and rule mismatches as olap_store_totals; more than 4e9 float64 cells on the device (outputs plus the
 * inputs that only formulas read, times the extended cube: "totals: ..." — ask measure by measure).
 * host_values receives n_outputs * ext float64, output k at k * ext, ext = prod(lens[d] + 1).  On the device a stored
 * output's E is built straight into its slot of the one output slab, inputs that only formulas read get scratch cubes,
 * and ONE launch evaluates every formula; one copy to the host, the call's only wait for device work (the formulas'
 * programs are uploaded before the first launch, while the stream is idle).
 * *launches: ext <= 12288 — per distinct cell type ceil(inputs of that type / 8), plus 1 when any output is a formula;
 * larger — the sum over the inputs of what olap_store_totals reports, plus the same 1.  *bytes_read: every input's passes
 * once, plus out_n_inputs[k] * ext * 8 per formula.  DESIGN.md §3 K6. */
#define OLAP_REPORT_MAX_INPUTS 32
#define OLAP_REPORT_MAX_OUTPUTS 32
int olap_totals_report(int n_inputs, const olap_store *const *inputs, int ndim, const uint32_t *lens, const int *methods,
                       int n_outputs, const int *out_stored, const int *out_n_code, const int32_t *code, const int *out_n_consts,
                       const double *consts, const int *out_n_inputs, const int *formula_inputs, double *host_values,
                       int *launches, uint64_t *bytes_read);

/* Cube.scan / Cube.iterateOverDimension (src/cube.js:811-823): what every combination of the scanned dimensions' items
 * receives, for n stores of one cube (size = prod(lens) cells each; cell types and defaults may differ), in one device
 * pass.  scanned[d] != 0 marks a scanned dimension, the others are kept.  C = the product of the scanned lengths, B =
 * the product of the kept ones; c = the row-major index over the scanned dimensions in cube order (the order of the
 * combinations), b = the row-major index over the kept ones.  host_values[k * size + c * B + b] = what
 * olap_store_get_data_f64(stores[k]) puts at that cell's flat index (the value as float64, the store's default in an
 * unset cell): per store, get_data_f64 transposed to [scanned..., kept...].  One device slab, one copy to the host, the
 * call's only wait.  Two kernels, chosen on the host: the innermost cube dimension kept — rows stay contiguous on both
 * sides, a converting row gather; the innermost scanned — a padded LDS tile transpose between it and the last kept
 * dimension, converted on the way out.  Stores that share cell type, default and whether they keep a mask leave in
 * launches of up to 8; *launches (may be NULL) = the sum of ceil(group / 8) over the groups.
 * Refused on the host before any device work, with the same codes and messages on a machine without a device, in this
 * order: a NULL list or n < 0; a NULL entry ("store i of the batch is NULL"); ndim, the length vector and the flags; no
 * scanned dimension, or B == 0 or C == 0; a store whose size is not prod(lens) (OLAP_ERR_LENGTH_MISMATCH); stores on
 * two devices; a tracked store ("ordered: ..."); n * size * 8 above OLAP_BLOCKS_MAX_BYTES ("blocks: ...": the caller
 * goes combination by combination; the environment variable OLAP_BLOCKS_MAX_BYTES lowers the cap, for tests).  Sharded
 * stores have no such call.  DESIGN.md §3 K11. */
#define OLAP_BLOCKS_MAX_BYTES (1ull << 30)
int olap_store_blocks_report(int n, const olap_store *const *stores, int ndim, const uint32_t *lens,
                             const uint8_t *scanned /* ndim flags */, double *host_values, int *launches);

/* Filtered totals and copies over a cartesian selection given as nlev LEVELS in nesting order, the first outermost
 * (getCombinations, src/cube.js:19-32: the filter's keys in their own order, then the unfiltered dimensions in cube
 * order).  axis[l] is a cube dimension (each exactly once) or -1 for a filter key that is not a dimension (it only
 * multiplies the combinations); sel[l] holds n_sel[l] item indices, repeats allowed, -1 = a cell that does not exist
 * (read as the default).  An empty level gives no combination.  lens[ndim] describes the store's cells.
 * getTotalForDimensionItems (src/cube.js:679-707): *total = the float64 sum, from +0 in nesting order, of getValue
 * (in-memory.js:118-120: the default for an unset cell) over the combinations.  One order-free reduction with an
 * exactness certificate; when the certificate cannot prove the result equal to the sequential sum, the values are
 * gathered in nesting order and added on the host.  *exact_path (optional): 1 = the reduction's result, 0 = the
 * sequential one.  DESIGN.md §3 K8. */
int olap_store_select_total(const olap_store *store, int ndim, const uint32_t *lens, int nlev, const int *axis,
                            const uint32_t *n_sel, const int32_t *const *sel, double *total, int *exact_path);
/* copyMeasureData (src/cube.js:859-888): target.setValue(pos, source.getValue(pos)) for every combination in nesting
 * order, with setValue's conversion and delete-on-default (in-memory.js:122-133); cell types and defaults of the two
 * stores may differ, both live on one device.  Entries must be >= 0.  A tracked target gets the reference's key order. */
int olap_store_copy_select(olap_store *target, const olap_store *source, int ndim, const uint32_t *lens, int nlev,
                           const int *axis, const uint32_t *n_sel, const int32_t *const *sel);
/* olap_store_select_total of a computed measure: the value of a combination is the formula program (olap_eval_formula's
 * code and constants, no SCALAR operand) evaluated at its cell over n_inputs (1..OLAP_FORMULA_MAX_INPUTS) stores of
 * any cell types and defaults, each of the product of lens cells, on one device.  A -1 entry evaluates the program on
 * every input's own default.  Same certificate and sequential fallback; the values are those of olap_eval_formula. */
int olap_formula_select_total(const int32_t *code, int n_code, const double *consts, int n_consts, int n_inputs,
                              const olap_store *const *inputs, int ndim, const uint32_t *lens, int nlev, const int *axis,
                              const uint32_t *n_sel, const int32_t *const *sel, double *total, int *exact_path);
/* olap_store_copy_select with the formula as the source: target.setValue(pos, formula(pos)) over the distinct
 * combinations.  The target may be one of the inputs (each cell is read before it is written; a selection with
 * repeats or free keys revisits cells, which the caller then copies cell by cell).  Entries must be >= 0. */
int olap_store_copy_select_formula(olap_store *target, const int32_t *code, int n_code, const double *consts, int n_consts,
                                   int n_inputs, const olap_store *const *inputs, int ndim, const uint32_t *lens, int nlev,
                                   const int *axis, const uint32_t *n_sel, const int32_t *const *sel);

/* olap_eval_formula over stores (all of the same size) into a host float64 array */
int olap_store_eval_formula(const int32_t *code, int n_code, const double *consts, int n_consts, int n_inputs,
                            const olap_store *const *inputs, const double *scalars, int n_scalars,
                            double *host_out);

/* olap_store_set_data_f64(target, olap_store_eval_formula(...)) without the host: the program is evaluated at every cell
 * and written into `target` as typed cells (and its mask, where the store keeps one) by one launch — the same bits, and a
 * tracked target ends with the same key order.  Refused before any device work: the program checks of olap_eval_formula,
 * n_inputs < 1 or a NULL input, inputs of another size than the target (OLAP_ERR_LENGTH_MISMATCH), a target that is one of
 * the inputs, inputs on another device than the target.  A target of 0 cells is left alone. */
int olap_store_set_formula(olap_store *target, const int32_t *code, int n_code, const double *consts, int n_consts,
                           int n_inputs, const olap_store *const *inputs, const double *scalars, int n_scalars);

/* The five bulk operations; each returns a NEW store (load mutates `store`). */
int olap_store_drillup(const olap_store *store, olap_store **out, int ndim, const uint32_t *old_len,
                       const uint32_t *new_len, const uint32_t *const *maps, int method);
/* drillUp of n stores — the stored measures of one cube — by the same maps and rule: one plan and one launch when
 * the stores share cell type, default, size and device and none tracks its insertion order (olap_plan_run_batch);
 * otherwise the stores are rolled up one by one.  out[i] receives the new store of stores[i]; on an error none is
 * returned.  Replaces the per-measure loop of src/cube.js:1012-1020 for measures with the same rule. */
int olap_store_drillup_batch(int n, const olap_store *const *stores, olap_store **out, int ndim, const uint32_t *old_len,
                             const uint32_t *new_len, const uint32_t *const *maps, int method);
/* The same for stored measures with a rule EACH (methods[i], one of the seven reference methods): what Cube.drillUp does
 * for every stored measure of a cube, `store.drillUp(oldDims, newDims, storedMeasuresRules[id][dimensionId])`
 * (src/cube.js:1012-1020).  Measures that share cell type, default and size leave in ONE launch even when their rules
 * differ, when the roll-up runs in the row regime with full 16-byte lanes (the rule of a measure is a workgroup-uniform
 * switch: config 5's sum / average / first / last); otherwise one launch per rule (olap_store_drillup_batch), and
 * stores that fit no group one by one.  Same results as n olap_store_drillup calls. */
int olap_store_drillup_multi(int n, const olap_store *const *stores, const int *methods, olap_store **out, int ndim,
                             const uint32_t *old_len, const uint32_t *new_len, const uint32_t *const *maps);
int olap_store_drilldown(const olap_store *store, olap_store **out, int ndim,
                         const uint32_t *old_len, const uint32_t *new_len,
                         const uint32_t *const *maps, int method, const double *distributions,
                         uint64_t n_dist);
int olap_store_dice(const olap_store *store, olap_store **out, int ndim, const uint32_t *old_len,
                    const uint32_t *new_len, const int32_t *const *sel);
int olap_store_dice_drillup(const olap_store *store, olap_store **out, int ndim, const uint32_t *old_len,
                            const uint32_t *mid_len, const uint32_t *new_len, const int32_t *const *sel,
                            const uint32_t *const *maps, int method);
int olap_store_reorder(const olap_store *store, olap_store **out, int ndim,
                       const uint32_t *old_len, const int32_t *perm);
/* dice, the fused dice -> drillUp and drillDown of n stores — ALL stored measures of one cube, which Cube._derive and
 * Cube.drillUp hand to the store one by one: the same tables for every store, a rule each where the operation has one
 * (methods[i]; olap_store_drilldown_multi takes OLAP_DRILLDOWN_INTEGER_MEASURE in it and has no distributions).
 * Stores that share cell type, default, device and rule share one plan and leave in launches of up to 8
 * (olap_plan_run_batch, which also names what stays pair by pair behind the call); a store alone in its group runs as
 * the single-store call does.  out[i] receives the new store of stores[i]; on an error none is returned.  Checked on
 * the host before any device work, with the same codes and messages on a machine without a device: a NULL list or
 * n < 0, a NULL entry ("store i of the batch is NULL"), a rule outside the seven reference methods
 * (OLAP_ERR_UNSUPPORTED_METHOD), a tracked store ("ordered: ...": its key order needs the single-store call), ndim
 * and the length vectors, a store whose size is not the product of old_len (OLAP_ERR_LENGTH_MISMATCH).  *launches
 * (may be NULL): the kernel launches the call made.  Same results as n single-store calls. */
int olap_store_dice_multi(int n, const olap_store *const *stores, olap_store **out, int ndim, const uint32_t *old_len,
                          const uint32_t *new_len, const int32_t *const *sel, int *launches);
int olap_store_dice_drillup_multi(int n, const olap_store *const *stores, const int *methods, olap_store **out, int ndim,
                                  const uint32_t *old_len, const uint32_t *mid_len, const uint32_t *new_len,
                                  const int32_t *const *sel, const uint32_t *const *maps, int *launches);
int olap_store_drilldown_multi(int n, const olap_store *const *stores, const int *methods, olap_store **out, int ndim,
                               const uint32_t *old_len, const uint32_t *new_len, const uint32_t *const *maps, int *launches);
int olap_store_load(olap_store *store, const olap_store *other, int ndim, const uint32_t *my_len,
                    const uint32_t *his_len, const int32_t *const *his_to_mine);
/* targets[i].load(sources[i]) for n pairs — the measures two cubes share, which Cube.hydrateFromCube hands to the store
 * one by one: the same lengths and maps for every pair, targets updated in place.  Cell types may differ WITHIN a pair
 * (olap_load_plan_typed; n == 1 is the way to load across cell types: olap_store_load refuses them).  Pairs that share
 * (source type, target type, both defaults, device) share one plan, kept by the plan cache (its tables are built and
 * uploaded once per group, and not at all when the call is repeated), and leave in launches of up to 8
 * (olap_plan_run_batch).  Checked on the host before any device work, with the same codes and messages on a machine
 * without a device, in this order: a NULL list or n < 0; a NULL entry ("store i of the batch is NULL"); ndim and the
 * length vectors; a map entry outside my dimension (OLAP_ERR_INDEX_RANGE, the message of olap_load_plan); a store whose
 * size is not the product of its lengths (OLAP_ERR_LENGTH_MISMATCH); a pair on two devices; a tracked target
 * ("ordered: ...": its key order needs the single-store call); a target that appears twice or is also a source
 * (OLAP_ERR_INVALID_ARGUMENT).  On such an error no target has been touched.  *launches (may be NULL): the kernel
 * launches the call made. */
int olap_store_load_multi(int n, olap_store *const *targets, const olap_store *const *sources, int ndim,
                          const uint32_t *my_len, const uint32_t *his_len,
                          const int32_t *const *his_to_mine, int *launches);
/* The stored measures of ONE source cube brought onto the dimensions of a composed cube (Cube.compose): out[i] is a new
 * store of prod(my_len) cells with sources[i]'s cell type and default that ends, bit for bit in values and mask, as
 *   olap_store_create; olap_store_fill(fill[i]) where has_fill && has_fill[i]; olap_store_load(sources[i], same lengths and maps)
 * would leave it — in one pass that writes every cell of the new store exactly once: nothing is cleared or filled
 * first, and a cell takes the cell of his that maps onto it, or the fill, or stays unset.  his_to_mine is load's (-1: an
 * item I do not have); it is inverted on the host, per dimension, the LAST of his items that name one item of mine
 * winning, as the last write of a load does.  The fill value is converted, and kept or dropped, as olap_store_fill does
 * it (NaN under a NaN default and 0 under a 0 default leave the cells unset).  fill / has_fill may be NULL.  n == 0 or a
 * target of 0 cells launches nothing; ndim == 0 is a single cell.  Sources that share (cell type, default, device)
 * share one plan (olap_compose_plan), kept by the plan cache, and leave in launches of up to 8: *launches (may be NULL)
 * is the sum of ceil(group size / 8) over the groups.  A mask is read and written only where it is primary (integer
 * cells under a NaN default): a Float32 measure moves 4 bytes in and 4 bytes out per cell of the new store.
 * Checked on the host before any device work, with the same codes and messages on a machine without a device, in this
 * order: a NULL list or n < 0; a NULL entry ("store i of the batch is NULL"); ndim, the length vectors and the map
 * entries (as olap_store_load_multi); a source whose size is not the product of his_len (OLAP_ERR_LENGTH_MISMATCH);
 * sources on two devices; a tracked source ("ordered: ...": the key order of fill + load is not a gather's); a NULL
 * `out`.  On an error no store is created and out[] is untouched.  The sources are only read. */
int olap_store_compose_multi(int n, const olap_store *const *sources, const double *fill, const uint8_t *has_fill,
                             olap_store **out, int ndim, const uint32_t *my_len, const uint32_t *his_len,
                             const int32_t *const *his_to_mine, int *launches);
/* olap_store_reorder of n stores — all stored measures of one cube (Cube.reorderDimensions) — with the checks, the
 * grouping and the results of the *_multi calls above.  Reorders that run as a gather or through bricks leave in
 * launches of up to 8; the two-axis transpose runs pair by pair behind the call. */
int olap_store_reorder_multi(int n, const olap_store *const *stores, olap_store **out, int ndim,
                             const uint32_t *old_len, const int32_t *perm, int *launches);
/* Running aggregates along one dimension (Cube.cumulate) of n stores — the stored measures of one cube, a rule each
 * (methods[i]); a single store is a batch of one.  The cube is lens[0..ndim) in row-major order, `axis` the dimension
 * the aggregate runs along and map[k] < n_groups the group of its item k (NULL: the whole dimension is one group and
 * n_groups is not read).  out[i] is a new store of the same cells, type and default as stores[i].  Its cell at item k
 * of `axis`, every other coordinate fixed, holds what the single item of that dimension holds after
 *   dice(axis: the items of k's group at positions <= k)  ->  drillUp(axis -> one item, methods[i])
 * i.e. the state of the reference's drillUp loop (in-memory.js:298-331) after each contribution instead of only after
 * the last one: contributions arrive in ascending item order; an unset cell contributes nothing and receives the
 * carried running value (it stays unset only while its group has contributed nothing); a running value equal to the
 * default is unset at that position and the aggregate restarts with the next contribution (setValue's delete,
 * :126-131); `average` divides at each position by the contribution count modulo 65 536 and leaves the sum when that
 * is 0; the float64 state is converted to the cell type once per output cell and never rounded in between.
 * Every series-and-group is walked sequentially by one lane (olap_cumulate.hip), so float64 sums associate exactly as
 * the reference's loop does.  One stated deviation OF THE DEFINING CHAIN, not of this call: where that chain lands in
 * the few-outputs regime of drillUp (fewer than 131 072 outputs and groups of >= 256 members) it re-associates
 * float64 sums; there this call keeps the reference's order and the chain is the one ~1e-16 off.
 * Stores that share cell type, default and device share one plan (kept by the plan cache), whatever their rules (a
 * workgroup reads its pair's rule), and leave in launches of up to 8: *launches (may be NULL) is the sum of
 * ceil(group size / 8) over the groups.  A mask is read and written
 * only where it is primary.  n == 0 or a cube of 0 cells launches nothing.
 * Checked on the host before any device work, with the same codes and messages on a machine without a device, in this
 * order: a NULL list or n < 0; a NULL entry ("store i of the batch is NULL"); a rule outside the seven reference
 * methods (OLAP_ERR_UNSUPPORTED_METHOD); ndim and the length vector; axis outside [0, ndim); n_groups above the items of the
 * dimension (groups nobody maps to may exist, but not more groups than items); a map entry >= n_groups
 * (OLAP_ERR_INDEX_RANGE); a tracked store ("ordered: ..."); a store whose size is not the product of lens
 * (OLAP_ERR_LENGTH_MISMATCH); stores on different devices.  On an error no store is created.  The stores are only read. */
int olap_store_cumulate_multi(int n, const olap_store *const *stores, const int *methods, olap_store **out, int ndim,
                              const uint32_t *lens, int axis, uint32_t n_groups, const uint32_t *map, int *launches);
/* Rolling-window aggregates along one dimension (Cube.rolling, Cube.shift) of n stores, with the arguments, the
 * grouping into launches, the results and the mask handling of olap_store_cumulate_multi.  The cell of out[i] at item
 * k of `axis`, every other coordinate fixed, holds what the single item of that dimension holds after
 *   dice(axis: the items j of k's group with k - before <= j <= k + after, 0 <= j < K)  ->  drillUp(axis -> one item, methods[i])
 * and is unset when no item is left (the window lies off the dimension, or outside k's group).  before and after may
 * each be negative (before = -after = d is a shift by d: a lag for d > 0, a lead for d < 0, the same under every rule);
 * beyond +-K they act as +-K.  The fold is the reference's drillUp loop (in-memory.js:298-331), started afresh for every
 * window: set members in ascending item order, a running value equal to the default drops and the fold restarts with
 * the next member, `average` divides once at the end by the contribution count modulo 65 536 (and leaves the sum when
 * that is 0), the float64 state is converted to the cell type once per output cell.  No value ever leaves a window by
 * subtraction and nothing re-associates: a float64 window sum associates as the chain's does.
 * Cost (olap_rolling.hip): a workgroup stages the rows of its windows in LDS once, `rows + before + after` input rows
 * for `rows` output rows with rows >= before + after, so a cell is read from device memory at most twice, and folds
 * each window out of LDS: O(W) LDS reads per cell, W = before + after + 1.  The cliff: a window whose rows do not fit a
 * tile (16 KiB of input rows: beyond W = 129 for rows of 64 bytes or more once the dimension has more than 256 items;
 * olap_diag_rolling_choice tells) is folded straight from device memory, O(W) global reads per cell.
 * Stores that share cell type, default and device share one plan, whatever their rules; the plan-cache key holds
 * before and after.  Checked on the host before any device work, in cumulate's order and with cumulate's messages
 * (`rolling` in place of `cumulate`); after the axis and before the groups: before + after < 0
 * (OLAP_ERR_INVALID_ARGUMENT, "rolling: empty window (before %d, after %d)").  On an error no store is created. */
int olap_store_rolling_multi(int n, const olap_store *const *stores, const int *methods, olap_store **out, int ndim,
                             const uint32_t *lens, int axis, int32_t before, int32_t after, uint32_t n_groups,
                             const uint32_t *map, int *launches);
/* What olap_store_rolling_multi's planner chooses for cells of cell_bytes (4 or 8) in the view [outer, K, inner] —
 * host only, no device needed.  choice: the form (0: tiles of whole-width series, 1: tiles of columns, 2: direct),
 * series per tile, output rows per tile, cells per tile row (0, 0, 0 for the direct form).  has_map: whether a K -> G
 * map travels (it does not change the cuts today). */
int olap_diag_rolling_choice(int cell_bytes, uint64_t outer, uint64_t K, uint64_t inner, int32_t before, int32_t after,
                             int has_map, uint32_t choice[4]);
/* Order statistics along one dimension (Cube.quantile, Cube.median) of n stores, with the arguments, the grouping into
 * launches and the mask handling of olap_store_cumulate_multi, and no `methods` list: a measure's rule is not consulted.
 * out[i] is a new store of outer * G * inner cells — outer and inner the products of the lengths before and after
 * `axis`, G = n_groups (1 when map is NULL) — of the type and default of stores[i].  Its cell (o, g, i) holds the
 * q-quantile of the SET cells (o, k, i) with map[k] == g; a group nobody maps to, or without a set cell, gives an unset
 * cell.  With the n members sorted ascending by the IEEE total order on values (-0 before +0, every NaN last) as
 * float64 v[0..n):  h = q * (n - 1), lo = floor(h), frac = h - lo, and the cell is v[lo] + frac * (v[lo + 1] - v[lo])
 * where frac > 0 and v[lo] otherwise — every operation rounded on its own, nothing fused — converted to the cell type
 * once, as every other operation converts; a result equal to the default is unset; a NaN result is the one quiet NaN
 * (0x7FF8000000000000 before the conversion).  Selection is exact (olap_quantile.hip): the two order statistics are
 * found by counting on an order-preserving integer key of the cell and decoded from their keys.
 * Cost: where the rows of the largest group (or, for rows of fewer than four 16-byte slots, a whole series) fit a tile
 * of 32 KiB of LDS, every cell is read from device memory once and selected out of LDS; beyond that the selection reads
 * the group straight from device memory once per pass (34 passes for 4-byte cells, 66 for Float64) — no shape goes to
 * the host.  olap_diag_quantile_choice tells which.
 * Stores that share cell type, default and device share one plan; q is NOT part of the plan-cache key (it travels as
 * a launch argument).  *launches as olap_store_cumulate_multi counts them.  Checked on the host before any device work,
 * in cumulate's order and with cumulate's messages (`quantile` in place of `cumulate`; the list message is "store list
 * is NULL"); after the axis and before the groups: q outside [0, 1], NaN included (OLAP_ERR_INVALID_ARGUMENT,
 * "quantile: q must lie in [0, 1] (got %g)").  One deliberate difference: a store that tracks its insertion order is
 * ACCEPTED — a quantile does not depend on order, and values and mask are dense whatever the order; the result is an
 * ordinary untracked store.  On an error no store is created.  The stores are only read. */
int olap_store_quantile_multi(int n, const olap_store *const *stores, olap_store **out, int ndim, const uint32_t *lens,
                              int axis, double q, uint32_t n_groups, const uint32_t *map, int *launches);
/* What olap_store_quantile_multi's planner chooses for cells of cell_bytes (4 or 8; has_mask: integer cells under a
 * NaN default, whose mask tile shares the LDS) in the view [outer, K, inner] with n_groups groups, the largest of
 * `longest` members — host only, no device needed.  choice: the form (0: column, 1: row, 2: direct, a lane per output
 * cell, 3: direct, a workgroup per output cell), the cells a tile may hold (OLAP_QUANTILE_TILE lowers it), series per
 * tile and LDS pitch between two series (row form), cells per tile row and rows per tile (column form); 0 where a
 * form does not use a cut.  contiguous: whether every group is a run of neighbouring items (it does not change the
 * cuts today: interleaved groups are staged member by member). */
int olap_diag_quantile_choice(int cell_bytes, int has_mask, uint64_t outer, uint64_t K, uint64_t inner,
                              uint32_t n_groups, uint32_t longest, int contiguous, uint32_t choice[6]);
/* Dispersion along one dimension (Cube.variance, Cube.stddev) of n stores, with the arguments, the grouping into
 * launches and the mask handling of olap_store_quantile_multi: no `methods` list, a measure's rule is not consulted.
 * out[i] is a new store of outer * G * inner cells of the type and default of stores[i].  Its cell (o, g, i) holds the
 * variance (kind 0) or the standard deviation (kind 1) of the SET cells (o, k, i) with map[k] == g, by two passes in
 * float64 — never E[x^2] - E[x]^2.  With the n members in ascending item order as float64 v[0..n):  n - ddof <= 0
 * gives an unset cell (a group nobody maps to, a group without a set cell, one member with ddof 1); otherwise
 * s = v[0], s += v[k];  mean = s / n;  m2 = 0, d = v[k] - mean, p = d * d, m2 += p;  r = m2 / (n - ddof);  kind 1:
 * r = sqrt(r) — every operation rounded on its own, nothing fused — converted to the cell type once, as every other
 * operation converts; a NaN result is the one quiet NaN (0x7FF8000000000000 before the conversion); a result equal to
 * the default is unset.  Two consequences: a variance of 0 (one member, equal members) is an UNSET cell under a 0
 * default and a SET 0 under a NaN default; a group that contains +-Infinity or a set NaN gives NaN.
 * Forms (olap_variance.hip; olap_diag_variance_choice tells which): where the rows of the largest group (or, for rows
 * of fewer than four 16-byte slots, a whole series) fit a tile of 32 KiB of LDS, every cell is read from device memory
 * once and folded twice out of LDS by one lane per output cell; a group beyond a tile is walked twice straight from
 * device memory by one lane per output cell.  These three one-lane forms equal the definition bit for bit.  At most
 * 65536 output cells whose largest group has 1024 members or more take a workgroup per output cell, which adds the
 * members' sum, then m2, by a tree of fixed shape: this is the one RE-ASSOCIATED form (as the reduce regime K1r is
 * for drillUp) — its additions are grouped differently from the definition's, so its result may differ from it by
 * rounding, within 4 * (N u + N^2 k^2 u^2) relative for N members (u = 2^-53, k^2 = 1 + mean^2 / variance: twice the sum
 * of the two sides' two-pass bounds); the grouping is fixed by the plan and never by timing, no atomics on values, and
 * a second run gives the same bytes.  No shape goes to the host.
 * Stores that share cell type, default and device share one plan; kind and ddof are NOT part of the plan-cache key
 * (they travel as launch arguments).  *launches as olap_store_cumulate_multi counts them.  Checked on the host before
 * any device work, in cumulate's order and with cumulate's messages (`variance` in place of `cumulate`; the list
 * message is "store list is NULL"); after the axis and before the groups: kind outside {0, 1} ("variance: kind must be
 * 0 or 1 (got %d)"), then ddof outside {0, 1} ("variance: ddof must be 0 or 1 (got %d)"), both
 * OLAP_ERR_INVALID_ARGUMENT.  A store that tracks its insertion order is ACCEPTED — the definition walks item order,
 * not insertion order, and values and mask are dense; the result is an ordinary untracked store.  On an error no
 * store is created.  The stores are only read. */
int olap_store_variance_multi(int n, const olap_store *const *stores, olap_store **out, int ndim, const uint32_t *lens,
                              int axis, int kind /* 0 variance, 1 stddev */, int ddof, uint32_t n_groups,
                              const uint32_t *map, int *launches);
/* What olap_store_variance_multi's planner chooses, with the arguments of olap_diag_quantile_choice — host only, no
 * device needed.  choice: the form (0: column, 1: row, 2: direct, a lane per output cell, 3: direct, a workgroup per
 * output cell — the re-associated form), the cells a tile may hold (OLAP_VARIANCE_TILE lowers it), series per tile and
 * LDS pitch between two series (row form), cells per tile row and rows per tile (column form); 0 where a form does not
 * use a cut.  contiguous does not change the cuts today: interleaved groups are staged member by member. */
int olap_diag_variance_choice(int cell_bytes, int has_mask, uint64_t outer, uint64_t K, uint64_t inner,
                              uint32_t n_groups, uint32_t longest, int contiguous, uint32_t choice[6]);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU: a cube partitioned along its OUTERMOST dimension.  Row-major layout
 * (src/cube.js:709-728) makes a dimension-0 partition a set of contiguous slabs: rank r owns rows
 * [bounds[r], bounds[r+1]).  Every store operation that leaves dimension 0 alone runs per shard with
 * no communication.  drillUp ON dimension 0 (in-memory.js:265-334 with a non-identity map on the
 * sharded axis — the per-measure store call of src/cube.js:1012-1020) reduces each rank's own rows
 * into a partial [G, inner0] cube with the ordinary kernels and a row sub-map, then ONE RCCL
 * collective over xGMI combines the partials (olap_shard_recipe below says which).
 *
 * A communicator names the ranks and where they run:
 *   olap_comm_init_all     one process drives n devices (the Node.js host); ranks 0..n-1 are all local
 *   olap_comm_init_rank    one process per GPU (bench.py under torch.distributed.run); the 128-byte
 *                          unique id of rank 0 (olap_comm_unique_id) reaches the others out of band
 *   olap_comm_init_detached no transport: olap_shard_drillup_exchange() fails, the caller moves the
 *                          payloads itself (rehearsals over gloo; tests)
 * Ranks that share one device (init_all with a repeated device, e.g. {0,0}) exchange by reading
 * each other's buffers directly — RCCL refuses two ranks on one device — so a one-GPU machine can
 * run the sharded store end to end.
 * ---------------------------------------------------------------------------------------- */
typedef struct olap_comm olap_comm;
#define OLAP_UNIQUE_ID_BYTES 128
int olap_comm_unique_id(char id[OLAP_UNIQUE_ID_BYTES]);
int olap_comm_init_rank(olap_comm **comm, const char id[OLAP_UNIQUE_ID_BYTES], int world, int rank, int device);
int olap_comm_init_all(olap_comm **comm, const int *devices, int n);
int olap_comm_init_detached(olap_comm **comm, int world, int rank, int device);
void olap_comm_destroy(olap_comm *comm);
int olap_comm_world(const olap_comm *comm);
int olap_comm_local_count(const olap_comm *comm);            /* ranks driven by this process */
int olap_comm_local_rank(const olap_comm *comm, int local);  /* global rank of local rank `local` */
int olap_comm_local_device(const olap_comm *comm, int local);
/* "rccl" | "direct" (same-device ranks) | "detached" */
const char *olap_comm_transport(const olap_comm *comm);

/* Host-only partition arithmetic (no device needed).
 * olap_shard_bounds: contiguous balanced split of n_rows over `world` ranks, the first
 *   n_rows % world ranks get one more row; bounds has world + 1 entries.
 * olap_shard_dice_bounds: the partition left by a dice of dimension 0 with the strictly ascending
 *   row list `rows` (every rank keeps its own selected rows, no data moves): new_bounds[r] = number
 *   of selected rows below bounds[r].  Fails (OLAP_ERR_INVALID_ARGUMENT) when `rows` is not
 *   strictly ascending inside [0, bounds[world]). */
int olap_shard_bounds(uint32_t n_rows, int world, uint32_t *bounds);
int olap_shard_dice_bounds(const uint32_t *bounds, int world, const int32_t *rows, uint32_t n_rows_selected,
                           uint32_t *new_bounds);

/* What one sharded drillUp of dimension 0 ships and how the partials are combined. */
typedef enum { OLAP_XCHG_SUM = 0, OLAP_XCHG_MAX = 1, OLAP_XCHG_GATHER = 2 } olap_xchg_op;
typedef enum {
  OLAP_FINISH_NONE = 0,     /* sum over a 0 default: the reduced values ARE the result (set <=> != 0) */
  OLAP_FINISH_RESTORE = 1,  /* sum over a NaN default: cells no rank contributed to get the default back */
  OLAP_FINISH_AVERAGE = 2,  /* (sum, contribution count) -> in-memory.js:323-331, count modulo 65536 */
  OLAP_FINISH_COMBINE = 3,  /* highest/lowest/first/last/product: the same drillUp over the rank axis */
  OLAP_FINISH_ROUND = 4     /* sum of Float32 cells: the float64 partial sums, added in float64, are rounded to the cell
                             * type ONCE (as the one-device kernels round their float64 accumulator); a cell is set iff
                             * somebody contributed (NaN default: contribution counts travel too) and the rounded sum
                             * is not the default */
} olap_shard_finish;
typedef enum {
  OLAP_PLACE_SCATTER = 0,   /* additive methods: rank r keeps flat cells [r*per, (r+1)*per), per = ceil(n_out/world) */
  OLAP_PLACE_ALL = 1,       /* every rank holds the whole result */
  OLAP_PLACE_ROOT = 2,      /* rank 0 holds the whole result */
  OLAP_PLACE_SCATTER_ROWS = 3 /* like SCATTER in blocks of whole rows of the new leading dimension: rank r keeps rows
                               * [r*p, (r+1)*p) of it, p = ceil(new_len[0] / world) (what a sharded store needs) */
} olap_shard_placement;
typedef struct {
  int local_method;     /* olap_method run by each rank over its own rows */
  int zero_unset;       /* float64 cells over a NaN default, `sum`: unset partial cells are shipped as 0, never as NaN */
  int n_payloads;       /* 1 or 2 */
  int payload_dtype[2]; /* [0]: the cell type — OLAP_FLOAT64 for `average` and for `sum` of Float32 cells, whose partials
                         * are the float64 accumulators (twice the bytes on the wire); [1]: OLAP_INT32 (mask, or
                         * contribution counts) */
  int payload_op[2];    /* olap_xchg_op; masks are combined with MAX (an OR of 0 / 0x2), never added */
  int finish;           /* olap_shard_finish */
} olap_shard_recipe;
/* host-only; `method` is one of the seven reference methods */
int olap_shard_recipe_get(int dtype, int default_kind, int method, olap_shard_recipe *recipe);

/* Reusable sharded drillUp of dimension 0.  lens[ndim] are the GLOBAL old lengths, bounds[world+1]
 * the row partition, maps[d] as in olap_drillup_plan with maps[0] over the global rows (every rank
 * takes its own slice), new_len the global new lengths.  The object owns, per local rank, the
 * partial / exchange / result buffers (two sets when depth == 2) and one stream for the exchange.
 *
 * olap_shard_drillup_step(): for every local rank i — local reduction of in_values[i] on
 * streams[i], then the exchange and the finishing kernels on the exchange stream, ordered by
 * events only (no host wait).  With depth 2 consecutive steps are independent queries and the
 * exchange of step k overlaps the local reduction of step k+1.  olap_shard_drillup_wait() makes
 * streams[i] wait for everything issued so far.  The three phases can also be called one by one
 * (rehearsals that move the payloads themselves call _local, their own collective on the buffers
 * olap_shard_drillup_payload() names, then _finish).  Not thread-safe. */
typedef struct olap_shard_drillup olap_shard_drillup;
int olap_shard_drillup_create(olap_shard_drillup **op, olap_comm *comm, int dtype, int default_kind, int method,
                              int ndim, const uint32_t *lens, const uint32_t *new_len, const uint32_t *bounds,
                              const uint32_t *const *maps, int placement, int depth);
void olap_shard_drillup_destroy(olap_shard_drillup *op);
uint64_t olap_shard_drillup_out_cells(const olap_shard_drillup *op);     /* cells of the global result */
uint64_t olap_shard_drillup_local_cells(const olap_shard_drillup *op, int local);
const char *olap_shard_drillup_kernel_name(const olap_shard_drillup *op, int local);
int olap_shard_drillup_step(olap_shard_drillup *op, const void *const *in_values, const int32_t *const *in_status,
                            void *const *streams);
int olap_shard_drillup_wait(olap_shard_drillup *op, void *const *streams);
int olap_shard_drillup_local(olap_shard_drillup *op, int local, const void *in_values, const int32_t *in_status, void *stream);
int olap_shard_drillup_exchange(olap_shard_drillup *op, void *const *streams);
int olap_shard_drillup_finish(olap_shard_drillup *op, int local, void *stream);
/* payload p of local rank `local` in the buffer set of the LAST step: what is sent, where the combined
 * data must land (recv holds count cells for SUM / MAX under PLACE_ALL / ROOT, per cells under SCATTER,
 * world * count cells for GATHER), their element type and the combining operation */
int olap_shard_drillup_payload(const olap_shard_drillup *op, int local, int p, void **send, void **recv,
                               uint64_t *count, int *dtype, int *xchg_op);
/* result of the LAST step on local rank `local` (device pointers; *status may come back NULL when the
 * mask is a function of the values): flat range [*first, *first + *count) of the global output */
int olap_shard_drillup_result(const olap_shard_drillup *op, int local, void **values, int32_t **status,
                              uint64_t *first, uint64_t *count);

/* Sharded store handle: one measure whose dimension 0 is split over the ranks of `comm`; each local
 * rank's slab is an ordinary olap_store on its device.  In a one-process communicator the host-facing
 * accessors see the whole measure; with one process per GPU they see this process' rows only
 * (host arrays are still full-size: only the local slabs are read or written). */
typedef struct olap_sharded_store olap_sharded_store;
int olap_sharded_store_create(olap_sharded_store **store, olap_comm *comm, int ndim, const uint32_t *lens,
                              int dtype, int default_kind, const uint32_t *bounds /* NULL: balanced */);
void olap_sharded_store_destroy(olap_sharded_store *store);
uint64_t olap_sharded_store_size(const olap_sharded_store *store);
int olap_sharded_store_ndim(const olap_sharded_store *store);
const uint32_t *olap_sharded_store_lens(const olap_sharded_store *store);
const uint32_t *olap_sharded_store_bounds(const olap_sharded_store *store);  /* world + 1 entries */
/* Re-describes the dimensions without moving a cell (the reference's Cube inserts and drops one-item
 * dimensions around store calls, src/cube.js:919-927, :950-964): lens[0] must stay the sharded extent and
 * the product of the others the row size; otherwise OLAP_ERR_INVALID_ARGUMENT, message "sharded: ...". */
int olap_sharded_store_reshape(olap_sharded_store *store, int ndim, const uint32_t *lens);
olap_comm *olap_sharded_store_comm(const olap_sharded_store *store);
olap_store *olap_sharded_store_shard(const olap_sharded_store *store, int local);  /* borrowed */
int olap_sharded_store_fill_seeded(olap_sharded_store *store, uint32_t seed, double frac);
int olap_sharded_store_set_data_f64(olap_sharded_store *store, const double *host_values, uint64_t n);
int olap_sharded_store_get_data_f64(const olap_sharded_store *store, double *host_values);
int olap_sharded_store_get_status(const olap_sharded_store *store, int32_t *host_status);
int olap_sharded_store_get_value(const olap_sharded_store *store, uint64_t index, double *value, int *is_set);
int olap_sharded_store_set_value(olap_sharded_store *store, uint64_t index, double value, int is_null);
/* olap_store_set_values: the entries are split by shard on the host (list order kept within a shard) and written
 * per shard; an index of a rank this process does not drive gives OLAP_ERR_INDEX_RANGE before anything is written */
int olap_sharded_store_set_values(olap_sharded_store *store, uint64_t n, const uint64_t *indexes,
                                  const double *values, const uint8_t *is_null);
int olap_sharded_store_fill(olap_sharded_store *store, double value);
/* sum of the set cells of the WHOLE measure: with one process per GPU over RCCL every rank must call it (a
 * collective); on a detached communicator it is the sum of this process' slabs only */
int olap_sharded_store_total(const olap_sharded_store *store, double *total);
int olap_sharded_store_clone(const olap_sharded_store *store, olap_sharded_store **out);
/* olap_store_eval_formula over sharded inputs that are partitioned alike: evaluated per shard, every local slab of
 * host_out (full size) is filled */
int olap_sharded_store_eval_formula(const int32_t *code, int n_code, const double *consts, int n_consts, int n_inputs,
                                    const olap_sharded_store *const *inputs, const double *scalars, int n_scalars,
                                    double *host_out);
/* olap_store_set_formula over a sharded target and sharded inputs, one launch per shard on the shard's device; the
 * scalars are the same for every shard.  Target and inputs must be partitioned alike: anything else answers "sharded: …" */
int olap_sharded_store_set_formula(olap_sharded_store *target, const int32_t *code, int n_code, const double *consts,
                                   int n_consts, int n_inputs, const olap_sharded_store *const *inputs,
                                   const double *scalars, int n_scalars);
/* whole measure on the device of local rank 0 as an ordinary store, and back (one-process
 * communicators: device-to-device copies; one process per GPU: RCCL broadcasts of the slabs) */
int olap_sharded_store_gather(const olap_sharded_store *store, olap_store **out);
int olap_sharded_store_scatter(olap_sharded_store **store, olap_comm *comm, const olap_store *whole, int ndim,
                               const uint32_t *lens);
/* The bulk operations.  Dimension 0 untouched (identity map / selection / perm[0] == 0): per shard,
 * no communication, *out_sharded keeps the partition.  drillUp that changes dimension 0: partial +
 * ONE collective; when the new leading dimension still has a row per rank (day -> month on a sharded time
 * axis) the result stays sharded along it (reduce-scatter of whole rows, rank r keeps rows [r*p, (r+1)*p),
 * p = ceil(G0 / world)), otherwise ('all') the (K0 / G0 times smaller) result arrives as an ordinary store
 * in *out_whole on the device of local rank 0 (every process gets it when there is one process per GPU).  dice of
 * dimension 0 by a strictly ascending list of existing rows: per shard, the partition becomes
 * uneven.  Anything else that touches dimension 0 (reordering it, refining it, selections that
 * repeat, permute or invent rows): OLAP_ERR_INVALID_ARGUMENT with a message starting "sharded:" —
 * gather first.  Exactly one of *out_sharded / *out_whole is set on success. */
int olap_sharded_store_drillup(const olap_sharded_store *store, olap_sharded_store **out_sharded, olap_store **out_whole,
                               const uint32_t *new_len, const uint32_t *const *maps, int method);
int olap_sharded_store_dice(const olap_sharded_store *store, olap_sharded_store **out, const uint32_t *new_len,
                            const int32_t *const *sel);
int olap_sharded_store_drilldown(const olap_sharded_store *store, olap_sharded_store **out, const uint32_t *new_len,
                                 const uint32_t *const *maps, int method, const double *distributions, uint64_t n_dist);
int olap_sharded_store_reorder(const olap_sharded_store *store, olap_sharded_store **out, const int32_t *perm);
/* olap_store_select_total / olap_store_copy_select over sharded stores (one-process communicators).  The total adds
 * the shards' certified partials on the host; when the certificate fails the sequential order needs the whole measure:
 * OLAP_ERR_INVALID_ARGUMENT, message "sharded: ..." (gather first).  The copy runs per shard and needs source and target
 * partitioned alike and a target that does not track its order (otherwise "sharded: ..."). */
int olap_sharded_store_select_total(const olap_sharded_store *store, int nlev, const int *axis, const uint32_t *n_sel,
                                    const int32_t *const *sel, double *total, int *exact_path);
int olap_sharded_store_copy_select(olap_sharded_store *target, const olap_sharded_store *source, int nlev, const int *axis,
                                   const uint32_t *n_sel, const int32_t *const *sel);

#ifdef __cplusplus
}
#endif
#endif /* OLAP_HIP_H */
