"""olap_store_dice_multi / olap_store_dice_drillup_multi / olap_store_drilldown_multi: dice, the fused dice -> drillUp
and drillDown of ALL stored measures of a cube in one call.  Every result must equal, bit for bit (values, status mask
and key order), what the single-store call gives on the same inputs; one case per operation is also compared with the
CPU oracle; *launches must be the number of (cell type, rule) groups, counted in eights, wherever the operation runs
batched (and twice the number of measures for the two-pass drillDown, which stays pair by pair behind the call).

Shapes are the smallest at which each kernel form can go wrong (the plan's kernel name is asserted where the shape is
there for one form): 16-byte lanes on a contiguous run, rows that are not whole 16-byte groups, odd extents, several
workgroups times several pairs, rows on and off 128-byte lines, the integer remainder spreading.  The row forms of
drillDown need rows of 128 lanes at least and dice_direct_kernel a middle dimension over odd rows: those cases stand
beside the narrow ones, which run pair by pair behind the call."""
import math

import numpy as np
import pytest

from conftest import load_package
from golden_util import same_typed
from oracle.oracle import OracleStore

pytestmark = pytest.mark.gpu

pkg = load_package()
HipStore, Plan = pkg.HipStore, pkg.hipstore.Plan
NAN = float("nan")

CELLS = {"float32": ("float32", 0.0), "float64": ("float64", 0.0), "int32-nan": ("int32", NAN)}  # the last one carries masks
COUNTS = (1, 2, 8, 9)  # nine measures of one group make two launches
RULES = ("sum", "average", "highest", "product")


def ident(n):
    return list(range(n))


def groups_of(sizes):
    """children per parent -> (new length, the parent of every child); children of one parent are adjacent"""
    parents = [g for g, size in enumerate(sizes) for _ in range(size)]
    return len(parents), parents


def make_stores(rng, cell, n, shape, ints_only=False):
    """n measures over `shape`: small integers (every rule's result is then exact in every cell type), a third of the
    cells unset (0 under a 0 default, NaN under a NaN default)"""
    dtype, default = CELLS[cell]
    size = int(np.prod(shape))
    out = []
    for _ in range(n):
        vals = rng.integers(1, 7, size=size).astype(np.float64)
        vals[rng.random(size) < 0.33] = default
        s = HipStore(size, dtype, default)
        s.set_data_f64(vals)
        out.append(s)
    return out


def same(a, b):
    """bit for bit: the typed cells, the mask and the key order"""
    return (a.size == b.size and a.type == b.type and a.get_data().tobytes() == b.get_data().tobytes() and
            np.array_equal(a.get_status(), b.get_status()) and np.array_equal(a.keys(), b.keys()))


def expected_launches(stores, rules=None, per_pair=1, batched=True):
    if not batched:
        return per_pair * len(stores)
    groups = {}
    for i, s in enumerate(stores):
        key = (s.type, s.default_is_nan, rules[i] if rules else None)
        groups[key] = groups.get(key, 0) + 1
    return sum(math.ceil(m / 8) for m in groups.values())


def oracle_of(store):
    o = OracleStore(store.size, store.type, NAN if store.default_is_nan else 0.0)
    o.set_data(np.where((store.get_status() & 2) != 0, store.get_data_f64(), NAN if store.default_is_nan else 0.0))
    return o


def same_as_oracle(store, o):
    ev, es = o.typed()
    return store.get_data().tobytes() == ev.tobytes() and np.array_equal(store.get_status(), es)


# ---------------------------------------------------------------------------------------------------------- dice
DICE_CASES = {
    # [6,5,8], dimension 1 to 3 items in reversed order plus an item the cube does not have: 16-byte lanes on a contiguous innermost run
    "middle-reversed": ([6, 5, 8], [6, 4, 8], [ident(6), [4, 2, -1, 0], ident(8)], "gather"),
    # the last dimension to 5 items
    "innermost": ([7, 9], [7, 5], [ident(7), [8, 0, 3, 4, 6]], "gather"),
    # a middle dimension over rows of 7 cells, which are not whole 16-byte groups: dice_direct_kernel (3 workgroups of
    # float32 cells per pair), with an item the cube does not have
    "direct-odd-rows": ([30, 5, 7], [30, 4, 7], [ident(30), [4, 2, -1, 0], ident(7)], "dice_direct_kernel"),
    # two dimensions diced, odd extents throughout
    "two-dimensions": ([5, 3, 7], [3, 3, 4], [[4, 0, 2], ident(3), [6, 1, 0, 3]], "gather"),
    # several workgroups times several pairs
    "several-workgroups": ([40, 33, 24], [40, 17, 24], [ident(40), list(range(32, -1, -2)), ident(24)], "gather"),
}


@pytest.mark.parametrize("form", ["blocks", "pairs"])  # the batched gather: blockIdx.y picks the pair | a lane loops over the pairs
@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("case", list(DICE_CASES))
def test_dice_multi_equals_the_single_store_calls(case, cell, form, monkeypatch):
    monkeypatch.setenv("OLAP_GATHER_BATCH_FORM", form)  # (read at every launch)
    old, new, sel, kernel = DICE_CASES[case]
    dtype, default = CELLS[cell]
    assert kernel in Plan.dice(dtype, default, old, new, sel).kernel_name
    rng = np.random.default_rng(11)
    for n in COUNTS:
        stores = make_stores(rng, cell, n, old)
        got, launches = HipStore.dice_multi(stores, old, new, sel)
        assert len(got) == n
        for s, g in zip(stores, got):
            assert same(g, s.dice(old, new, sel)), (case, cell, n)
        assert launches == expected_launches(stores), (case, cell, n)
    if cell != "int32-nan":
        assert same_as_oracle(got[-1], oracle_of(stores[-1]).dice(old, new, sel))


# ------------------------------------------------------------------------------------------ fused dice -> drillUp
UNEVEN = [0, 0, 0, 0, 1, 1, 1, 2, 2, 2]  # 10 items into groups of 4, 3 and 3
FUSED_CASES = {
    # slice dimension 0 to one item, then roll dimension 1 up into 3 uneven groups
    "slice-then-roll": ([6, 10, 8], [1, 10, 8], [1, 3, 8], [[4], ident(10), ident(8)], [[0], UNEVEN, ident(8)]),
    # the same with a selected item that has no source
    "missing-row": ([6, 10, 8], [1, 10, 8], [1, 3, 8], [[4], [0, 1, 2, -1, 4, 5, 6, 7, 8, 9], ident(8)], [[0], UNEVEN, ident(8)]),
    # roll-up of the contiguous (innermost) dimension
    "innermost": ([12, 7], [5, 7], [5, 3], [[11, 0, 3, 4, 7], ident(7)], [ident(5), [0, 0, 1, 1, 1, 2, 2]]),
}


@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("case", list(FUSED_CASES))
def test_dice_drillup_multi_equals_the_single_store_calls(case, cell):
    old, mid, new, sel, maps = FUSED_CASES[case]
    rng = np.random.default_rng(12)
    for n in COUNTS:
        stores = make_stores(rng, cell, n, old)
        rules = [RULES[i % len(RULES)] for i in range(n)]
        got, launches = HipStore.dice_drillup_multi(stores, rules, old, mid, new, sel, maps)
        for s, rule, g in zip(stores, rules, got):
            assert same(g, s.dice_drillup(old, mid, new, sel, maps, rule)), (case, cell, n, rule)
        assert launches == expected_launches(stores, rules), (case, cell, n)  # one launch per rule group
    if cell != "int32-nan":
        for s, rule, g in zip(stores[:4], rules[:4], got[:4]):
            assert same_as_oracle(g, oracle_of(s).dice(old, mid, sel).drill_up(mid, new, maps, rule)), (case, cell, rule)


# ------------------------------------------------------------------------------------------------------ drillDown
K7, PARENTS7 = groups_of([3, 2, 2])  # dimension 1 from 3 parents to 7 children
ROWS, LINES = "drilldown_rows_kernel", "drilldown_rows_lines_kernel"
DRILLDOWN_CASES = {
    # rows of 32 and of 20 cells, on and off 128-byte lines: too narrow for the row forms (128 lanes per row at least),
    # they take the two-pass form (float cells) or the per-cell one — pair by pair behind the call
    "narrow-on-lines": ([4, 3, 32], [4, K7, 32], [ident(4), PARENTS7, ident(32)], "sum", {"float32": "drilldown_scale_kernel"}),
    "narrow-off-lines": ([4, 3, 20], [4, K7, 20], [ident(4), PARENTS7, ident(20)], "sum", {"float32": "drilldown_scale_kernel"}),
    # the row form: rows of 1056 cells are whole 128-byte lines in every cell type, two workgroups per row
    "rows-on-lines": ([2, 3, 1056], [2, K7, 1056], [ident(2), PARENTS7, ident(1056)], "sum", {"float32": ROWS, "float64": ROWS, "int32-nan": ROWS}),
    # rows of 516 cells start off the 128-byte lines but are whole 16-byte groups: the lines kernel (int32 `sum` spreads
    # remainders, which only the row kernel does)
    "rows-off-lines": ([2, 3, 516], [2, K7, 516], [ident(2), PARENTS7, ident(516)], "sum", {"float32": LINES, "float64": LINES, "int32-nan": ROWS}),
    # rows of 515 cells are not even whole 16-byte groups: the lines kernel's cell-by-cell staging
    "rows-odd": ([2, 3, 515], [2, K7, 515], [ident(2), PARENTS7, ident(515)], "sum", {"float32": LINES, "float64": LINES, "int32-nan": ROWS}),
    # any other rule copies the parent (for int32 cells too: the lines kernel)
    "copy": ([2, 3, 516], [2, K7, 516], [ident(2), PARENTS7, ident(516)], "average", {"float32": LINES, "float64": LINES, "int32-nan": LINES}),
    # two refined dimensions: no row form; float cells take the two-pass form, pair by pair behind the call
    "two-pass": ([3, 4], [5, 9], [[0, 0, 1, 2, 2], [0, 0, 0, 1, 1, 2, 3, 3, 3]], "sum", {"float32": "drilldown_scale_kernel", "float64": "drilldown_scale_kernel"}),
}


@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("case", list(DRILLDOWN_CASES))
def test_drilldown_multi_equals_the_single_store_calls(case, cell):
    old, new, maps, rule, kernels = DRILLDOWN_CASES[case]
    dtype, default = CELLS[cell]
    name = Plan.drilldown(dtype, default, rule, old, new, maps).kernel_name
    if cell in kernels:
        assert kernels[cell] in name
    rng = np.random.default_rng(13)
    for n in COUNTS:
        stores = make_stores(rng, cell, n, old)
        got, launches = HipStore.drill_down_multi(stores, [rule] * n, old, new, maps)
        for s, g in zip(stores, got):
            assert same(g, s.drill_down(old, new, maps, rule)), (case, cell, n)
        if "drilldown_rows" in name:
            assert launches == expected_launches(stores, [rule] * n), (case, cell, n)
        elif "drilldown_scale" in name:
            assert launches == 2 * n
    if cell != "int32-nan":
        assert same_as_oracle(got[-1], oracle_of(stores[-1]).drill_down(old, new, maps, rule))


@pytest.mark.parametrize("cell,flag", [("int32-nan", False), ("float64", True)])
def test_drilldown_multi_spreads_integer_remainders(cell, flag):
    """100 -> 34, 33, 33 and 14 -> 5, 4, 5 (in-memory.js:403-417) in the row form: int32 cells, and a measure declared int32
    in float64 cells.  Dimension 0 goes from 2 parents to 3 + 3 children over rows of 520 cells."""
    k, parents = groups_of([3, 3])
    width = 520
    old, new, maps = [2, width], [k, width], [parents, ident(width)]
    dtype, default = CELLS[cell]
    for n in COUNTS:
        stores = []
        for i in range(n):
            vals = np.concatenate([np.full(width, 100.0), np.full(width, 14.0)])
            vals[1], vals[2], vals[width + 3] = 7.0 + i, default, default
            s = HipStore(2 * width, dtype, default)
            s.set_data_f64(vals)
            stores.append(s)
        got, launches = HipStore.drill_down_multi(stores, ["sum"] * n, old, new, maps, [flag] * n)
        for s, g in zip(stores, got):
            assert same(g, s.drill_down(old, new, maps, "sum", integer_measure=flag)), (cell, n)
        assert got[0].get_data_f64().reshape(k, width)[:, 0].tolist() == [34.0, 33.0, 33.0, 5.0, 4.0, 5.0]
        assert launches == expected_launches(stores, ["sum"] * n)
    # the issue's own small case, 2 x 2 parents: too narrow for the row form, one by one behind the call
    old, new, maps = [2, 2], [2, k], [ident(2), parents]
    stores = []
    for i in range(3):
        s = HipStore(4, dtype, default)
        s.set_data_f64(np.array([100.0, 14.0, 7.0 + i, default]))
        stores.append(s)
    small, _ = HipStore.drill_down_multi(stores, ["sum"] * 3, old, new, maps, [flag] * 3)
    for s, g in zip(stores, small):
        assert same(g, s.drill_down(old, new, maps, "sum", integer_measure=flag))
    assert small[0].get_data_f64()[:6].tolist() == [34.0, 33.0, 33.0, 5.0, 4.0, 5.0]
    old, new, maps = [2, width], [k, width], [parents, ident(width)]
    # the flag is part of the group: flagged and plain float64 measures do not share a launch
    if flag:
        wide = []
        for _ in range(2):
            s = HipStore(2 * width, dtype, default)
            s.set_data_f64(np.concatenate([np.full(width, 100.0), np.full(width, 14.0)]))
            wide.append(s)
        got, launches = HipStore.drill_down_multi(wide, ["sum"] * 2, old, new, maps, [True, False])
        assert got[0].get_data_f64().reshape(k, width)[:3, 0].tolist() == [34.0, 33.0, 33.0] and got[1].get_data_f64()[0] == 100.0 / 3.0
        assert launches == 2


# ------------------------------------------------------------------------------------------ mixed types, alignment
def test_mixed_cell_types_are_grouped_behind_the_call():
    old, new, sel, _ = DICE_CASES["middle-reversed"]
    rng = np.random.default_rng(14)
    cells = ("float32", "float64", "float32", "int32-nan", "float64", "float32")
    stores = [make_stores(rng, cell, 1, old)[0] for cell in cells]
    got, launches = HipStore.dice_multi(stores, old, new, sel)
    for s, g in zip(stores, got):
        assert same(g, s.dice(old, new, sel))
    assert launches == 3
    old, mid, new2, sel2, maps = FUSED_CASES["slice-then-roll"]
    stores = [make_stores(rng, cell, 1, old)[0] for cell in cells]
    rules = ["sum", "sum", "average", "sum", "sum", "sum"]
    got, launches = HipStore.dice_drillup_multi(stores, rules, old, mid, new2, sel2, maps)
    for s, rule, g in zip(stores, rules, got):
        assert same(g, s.dice_drillup(old, mid, new2, sel2, maps, rule))
    assert launches == 4  # float32 sum, float32 average, float64 sum, int32 sum


def test_plan_batch_off_the_16_byte_grid_falls_back_pair_by_pair():
    """olap_plan_run_batch on raw pointers 4 bytes off the 16-byte grid: the pairs run one by one with one cell per lane,
    and give what olap_plan_run gives on the same pointers — and what the aligned batch gives."""
    old, new, sel, _ = DICE_CASES["middle-reversed"]
    n_in, n_out = int(np.prod(old)), int(np.prod(new))
    plan = Plan.dice("float32", 0.0, old, new, sel)
    rng = np.random.default_rng(15)
    ins, batch, single, aligned = [], [], [], []
    for _ in range(3):
        vals = rng.integers(1, 7, size=n_in + 4).astype(np.float32)
        s = HipStore(n_in + 4, "float32", 0.0)
        s.set_data(vals)
        ins.append(s)
        batch.append(HipStore(n_out + 4, "float32", 0.0))
        single.append(HipStore(n_out + 4, "float32", 0.0))
        aligned.append(HipStore(n_out + 4, "float32", 0.0))
    plan.run_batch([s.values_ptr + 4 for s in ins], None, [s.values_ptr + 4 for s in batch], None)
    for i, o in zip(ins, single):
        plan.run(i.values_ptr + 4, None, o.values_ptr + 4, None)
    for b, s in zip(batch, single):
        assert b.get_data().tobytes() == s.get_data().tobytes()
        assert b.get_data()[0] == 0 and not b.get_data()[n_out + 1:].any()  # nothing written outside the pair's cells
    # the same cells from aligned buffers, batched in one launch
    shifted = []
    for s in ins:
        t = HipStore(n_in + 4, "float32", 0.0)
        t.set_data(np.roll(s.get_data(), -1))
        shifted.append(t)
    plan.run_batch([s.values_ptr for s in shifted], None, [s.values_ptr for s in aligned], None)
    for b, a in zip(batch, aligned):
        assert b.get_data()[1:1 + n_out].tobytes() == a.get_data()[:n_out].tobytes()


# ------------------------------------------------------- interleaved groups and a second chunk, against the oracle
# four groups of (cell type, default), interleaved in the list
INTERLEAVED = [("float32", 0.0), ("float64", NAN), ("float32", 0.0), ("int32", 0.0), ("float64", NAN), ("float32", NAN)]


def small_stores(rng, kinds, size):
    out = []
    for dtype, default in kinds:
        vals = rng.integers(1, 7, size=size).astype(np.float64)
        vals[rng.random(size) < 0.33] = default
        s = HipStore(size, dtype, default)
        s.set_data_f64(vals)
        out.append(s)
    return out


def equals_oracle(store, o):
    ev, es = o.typed()
    return store.type == o.type and np.array_equal(store.get_status(), es) and same_typed(store.get_data(), ev)


def test_interleaved_groups_land_at_their_own_index():
    """Every result of a list whose groups are interleaved sits at its store's index and equals the oracle's; the launches
    are the number of groups (groups in the order of their first member, members ascending)."""
    rng = np.random.default_rng(16)
    # dice [3, 4] -> [2, 4]
    old, new, sel = [3, 4], [2, 4], [[2, 0], ident(4)]
    stores = small_stores(rng, INTERLEAVED, 12)
    got, launches = HipStore.dice_multi(stores, old, new, sel)
    for i, (s, g) in enumerate(zip(stores, got)):
        assert equals_oracle(g, oracle_of(s).dice(old, new, sel)), ("dice", i)
    assert launches == 4
    # the fused dice -> drillUp [3, 4] -> [2, 4] -> [2, 2] with two rules interleaved as well: float32/0 sum (0, 2),
    # float64/NaN highest (1, 4), int32/0 sum, float32/NaN sum, float32/0 highest
    mid, rolled, maps = [2, 4], [2, 2], [ident(2), [0, 0, 1, 1]]
    kinds = INTERLEAVED + [("float32", 0.0)]
    rules = ["sum", "highest", "sum", "sum", "highest", "sum", "highest"]
    stores = small_stores(rng, kinds, 12)
    got, launches = HipStore.dice_drillup_multi(stores, rules, old, mid, rolled, sel, maps)
    for i, (s, rule, g) in enumerate(zip(stores, rules, got)):
        assert equals_oracle(g, oracle_of(s).dice(old, mid, sel).drill_up(mid, rolled, maps, rule)), ("fused", i, rule)
    assert launches == 5
    # drillDown [3, 516] -> [5, 516] in the row form (the form that batches), `sum` and a copying rule interleaved
    k, parents = groups_of([2, 1, 2])
    old, new, maps = [3, 516], [k, 516], [parents, ident(516)]
    rules = ["sum", "average", "sum", "sum", "average", "sum", "average"]
    for (dtype, default), rule in zip(kinds, rules):
        assert "drilldown_rows" in Plan.drilldown(dtype, default, rule, old, new, maps).kernel_name
    stores = small_stores(rng, kinds, 3 * 516)
    got, launches = HipStore.drill_down_multi(stores, rules, old, new, maps)
    for i, (s, rule, g) in enumerate(zip(stores, rules, got)):
        assert equals_oracle(g, oracle_of(s).drill_down(old, new, maps, rule)), ("drillDown", i, rule)
    assert launches == 5


def test_nine_of_one_group_make_a_second_chunk_of_the_fused_call():
    old, mid, new, sel, maps = [3, 4], [2, 4], [2, 2], [[2, 0], ident(4)], [ident(2), [0, 0, 1, 1]]
    stores = small_stores(np.random.default_rng(17), [("float32", 0.0)] * 9, 12)
    got, launches = HipStore.dice_drillup_multi(stores, ["sum"] * 9, old, mid, new, sel, maps)
    assert launches == 2
    for i, (s, g) in enumerate(zip(stores, got)):
        assert equals_oracle(g, oracle_of(s).dice(old, mid, sel).drill_up(mid, new, maps, "sum")), i
