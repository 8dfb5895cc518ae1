"""olap_store_load_multi / olap_store_reorder_multi: the measures two cubes share loaded (and the measures of a cube
reordered) in one call, in launches of up to 8 pairs per group of (source type, target type, both defaults) — the same
cells and masks as the single-store calls leave."""
import numpy as np
import pytest

from conftest import load_package
from golden_util import same_typed
from oracle.oracle import OracleStore

pytestmark = pytest.mark.gpu

pkg = load_package()
NAN = float("nan")

# each: (my lengths, his lengths, maps, the kernel a same-type plan takes)
def lane_case():
    return [6, 8, 12], [4, 8, 12], [np.array([4, -1, 0, 2], np.int32), np.arange(8, dtype=np.int32), np.arange(12, dtype=np.int32)], "load_scatter (16-byte lanes)"


def permuted_rows_case():
    return [5, 7], [5, 7], [np.arange(5, dtype=np.int32), np.array([3, 0, 6, 1, 5, 2, 4], np.int32)], "load_permute_rows_kernel"


def run_case():
    return [4, 10], [6, 10], [np.array([3, -1, 0, 2, -1, 1], np.int32), np.array([9, 3, 0, 7, 1, 8, 2, 6, 4, 5], np.int32)], "load_scatter (16-byte runs of the other store)"


FORMS = {"lanes": lane_case, "runs": run_case, "permuted rows": permuted_rows_case}


def store(type_name, default, dense):
    s = pkg.HipStore(len(dense), type_name, default)
    s.set_data_f64(dense)
    return s


def pair(rng, my_type, his_type, my_default, his_default, n_my, n_his):
    """(target, a second target with the same cells, source)"""
    mine = np.where(rng.random(n_my) < 0.5, my_default, rng.integers(1, 50, size=n_my).astype(np.float64))
    his = np.where(rng.random(n_his) < 0.4, his_default, rng.integers(50, 99, size=n_his).astype(np.float64))
    return store(my_type, my_default, mine), store(my_type, my_default, mine), store(his_type, his_default, his)


def same_store(a, b):
    return np.array_equal(a.get_status(), b.get_status()) and same_typed(a.get_data(), b.get_data())


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("type_name,my_default,his_default", [("float32", 0.0, 0.0), ("int32", NAN, NAN), ("float64", 0.0, NAN)])
def test_same_typed_pairs_leave_in_launches_of_eight(form, type_name, my_default, his_default):
    my_len, his_len, maps, kernel = FORMS[form]()
    assert pkg.Plan.load(type_name, my_default, his_default, my_len, his_len, maps).kernel_name == kernel
    n_my, n_his = int(np.prod(my_len)), int(np.prod(his_len))
    rng = np.random.default_rng(4100)
    for n, want in [(1, 1), (2, 1), (8, 1), (9, 2)]:
        trios = [pair(rng, type_name, type_name, my_default, his_default, n_my, n_his) for _ in range(n)]
        for _, ref, his in trios:
            ref.load(his, my_len, his_len, maps)
        launches = pkg.HipStore.load_many([t[0] for t in trios], [t[2] for t in trios], my_len, his_len, maps)
        assert launches == want, (form, n)
        for i, (mine, ref, _) in enumerate(trios):
            assert same_store(mine, ref), (form, n, i)


def test_groups_by_types_and_defaults_and_a_repeat_gives_the_same():
    """{f32 <- f32 x3, f32 <- f64 x2, f64 <- f64 under a NaN default x1}: three groups, three launches; the pair with the
    other default sits in the middle of the list.  The repeat of the call finds its three plans in the plan cache (which
    shows nothing to a test): the same launches and the same cells."""
    my_len, his_len, maps, _ = lane_case()
    n_my, n_his = int(np.prod(my_len)), int(np.prod(his_len))
    rng = np.random.default_rng(4200)
    kinds = [("float32", "float32", 0.0, 0.0), ("float32", "float64", 0.0, 0.0), ("float32", "float32", 0.0, 0.0),
             ("float64", "float64", NAN, NAN), ("float32", "float64", 0.0, 0.0), ("float32", "float32", 0.0, 0.0)]
    trios = [pair(rng, mt, ht, md, hd, n_my, n_his) for mt, ht, md, hd in kinds]
    for (mt, ht, md, hd), (_, ref, his) in zip(kinds, trios):
        if mt == ht:
            ref.load(his, my_len, his_len, maps)
        else:
            tmp = pkg.HipStore(n_his, mt, hd)
            tmp.set_data_f64(his.get_data_f64())
            ref.load(tmp, my_len, his_len, maps)
    for attempt in range(2):
        launches = pkg.HipStore.load_many([t[0] for t in trios], [t[2] for t in trios], my_len, his_len, maps)
        assert launches == 3, attempt
        for i, (mine, ref, _) in enumerate(trios):
            assert same_store(mine, ref), (attempt, i)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("his_type", ["int32", "float32"])
def test_pairs_with_and_without_a_source_mask_in_one_batch(form, his_type):
    """olap_plan_run_batch over a load plan: pairs of which only some carry a source mask run pair by pair behind the
    call and give what olap_plan_run gives for each."""
    my_len, his_len, maps, _ = FORMS[form]()
    n_my, n_his = int(np.prod(my_len)), int(np.prod(his_len))
    rng = np.random.default_rng(4300)
    plan = pkg.Plan.load_typed("int32", his_type, NAN, NAN, my_len, his_len, maps)
    trios = [pair(rng, "int32", his_type, NAN, NAN, n_my, n_his) for _ in range(3)]
    masks = [t[2].status_ptr if i != 1 else 0 for i, t in enumerate(trios)]
    for (_, ref, his), m in zip(trios, masks):
        plan.run(his.values_ptr, m, ref.values_ptr, ref.status_ptr)
    plan.run_batch([t[2].values_ptr for t in trios], masks, [t[0].values_ptr for t in trios], [t[0].status_ptr for t in trios])
    for i, (mine, ref, _) in enumerate(trios):
        assert same_store(mine, ref), (form, i)
    # all with a mask: one launch's worth of pairs, the same cells as pair by pair
    trios = [pair(rng, "int32", his_type, NAN, NAN, n_my, n_his) for _ in range(3)]
    for _, ref, his in trios:
        plan.run(his.values_ptr, his.status_ptr, ref.values_ptr, ref.status_ptr)
    plan.run_batch([t[2].values_ptr for t in trios], [t[2].status_ptr for t in trios], [t[0].values_ptr for t in trios],
                   [t[0].status_ptr for t in trios])
    for i, (mine, ref, _) in enumerate(trios):
        assert same_store(mine, ref), (form, "masks", i)


@pytest.mark.parametrize("perm", [[2, 0, 1], [1, 0, 2]])
@pytest.mark.parametrize("type_name,default", [("float32", 0.0), ("int32", NAN), ("float64", NAN)])
def test_reorder_many_in_launches_of_eight(type_name, default, perm):
    """[4, 6, 10] by [2, 0, 1] moves the innermost dimension (the brick forms, or the gather for 8-byte cells), by
    [1, 0, 2] leaves it alone (the gather with 16-byte lanes): both leave in launches of up to 8 stores."""
    old_len = [4, 6, 10]
    name = pkg.Plan.reorder(type_name, default, old_len, perm).kernel_name
    print("reorder %s by %s: %s" % (type_name, perm, name))
    assert name != "transpose_xy_kernel"
    if perm == [1, 0, 2]:
        assert name == "gather(reorder)"
    rng = np.random.default_rng(4400)
    for n, want in [(3, 1), (9, 2)]:
        stores = [store(type_name, default, np.where(rng.random(240) < 0.4, default, rng.integers(1, 99, size=240).astype(np.float64))) for _ in range(n)]
        outs, launches = pkg.HipStore.reorder_many(stores, old_len, perm)
        assert launches == want, n
        for i, (s, o) in enumerate(zip(stores, outs)):
            assert same_store(o, s.reorder(old_len, perm)), (n, i)


def test_reorder_many_as_a_transpose():
    old_len, perm = [33, 65], [1, 0]
    assert pkg.Plan.reorder("float32", 0.0, old_len, perm).kernel_name == "transpose_xy_kernel"
    rng = np.random.default_rng(4500)
    stores = [store("float32", 0.0, np.where(rng.random(33 * 65) < 0.4, 0.0, rng.integers(1, 99, size=33 * 65).astype(np.float64))) for _ in range(3)]
    outs, launches = pkg.HipStore.reorder_many(stores, old_len, perm)
    print("reorder_many, two-axis transpose of 3 stores: %d launches" % launches)
    assert launches == 3  # the transpose runs pair by pair behind the call
    for i, (s, o) in enumerate(zip(stores, outs)):
        assert same_store(o, s.reorder(old_len, perm)), i


def test_mixed_reorder_group_and_no_stores():
    old_len, perm = [4, 6, 10], [2, 0, 1]
    rng = np.random.default_rng(4600)
    kinds = [("float32", 0.0), ("float64", 0.0), ("float32", 0.0), ("float32", NAN)]
    stores = [store(t, d, np.where(rng.random(240) < 0.4, d, rng.integers(1, 99, size=240).astype(np.float64))) for t, d in kinds]
    outs, launches = pkg.HipStore.reorder_many(stores, old_len, perm)
    assert launches == 3
    for s, o in zip(stores, outs):
        assert (o.type, o.default_is_nan) == (s.type, s.default_is_nan) and same_store(o, s.reorder(old_len, perm))
    assert pkg.HipStore.reorder_many([], old_len, perm) == ([], 0)
    assert pkg.HipStore.load_many([], [], old_len, old_len, [np.arange(l, dtype=np.int32) for l in old_len]) == 0


# four groups of (cell type, default), interleaved in the list
INTERLEAVED = [("float32", 0.0), ("float64", NAN), ("float32", 0.0), ("int32", 0.0), ("float64", NAN), ("float32", NAN)]


def small_dense(rng, n, default, low):
    return np.where(rng.random(n) < 0.4, default, rng.integers(low, low + 9, size=n).astype(np.float64))


def oracle_store(type_name, default, dense):
    o = OracleStore(len(dense), type_name, default)
    o.set_data(dense)
    return o


def equals_oracle(store, o):
    values, status = o.typed()
    return store.type == o.type and np.array_equal(store.get_status(), status) and same_typed(store.get_data(), values)


def test_interleaved_groups_land_at_their_own_index_as_the_oracle_has_them():
    """load [3, 4] <- [2, 4] and reorder [2, 3, 4] over a list whose groups are interleaved: every result sits at its own
    index and equals the oracle's; the launches are the number of groups."""
    rng = np.random.default_rng(4700)
    my_len, his_len, maps = [3, 4], [2, 4], [np.array([2, 0], np.int32), np.arange(4, dtype=np.int32)]
    mine = [small_dense(rng, 12, d, 1) for _, d in INTERLEAVED]
    his = [small_dense(rng, 8, d, 50) for _, d in INTERLEAVED]
    targets = [store(t, d, v) for (t, d), v in zip(INTERLEAVED, mine)]
    sources = [store(t, d, v) for (t, d), v in zip(INTERLEAVED, his)]
    assert pkg.HipStore.load_many(targets, sources, my_len, his_len, maps) == 4
    for i, (t, d) in enumerate(INTERLEAVED):
        want = oracle_store(t, d, mine[i])
        want.load(oracle_store(t, d, his[i]), my_len, his_len, maps)
        assert equals_oracle(targets[i], want), i
    old_len, perm = [2, 3, 4], [2, 0, 1]
    dense = [small_dense(rng, 24, d, 1) for _, d in INTERLEAVED]
    stores = [store(t, d, v) for (t, d), v in zip(INTERLEAVED, dense)]
    outs, launches = pkg.HipStore.reorder_many(stores, old_len, perm)
    assert launches == 4
    for i, (t, d) in enumerate(INTERLEAVED):
        assert equals_oracle(outs[i], oracle_store(t, d, dense[i]).reorder(old_len, perm)), i
