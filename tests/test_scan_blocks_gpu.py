"""olap_store_blocks_report: what every combination of the scanned dimensions' items receives (Cube.scan,
Cube.iterateOverDimension), for several measures of one cube, in one device pass.  The reference is numpy —
get_data_f64().reshape(lens).transpose(scanned + kept) of stores filled through set_data_f64 / set_value — compared bit
for bit wherever the expected value is not NaN (the sign of zero counts; NaN payloads do not: isnan must match).

The transposing kernel moves tiles of up to 64 x 64 cells: [65, 3, 67] puts one cell past that edge on both axes."""
import itertools
import sys

import numpy as np
import pytest

from conftest import load_package

pytestmark = pytest.mark.gpu

pkg = load_package()
capi = pkg.capi
hipstore = sys.modules[pkg.HipStore.__module__]
NAN = float("nan")
TYPES = ["int32", "uint32", "float32", "float64"]
ALL_KINDS = [(t, d) for t in TYPES for d in (0.0, NAN)]


def dense_values(rng, type_name, default, size):
    """`size` float64 values of which about half are the default (unset cells); the set ones are exact in the cell type
    and include the values that tell a wrong conversion or an ignored mask apart"""
    if type_name == "int32":
        vals = rng.integers(-2**31, 2**31, size=size).astype(np.float64)
        special = [-2.0**31, 0.0] if np.isnan(default) else [-2.0**31, 2.0**31 - 1]
    elif type_name == "uint32":
        vals = rng.integers(1, 2**32, size=size).astype(np.float64)
        special = [0.0, 2.0**32 - 1] if np.isnan(default) else [2.0**32 - 1, 1.0]
    else:
        cell = np.float32 if type_name == "float32" else np.float64
        vals = (rng.standard_normal(size) * 1000).astype(cell).astype(np.float64)
        special = [-0.0, np.inf, -np.inf] if np.isnan(default) else [NAN, np.inf, -np.inf]
    if not np.isnan(default):
        vals[vals == 0] = 1.0
    unset = rng.random(size) < 0.5
    is_set = ~unset
    vals[unset] = default
    at = np.flatnonzero(is_set)[: len(special)]  # the special values go into cells that are set
    vals[at] = special
    return vals, is_set


def make_store(rng, type_name, default, size):
    vals, is_set = dense_values(rng, type_name, default, size)
    # the inputs themselves: a kernel that ignores the mask, or the default, cannot pass on them
    assert is_set.sum() * 4 >= size and (~is_set).sum() * 4 >= size, (type_name, default, size)
    s = pkg.HipStore(size, type_name, default)
    s.set_data_f64(vals)
    if size > 2:  # one cell through the other writer
        i = int(np.flatnonzero(is_set)[-1])
        s.set_value(i, 7.0)
    return s


def expected(store, lens, flags):
    scanned = [d for d, f in enumerate(flags) if f]
    kept = [d for d, f in enumerate(flags) if not f]
    combos = int(np.prod([lens[d] for d in scanned])) if scanned else 1
    return np.ascontiguousarray(store.get_data_f64().reshape(lens).transpose(scanned + kept)).reshape(combos, -1)


def assert_same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan]), what


_stores = {}


def stores_of(lens, kinds):
    """one store per (type, default) of `kinds` for a cube of `lens`, made once per test session"""
    key = (tuple(lens), tuple((t, str(d)) for t, d in kinds))
    if key not in _stores:
        rng = np.random.default_rng(811)
        _stores[key] = [make_store(rng, t, d, int(np.prod(lens))) for t, d in kinds]
    return _stores[key]


def check_case(lens, flags, kinds, want_launches):
    stores = stores_of(lens, kinds)
    got, launches = hipstore.blocks_report(stores, lens, flags)
    assert launches == want_launches, (lens, flags)
    for k, s in enumerate(stores):
        assert_same_bits(got[k], expected(s, lens, flags), (lens, flags, kinds[k]))


SUBSETS_3 = [f for f in itertools.product([0, 1], repeat=3) if any(f)]  # every non-empty subset, all three (B = 1) included


@pytest.mark.parametrize("flags", SUBSETS_3)
def test_odd_extents_every_subset_of_scanned_dimensions(flags):
    # 8 stores, 8 groups (cell type x default): both kernels, every vector width with a tail
    check_case([3, 5, 7], list(flags), ALL_KINDS, 8)


@pytest.mark.parametrize("scanned", [(2,), (0,), (0, 2), (1,)])
def test_one_cell_past_the_tile_edge(scanned):
    flags = [1 if d in scanned else 0 for d in range(3)]
    check_case([65, 3, 67], flags, [("float32", 0.0), ("int32", NAN), ("float64", NAN), ("uint32", 0.0)], 4)


@pytest.mark.parametrize("flags", [[1, 0, 1, 0, 1, 0], [0, 1, 0, 1, 0, 1]])
def test_six_dimensions_alternating(flags):
    check_case([2, 3, 2, 3, 2, 3], flags, [("float32", NAN), ("int32", NAN), ("float64", 0.0)], 3)


@pytest.mark.parametrize("flags", [[0, 0, 1], [1, 0, 0], [0, 1, 0]])
def test_nine_measures_cross_the_launch_boundary(flags):
    lens = [3, 5, 7]
    rng = np.random.default_rng(812)
    stores = [make_store(rng, "float32", 0.0, 105) for _ in range(9)]
    got, launches = hipstore.blocks_report(stores, lens, flags)
    assert launches == 2
    wants = [expected(s, lens, flags) for s in stores]
    for k in range(9):
        assert_same_bits(got[k], wants[k], (flags, k))
    # every measure in its own slot: no two measures hold the same cells
    assert len({w.tobytes() for w in wants}) == 9


def test_launches_equal_the_number_of_groups():
    lens = [3, 5, 7]
    rng = np.random.default_rng(813)
    # 8 stores in four groups of two, interleaved
    kinds = [("int32", NAN), ("float32", 0.0), ("uint32", 0.0), ("float64", NAN)] * 2
    stores = [make_store(rng, t, d, 105) for t, d in kinds]
    got, launches = hipstore.blocks_report(stores, lens, [0, 1, 1])
    assert launches == 4
    for k, s in enumerate(stores):
        assert_same_bits(got[k], expected(s, lens, [0, 1, 1]), kinds[k])
    got, launches = hipstore.blocks_report(stores_of(lens, ALL_KINDS), lens, [1, 1, 0])
    assert launches == 8


def test_refusals_that_need_a_device(monkeypatch):
    lens = [3, 5, 7]
    rng = np.random.default_rng(814)
    a, b = make_store(rng, "float32", 0.0, 105), make_store(rng, "float32", 0.0, 105)
    tracked = make_store(rng, "float32", 0.0, 105)
    tracked.track_order()
    with pytest.raises(pkg.OlapError) as e:
        hipstore.blocks_report([a, tracked], lens, [1, 0, 0])
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and str(e.value).startswith("ordered: store 1 of the batch tracks its insertion order")
    with pytest.raises(pkg.OlapError) as e:
        hipstore.blocks_report([a, make_store(rng, "float32", 0.0, 104)], lens, [1, 0, 0])
    assert e.value.code == capi.ERR_LENGTH_MISMATCH and str(e.value) == "store holds 104 cells but the dimensions describe 105"
    # a size mismatch is reported before a tracked store
    with pytest.raises(pkg.OlapError) as e:
        hipstore.blocks_report([tracked, make_store(rng, "float32", 0.0, 104)], lens, [1, 0, 0])
    assert e.value.code == capi.ERR_LENGTH_MISMATCH
    # the byte cap, lowered through the environment: two stores of 105 cells are 1680 bytes
    monkeypatch.setenv("OLAP_BLOCKS_MAX_BYTES", "1679")
    with pytest.raises(pkg.OlapError) as e:
        hipstore.blocks_report([a, b], lens, [1, 0, 0])
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and str(e.value).startswith("blocks: ")
    monkeypatch.setenv("OLAP_BLOCKS_MAX_BYTES", "1680")
    got, launches = hipstore.blocks_report([a, b], lens, [1, 0, 0])
    assert launches == 1
    assert_same_bits(got[1], expected(b, lens, [1, 0, 0]), "at the cap")
