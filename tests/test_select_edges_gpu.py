"""select_total / copy_select / the sharded total at the edges of their layouts and of the exactness certificate
(DESIGN K8), against the plain references of tests/select_reference.py.  Every total must equal, bit for bit, the
left-to-right float64 sum in nesting order; the path it took must be the one the certificate, restated in exact
arithmetic, predicts; and a certified total must be the exact sum.  Under a NaN default the selections read set cells,
except where a case is about missing or unset cells (NaN would hide every other error)."""
import math
import struct
import zlib

import numpy as np
import pytest

from conftest import load_package
from select_reference import exact_total, nesting_positions, predict_path, sequential_total, split_free, terms_at

pytestmark = pytest.mark.gpu

pkg = load_package()
DTYPES = ["int32", "uint32", "float32", "float64"]
NAN = float("nan")
P = math.ldexp


def bits(x):
    return struct.pack("<d", x) if x == x else b"nan"


def get_values(store):
    """getValue of every cell (the default where unset)"""
    data, st = store.get_data_f64(), store.get_status()
    default = NAN if store.default_is_nan else 0.0
    return np.where((st & 2) != 0, data, default)


def make_store(dtype, nan_default, dense):
    dense = np.asarray(dense, dtype=np.float64)
    s = pkg.HipStore(dense.size, dtype, NAN if nan_default else 0.0)
    s.set_data_f64(dense)
    return s


def check_total(store, lens, levels, values=None, label=None):
    """the three promises of one select_total; returns the path"""
    values = get_values(store) if values is None else values
    default = NAN if store.default_is_nan else 0.0
    want = sequential_total(values, default, nesting_positions(lens, levels))
    dims, m = split_free(levels)
    terms = terms_at(values, default, nesting_positions(lens, dims))
    got, path = store.select_total(lens, levels)
    assert bits(got) == bits(want), (label, got, want)
    assert path == predict_path(terms, m), (label, path)
    if path == "device":
        exact = exact_total(terms)
        if exact is not None:
            assert got == float(exact * m), (label, got, float(exact * m))
    return path


def fits(dtype, terms):
    t = np.asarray(terms, dtype=np.float64)
    if dtype == "float64":
        return True
    if dtype == "float32":
        return bool(np.all(np.abs(t) < 3.4e38) and np.all(t.astype(np.float32).astype(np.float64) == t))
    lo, hi = (-(2 ** 31), 2 ** 31) if dtype == "int32" else (0, 2 ** 32)
    return bool(np.all(t == np.floor(t)) and np.all(t >= lo) and np.all(t < hi))


# ---- 1. the certificate at its bounds --------------------------------------------------------------------------
# (terms, m): the worked cases of tests/test_select_reference.py, where the bound, the subnormal exponents, the
# overflow of A and the free-level multiplier each decide the path
BOUNDARY = [
    ([P(1, 51), P(1, 51) - 1, 1.0], 1),
    ([P(1, 51), P(1, 51), 1.0], 1),
    ([P(1, 52), 1.0, P(1, 52), 1.0], 1),
    ([P(1, 40) + 1, P(1, 40) - 1], 2048),
    ([P(1, 40) + 1, P(1, 40) - 1], 2049),
    ([P(1, -1023), P(1, -1074)], 1),
    ([P(1, -1022), P(1, -1074)], 1),
    ([P(1, 1023), -P(1, 1022)], 1),
    ([P(1, 1023), P(1, 1022), -P(1, 1022)], 1),
    ([P(1, 1023), P(1, 1023), -P(1, 1023)], 1),
    ([3 * P(1, -149), P(1, -127)], 1),
    ([P(1, -149), 1.5], 1),
    ([float(2 ** 32 - 1)] * (1 << 20), 1),
    ([float(2 ** 31 - 1), -float(2 ** 31)] * 7, 3),  # the Int32 extremes
]


def layout(kind, terms, rng):
    """(lens, dense cells, levels) holding `terms` once among zero cells: "1d" (an identity list), "flat" (the terms
    scattered over a 2-D cube read through permuted lists: short runs) or "row" (inside a row of >= 1024 cells, the
    row picked among others: 16-byte loads)"""
    k = len(terms)
    if kind == "1d":
        return [k], np.asarray(terms), [(0, list(range(k)))]
    if kind == "flat":
        a, b = 3, k // 3 + 2
        dense = np.zeros(a * b)
        dense[rng.permutation(a * b)[:k]] = terms
        p1, p0 = rng.permutation(b), rng.permutation(a)
        if np.array_equal(p1, np.arange(b)):
            p1 = p1[::-1]
        return [a, b], dense, [(1, [int(x) for x in p1]), (0, [int(x) for x in p0])]
    r = max(1024, k + 5)
    dense = np.zeros(3 * r)
    dense[r + 3: r + 3 + k] = terms
    return [3, r], dense, [(0, [1, 2, 0]), (1, list(range(r)))]


@pytest.mark.parametrize("kind", ["1d", "flat", "row"])
@pytest.mark.parametrize("nan_default", [False, True])
def test_certificate_boundaries(kind, nan_default):
    rng = np.random.default_rng(17)
    paths = set()
    for ci, (terms, m) in enumerate(BOUNDARY):
        lens, dense, levels = layout(kind, terms, rng)
        if m > 1:  # the free levels give m, at the front, inside or at the back of the nesting order
            at = {"1d": len(levels), "flat": 1, "row": 0}[kind]
            levels = levels[:at] + [(-1, [0] * m)] + levels[at:]
        for dtype in DTYPES:
            if not fits(dtype, terms):
                continue
            s = make_store(dtype, nan_default, dense)
            values = get_values(s)
            held = terms_at(values, 0.0, nesting_positions(lens, split_free(levels)[0]))
            assert sorted(held[held != 0].tolist()) == sorted(t for t in terms if t != 0), (ci, dtype)  # nothing flushed
            paths.add(check_total(s, lens, levels, values, label=(ci, dtype, kind)))
            del s
    assert paths == {"device", "sequential"}


# ---- 2. real-valued random data ----------------------------------------------------------------------------------

def random_levels(rng, lens, allow_missing, max_combos=200_000):
    while True:
        levels = []
        for d in rng.permutation(len(lens)):
            d = int(d)
            r = rng.random()
            if r < 0.3:
                e = list(range(lens[d]))  # whole and in order: folds into the contiguous run
            elif r < 0.5:
                e = [int(x) for x in rng.permutation(lens[d])]
            else:
                e = [int(x) for x in rng.integers(0, lens[d], size=int(rng.integers(1, min(lens[d], 12) + 3)))]
            if allow_missing and e and rng.random() < 0.3:
                e[int(rng.integers(0, len(e)))] = -1
            levels.append((d, e))
        for _ in range(int(rng.integers(0, 3))):
            levels.insert(int(rng.integers(0, len(levels) + 1)), (-1, [0] * int(rng.integers(1, 4))))
        if np.prod([len(e) for _, e in levels], dtype=np.float64) <= max_combos:
            return levels


def random_lens(rng):
    lens = [int(x) for x in rng.integers(1, 41, size=int(rng.integers(1, 6)))]
    while np.prod(lens, dtype=np.float64) > 60_000:
        i = int(np.argmax(lens))
        lens[i] = max(1, lens[i] // 2)
    return lens


@pytest.mark.parametrize("kind", ["float64", "float32", "dyadic"])
@pytest.mark.parametrize("nan_default", [False, True])
def test_real_valued_random_selections(kind, nan_default):
    rng = np.random.default_rng(100 + 2 * ["float64", "float32", "dyadic"].index(kind) + int(nan_default))
    paths = {"device": 0, "sequential": 0}
    for trial in range(45):
        lens = random_lens(rng)
        n = int(np.prod(lens))
        if kind == "dyadic":  # k * 2^-20: not integers, yet certified
            dtype = "float64" if trial % 2 else "float32"
            vals = rng.integers(-3000, 3000, size=n) * P(1, -20)
        else:
            dtype = kind
            vals = rng.standard_normal(n) * [1.0, 1e3, 1e-3, 1e30][trial % 4]
        if not nan_default:
            vals[rng.random(n) < 0.3] = 0.0  # unset
        s = make_store(dtype, nan_default, vals)
        levels = random_levels(rng, lens, allow_missing=not nan_default)
        paths[check_total(s, lens, levels, label=(trial, lens, levels))] += 1
    if kind == "dyadic":
        assert paths["sequential"] == 0
    elif kind == "float64":
        assert paths["sequential"] >= 20  # full 53-bit mantissas: the fallback carries these
    else:
        assert paths["device"] >= 20  # 24-bit mantissas leave the certificate 29 bits of room: mostly certified


# ---- 3. the layouts of select_total_kernel ----------------------------------------------------------------------

def int_data(rng, dtype, n):
    """small integers; the zeros are unset under a 0 default and set zeros under a NaN default"""
    return rng.integers(0 if dtype == "uint32" else -9, 10, size=n).astype(np.float64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nan_default", [False, True])
def test_layout_sweep(dtype, nan_default):
    rng = np.random.default_rng(7 + DTYPES.index(dtype))
    cases = []
    for run in (1023, 1024, 1025, 4099):  # the FLAT / ROW switch, and rows whose length is no multiple of 16
        cases.append(([5, run], [(0, [3, 1, 4, 1, 0]), (1, list(range(run)))]))
        cases.append(([5, run], [(1, list(range(run))), (-1, [0, 0]), (0, [4, 4, 2])]))
    cases.append(([2, 3, 700], [(0, [1, 0]), (1, [0, 1, 2]), (2, list(range(700)))]))  # two dimensions fold: 2 100-cell run
    # 2 100 rows > kSelBlocks: the unit loop; 2 100 entries: the lists live on the device
    cases.append(([2100, 1030], [(0, [int(x) for x in rng.permutation(2100)]), (1, list(range(1030)))]))
    # 512 entries travel inline, 513 are uploaded (FLAT and ROW)
    for k in (511, 512):
        sel0 = [int(x) for x in rng.integers(0, 600, size=k)]
        cases.append(([600, 7], [(0, sel0), (1, [4])]))
        cases.append(([600, 7], [(1, [6, 0]), (0, sel0)]))
    sel0 = [int(x) for x in rng.integers(0, 600, size=513)]
    cases.append(([600, 1100], [(0, sel0), (1, list(range(1100)))]))
    for lens, levels in cases:
        s = make_store(dtype, nan_default, int_data(rng, dtype, int(np.prod(lens))))
        assert check_total(s, lens, levels, label=(lens, [len(e) for _, e in levels])) == "device"
        del s


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nan_default", [False, True])
def test_missing_rows_in_row_mode(dtype, nan_default):
    rng = np.random.default_rng(3)
    lens = [6, 1500]
    s = make_store(dtype, nan_default, int_data(rng, dtype, 9000))
    for sel0 in ([2, -1, 5, -1], [-1], [-1, -1, 0]):
        got = s.select_total(lens, [(0, sel0), (1, list(range(1500)))])
        assert check_total(s, lens, [(0, sel0), (1, list(range(1500)))]) == "device"
        assert math.isnan(got[0]) == nan_default


@pytest.mark.parametrize("dtype", ["int32", "uint32"])
def test_integer_cells_under_a_nan_default(dtype):
    """the status mask decides which integer cells are set: loaded beside the values on the 16-byte path"""
    rng = np.random.default_rng(21)
    lens = [8, 1040]
    vals = int_data(rng, dtype, 8 * 1040)
    unset = [5, 1039, 7 * 1040 + 12, 7 * 1040 + 1039]  # rows 0 and 7 only
    vals[unset] = NAN
    s = make_store(dtype, True, vals)
    st = s.get_status()
    assert not np.any(st[unset] & 2) and np.all(st[1040: 7 * 1040] & 2)
    full = list(range(1040))
    for levels in ([(0, [1, 2, 3, 4, 5, 6]), (1, full)], [(1, full), (0, [6, 1])], [(0, [3, 0]), (1, full)], [(0, [7]), (1, full)],
                   [(1, [int(x) for x in rng.permutation(1040)]), (0, [2, 6])], [(0, [7, 2]), (1, [12, 3])], [(0, [7, 0]), (1, [1039, 3])]):
        got, _ = s.select_total(lens, levels)
        assert check_total(s, lens, levels, label=levels) == "device"
        assert math.isnan(got) == bool(np.isin(nesting_positions(lens, levels), unset).any()), levels


# ---- 4. the sequential fallback ----------------------------------------------------------------------------------

def with_big_pair(rng, vals, cells):
    """2^53 and -2^53 at two of the selected cells: the certificate fails and the nesting order decides (2^53 + 1 is
    2^53 in float64, so small terms after the big one vanish until -2^53 comes)"""
    a, b = rng.choice(np.asarray(cells), size=2, replace=False)
    vals[int(a)], vals[int(b)] = P(1, 53), -P(1, 53)
    return vals


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("nan_default", [False, True])
def test_sequential_fallback_sweep(dtype, nan_default):
    rng = np.random.default_rng(31 + int(nan_default))
    miss = not nan_default
    perm300 = [int(x) for x in rng.permutation(300)]
    cases = [
        ([7, 5, 6], [(2, [5, 0, 5, 3]), (0, [6, 2, 2, 0, 1]), (1, [4, 1, 3])]),
        ([7, 5, 6], [(1, [4, 1, 3, 1]), (2, list(range(6))), (0, list(range(7)))]),
        # free levels first, inside and last; the list after each starts with -1 where cells may be missing
        ([7, 5, 6], [(-1, [0, 0, 0]), (0, [-1, 6, 2] if miss else [1, 6, 2]), (2, [5, 0, 3]), (1, list(range(5)))]),
        ([7, 5, 6], [(2, [5, 0, 3]), (-1, [0, 0]), (0, [-1, 6, 2, 2] if miss else [3, 6, 2, 2]), (1, [4, 0])]),
        ([7, 5, 6], [(1, [0, 4]), (2, [5, 5, 1]), (0, [6, 0, 3]), (-1, [0, 0, 0])]),
        ([7, 5, 6], [(-1, [0, 0]), (1, [2, 3]), (-1, [0, 0, 0]), (0, [1, 4]), (2, list(range(6))), (-1, [0, 0])]),
        # more than 256 entries: the lists live on the device
        ([300, 4], [(1, [3, 0, 2]), (0, perm300 + perm300[:40])]),
        ([300, 4], [(0, perm300), (-1, [0, 0]), (1, [-1, 2, 1] if miss else [0, 2, 1])]),
    ]
    for lens, levels in cases:
        n = int(np.prod(lens))
        vals = rng.integers(-9, 10, size=n).astype(np.float64)
        if dtype == "float32":
            vals = vals * 0.5
        cells = nesting_positions(lens, split_free(levels)[0])
        vals = with_big_pair(rng, vals, np.unique(cells[cells >= 0]))
        s = make_store(dtype, nan_default, vals)
        assert check_total(s, lens, levels, label=(lens, levels)) == "sequential"
        del s


def test_sequential_fallback_in_several_chunks():
    """2 x (2^23 + 4097) combinations: the gather runs in two full 2^23 chunks and a remainder"""
    n = (1 << 23) + 4097
    rng = np.random.default_rng(41)
    vals = rng.standard_normal(n)
    vals[[3, n - 2]] = [P(1, 53), -P(1, 53)]
    s = make_store("float64", False, vals)
    levels = [(-1, [0, 0]), (0, list(range(n)))]
    got, path = s.select_total([n], levels)
    held = get_values(s)
    want = float(np.cumsum(np.concatenate([[0.0], held, held]))[-1])
    assert bits(got) == bits(want) == bits(sequential_total(held, 0.0, nesting_positions([n], levels)))
    # a subset of the terms already fails the certificate (A / 2^E >= 2^53), and adding terms only lowers E and
    # raises A, so the whole selection fails it too
    assert path == "sequential" and predict_path(held[:16], 2) == "sequential" and held[3] == P(1, 53)


# ---- 5. copy_select with device-resident lists ------------------------------------------------------------------

def per_cell_copy(target, source, lens, levels):
    for pos in nesting_positions(lens, levels).tolist():
        v, _ = source.get_value(pos)
        target.set_value(pos, v)


def assert_same_store(a, b):
    assert np.array_equal(a.get_status(), b.get_status())
    assert np.array_equal(a.get_data_f64(), b.get_data_f64(), equal_nan=True)
    assert np.array_equal(a.keys(), b.keys())
    ia, va = a.to_sparse()
    ib, vb = b.to_sparse()
    assert ia.tobytes() == ib.tobytes() and va.tobytes() == vb.tobytes()


@pytest.mark.parametrize("src_type,dst_type,tracked", [("float64", "int32", 0), ("int32", "float32", 1), ("float32", "uint32", 2),
                                                       ("uint32", "float64", 1), ("float64", "float32", 2)])
def test_copy_select_with_device_lists(src_type, dst_type, tracked):
    rng = np.random.default_rng(zlib.crc32(repr((src_type, dst_type, tracked)).encode()))
    lens = [320, 9]
    n = 320 * 9
    src_nan, dst_nan = bool(tracked % 2), tracked == 2
    src_vals = rng.integers(0 if src_type == "uint32" else -6, 7, size=n).astype(np.float64)
    if src_type.startswith("float"):
        src_vals = src_vals * 0.75  # fractions: truncated or kept by the target's type
    src = make_store(src_type, src_nan, src_vals)
    dst = pkg.HipStore(n, dst_type, NAN if dst_nan else 0.0)
    dst.set_data_f64(np.where(rng.random(n) < 0.5, rng.integers(1, 9, size=n).astype(np.float64), 0.0))
    if tracked:
        dst.track_order()
        if tracked == 2:  # an explicit order
            for i in rng.permutation(n)[:200]:
                dst.set_value(int(i), float(rng.integers(1, 5)))
    distinct = [int(x) for x in rng.permutation(320)[:300]]
    sel0 = distinct + [int(x) for x in rng.choice(distinct, size=60)]  # 300 distinct entries, repeats after
    rng.shuffle(sel0)
    levels = [(1, [8, 2, 2, 5, 0, 7]), (0, sel0)]
    if tracked == 1:
        levels.insert(1, (-1, [0, 0]))
    want = dst.clone()
    per_cell_copy(want, src, lens, levels)
    dst.copy_select(src, lens, levels)
    assert_same_store(dst, want)


# ---- 6. the sharded total ----------------------------------------------------------------------------------------

def sharded(comm, lens, dtype, nan_default, vals):
    from olap_in_memory_amd.sharded import ShardedStore

    return ShardedStore(comm, lens, dtype, NAN if nan_default else 0.0).set_data_f64(np.asarray(vals, dtype=np.float64))


@pytest.fixture(scope="module", params=[2, 3], ids=["two", "three"])
def comm(request):
    from olap_in_memory_amd.sharded import Comm

    c = Comm.init_all([0] * request.param)
    yield c
    c.destroy()


def comm_bounds(comm, rows):
    from olap_in_memory_amd.sharded import ShardedStore

    return ShardedStore(comm, [rows, 1], "float32", 0.0).bounds


def test_sharded_each_shard_certified_but_not_the_union(comm):
    w = comm.world
    lens = [w, 3]
    vals = np.zeros(w * 3)
    vals[0], vals[3] = P(1, 52), 1.0  # rank 0: A = 2^52, E = 52; rank 1: A = 1, E = 0; together A = 2^52 + 1 > 2^52
    if w == 3:
        vals[6] = 2.0
    whole = make_store("float64", False, vals)
    levels = [(0, list(range(w))), (1, [0, 1, 2])]
    assert check_total(whole, lens, levels) == "sequential"
    sh = sharded(comm, lens, "float64", False, vals)
    with pytest.raises(pkg.OlapError, match="^sharded:"):
        sh.select_total(levels)
    for r in range(w):  # each shard alone is certified
        got, path = sh.select_total([(0, [r]), (1, [0, 1, 2])])
        assert path == "device" and got == float(vals[3 * r: 3 * r + 3].sum())


def test_sharded_opposite_infinities_on_different_shards(comm):
    w = comm.world
    lens = [w, 4]
    vals = np.arange(1.0, w * 4 + 1)
    vals[1], vals[4 * (w - 1) + 2] = math.inf, -math.inf
    for nan_default in (False, True):
        sh = sharded(comm, lens, "float64", nan_default, vals)
        whole = make_store("float64", nan_default, vals)
        levels = [(1, [2, 1, 0]), (0, list(range(w)))]
        got, path = sh.select_total(levels)
        assert math.isnan(got) and path == "device"
        assert check_total(whole, lens, levels) == "device"
        got, path = sh.select_total([(0, [0]), (1, [1, 3])])  # one infinity alone
        assert got == math.inf and path == "device"


def test_sharded_missing_rows_counted_once(comm):
    rng = np.random.default_rng(51)
    lens = [5, 3, 4]
    n = 60
    for dtype in DTYPES:
        vals = rng.integers(1, 9, size=n).astype(np.float64)  # every cell set
        for nan_default in (False, True):
            sh = sharded(comm, lens, dtype, nan_default, vals)
            whole = make_store(dtype, nan_default, vals)
            for levels in ([(0, [1, -1, 4]), (1, [2, 0]), (2, list(range(4)))], [(2, [3, 1]), (0, [-1]), (1, [0, 1, 2])],
                           [(0, [-1, -1, 0, 3]), (-1, [0, 0]), (1, [1]), (2, [0, 2])]):
                got, path = sh.select_total(levels)
                want, wpath = whole.select_total(lens, levels)
                assert bits(got) == bits(want) and path == wpath == "device", (dtype, nan_default, levels)
                assert math.isnan(got) == nan_default
                check_total(whole, lens, levels)


def test_sharded_rank_without_rows():
    """dimension 0 of length 2 over three shards: the last rank holds no rows"""
    from olap_in_memory_amd.sharded import Comm

    comm = Comm.init_all([0, 0, 0])
    try:
        rng = np.random.default_rng(61)
        lens = [2, 5]
        assert comm_bounds(comm, 2) == [0, 1, 2, 2]
        for dtype in DTYPES:
            for nan_default in (False, True):
                vals = rng.integers(1, 9, size=10).astype(np.float64)
                sh = sharded(comm, lens, dtype, nan_default, vals)
                whole = make_store(dtype, nan_default, vals)
                for levels in ([(0, [1, 0, 1]), (1, [4, 0])], [(1, list(range(5))), (0, [1])], [(0, [0, 1]), (1, list(range(5)))],
                               [(-1, [0, 0, 0]), (0, [1, -1]), (1, [2])]):
                    got, path = sh.select_total(levels)
                    assert bits(got) == bits(whole.select_total(lens, levels)[0]) and path == "device", (dtype, levels)
                    check_total(whole, lens, levels)
    finally:
        comm.destroy()


def test_sharded_random_real_data(comm):
    """certified exactly when the whole selection is: then bit for bit the one-device total, else an error"""
    rng = np.random.default_rng(71)
    lens = [5, 4, 3]
    n = 60
    seen = set()
    for trial in range(40):
        dtype = "float64" if trial % 2 else "float32"
        vals = rng.standard_normal(n) * (1.0 if trial % 4 < 2 else 1e6)
        if trial % 3 == 0:
            vals = np.round(vals * 64) / 64  # dyadic: mostly certified
        whole = make_store(dtype, False, vals)
        sh = sharded(comm, lens, dtype, False, vals)
        levels = random_levels(rng, lens, allow_missing=True)
        if trial % 5 == 0:  # small selections: often a single term
            levels = [(a, e[:1]) if a >= 0 else (a, e) for a, e in levels]
        dims, m = split_free(levels)
        values = get_values(whole)
        predicted = predict_path(terms_at(values, 0.0, nesting_positions(lens, dims)), m)
        seen.add(predicted)
        if predicted == "sequential":
            with pytest.raises(pkg.OlapError, match="^sharded:"):
                sh.select_total(levels)
        else:
            got, path = sh.select_total(levels)
            assert path == "device" and bits(got) == bits(whole.select_total(lens, levels)[0]), (trial, levels)
        check_total(whole, lens, levels, values)
    assert seen == {"device", "sequential"}


# ---- 9. the store total and count_set (total_kernel) -------------------------------------------------------------

def _sizes(dtype):
    v = 16 // (8 if dtype == "float64" else 4)
    per_block = 256 * v * 4  # cells one sweep of a workgroup covers
    out = set(range(1, 3 * v + 2))
    for k in (1, 2, 3, 2048, 2049):
        out |= {k * per_block - 1, k * per_block, k * per_block + 1}
    return sorted(out)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nan_default", [False, True])
def test_store_total_and_count_set(dtype, nan_default):
    rng = np.random.default_rng(81 + DTYPES.index(dtype) * 2 + int(nan_default))
    for n in _sizes(dtype):
        vals = rng.integers(0 if dtype == "uint32" else -99, 100, size=n).astype(np.float64)
        vals[rng.random(n) < 0.2] = 0.0  # unset under a 0 default, a set zero under NaN
        if nan_default:
            vals[rng.random(n) < 0.2] = NAN  # unset; integer cells keep them in the status mask
        s = make_store(dtype, nan_default, vals)
        set_ = ~np.isnan(vals) if nan_default else vals != 0
        want = int(vals[set_].astype(np.int64).sum())
        assert s.total == float(want), (n, s.total, want)
        assert s.count_set() == int(set_.sum()), n
        # the last cell alone: the n % V tail
        if n > 1:
            s.set_value(n - 1, 12345.0)
            assert s.total == float(want - (int(vals[n - 1]) if set_[n - 1] else 0) + 12345), n
        del s
