"""olap_store_set_formula (a computed measure written straight into a stored one) against the chain it replaces:
target.set_data_f64(olap_store_eval_formula(...)) on a twin store.  Typed cells, mask, get_data_f64 and the tracked key
order are compared bit for bit (a NaN cell compares as NaN); programs of the opcodes numpy restates are also checked
against that restatement, converted as a TypedArray store converts."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_package

pytestmark = pytest.mark.gpu

pkg = load_package()
capi = pkg.capi
DTYPES = ["int32", "uint32", "float32", "float64"]
NAN = float("nan")

# opcodes (js/formula.js OP, csrc FormulaOp)
CONST, INPUT, SCALAR, ADD, SUB, MUL, DIV, MOD, POW, NEG, NANADD, SELECT, MIN, MAX, ATAN2, HYPOT, ROUNDTO, ISNAN = range(18)
ABS, CEIL, FLOOR, ROUND, TRUNC, SQRT, CBRT, EXP, LN, LOG10, LOG2, SIGN, SIN, COS, TAN, ASIN, ACOS, ATAN, NOT = range(20, 39)
UNARY = [NEG, ISNAN, ABS, CEIL, FLOOR, TRUNC, SQRT, SIGN, NOT]  # what evaluate() below restates
BINARY = [ADD, SUB, MUL, DIV, MOD, NANADD, MIN, MAX]
ALL_UNARY = [NEG, ISNAN] + list(range(ABS, NOT + 1))
ALL_BINARY = [ADD, SUB, MUL, DIV, MOD, POW, NANADD, MIN, MAX, ATAN2, HYPOT, ROUNDTO]

# one trip of the kernel's grid-stride loop covers at most 2 048 workgroups x 256 lanes x 4 cells
ONE_TRIP = 2048 * 256 * 4
SIZES = [1, 3, 4, 5, 255, 256, 257, 1021, 1024, 1025]


def _js_minmax(a, b, lo):
    both_zero = (a == 0) & (b == 0)
    pick_a = np.where(both_zero, np.signbit(a) == lo, (a < b) if lo else (a > b))
    r = np.where(pick_a, a, b)
    return np.where(np.isnan(a) | np.isnan(b), np.nan, r)


def evaluate(code, consts, inputs, scalars=()):
    """the postfix program over float64 arrays, with the JS semantics of js/formula.js evaluate()"""
    st = []
    pc = 0
    with np.errstate(all="ignore"):
        while pc < len(code):
            op = code[pc]
            if op == CONST:
                pc += 1
                st.append(np.full_like(inputs[0], consts[code[pc]]))
            elif op == SCALAR:
                pc += 1
                st.append(np.full_like(inputs[0], scalars[code[pc]]))
            elif op == INPUT:
                pc += 1
                st.append(np.asarray(inputs[code[pc]], dtype=np.float64))
            elif op == SELECT:
                c, a, b = st[-3], st[-2], st[-1]
                del st[-3:]
                st.append(np.where((c == c) & (c != 0), a, b))
            elif op in UNARY:
                a = st.pop()
                st.append({NEG: lambda: -a, ISNAN: lambda: np.isnan(a).astype(np.float64), ABS: lambda: np.abs(a), CEIL: lambda: np.ceil(a),
                           FLOOR: lambda: np.floor(a), TRUNC: lambda: np.trunc(a), SQRT: lambda: np.sqrt(a),
                           SIGN: lambda: np.where(np.isnan(a), a, np.where(a > 0, 1.0, np.where(a < 0, -1.0, a))),
                           NOT: lambda: np.where((a == a) & (a != 0), 0.0, 1.0)}[op]())
            else:
                b = st.pop()
                a = st.pop()
                st.append({ADD: lambda: a + b, SUB: lambda: a - b, MUL: lambda: a * b, DIV: lambda: a / b, MOD: lambda: np.fmod(a, b),
                           NANADD: lambda: np.where(np.isnan(a) & ~np.isnan(b), b, np.where(~np.isnan(a) & np.isnan(b), a, a + b)),
                           MIN: lambda: _js_minmax(a, b, True), MAX: lambda: _js_minmax(a, b, False)}[op]())
            pc += 1
    return st[-1]


def numpy_knows(code):
    pc = 0
    while pc < len(code):
        if code[pc] in (CONST, INPUT, SCALAR):
            pc += 1
        elif code[pc] != SELECT and code[pc] not in UNARY and code[pc] not in BINARY:
            return False
        pc += 1
    return True


def stored(v, dtype, def_nan):
    """get_data_f64 of a store of `dtype` after set_data_f64(v): setValue on the number (the default unsets), then the
    TypedArray conversion (ToInt32 / ToUint32 wrap, Math.fround), then unset where the typed cell is the default"""
    v = np.asarray(v, np.float64)
    unset = np.isnan(v) if def_nan else (v == 0)
    with np.errstate(all="ignore"):
        if dtype in ("int32", "uint32"):
            m = np.fmod(np.trunc(np.where(np.isfinite(v), v, 0.0)), 4294967296.0)
            u = np.where(m < 0, m + 4294967296.0, m).astype(np.uint64).astype(np.uint32)
            t = (u.view(np.int32) if dtype == "int32" else u).astype(np.float64)
        else:
            t = v.astype(np.float32).astype(np.float64) if dtype == "float32" else v
    unset = unset | (np.isnan(t) if def_nan else (t == 0))
    return np.where(unset, NAN if def_nan else 0.0, t)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    eq = a.view("u%d" % a.dtype.itemsize) == b.view("u%d" % b.dtype.itemsize)
    if a.dtype.kind == "f":
        eq = eq | (np.isnan(a) & np.isnan(b))
    return bool(np.all(eq))


def eval_formula(code, consts, inputs, scalars=()):
    """olap_store_eval_formula: the float64 cube the host path carries"""
    from olap_in_memory_amd.hipstore import _formula

    prog = _formula(code, consts, inputs)
    sc = (C.c_double * max(len(scalars), 1))(*scalars)
    out = np.zeros(max(inputs[0].size, 1), np.float64)
    capi.check(capi.lib().olap_store_eval_formula(*prog[:-1], sc, len(scalars), out.ctypes.data_as(capi._pdbl)))
    return out[: inputs[0].size]


def make_input(values, dtype, def_nan):
    s = pkg.HipStore(len(values), dtype, NAN if def_nan else 0.0)
    s.set_data_f64(values)
    return s


def random_values(rng, n, dtype, def_nan):
    vals = rng.integers(-40, 40, size=n).astype(np.float64)
    if dtype == "uint32":
        vals = np.abs(vals)
    if dtype in ("float32", "float64"):
        vals = vals * 0.25 + (rng.random(n) < 0.2) * 0.1  # some cells with a full float32 / float64 mantissa
    vals[rng.random(n) < 0.25] = 0.0
    if def_nan:
        vals[rng.random(n) < 0.25] = np.nan
    return vals


def state(s, tracked):
    return (s.get_data(), s.get_status(), s.get_data_f64(), s.keys() if tracked else None, s.order_tracked)


def check(dtype, def_nan, code, consts, inputs, scalars=(), prepare=None, tracked=False):
    """set_formula on one store, the host chain on its twin; both start from prepare(store)"""
    n = inputs[0].size
    target, twin = (pkg.HipStore(n, dtype, NAN if def_nan else 0.0) for _ in range(2))
    for s in (target, twin):
        if tracked:
            s.track_order()
        if prepare:
            prepare(s)
    cube = eval_formula(code, consts, inputs, scalars)
    twin.set_data_f64(cube)
    target.set_formula(code, consts, inputs, scalars)
    got, want = state(target, tracked), state(twin, tracked)
    what = (dtype, def_nan, n, list(code))
    for g, w, name in zip(got[:3], want[:3], ("values", "status", "get_data_f64")):
        assert same_bits(g, w), what + (name,)
    if tracked:
        assert list(got[3]) == list(want[3]), what
    assert got[4] == want[4], what
    if numpy_knows(code):
        from_numpy = evaluate(code, consts, [s.get_data_f64() for s in inputs], scalars)
        assert same_bits(cube, from_numpy), what
        assert same_bits(got[2], stored(from_numpy, dtype, def_nan)), what
    return target


MIXED = [("int32", True), ("uint32", True), ("float32", False), ("float64", True), ("int32", False), ("uint32", False), ("float32", True),
         ("float64", False)]
MIXED_PROGRAM = ([INPUT, 0, INPUT, 1, NANADD, INPUT, 2, MUL, INPUT, 3, SUB, INPUT, 4, INPUT, 5, ADD, INPUT, 6, INPUT, 7, MIN, MAX, ADD, CONST, 0, DIV], [4.0])


@pytest.fixture(scope="module")
def mixed_inputs():
    """per size: eight inputs, one of every cell type under each default (int32 / uint32 under NaN read through their mask)"""
    rng = np.random.default_rng(20240607)
    return {n: [make_input(random_values(rng, n, dt, dn), dt, dn) for dt, dn in MIXED] for n in SIZES + [ONE_TRIP + 5]}


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_types(mixed_inputs, n):
    code, consts = MIXED_PROGRAM
    for dtype in DTYPES:
        for def_nan in (False, True):
            check(dtype, def_nan, code, consts, mixed_inputs[n])


def test_past_one_trip_of_the_grid(mixed_inputs):
    code, consts = MIXED_PROGRAM
    inputs = mixed_inputs[ONE_TRIP + 5]
    check("float32", False, code, consts, inputs)  # four cells per lane: two trips and a tail
    check("int32", True, code, consts, inputs)  # the same with a mask written
    check("float64", True, [INPUT, 2, INPUT, 3, SUB], [], inputs)  # two cells per lane


def test_values_where_conversion_and_delete_on_default_show():
    special = [0.0, -0.0, NAN, 2.0 ** 31, -2.0 ** 31 - 1, 2.0 ** 32, 1e20, -1e20, 16777217.0, -16777217.0, np.inf, -np.inf, 2.0 ** 31 - 1, -2.0 ** 31,
               2.0 ** 32 - 1, 2.0 ** 32 + 1, 0.5, -0.5, 1e-46, -1e-46, 3.0e38, 3.5e38, 1.0, -1.0, 4294967295.5, -4294967295.5, 2.0 ** 53, 1e300]
    # every special value times 1, -1 and 0 (0 * -1 = -0, inf * 0 = NaN), five cells over so that the tail sees some
    a = np.array(special * 3 + special[:5], np.float64)
    b = np.array([1.0] * len(special) + [-1.0] * len(special) + [0.0] * len(special) + [1.0] * 5)
    ia, ib = make_input(a, "float64", True), make_input(b, "float64", False)
    assert ia.size % 4 == 1
    for dtype in DTYPES:
        for def_nan in (False, True):
            check(dtype, def_nan, [INPUT, 0, INPUT, 1, MUL], [], [ia, ib])
            check(dtype, def_nan, [INPUT, 0], [], [ia])
    # spot checks of what the comparison above stands on
    t = check("int32", False, [INPUT, 0], [], [ia])
    got = dict(zip(special, t.get_data_f64()[: len(special)]))
    assert got[2.0 ** 31] == -2.0 ** 31 and got[-2.0 ** 31 - 1] == 2.0 ** 31 - 1 and got[2.0 ** 32] == 0 and got[1e20] == 1661992960.0
    t = check("float32", False, [INPUT, 0], [], [ia])
    assert t.get_data_f64()[special.index(16777217.0)] == 16777216.0
    t = check("float64", False, [INPUT, 0, INPUT, 1, MUL], [], [ia, ib])
    neg_zero = len(special)  # 0 * -1
    assert t.get_status()[neg_zero] == 0 and not np.signbit(t.get_data_f64()[neg_zero])  # -0 is the 0 default: unset, stored as +0


@pytest.fixture(scope="module")
def opcode_inputs():
    rng = np.random.default_rng(7)
    n = 1025
    a = rng.normal(0, 3, n)
    b = rng.normal(0, 2, n)
    a[::7] = np.round(a[::7])
    b[::5] = np.round(b[::5])
    a[3::11] = 0.0
    b[4::13] = 0.0
    a[5::17] = np.nan
    b[6::19] = np.nan
    a[8::29] *= 0.1  # |a| < 1 for asin / acos
    c = rng.integers(-1, 2, n).astype(np.float64)
    return [make_input(a, "float64", True), make_input(b, "float64", True), make_input(c, "float32", False)]


@pytest.mark.parametrize("dtype,def_nan", [("float64", True), ("float32", False)])
def test_each_opcode_once(opcode_inputs, dtype, def_nan):
    for op in ALL_UNARY:
        check(dtype, def_nan, [INPUT, 0, op], [], opcode_inputs)
    for op in ALL_BINARY:
        check(dtype, def_nan, [INPUT, 0, INPUT, 1, op], [], opcode_inputs)
    check(dtype, def_nan, [INPUT, 2, INPUT, 0, INPUT, 1, SELECT], [], opcode_inputs)
    check(dtype, def_nan, [INPUT, 0, CONST, 1, ROUNDTO], [0.0, 2.0], opcode_inputs)
    check(dtype, def_nan, [INPUT, 0, CONST, 0, MUL, SCALAR, 1, ADD], [2.5], opcode_inputs, scalars=(0.0, -7.25))
    check(dtype, def_nan, [INPUT, 0, SIN, INPUT, 1, COS, MUL, INPUT, 0, INPUT, 1, POW, HYPOT], [], opcode_inputs)  # library routines, mixed


def deep_program(depth, n_inputs, n_scalars):
    """`depth` operands pushed (inputs and scalars in turn), then folded from the top with operations whose order matters"""
    code = []
    for j in range(depth):
        if n_scalars and j % 5 == 4:
            code += [SCALAR, (j // 5) % n_scalars]
        else:
            code += [INPUT, j % n_inputs]
    for j in range(depth - 1):
        code.append([SUB, ADD, MUL, NANADD, MAX][j % 5])
    return code


# the stack below its top lives in LDS, 8 KB (4-byte cells) or 4 KB (8-byte cells) per level and workgroup: depth 1 needs
# none, depth 7 is the last that fits 48 KB with 4-byte cells (13 with 8-byte cells), 16 is the deepest a program may get
@pytest.mark.parametrize("depth", [1, 2, 3, 7, 8, 13, 14, 15, 16])
def test_stack_depths(mixed_inputs, depth):
    inputs = mixed_inputs[1025]
    scalars = (1.5, -2.0, 0.25)
    code = deep_program(depth, 8, 3)
    check("float32", False, code, [], inputs, scalars)
    check("float64", True, code, [], inputs, scalars)
    check("uint32", True, code, [], inputs, scalars)
    if depth >= 8:  # the same depth with a library routine on top: the other instantiation
        check("float32", True, code + [CBRT], [], inputs, scalars)


def test_target_that_holds_data(mixed_inputs):
    inputs = mixed_inputs[257]
    rng = np.random.default_rng(3)
    old = rng.integers(1, 9, 257).astype(np.float64)  # every cell set: each one is overwritten or unset

    def prepare(s):
        s.set_data_f64(old)
        s.get_status()  # a lazily built mask is dropped by the bulk write, as set_data_f64 drops it

    for dtype in DTYPES:
        for def_nan in (False, True):
            check(dtype, def_nan, [INPUT, 2, INPUT, 3, MUL], [], inputs, prepare=prepare)


def test_tracked_targets(mixed_inputs):
    inputs = mixed_inputs[257]

    def out_of_order(s):  # the order leaves the flat index: a seq is attached
        for i in (200, 3, 77, 4):
            s.set_value(i, 5.0)
        assert s.order_tracked == 2

    for dtype, def_nan in (("float32", False), ("float64", True), ("int32", True)):
        lazy = check(dtype, def_nan, [INPUT, 2, INPUT, 3, SUB], [], inputs, tracked=True)
        assert lazy.order_tracked == 1  # nothing was written before: the order stays the flat index
        check(dtype, def_nan, [INPUT, 2, INPUT, 3, SUB], [], inputs, prepare=out_of_order, tracked=True)


def test_refusals_leave_the_target_untouched(mixed_inputs):
    inputs = mixed_inputs[257]
    t = pkg.HipStore(257, "float32", 0.0).track_order()
    t.set_data_f64(np.arange(257.0))
    before = state(t, True)
    other = make_input(np.ones(256), "float32", False)
    for bad, code in (([inputs[0], t], capi.ERR_INVALID_ARGUMENT), ([inputs[0], other], capi.ERR_LENGTH_MISMATCH)):
        with pytest.raises(pkg.OlapError) as ei:
            t.set_formula([INPUT, 0, INPUT, 1, ADD], [], bad)
        assert ei.value.code == code
        after = state(t, True)
        assert all(same_bits(g, w) for g, w in zip(after[:3], before[:3])) and list(after[3]) == list(before[3]) and after[4] == before[4]


def test_sharded_target():
    """two ranks on one device: one launch per shard, the scalars the same for both"""
    from olap_in_memory_amd.sharded import Comm, ShardedStore

    comm = Comm.init_all([0, 0])
    lens = [7, 5, 3]
    n = 105
    rng = np.random.default_rng(11)
    va, vb = random_values(rng, n, "float32", False), random_values(rng, n, "int32", True)
    a = ShardedStore(comm, lens, "float32", 0.0).set_data_f64(va)
    b = ShardedStore(comm, lens, "int32", NAN).set_data_f64(vb)
    wa, wb = make_input(va, "float32", False), make_input(vb, "int32", True)
    code, scalars = [INPUT, 0, INPUT, 1, NANADD, SCALAR, 0, MUL], (0.5,)
    for dtype, def_nan in (("float32", False), ("uint32", True)):
        t = ShardedStore(comm, lens, dtype, NAN if def_nan else 0.0).set_formula(code, [], [a, b], scalars)
        whole = pkg.HipStore(n, dtype, NAN if def_nan else 0.0).set_formula(code, [], [wa, wb], scalars)
        assert same_bits(t.get_data_f64(), whole.get_data_f64()) and same_bits(t.get_status(), whole.get_status())
    t = ShardedStore(comm, lens, "float32", 0.0).set_data_f64(va)
    before = (t.get_data_f64(), t.get_status())
    short = ShardedStore(comm, [7, 5], "float32", 0.0)
    for bad, code in (([a, short], capi.ERR_LENGTH_MISMATCH), ([a, t], capi.ERR_INVALID_ARGUMENT)):  # the sharded form's own refusals
        with pytest.raises(pkg.OlapError) as ei:
            t.set_formula([INPUT, 0, INPUT, 1, ADD], [], bad)
        assert ei.value.code == code
        assert same_bits(t.get_data_f64(), before[0]) and same_bits(t.get_status(), before[1])
    other = ShardedStore(comm, [5, 21], "float32", 0.0)  # as many cells, another partition
    with pytest.raises(pkg.OlapError, match="^sharded:"):
        ShardedStore(comm, lens, "float32", 0.0).set_formula([INPUT, 0], [], [other])
