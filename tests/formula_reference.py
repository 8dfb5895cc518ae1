"""What js/formula.js's evaluate() gives for the opcodes that call into a math library, written from ECMA-262 (Math.*,
Number::exponentiate, Number::remainder) and from formula.js, without a line of the device interpreter: Python floats in,
a Python float out.  Every special value is a written-out rule; a finite result of a library function is computed by
mpmath at PREC bits and rounded ONCE to the nearest double (ties to even, subnormals included), so it is the correctly
rounded value of the function, which no double-precision library is obliged to return.  `exact(op, ...)` gives the
unrounded value, `reference(op, ...)` the double, `ulps(got, exact)` the distance between a result and the truth in units
in the last place of the correctly rounded result.

tests/test_formula_reference.py pins this file to V8; tests/test_formula_ops_gpu.py compares the device with it."""
import math

import mpmath

PREC = 400
mp = mpmath.mp.clone()
mp.prec = PREC
NAN, INF = math.nan, math.inf

# opcodes (js/formula.js OP, csrc FormulaOp)
MOD, POW, ATAN2, HYPOT, ROUNDTO = 7, 8, 14, 15, 16
ROUND, CBRT, EXP, LN, LOG10, LOG2, SIN, COS, TAN, ASIN, ACOS, ATAN = 23, 26, 27, 28, 29, 30, 32, 33, 34, 35, 36, 37
UNARY_OPS = [ROUND, CBRT, EXP, LN, LOG10, LOG2, SIN, COS, TAN, ASIN, ACOS, ATAN]
BINARY_OPS = [MOD, POW, ATAN2, HYPOT, ROUNDTO]
NAMES = {MOD: "MOD", POW: "POW", ATAN2: "ATAN2", HYPOT: "HYPOT", ROUNDTO: "ROUNDTO", ROUND: "ROUND", CBRT: "CBRT", EXP: "EXP", LN: "LN",
         LOG10: "LOG10", LOG2: "LOG2", SIN: "SIN", COS: "COS", TAN: "TAN", ASIN: "ASIN", ACOS: "ACOS", ATAN: "ATAN"}


def is_nan(x):
    return x != x


def neg_zero(x):
    return x == 0 and math.copysign(1.0, x) < 0


def to_double(v):
    """an mpf (or a float) rounded to the nearest double, ties to even; gradual underflow, overflow to an infinity"""
    if isinstance(v, float):
        return v
    sign, man, exp, _bc = v._mpf_
    if man == 0:
        if v == 0:
            return 0.0
        return float(v)  # mpmath's own inf / nan
    try:
        r = float(man << exp) if exp >= 0 else man / (1 << -exp)  # int -> float and int / int round correctly
    except OverflowError:
        r = INF
    return -r if sign else r


def _signed(sign_of, v):
    """v (>= 0) with the sign of `sign_of`; a result that rounds to zero keeps the sign"""
    return -v if math.copysign(1.0, sign_of) < 0 else v


# ---------------------------------------------------------------------------------------------------- one argument
def round_exact(x):
    """Math.round (ECMA-262 21.3.2.28): the integer nearest x, ties towards +inf; -0 for x in [-0.5, -0]"""
    if is_nan(x) or math.isinf(x) or x == 0:
        return x
    if 0 < x < 0.5:
        return 0.0
    if -0.5 <= x < 0:
        return -0.0
    if abs(x) >= 2.0 ** 52:
        return x  # already an integer
    f = math.floor(x)
    return float(f + 1 if x - f >= 0.5 else f)  # x - f is exact below 2^52


def cbrt_exact(x):
    if is_nan(x) or math.isinf(x) or x == 0:
        return x
    return _signed(x, mp.cbrt(mp.mpf(abs(x))))


def exp_exact(x):
    if is_nan(x):
        return NAN
    if x == 0:
        return 1.0
    if x > 710.0:  # e^710 > 2^1024
        return INF
    if x < -746.0:  # e^-746 < 2^-1075
        return 0.0
    return mp.exp(mp.mpf(x))


def _log(fn, x):
    if is_nan(x) or x < 0:
        return NAN
    if x == 0:
        return -INF
    if x == INF:
        return INF
    if x == 1:
        return 0.0
    return fn(mp.mpf(x))


def ln_exact(x):
    return _log(mp.log, x)


def log10_exact(x):
    return _log(mp.log10, x)


def log2_exact(x):
    return _log(lambda v: mp.log(v) / mp.log(2), x)


def sin_exact(x):
    if is_nan(x) or math.isinf(x):
        return NAN
    if x == 0:
        return x
    return mp.sin(mp.mpf(x))  # mpmath reduces by pi at the precision the argument's size asks for


def cos_exact(x):
    if is_nan(x) or math.isinf(x):
        return NAN
    if x == 0:
        return 1.0
    return mp.cos(mp.mpf(x))


def tan_exact(x):
    if is_nan(x) or math.isinf(x):
        return NAN
    if x == 0:
        return x
    return mp.tan(mp.mpf(x))


def asin_exact(x):
    if is_nan(x) or abs(x) > 1:
        return NAN
    if x == 0:
        return x
    return mp.asin(mp.mpf(x))


def acos_exact(x):
    if is_nan(x) or abs(x) > 1:
        return NAN
    if x == 1:
        return 0.0
    return mp.acos(mp.mpf(x))


def atan_exact(x):
    if is_nan(x) or x == 0:
        return x
    if math.isinf(x):
        return _signed(x, mp.pi / 2)
    return mp.atan(mp.mpf(x))


# --------------------------------------------------------------------------------------------------- two arguments
def mod_exact(a, b):
    """a % b (Number::remainder): C's fmod, exact, with the sign of the dividend"""
    if is_nan(a) or is_nan(b) or math.isinf(a) or b == 0:
        return NAN
    if math.isinf(b) or a == 0:
        return a
    return math.fmod(a, b)  # a zero result carries a's sign


def _odd_integer(y):
    return abs(y) < 2.0 ** 53 and y == math.floor(y) and math.fmod(y, 2.0) != 0


def pow_exact(b, e):
    """Math.pow (Number::exponentiate, ECMA-262 6.1.6.1.3), rule by rule"""
    if is_nan(e):
        return NAN
    if e == 0:
        return 1.0
    if is_nan(b):
        return NAN
    if b == INF:
        return INF if e > 0 else 0.0
    if b == -INF:
        if e > 0:
            return -INF if _odd_integer(e) else INF
        return -0.0 if _odd_integer(e) else 0.0
    if b == 0 and not neg_zero(b):
        return 0.0 if e > 0 else INF
    if b == 0:
        if e > 0:
            return -0.0 if _odd_integer(e) else 0.0
        return -INF if _odd_integer(e) else INF
    if math.isinf(e):
        if abs(b) == 1:
            return NAN  # where C99 says 1
        return INF if (abs(b) > 1) == (e > 0) else 0.0
    if b < 0 and e != math.floor(e):
        return NAN
    negative = b < 0 and _odd_integer(e)
    if abs(b) == 1:
        return -1.0 if negative else 1.0
    size = e * math.log2(abs(b))  # the result's binary exponent, near enough to leave the representable range alone
    if size > 1030:
        v = INF
    elif size < -1080:
        v = 0.0
    else:
        v = mp.power(mp.mpf(abs(b)), mp.mpf(e))
    return -v if negative else v


def atan2_exact(y, x):
    """Math.atan2(y, x) (ECMA-262 21.3.2.8)"""
    if is_nan(y) or is_nan(x):
        return NAN
    x_neg = math.copysign(1.0, x) < 0
    if y == 0:
        return _signed(y, mp.pi) if x_neg else y  # x < 0 or -0: +-pi; x > 0 or +0: +-0
    if x == 0:
        return _signed(y, mp.pi / 2)
    if math.isinf(y):
        if math.isinf(x):
            return _signed(y, 3 * mp.pi / 4 if x_neg else mp.pi / 4)
        return _signed(y, mp.pi / 2)
    if math.isinf(x):
        return _signed(y, mp.pi) if x_neg else _signed(y, 0.0)
    return mp.atan2(mp.mpf(y), mp.mpf(x))


def hypot_exact(a, b):
    """Math.hypot of two values: an infinity beats a NaN"""
    if math.isinf(a) or math.isinf(b):
        return INF
    if is_nan(a) or is_nan(b):
        return NAN
    if a == 0 and b == 0:
        return 0.0
    with mp.workprec(2 * 53 + 2 * 1074 + 64):  # a^2 + b^2 without rounding, whatever the two magnitudes
        s = mp.mpf(a) * mp.mpf(a) + mp.mpf(b) * mp.mpf(b)
    return mp.sqrt(s)


def _mul(a, b):
    return a * b  # IEEE: Python floats overflow to an infinity and give NaN for inf * 0


def _div(a, b):
    if is_nan(a) or is_nan(b):
        return NAN
    if b == 0:
        if a == 0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)
    if math.isinf(a) and math.isinf(b):
        return NAN
    return a / b


def roundto_exact(v, digits):
    """formula.js: f = Math.pow(10, Math.trunc(digits || 0)); Math.round(v * f) / f — `||` sends NaN and both zeros to 0.
    Math.pow(10, k) is taken correctly rounded: ECMA-262 leaves its last bit open, and V8 returns that value wherever it is an integer."""
    d = 0.0 if (is_nan(digits) or digits == 0) else digits
    f = to_double(pow_exact(10.0, float(math.trunc(d)) if math.isfinite(d) else d))
    return _div(round_exact(_mul(v, f)), f)


EXACT = {ROUND: round_exact, CBRT: cbrt_exact, EXP: exp_exact, LN: ln_exact, LOG10: log10_exact, LOG2: log2_exact, SIN: sin_exact, COS: cos_exact,
         TAN: tan_exact, ASIN: asin_exact, ACOS: acos_exact, ATAN: atan_exact, MOD: mod_exact, POW: pow_exact, ATAN2: atan2_exact,
         HYPOT: hypot_exact, ROUNDTO: roundto_exact}


def exact(op, *args):
    """the unrounded value (an mpf), or a float where a rule or exact arithmetic fixes the result"""
    return EXACT[op](*(float(a) for a in args))


def reference(op, *args):
    return to_double(exact(op, *args))


def hypot_fold(*args):
    """hypot(a, b, c, ...) as the device computes it: hypot(hypot(a, b), c), every step rounded to a double"""
    r = float(args[0])
    for x in args[1:]:
        r = reference(HYPOT, r, x)
    return r


def classify(x):
    """what a result is when it is not an ordinary number: 'nan', '+inf', '-inf', '+0', '-0'; None otherwise"""
    x = to_double(x)
    if is_nan(x):
        return "nan"
    if math.isinf(x):
        return "+inf" if x > 0 else "-inf"
    if x == 0:
        return "-0" if neg_zero(x) else "+0"
    return None


def ulps(got, truth):
    """|got - truth| in units in the last place of the correctly rounded `truth` (an mpf or a float); 0 where both are the
    same non-number, infinite where only one of them is or where the two zeros differ"""
    got, want = float(got), to_double(truth)
    cg, cw = classify(got), classify(want)
    if cg == cw and cg is not None:
        return 0.0
    not_numbers = ("nan", "+inf", "-inf")
    if cg in not_numbers or cw in not_numbers or (cg is not None and cw is not None):
        return INF
    err = abs(mp.mpf(got) - (mp.mpf(truth) if isinstance(truth, float) else truth))
    return float(err / mp.mpf(math.ulp(want)))  # math.ulp(0.0) is the smallest subnormal
