"""Inputs, references, error measures and bounds of the per-operator accuracy tests of the REAL types (tests/test_operator_accuracy_host.py
on the CPU oracle, tests/test_gpu_operator_accuracy.py on the device).  A plain helper module: no fixtures, no collection hooks.

Tables.  One entry per opcode of include/de_opcodes.h (53): the true value `f` and the true partial(s) `f'` as mpmath callables at 160
bits, the partials as ANALYTIC derivatives (gamma' = gamma psi through mpmath.digamma) under the conventions of DESIGN.md §6, and, for
every partial that is not an exact row, its pointwise bound.

Inputs.  Every population is seeded (PCG64, seed = crc32 of its name), built in the working dtype and only then widened, so the
reference sees exactly the bits the kernel sees.  A region of a partial population has 1500 points (mpmath is the cost), a region of a
Float32 value population 20000 (its reference is float64 libm, whose error is below 2^-20 Float32 ulp; mpmath for gamma).  The regions
of one (operator, dtype) are concatenated so that a test needs one device call and one oracle call; references are cached per
(operator, dtype).

Error measure.  E = |got - true| / (eps |true|), eps = 2^-23 / 2^-52, the truth held as hi + lo Float64.  Values are also measured in
ulps (np.spacing of the truth rounded to the dtype).

Pointwise bound of a partial: the first-order forward error of the formula AS WRITTEN in unary_vg / binary_vg (csrc/de_grad_common.h;
oracle/de_oracle_ops.h states the same formulas),

    B(x; s) = sum over the steps of  kappa_step(x) * slack_step,

slack = 0.5 for an IEEE operation or a rounded constant, s for a library call (s = 0.5 for the oracle, which evaluates library functions
in the wider type and rounds once; the project's asserted 2 ulp Float32 / 1 ulp Float64 for the device), kappa the relative sensitivity of
the result to that step, evaluated in mpmath.  Asserted as E <= 1.01 B + 2^-9 (second-order terms; the reference's own rounding).

Kept points (conditions, not measurements): the true value and the true partial are finite and normal in the dtype and
B(x; s_device) <= 2^10.  Every region keeps >= 90 % of its points, which both test files assert; the region limits below are chosen
so: where an intermediate of the formula would overflow although the partial is representable (x*x in asinh' beyond sqrt(floatmax)) the
region ends before it, `^` draws its exponent from [-30, 30] cut to where the power stays representable, tanh' ends at 3.5 (at 8 half
the points would have B > 2^10), the root of psi is approached to 0.1 (Float64: 0.2; the digamma bound grows as 1 / |psi|)."""
import functools
import zlib
from collections import namedtuple
from fractions import Fraction

import numpy as np

import dynamicexpressions_jl_amd as de
from dynamicexpressions_jl_amd.operators import _B, _T, _U

DTYPES = (np.float32, np.float64)
NPTS = 1500          # points per region of a partial population
NVAL = 20000         # points per region of a Float32 value population
MP_PREC = 160
MIN_KEPT = 0.90
B_MAX = 2.0 ** 10
SECOND_ORDER = 1.01
REF_ROUNDING = 2.0 ** -9
S_ORACLE = 0.5
S_DEVICE = {np.float32: 2.0, np.float64: 1.0}   # tests/test_gpu_ops.py; tests/test_gpu_ulp_f64.py
PSI_ROOT = 1.4616321449683623

UNARY, BINARY, TERNARY = tuple(_U), tuple(_B), tuple(_T)
OPS = [(n, 1) for n in UNARY] + [(n, 2) for n in BINARY] + [(n, 3) for n in TERNARY]   # the 53 opcodes
SAFE_OF = {"safe_log": "log", "safe_log2": "log2", "safe_log10": "log10", "safe_log1p": "log1p", "safe_sqrt": "sqrt", "safe_acosh": "acosh"}
# partials that are exact rows (EXACT_PARTIALS below writes them out); every other operator has mpmath partials and bounds
EXACT = {("neg", 1), ("abs", 1), ("square", 1), ("relu", 1), ("sign", 1), ("round", 1), ("floor", 1), ("ceil", 1), ("+", 2), ("-", 2),
         ("*", 2), ("max", 2), ("min", 2), ("mod", 2), ("rem", 2), ("greater", 2), ("fma", 3), ("clamp", 3), ("+", 3), ("max", 3)}
BOUNDED = [k for k in OPS if k not in EXACT]


def eps_of(R):
    return float(np.finfo(R).eps)


def key_name(key):
    return f"{key[0]}({key[1]})"


def _rng(*key):
    return np.random.Generator(np.random.PCG64(zlib.crc32("/".join(str(k) for k in key).encode())))


# ---- tables: true values and true partials (mpmath) ----------------------------------------------------------------------------------
def _mp_tables():
    import mpmath as mp
    one, zero, nan = mp.mpf(1), mp.mpf(0), mp.nan
    ln2, ln10 = mp.log(2), mp.log(10)

    def jl_mod(x, y):
        r = x - y * mp.floor(x / y)
        return r

    def sign(x):
        return mp.sign(x)

    f = {
        ("neg", 1): lambda x: -x, ("abs", 1): abs, ("square", 1): lambda x: x * x, ("cube", 1): lambda x: x * x * x,
        ("relu", 1): lambda x: zero if x < 0 else x, ("sign", 1): sign, ("round", 1): mp.nint,  # half to even
        ("floor", 1): mp.floor, ("ceil", 1): mp.ceil, ("inv", 1): lambda x: one / x, ("sqrt", 1): mp.sqrt, ("cbrt", 1): lambda x: sign(x) * mp.cbrt(abs(x)),
        ("exp", 1): mp.exp, ("exp2", 1): lambda x: mp.power(2, x), ("log", 1): mp.log, ("log2", 1): lambda x: mp.log(x) / ln2,
        ("log10", 1): lambda x: mp.log(x) / ln10, ("log1p", 1): mp.log1p, ("sin", 1): mp.sin, ("cos", 1): mp.cos, ("tan", 1): mp.tan,
        ("sinh", 1): mp.sinh, ("cosh", 1): mp.cosh, ("tanh", 1): mp.tanh, ("asin", 1): mp.asin, ("acos", 1): mp.acos, ("atan", 1): mp.atan,
        ("asinh", 1): mp.asinh, ("acosh", 1): mp.acosh, ("atanh", 1): mp.atanh,
        ("custom_cos", 1): lambda x: mp.cos(x) ** 2, ("gamma", 1): mp.gamma,
        ("+", 2): lambda x, y: x + y, ("-", 2): lambda x, y: x - y, ("*", 2): lambda x, y: x * y, ("/", 2): lambda x, y: x / y,
        ("^", 2): lambda x, y: mp.power(x, y), ("max", 2): max, ("min", 2): min, ("mod", 2): jl_mod,
        ("rem", 2): lambda x, y: x - y * (mp.floor(x / y) if x / y >= 0 else mp.ceil(x / y)), ("greater", 2): lambda x, y: one if x > y else zero,
        ("pow_abs2", 2): lambda x, y: mp.power(abs(x), y),
        ("fma", 3): lambda x, y, z: x * y + z, ("clamp", 3): lambda x, lo, hi: hi if x > hi else (lo if x < lo else x),
        ("+", 3): lambda x, y, z: x + y + z, ("max", 3): lambda x, y, z: max(x, y, z),
    }
    # partials, DESIGN.md §6: a tuple per operator, one entry per argument
    d = {
        ("neg", 1): lambda x: (-one,), ("abs", 1): lambda x: (sign(x),), ("square", 1): lambda x: (2 * x,), ("cube", 1): lambda x: (3 * x * x,),
        ("relu", 1): lambda x: (zero if x < 0 else one,), ("sign", 1): lambda x: (zero,), ("round", 1): lambda x: (zero,),
        ("floor", 1): lambda x: (zero,), ("ceil", 1): lambda x: (zero,),
        ("inv", 1): lambda x: (-one / (x * x),), ("sqrt", 1): lambda x: (one / (2 * mp.sqrt(x)),),
        ("cbrt", 1): lambda x: (one / (3 * mp.cbrt(abs(x)) ** 2),), ("exp", 1): lambda x: (mp.exp(x),), ("exp2", 1): lambda x: (mp.power(2, x) * ln2,),
        ("log", 1): lambda x: (one / x,), ("log2", 1): lambda x: (one / (x * ln2),), ("log10", 1): lambda x: (one / (x * ln10),),
        ("log1p", 1): lambda x: (one / (one + x),), ("sin", 1): lambda x: (mp.cos(x),), ("cos", 1): lambda x: (-mp.sin(x),),
        ("tan", 1): lambda x: (one / mp.cos(x) ** 2,), ("sinh", 1): lambda x: (mp.cosh(x),), ("cosh", 1): lambda x: (mp.sinh(x),),
        ("tanh", 1): lambda x: (one / mp.cosh(x) ** 2,), ("asin", 1): lambda x: (one / mp.sqrt(one - x * x),),
        ("acos", 1): lambda x: (-one / mp.sqrt(one - x * x),), ("atan", 1): lambda x: (one / (one + x * x),),
        ("asinh", 1): lambda x: (one / mp.sqrt(x * x + one),), ("acosh", 1): lambda x: (one / mp.sqrt((x - one) * (x + one)),),
        ("atanh", 1): lambda x: (one / ((one - x) * (one + x)),),
        ("custom_cos", 1): lambda x: (-mp.sin(2 * x),), ("gamma", 1): lambda x: (mp.gamma(x) * mp.digamma(x),),
        ("+", 2): lambda x, y: (one, one), ("-", 2): lambda x, y: (one, -one), ("*", 2): lambda x, y: (y, x),
        ("/", 2): lambda x, y: (one / y, -x / (y * y)),
        ("^", 2): lambda x, y: (y * mp.power(x, y - 1), mp.power(x, y) * mp.log(abs(x))),
        ("max", 2): lambda x, y: (one, zero) if x > y else (zero, one), ("min", 2): lambda x, y: (zero, one) if x > y else (one, zero),
        ("mod", 2): lambda x, y: (nan, nan) if x / y == mp.floor(x / y) else (one, -mp.floor(x / y)),
        ("rem", 2): lambda x, y: (nan, nan) if x / y == mp.floor(x / y) else (one, -(mp.floor(x / y) if x / y >= 0 else mp.ceil(x / y))),
        ("greater", 2): lambda x, y: (zero, zero),
        ("pow_abs2", 2): lambda x, y: (y * mp.power(abs(x), y) / x, mp.power(abs(x), y) * mp.log(abs(x))),
        ("fma", 3): lambda x, y, z: (y, x, one),
        ("clamp", 3): lambda x, lo, hi: (zero, zero, one) if x > hi else ((zero, one, zero) if x < lo else (one, zero, zero)),
        ("+", 3): lambda x, y, z: (one, one, one),
        ("max", 3): lambda x, y, z: (zero, zero, one) if not max(x, y) > z else ((one, zero, zero) if x > y else (zero, one, zero)),
    }
    for safe, base in SAFE_OF.items():   # inside the domain the base operator; outside NaN with an exact zero partial (§6)
        edge, strict = {"log": (0, False), "log2": (0, False), "log10": (0, False), "log1p": (-1, False), "sqrt": (0, True), "acosh": (1, True)}[base]
        out = (lambda e, st: (lambda x: x < e if st else x <= e))(edge, strict)
        f[(safe, 1)] = (lambda o, g: lambda x: nan if o(x) else g(x))(out, f[(base, 1)])
        d[(safe, 1)] = (lambda o, g: lambda x: (zero,) if o(x) else g(x))(out, d[(base, 1)])
    return f, d


def digamma_error(x, s, unit=1.0):
    """The error of digamma AS WRITTEN (csrc/de_device_ops.h dev_digamma, oracle/de_oracle_ops.h o_digamma) at x, absolute, in units of
    eps of the working type: (rounding part, first omitted series term).  Rounding part: every rounding is at most half an ulp of a
    quantity no larger than S, the sum of the magnitudes of the terms (pi cot(pi x) of the reflection, the 1 / (x + k) of the recurrence
    to X >= 10, log X, 1 / 2X, the series), so R roundings give 0.5 R S: three per recurrence step (x + 1, 1 / x, the subtraction), four
    at the end (1 / 2X and three additions; the series' own roundings are below 2^-9 of the total), four in the reflection.  On top: log's slack
    times |log X|, and for the reflection tan's slack plus the conditioning kappa = |pi x / (sin cos)| of tan on its argument, which
    carries two roundings (pi, the product), times |pi cot|.  `unit`: eps of the type the algorithm runs in over eps of the working type
    (1 on the device; the oracle runs it in the wider type).  The omitted term is B_12 / (12 X^12) = 691 / 32760 X^-12, in absolute units."""
    import mpmath as mp
    S, extra, R = mp.mpf(0), mp.mpf(0), 0
    if x <= 0:
        t = mp.pi * x
        C = abs(mp.pi / mp.tan(t))
        extra += C * (s + abs(t / (mp.sin(t) * mp.cos(t))))
        S += C
        R += 4
        x = 1 - x
    n = 0
    while x < 10:
        S += 1 / x
        x += 1
        n += 1
    R += 3 * n + 4
    series = (1 / (12 * x ** 2)) + 1 / (120 * x ** 4)
    S += abs(mp.log(x)) + 0.5 / x + series
    extra += s * abs(mp.log(x))
    return (0.5 * R * S + extra) * unit, mp.mpf(691) / 32760 / x ** 12


def _bounds(R, s, unit):
    """op -> callable(args) -> tuple of B per partial, for slack s (derivations: the module docstring and the comments here)."""
    import mpmath as mp
    eps = mp.mpf(eps_of(R))

    def near_one(x):   # x^2 / (1 - x^2): how the rounding of x*x reaches 1 - x*x
        return x * x / ((1 - x) * (1 + x))

    def gamma_b(x):
        rounding, omitted = digamma_error(x, s, unit)
        return s + 0.5 + (rounding + omitted / eps) / abs(mp.digamma(x))

    def pow_abs2_b(x, y):
        v = s + abs(y * mp.log(abs(x))) * (s + 0.5)   # exp's slack + |m| x (log's slack + the product's rounding)
        return (v + 1.5, v + s + 0.5)                 # (v y)(1/a) sign: three roundings; v l: log's slack + one

    b = {
        "cube": lambda x: (1.0,),                            # (3 x) x
        "inv": lambda x: (1.5,),                             # y = 1 / x, y y
        "sqrt": lambda x: (1.0,),                            # 1 / (2 sqrt x)
        "cbrt": lambda x: (2 * s + 1.5,),                    # 1 / (3 (y y))
        "exp": lambda x: (s,), "exp2": lambda x: (s + 1.0,),   # y LN2
        "log": lambda x: (0.5,), "log2": lambda x: (1.5,), "log10": lambda x: (1.5,),   # (1 / x) / LN
        "log1p": lambda x: (1.0,),                           # 1 / (x + 1)
        "sin": lambda x: (s,), "cos": lambda x: (s,), "sinh": lambda x: (s,), "cosh": lambda x: (s,),
        "tan": lambda x: ((2 * s + 0.5) * mp.sin(x) ** 2 + 0.5,),     # 1 + y y: kappa = y^2 / (1 + y^2)
        "tanh": lambda x: ((2 * s + 0.5) * mp.sinh(x) ** 2 + 0.5,),   # 1 - y y: kappa = y^2 / (1 - y^2)
        "asin": lambda x: (0.5 * (0.5 * near_one(x) + 0.5) + 1.0,),   # 1 / sqrt(1 - x x)
        "acos": lambda x: (0.5 * (0.5 * near_one(x) + 0.5) + 1.0,),
        "atan": lambda x: (0.5 * x * x / (1 + x * x) + 1.0,),         # 1 / (1 + x x)
        "asinh": lambda x: (0.5 * (0.5 * x * x / (1 + x * x) + 0.5) + 1.0,),   # 1 / sqrt(x x + 1)
        "acosh": lambda x: (2.5,),                           # 1 / (sqrt(x - 1) sqrt(x + 1))
        "atanh": lambda x: (0.5 * near_one(x) + 1.0,),       # 1 / (1 - x x)
        "custom_cos": lambda x: (2 * s + 0.5,),              # (2 c)(-s)
        "gamma": lambda x: (gamma_b(x),),
        "/": lambda x, y: (0.5, 1.0),                        # 1 / y; -((x / y) / y)
        "^": lambda x, y: (s + 1.0, 2 * s + 0.5),            # (v y) / x; v log|x|
        "pow_abs2": pow_abs2_b,
    }
    for safe, base in SAFE_OF.items():
        b[safe] = b[base]
    return b


# ---- input regions --------------------------------------------------------------------------------------------------------------------
def _sgn(g, n):
    return g.choice([-1.0, 1.0], n)


def _logu(g, n, lo, hi, signed=False):
    x = 10.0 ** g.uniform(np.log10(lo), np.log10(hi), n)
    return x * _sgn(g, n) if signed else x


def _regions(key, R):
    """name -> (sampler(rng, n) -> tuple of Float64 arrays, used for partials?).  Value populations use every region."""
    fi = np.finfo(R)
    tiny, fmax, eps = float(fi.tiny), float(fi.max), float(fi.eps)
    lmax = np.log(fmax)
    op, deg = key
    op = SAFE_OF.get(op, op) if deg == 1 else op
    U = lambda f: (lambda g, n: (f(g, n),))
    ordinary = U(lambda g, n: _logu(g, n, 1e-3, 10, True))
    positive = U(lambda g, n: _logu(g, n, 1e-3, 10))
    wide = U(lambda g, n: _logu(g, n, 4 * tiny, fmax / 8, True))
    wide_pos = U(lambda g, n: _logu(g, n, 4 * tiny, fmax / 8))
    small = U(lambda g, n: _logu(g, n, 4 * tiny, 1e-3, True))
    if deg == 1:
        if op in ("neg", "abs", "relu", "sign", "cbrt"):
            return {"ordinary": (ordinary, True), "wide": (wide, True)}
        if op in ("round", "floor", "ceil"):
            return {"ordinary": (ordinary, True), "halves": (U(lambda g, n: g.integers(-1000, 1000, n) + g.choice([0.0, 0.5, 0.25], n)), True),
                    "wide": (wide, True)}
        if op == "square":
            return {"ordinary": (ordinary, True), "wide": (U(lambda g, n: _logu(g, n, 2 * np.sqrt(tiny), np.sqrt(fmax) / 2, True)), True)}
        if op == "cube":
            return {"ordinary": (ordinary, True), "wide": (U(lambda g, n: _logu(g, n, 2 * tiny ** (1 / 3), fmax ** (1 / 3) / 2, True)), True)}
        if op == "inv":   # y y = 1 / x^2 stays normal
            return {"ordinary": (ordinary, True), "wide": (U(lambda g, n: _logu(g, n, 2 / np.sqrt(fmax), 0.5 / np.sqrt(tiny), True)), True),
                    "whole": (wide, False)}
        if op == "sqrt":
            return {"ordinary": (positive, True), "wide": (wide_pos, True)}
        if op in ("exp", "exp2"):
            top, bot = (lmax - 1, np.log(tiny) + 1) if op == "exp" else (np.log2(fmax) - 1, np.log2(tiny) + 1)
            return {"ordinary": (ordinary, True), "wide": (U(lambda g, n: g.uniform(bot, top, n)), True), "small": (small, True)}
        if op in ("log", "log2", "log10"):
            return {"ordinary": (positive, True), "wide": (wide_pos, True),
                    "near1": (U(lambda g, n: 1 + _sgn(g, n) * _logu(g, n, eps, 0.4)), True)}
        if op == "log1p":
            return {"ordinary": (positive, True), "wide": (U(lambda g, n: _logu(g, n, 1e-3, fmax / 8)), True), "small": (small, True),
                    "near-1": (U(lambda g, n: -1 + _logu(g, n, 8 * eps, 0.5)), True)}
        if op in ("sin", "cos", "custom_cos"):
            return {"ordinary": (ordinary, True), "big": (U(lambda g, n: g.uniform(-1e4, 1e4, n)), True), "wide": (wide, True)}
        if op == "tan":
            return {"ordinary": (ordinary, True), "wide": (wide, True), "small": (small, True),
                    "poles": (U(lambda g, n: (g.integers(-5, 5, n) + 0.5) * np.pi + _sgn(g, n) * _logu(g, n, 1e-6, 0.1)), True)}
        if op in ("sinh", "cosh"):
            return {"ordinary": (ordinary, True), "wide": (U(lambda g, n: g.uniform(-(lmax - 1), lmax - 1, n)), True), "small": (small, True)}
        if op == "tanh":
            return {"ordinary": (U(lambda g, n: _logu(g, n, 1e-3, 3.0, True)), True), "to3.5": (U(lambda g, n: g.uniform(-3.5, 3.5, n)), True),
                    "small": (small, True), "wide": (wide, False)}
        if op in ("asin", "acos", "atanh"):
            return {"ordinary": (U(lambda g, n: g.uniform(-0.99, 0.99, n)), True),
                    "to1": (U(lambda g, n: _sgn(g, n) * (1 - _logu(g, n, 10 ** -3.5, 0.1))), True), "small": (small, True),
                    "to1_fine": (U(lambda g, n: _sgn(g, n) * (1 - _logu(g, n, 2 * eps, 1e-3))), False)}
        if op in ("atan", "asinh"):   # x x stays finite
            return {"ordinary": (ordinary, True), "wide": (U(lambda g, n: _logu(g, n, 4 * tiny, np.sqrt(fmax) / 4, True)), True), "small": (small, True),
                    "whole": (wide, False)}
        if op == "acosh":
            return {"ordinary": (U(lambda g, n: 1 + _logu(g, n, 1e-3, 10)), True), "near1": (U(lambda g, n: 1 + _logu(g, n, 4 * eps, 0.1)), True),
                    "wide": (U(lambda g, n: _logu(g, n, 2.0, fmax / 8)), True)}
        if op == "gamma":
            top = 34.0 if R == np.float32 else 170.0
            root_lo = 0.1 if R == np.float32 else 0.2   # Float64: the omitted series term, 95 eps at X = 10, is as large as the roundings

            def poles(lo, hi, kmax):
                return U(lambda g, n: -g.integers(0, kmax + 1, n) + _sgn(g, n) * _logu(g, n, lo, hi))
            return {"positive": (U(lambda g, n: g.uniform(0.05, 30, n)), True), "negative": (U(lambda g, n: -g.integers(0, 6, n) - g.uniform(0.1, 0.9, n)), True),
                    "poles": (poles(10 ** -1.7, 0.4, 5), True), "root": (U(lambda g, n: PSI_ROOT + _sgn(g, n) * _logu(g, n, root_lo, 10 ** -0.4)), True),
                    "top": (U(lambda g, n: g.uniform(30, top, n)), True), "poles_fine": (poles(2.0 ** -8, 10 ** -1.7, 11), False)}
        raise KeyError(key)
    if deg == 2:
        d = np.floor(np.log10(fmax) / 4.2)   # x / y^2 stays normal
        pair = lambda g, n: (_logu(g, n, 1e-3, 10, True), _logu(g, n, 1e-3, 10, True))
        wide2 = lambda g, n: (_logu(g, n, 10.0 ** -d, 10.0 ** d, True), _logu(g, n, 10.0 ** -d, 10.0 ** d, True))
        if op in ("+", "-"):
            def cancelling(g, n):
                x, y = pair(g, n)
                return x, (-x if op == "+" else x) * g.uniform(0.5, 2, n)
            return {"ordinary": (pair, True), "wide": (wide2, True), "cancelling": (cancelling, True)}
        if op in ("*", "/", "max", "min", "greater"):
            out = {"ordinary": (pair, True), "wide": (wide2, True)}
            if op in ("max", "min", "greater"):
                out["ties"] = (lambda g, n: (lambda x: (x, np.where(g.integers(0, 2, n) == 0, x, -x)))(_logu(g, n, 1e-3, 10, True)), True)
            return out
        if op in ("^", "pow_abs2"):
            lim = 0.9 * np.log10(fmax) - 3.5   # |y log10 x| <= lim: the power, and the power times y / x, stay representable
            signed = op == "pow_abs2"

            def wide_base(g, n):
                x = _logu(g, n, 1e-3, 1e3, signed)
                cap = np.minimum(30.0, lim / np.maximum(np.abs(np.log10(np.abs(x))), 1e-9))
                return x, g.uniform(-1, 1, n) * cap

            def near_base(g, n):
                return g.uniform(0.5, 2, n) * (_sgn(g, n) if signed else 1.0), g.uniform(-30, 30, n)
            return {"base_1e-3_1e3": (wide_base, True), "base_0.5_2": (near_base, True)}
        if op in ("mod", "rem"):
            def away(g, n):     # quotients k + U(0.25, 0.75), |k| <= 200: further than 2^-10 relative from an integer
                y = _logu(g, n, 1e-2, 1e3, True)
                return (g.integers(-200, 200, n) + g.uniform(0.25, 0.75, n)) * y, y

            def integer(g, n):  # exact integer quotients: y = m 2^j with a short m, x = k y
                y = g.integers(1, 64, n) * 2.0 ** g.integers(-6, 6, n) * _sgn(g, n)
                return g.integers(-200, 200, n) * y, y
            return {"away": (away, True), "integer": (integer, True)}
    if deg == 3:
        def triple(g, n):
            return tuple(_logu(g, n, 1e-3, 10, True) for _ in range(3))

        def cancel(g, n):       # fma: z next to -x y exposes a double rounding
            x, y, _ = triple(g, n)
            return x, y, -(x * y) * (1 + g.uniform(-8, 8, n) * eps)

        def ordered(g, n):      # clamp: lo <= hi, x below, between and above
            lo = _logu(g, n, 1e-3, 10, True)
            hi = lo + _logu(g, n, 1e-3, 10)
            return lo + (hi - lo) * g.uniform(-1, 2, n), lo, hi
        out = {"ordinary": (triple, True)}
        if op == "fma":
            out["cancelling"] = (cancel, True)
        if op == "clamp":
            out["ordered"] = (ordered, True)
        return out
    raise KeyError(key)


# ---- references -----------------------------------------------------------------------------------------------------------------------
HiLo = namedtuple("HiLo", "hi lo")
PartialPop = namedtuple("PartialPop", "key dtype args regions value partials b_dev b_orc keep")
ValuePop = namedtuple("ValuePop", "key args regions truth amp")


def _hilo(vals):
    import mpmath as mp
    hi = np.array([float(v) for v in vals])
    lo = np.array([float(v - mp.mpf(h)) if np.isfinite(h) else 0.0 for v, h in zip(vals, hi)])
    return HiLo(hi, lo)


def _build_args(key, R, n, only_partial, tag):
    names, chunks = [], []
    for name, (sampler, for_partials) in _regions(key, R).items():
        if only_partial and not for_partials:
            continue
        with np.errstate(over="raise"):
            cols = tuple(np.asarray(c, dtype=np.float64).astype(R) for c in sampler(_rng(tag, key_name(key), name, np.dtype(R).name), n))
        names.append(name)
        chunks.append(cols)
    regions, at = [], 0
    for name, ch in zip(names, chunks):
        regions.append((name, slice(at, at + len(ch[0]))))
        at += len(ch[0])
    args = tuple(np.concatenate([ch[k] for ch in chunks]) for k in range(key[1]))
    for a in args:
        a.setflags(write=False)
    return args, regions


def _normal(v, R):
    fi = np.finfo(R)
    a = np.abs(v)
    return np.isfinite(v) & (a >= float(fi.tiny)) & (a <= float(fi.max))


@functools.lru_cache(maxsize=None)
def _partial_population(key, dtype_name):
    import mpmath as mp
    R = np.dtype(dtype_name).type
    args, regions = _build_args(key, R, NPTS, True, "partial")
    n, deg = len(args[0]), key[1]
    f, d = _mp_tables()
    fk, dk = f[key], d[key]
    s_dev = S_DEVICE[R]
    unit = 2.0 ** -29 if R == np.float32 else 2.0 ** -11   # the oracle's wider type: double / x87 long double
    bd, bo = _bounds(R, s_dev, 1.0)[key[0]], _bounds(R, S_ORACLE, unit)[key[0]]
    vals, parts, b_dev, b_orc = [], [[] for _ in range(deg)], [[] for _ in range(deg)], [[] for _ in range(deg)]
    with mp.workprec(MP_PREC):
        cols = [[mp.mpf(float(v)) for v in a] for a in args]
        for i in range(n):
            x = [c[i] for c in cols]
            try:
                v, p, b1, b2 = fk(*x), dk(*x), bd(*x), bo(*x)
            except (ZeroDivisionError, ValueError):   # a pole, a point outside the domain: not kept
                v, p, b1, b2 = mp.nan, (mp.nan,) * deg, (mp.inf,) * deg, (mp.inf,) * deg
            vals.append(mp.mpf(v.real) if isinstance(v, mp.mpc) else v)
            for k in range(deg):
                parts[k].append(p[k])
                b_dev[k].append(float(b1[k]))
                b_orc[k].append(float(b2[k]))
    value = _hilo(vals)
    partials = tuple(_hilo(p) for p in parts)
    b_dev = tuple(np.array(b) for b in b_dev)
    b_orc = tuple(np.array(b) for b in b_orc)
    keep = tuple(_normal(value.hi, R) & _normal(p.hi, R) & (bb <= B_MAX) for p, bb in zip(partials, b_dev))
    return PartialPop(key, R, args, regions, value, partials, b_dev, b_orc, keep)


def partial_population(key, dtype):
    """The cached population of a BOUNDED operator: inputs, regions, true value and partials (hi + lo), B(x; s_device) and B(x; 0.5) per
    partial, and the kept mask per partial."""
    return _partial_population(key, np.dtype(dtype).name)


def partial_error(got, truth, R):
    """E = |got - true| / (eps |true|) per point (+inf where got is not finite)."""
    g = np.asarray(got, dtype=np.float64)
    with np.errstate(all="ignore"):
        e = np.abs((g - truth.hi) - truth.lo) / (eps_of(R) * np.abs(truth.hi))
    return np.where(np.isfinite(g), e, np.inf)


def partial_maxima(pop, k, got, bound):
    """Per region of partial k: kept share, max E, max B, worst E / (1.01 B + 2^-9) and where."""
    e = partial_error(got, pop.partials[k], pop.dtype)
    lim = SECOND_ORDER * bound + REF_ROUNDING
    out = {}
    for name, sl in pop.regions:
        keep = pop.keep[k][sl]
        ratio = np.where(keep, e[sl] / lim[sl], -1.0)
        i = int(np.argmax(ratio))
        out[name] = dict(kept=float(keep.mean()), max_E=float(np.where(keep, e[sl], -1.0).max()), max_B=float(np.where(keep, bound[sl], -1.0).max()),
                         worst_ratio=float(ratio[i]), E_at_worst=float(e[sl][i]), B_at_worst=float(bound[sl][i]), at=[float(a[sl][i]) for a in pop.args])
    return out


# ---- Float32 values -------------------------------------------------------------------------------------------------------------------
VALUE_EXACT = {("neg", 1), ("abs", 1), ("relu", 1), ("sign", 1), ("round", 1), ("floor", 1), ("ceil", 1), ("max", 2), ("min", 2), ("rem", 2),
               ("greater", 2), ("clamp", 3), ("max", 3)}
VALUE_ROUNDED = {("square", 1), ("inv", 1), ("sqrt", 1), ("safe_sqrt", 1), ("+", 2), ("-", 2), ("*", 2), ("/", 2), ("mod", 2), ("fma", 3)}
# composite operators, bounded in E (relative, in eps) for a library slack s: cube = (x x) x: two roundings; custom_cos = c c: twice the
# cosine's s and one rounding; pow_abs2 pointwise: exp's s + |y log|x|| (log's s + the product's 0.5).  (x + y) + z: bit-exact against
# the same two additions.
VALUE_COMPOSITE = {("cube", 1): lambda s: 1.0, ("custom_cos", 1): lambda s: 2 * s + 0.5}
LIBRARY_ULP = 2.0   # DESIGN.md §5, tests/test_gpu_ops.py: the project's asserted figure for the Float32 library functions


def _f64_value(key, args):
    """The Float64 (libm / exact) value of the operator on Float32 arguments widened to Float64."""
    op, deg = key
    a = [np.asarray(v, dtype=np.float64) for v in args]
    x = a[0]
    with np.errstate(all="ignore"):
        if deg == 1:
            op = SAFE_OF.get(op, op)
            if op == "gamma":
                import mpmath as mp
                with mp.workprec(80):
                    return np.array([float(mp.gamma(mp.mpf(float(v)))) for v in x])
            table = {"neg": lambda: -x, "abs": lambda: np.abs(x), "square": lambda: x * x, "cube": lambda: x * x * x, "relu": lambda: np.where(x < 0, 0.0, x),
                     "sign": lambda: np.sign(x), "round": lambda: np.rint(x), "floor": lambda: np.floor(x), "ceil": lambda: np.ceil(x),
                     "inv": lambda: 1 / x, "sqrt": lambda: np.sqrt(x), "cbrt": lambda: np.cbrt(x), "exp": lambda: np.exp(x), "exp2": lambda: np.exp2(x),
                     "log": lambda: np.log(x), "log2": lambda: np.log2(x), "log10": lambda: np.log10(x), "log1p": lambda: np.log1p(x),
                     "sin": lambda: np.sin(x), "cos": lambda: np.cos(x), "tan": lambda: np.tan(x), "sinh": lambda: np.sinh(x), "cosh": lambda: np.cosh(x),
                     "tanh": lambda: np.tanh(x), "asin": lambda: np.arcsin(x), "acos": lambda: np.arccos(x), "atan": lambda: np.arctan(x),
                     "asinh": lambda: np.arcsinh(x), "acosh": lambda: np.arccosh(x), "atanh": lambda: np.arctanh(x), "custom_cos": lambda: np.cos(x) ** 2}
            return table[op]()
        if deg == 2:
            y = a[1]
            table = {"+": lambda: x + y, "-": lambda: x - y, "*": lambda: x * y, "/": lambda: x / y, "^": lambda: np.power(x, y), "max": lambda: np.maximum(x, y),
                     "min": lambda: np.minimum(x, y), "rem": lambda: np.fmod(x, y), "greater": lambda: (x > y).astype(np.float64),
                     "mod": lambda: (lambda r: np.where(r == 0, np.copysign(r, y), np.where((r > 0) != (y > 0), r + y, r)))(np.fmod(x, y)),
                     "pow_abs2": lambda: np.power(np.abs(x), y)}
            return table[op]()   # (the sums, products and quotients of two Float32 values, fmod and mod are exact or correctly rounded in Float64)
        y, z = a[1], a[2]
        if op == "fma":
            return np.array([float(Fraction(float(p)) * Fraction(float(q)) + Fraction(float(r))) for p, q, r in zip(x, y, z)])
        if op == "clamp":
            return np.where(x > z, z, np.where(x < y, y, x))
        if op == "+":
            return ((args[0] + args[1]) + args[2]).astype(np.float64)   # both additions rounded to Float32 as the operator's definition does
        return np.maximum(np.maximum(x, y), z)


@functools.lru_cache(maxsize=None)
def value_population(key):
    """The cached Float32 value population of an operator: inputs, regions, the Float64 truth (amp: |y log|x|| of pow_abs2)."""
    args, regions = _build_args(key, np.float32, 2000 if key == ("gamma", 1) or key == ("fma", 3) else NVAL, False, "value")
    truth = _f64_value(key, args)
    amp = None
    if key == ("pow_abs2", 2):
        with np.errstate(all="ignore"):
            amp = np.abs(args[1].astype(np.float64) * np.log(np.abs(args[0].astype(np.float64))))
    return ValuePop(key, args, regions, truth, amp)


def value_bound(pop, s):
    """The bound per point for a library slack of s ulp: 0 exact, 0.5 correctly rounded, s library (in ulp: np.spacing of the truth rounded
    to Float32); the composites in E."""
    n, key = len(pop.truth), pop.key
    if key in VALUE_EXACT or key == ("+", 3):
        return np.zeros(n)
    if key in VALUE_ROUNDED:
        return np.full(n, 0.5)
    if key in VALUE_COMPOSITE:
        return np.full(n, VALUE_COMPOSITE[key](s))
    if key == ("pow_abs2", 2):
        return s + pop.amp * (s + 0.5)
    return np.full(n, float(s))


def value_in_E(key):
    return key in VALUE_COMPOSITE or key == ("pow_abs2", 2)


def value_maxima(pop, got, s=LIBRARY_ULP):
    """Per region: kept share, max error in ulp and in E over the normal truths, max error in subnormal steps over the truths below
    floatmin, and whether every point is within its bound (0: bit-exact; subnormal truths: 1.5 steps)."""
    fi = np.finfo(np.float32)
    t = pop.truth
    g = got.astype(np.float64)
    with np.errstate(all="ignore"):
        t32 = t.astype(np.float32)
        fin = np.isfinite(t) & np.isfinite(t32)
        normal = fin & (np.abs(t) >= float(fi.tiny))
        sub = fin & ~normal
        err = np.abs(g - t)
        ulp = err / np.spacing(np.abs(t32)).astype(np.float64)
        E = err / (eps_of(np.float32) * np.abs(t))
        steps = err / float(fi.smallest_subnormal)
    measure = E if value_in_E(pop.key) else ulp
    bound = value_bound(pop, s)
    lim = np.where(bound > 0, bound + REF_ROUNDING, 0.0)
    bad = (normal & ~(np.isfinite(g) & (measure <= lim))) | (sub & ~(np.isfinite(g) & (steps <= 1.5)))
    if pop.key in VALUE_EXACT or pop.key == ("+", 3):   # exact rows: the bits, signed zeros included
        bad |= fin & (got.view(np.uint32) != t32.view(np.uint32))
    out = {}
    for name, sl in pop.regions:
        m = np.where(normal[sl] & np.isfinite(g[sl]), measure[sl], np.where(normal[sl], np.inf, -1.0))
        i = int(np.argmax(m))
        out[name] = dict(kept=float(fin[sl].mean()), max_ulp=float(np.where(normal[sl], ulp[sl], 0.0).max()), max_E=float(np.where(normal[sl], E[sl], 0.0).max()),
                         max_subnormal_steps=float(np.where(sub[sl], steps[sl], 0.0).max()), bound=float(bound[sl][i]), worst=float(m[i]),
                         at=[float(a[sl][i]) for a in pop.args], bad=int(bad[sl].sum()),
                         first_bad=[float(a[sl][np.argmax(bad[sl])]) for a in pop.args] if bad[sl].any() else None)
    return out


# ---- exact rows -----------------------------------------------------------------------------------------------------------------------
def exact_partials(key, args):
    """The partials of an EXACT operator on `args` (arrays of the working dtype), written out from DESIGN.md §6: a tuple of arrays of
    that dtype.  mod / rem: 1 and -floor(x / y) / -trunc(x / y) of the EXACT quotient, NaN at integer quotients."""
    R = args[0].dtype.type
    x = args[0]
    n = len(x)
    one, zero = np.ones(n, dtype=R), np.zeros(n, dtype=R)
    op, deg = key
    if deg == 1:
        return ({"neg": lambda: -one, "abs": lambda: np.where(x > 0, one, np.where(x < 0, -one, x)), "square": lambda: x + x,
                 "relu": lambda: np.where(x < 0, zero, one), "sign": lambda: zero, "round": lambda: zero, "floor": lambda: zero, "ceil": lambda: zero}[op](),)
    y = args[1]
    if deg == 2:
        if op in ("mod", "rem"):
            gx, gy = np.empty(n, dtype=R), np.empty(n, dtype=R)
            for i in range(n):
                q = Fraction(float(x[i])) / Fraction(float(y[i]))
                if q.denominator == 1:
                    gx[i] = gy[i] = np.nan
                else:
                    fl = q.numerator // q.denominator
                    gx[i], gy[i] = 1, -(fl if op == "mod" or q > 0 else fl + 1)
            return gx, gy
        gt = x > y
        return {"+": lambda: (one, one), "-": lambda: (one, -one), "*": lambda: (y.copy(), x.copy()), "greater": lambda: (zero, zero),
                "max": lambda: (np.where(gt, one, zero), np.where(gt, zero, one)), "min": lambda: (np.where(gt, zero, one), np.where(gt, one, zero))}[op]()
    z = args[2]
    if op == "fma":
        return y.copy(), x.copy(), one
    if op == "+":
        return one, one, one
    if op == "clamp":   # clamp(x, lo = y, hi = z)
        above, below = x > z, ~(x > z) & (x < y)
        return np.where(above | below, zero, one), np.where(below, one, zero), np.where(above, one, zero)
    gt2 = np.maximum(x, y) > z
    return np.where(gt2 & (x > y), one, zero), np.where(gt2 & ~(x > y), one, zero), np.where(gt2, zero, one)


@functools.lru_cache(maxsize=None)
def _exact_population(key, dtype_name):
    R = np.dtype(dtype_name).type
    args, regions = _build_args(key, R, NPTS, True, "partial")
    return args, regions, exact_partials(key, args)


def exact_population(key, dtype):
    """(args, regions, expected partials) of an EXACT operator."""
    return _exact_population(key, np.dtype(dtype).name)


def edge_table(R):
    """[(key, args, expected partials)]: the conventions of DESIGN.md §6 at the points where they are decided, the expected values written
    out here (NaN: any NaN; everything else: the bits).  Rows with a non-finite ARGUMENT are marked by their inputs: the reference's
    gradient returns at the first non-finite array, so those rows go through the scalar entry points of the oracle."""
    fi = np.finfo(R)
    tiny, eps = R(fi.tiny), R(fi.eps)
    nan, inf = R(np.nan), R(np.inf)
    below1 = np.nextafter(R(1), R(0))
    ln2, ln10 = R(0.693147180559945309417232121458176568), R(2.302585092994045684017991454684364208)
    rows = [
        (("abs", 1), (0.0,), (0.0,)), (("abs", 1), (-0.0,), (-0.0,)),
        (("relu", 1), (0.0,), (1.0,)), (("relu", 1), (-0.0,), (1.0,)), (("relu", 1), (-tiny,), (0.0,)),
        # max: x > y ? (1, 0) : (0, 1), a tie goes to the second argument; min: a tie goes to the first
        (("max", 2), (2.0, 2.0), (0.0, 1.0)), (("max", 2), (-0.0, 0.0), (0.0, 1.0)), (("max", 2), (0.0, -0.0), (0.0, 1.0)), (("max", 2), (3.0, 2.0), (1.0, 0.0)),
        (("min", 2), (2.0, 2.0), (1.0, 0.0)), (("min", 2), (-0.0, 0.0), (1.0, 0.0)), (("min", 2), (0.0, -0.0), (1.0, 0.0)), (("min", 2), (3.0, 2.0), (0.0, 1.0)),
        (("greater", 2), (2.0, 2.0), (0.0, 0.0)),
        # x ^ y at x = 0 (_pow_grad_x: y = 1 -> 1, y = 0 or y > 1 -> 0, 0 < y < 1 -> Inf, y < 0 -> y x^y / x; _pow_grad_p: y > 0 -> 0, else NaN)
        (("^", 2), (0.0, 0.0), (0.0, nan)), (("^", 2), (0.0, 1.0), (1.0, 0.0)), (("^", 2), (0.0, -1.0), (-inf, nan)), (("^", 2), (0.0, -2.0), (-inf, nan)),
        (("^", 2), (0.0, 0.5), (inf, 0.0)), (("^", 2), (0.0, 2.0), (0.0, 0.0)), (("^", 2), (0.0, 3.5), (0.0, 0.0)),
        # ... and at x = +-Inf (y = 1 -> 1; else y x^y / x and x^y log|x| in IEEE arithmetic)
        (("^", 2), (inf, 1.0), (1.0, inf)), (("^", 2), (inf, 0.0), (0.0, inf)), (("^", 2), (inf, -1.0), (-0.0, nan)), (("^", 2), (inf, 0.5), (nan, inf)),
        (("^", 2), (inf, 2.0), (nan, inf)), (("^", 2), (-inf, 1.0), (1.0, -inf)), (("^", 2), (-inf, 0.0), (-0.0, inf)), (("^", 2), (-inf, -1.0), (-0.0, nan)),
        (("^", 2), (-inf, 2.0), (nan, inf)),
        # mod / rem at integer quotients
        (("mod", 2), (6.0, 3.0), (nan, nan)), (("mod", 2), (-6.0, 1.5), (nan, nan)), (("mod", 2), (0.0, 2.0), (nan, nan)), (("mod", 2), (7.0, 2.0), (1.0, -3.0)),
        (("mod", 2), (-7.0, 2.0), (1.0, 4.0)), (("rem", 2), (6.0, 3.0), (nan, nan)), (("rem", 2), (-6.0, 1.5), (nan, nan)), (("rem", 2), (0.0, 2.0), (nan, nan)),
        (("rem", 2), (7.0, 2.0), (1.0, -3.0)), (("rem", 2), (-7.0, 2.0), (1.0, 3.0)),
        # safe_*: on the edge of the domain, just outside and just inside
        (("safe_log", 1), (0.0,), (0.0,)), (("safe_log", 1), (-tiny,), (0.0,)), (("safe_log", 1), (tiny,), (R(1) / tiny,)), (("safe_log", 1), (-2.0,), (0.0,)),
        (("safe_log2", 1), (0.0,), (0.0,)), (("safe_log2", 1), (-tiny,), (0.0,)), (("safe_log2", 1), (1.0,), (R(1) / ln2,)),
        (("safe_log10", 1), (0.0,), (0.0,)), (("safe_log10", 1), (-tiny,), (0.0,)), (("safe_log10", 1), (1.0,), (R(1) / ln10,)),
        (("safe_log1p", 1), (-1.0,), (0.0,)), (("safe_log1p", 1), (np.nextafter(R(-1), R(-2)),), (0.0,)),
        (("safe_log1p", 1), (np.nextafter(R(-1), R(0)),), (R(2) / eps,)),   # x + 1 = eps / 2 exactly
        (("safe_sqrt", 1), (0.0,), (inf,)), (("safe_sqrt", 1), (-tiny,), (0.0,)), (("safe_sqrt", 1), (4.0,), (0.25,)),
        (("safe_acosh", 1), (1.0,), (inf,)), (("safe_acosh", 1), (below1,), (0.0,)), (("safe_acosh", 1), (0.0,), (0.0,)),
        # clamp(x, lo, hi): x > hi ? (0, 0, 1) : x < lo ? (0, 1, 0) : (1, 0, 0); the boundaries belong to the inside
        (("clamp", 3), (2.0, 1.0, 2.0), (1.0, 0.0, 0.0)), (("clamp", 3), (1.0, 1.0, 2.0), (1.0, 0.0, 0.0)), (("clamp", 3), (2.5, 1.0, 2.0), (0.0, 0.0, 1.0)),
        (("clamp", 3), (0.5, 1.0, 2.0), (0.0, 1.0, 0.0)), (("clamp", 3), (1.5, 2.0, 1.0), (0.0, 0.0, 1.0)), (("clamp", 3), (1.0, 1.0, 1.0), (1.0, 0.0, 0.0)),
        (("max", 3), (1.0, 1.0, 1.0), (0.0, 0.0, 1.0)), (("max", 3), (2.0, 2.0, 1.0), (0.0, 1.0, 0.0)), (("max", 3), (3.0, 2.0, 1.0), (1.0, 0.0, 0.0)),
    ]
    return [(k, tuple(R(a) for a in args), tuple(R(e) for e in exp)) for k, args, exp in rows]


def jacobian_rows(partials):
    """What forward mode makes of the partials of op(x1, .., xd): row k = sum_j g_j * (j == k) in IEEE arithmetic, so that a NaN or
    infinite partial of ANOTHER argument turns the row into NaN (Inf * 0), as it does in the reference."""
    R = np.asarray(partials[0]).dtype.type
    rows = []
    with np.errstate(all="ignore"):
        for k in range(len(partials)):
            acc = None
            for j, g in enumerate(partials):
                term = R(g) * R(1 if j == k else 0)
                acc = term if acc is None else R(acc + term)
            rows.append(acc)
    return tuple(rows)


def same_bits(got, want):
    """Element-wise: both NaN, or the same bits."""
    got, want = np.asarray(got), np.asarray(want)
    U = np.uint32 if got.dtype == np.float32 else np.uint64
    return (np.isnan(got) & np.isnan(want)) | (got.view(U) == want.view(U))


# ---- one-operator trees ---------------------------------------------------------------------------------------------------------------
def operator_enum(key):
    name, deg = key
    if deg == 1:
        return de.OperatorEnum(binary_operators=("+",), unary_operators=(name,))
    if deg == 2:
        return de.OperatorEnum(binary_operators=(name, "+") if name != "+" else ("+",))
    return de.OperatorEnum(binary_operators=("+",), ternary_operators=(name,))


def leaf_tree(key):
    """op(x1), op(x1, x2), op(x1, x2, x3)."""
    return de.Node(1, *[de.Node(feature=k + 1) for k in range(key[1])])


def accumulator_tree(key):
    """op(x1 + x2) for a unary operator (x2 == 0: the bits of op(x1))."""
    assert key[1] == 1
    return de.Node(1, de.Node(1, de.Node(feature=1), de.Node(feature=2)))


def feature_matrix(args, extra_zero_row=False):
    rows = list(args) + ([np.zeros_like(args[0])] if extra_zero_row else [])
    return np.asfortranarray(np.stack(rows))


def oracle_grad(oracle, key, args, tree=None, extra_zero_row=False):
    """The CPU oracle's (values, partial rows, element-wise flag) of the one-operator tree on `args`."""
    R = args[0].dtype.type
    tape, consts = de.flatten(tree or leaf_tree(key), operator_enum(key), R)
    return oracle.eval_grad_tree_array(tape, consts, feature_matrix(args, extra_zero_row), oracle.GRAD_VARIABLE, elementwise=True)


def oracle_scalar_partials(oracle, key, args):
    """A unary or binary operator's partials at one point through the oracle's scalar entry points."""
    R = np.asarray(args[0]).dtype.type
    code = de.OPCODES[key]
    g = oracle.unary_grad(code, args[0], R) if key[1] == 1 else oracle.binary_grad(code, args[0], args[1], R)
    return tuple(R(v) for v in (g if isinstance(g, tuple) else (g,)))


if __name__ == "__main__":   # the oracle's figures: kept share, max E, max B and the worst E / B per region
    from oracle import oracle
    for key in BOUNDED:
        for dt in DTYPES:
            p = partial_population(key, dt)
            _, grad, _ = oracle_grad(oracle, key, p.args)
            for k in range(key[1]):
                for name, m in partial_maxima(p, k, grad[k], p.b_orc[k]).items():
                    print(f"{key_name(key):14s} d{k} {np.dtype(dt).name:8s} {name:14s} kept {m['kept']:.3f}  E {m['max_E']:9.3f}  B {m['max_B']:9.3f}  "
                          f"E/B {m['worst_ratio']:6.3f} at {m['at']}")
