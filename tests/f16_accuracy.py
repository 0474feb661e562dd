"""Inputs, references and the acceptance rule of the per-operator accuracy tests of DE_F16 (tests/test_f16_accuracy_host.py on the CPU
Float16 oracle, tests/test_gpu_f16_accuracy.py on the device).  A plain helper module: no fixtures, no collection hooks.  DESIGN.md §13.1.

The rule.  A one-step opcode is r16(v), v a Float32 value within s Float32 ulps of the true value t.  So the admissible results at a point
are the binary16 values between r16(t - s ulp32(t)) and r16(t + s ulp32(t)) in the ordering of ord16 — almost everywhere ONE value, whose
bits the device must give; two neighbours where a rounding boundary of binary16 falls inside the window; never more (asserted).  Overflow
(from 65520 on: +-Inf) and the subnormal results follow from the same two roundings.  There is no tolerance besides s:

  s = 0    exact rows: the bits of the float64 value (every such result is a binary16 value).
  s = 0.5  correctly rounded rows (+ - * /, inv, square, sqrt, safe_sqrt): the Float32 value within half an ulp of t is THE correctly
           rounded Float32 value, so the admissible set is the single value r16(r32(t)); t in float64 is exact (+ - *, square) or decides
           both roundings (a quotient or a root of 11-bit significands that is no 12- / 25-bit value is further than 2^-27 relative from
           one, float64 is within 2^-53).  fma is the same row with the EXACT t (the contract: Float16(muladd(Float32...)), two roundings
           that are not innocuous), computed in error-free float64 arithmetic and checked against Fraction.
  s = 2    library functions (DESIGN.md §5's asserted device figure), t from float64 libm (numpy), mpmath for gamma; s is widened by
           2^-20 for the reference's own error (float64 libm is within 2^-20 Float32 ulp = 2^9 float64 ulp: held to mpmath on a strided
           subset by the host test).

Classes.  Where t is NaN (a NaN argument, a point outside the domain) the result must be NaN (sign and payload are not compared:
DESIGN.md §5); an infinite t must give that infinity; a zero result carries the sign of t.  The host test holds the CPU Float16 oracle to
these classes at every point, so at NaN / Inf arguments and outside the domains they ARE the oracle's (tests/test_f16_host.py pins it), and
the GPU test compares the device's class with the oracle's there once more.

Multi-step opcodes.  mod and +(x, y, z) are exact-arithmetic steps and have a single-valued model here; cube too.  custom_cos and pow_abs2
contain library steps: on the device they are compared bit for bit with their written-out trees (transitivity: the single steps are pinned
by the rule), on the host against the step models below built from the oracle's own single steps."""
import functools
import zlib
from collections import namedtuple
from fractions import Fraction

import numpy as np

import dynamicexpressions_jl_amd as de
from dynamicexpressions_jl_amd.operators import _B, _T, _U

H = np.float16
UNARY, BINARY, TERNARY = tuple(_U), tuple(_B), tuple(_T)
OPS = [(n, 1) for n in UNARY] + [(n, 2) for n in BINARY] + [(n, 3) for n in TERNARY]   # the 53 opcodes
SAFE_OF = {"safe_log": "log", "safe_log2": "log2", "safe_log10": "log10", "safe_log1p": "log1p", "safe_sqrt": "sqrt", "safe_acosh": "acosh"}

EXACT = {("neg", 1), ("abs", 1), ("relu", 1), ("sign", 1), ("round", 1), ("floor", 1), ("ceil", 1), ("max", 2), ("min", 2), ("rem", 2),
         ("greater", 2), ("clamp", 3), ("max", 3)}
ROUNDED = {("square", 1), ("inv", 1), ("sqrt", 1), ("safe_sqrt", 1), ("+", 2), ("-", 2), ("*", 2), ("/", 2), ("fma", 3)}
STEPS = {("cube", 1), ("mod", 2), ("+", 3)}                 # several exact-arithmetic steps: a single-valued numpy model
COMPOSITE = {("custom_cos", 1), ("pow_abs2", 2)}            # library steps inside: transitivity on the device, step models on the host
LIBRARY = [k for k in OPS if k not in EXACT | ROUNDED | STEPS | COMPOSITE]
S_LIBRARY = 2.0              # DESIGN.md §5, tests/operator_accuracy.py LIBRARY_ULP
REF_SLACK = 2.0 ** -20       # the float64 reference's own error, in Float32 ulp
MAX_TWO_VALUED = 0.005       # per opcode: the share of finite-result points whose admissible set has two members


def key_name(key):
    return f"{key[0]}({key[1]})"


def slack(key):
    return 0.0 if key in EXACT else (0.5 if key in ROUNDED else (S_LIBRARY if key in LIBRARY else None))


def _rng(*key):
    return np.random.Generator(np.random.PCG64(zlib.crc32("/".join(str(k) for k in key).encode())))


# ---- binary16 bits --------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=H).view(np.uint16)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint16).view(H)


def ord16(a):
    """binary16 values -> integers that order like the values (ulp distance = difference; -0 and +0 are both 0, Inf = 65504's + 1)."""
    u = bits(a).astype(np.int64)
    return np.where(u & 0x8000, -(u & 0x7FFF), u)


def r16(t):
    """float64 -> binary16, one rounding to nearest even (numpy converts directly: no intermediate Float32)."""
    with np.errstate(all="ignore"):
        return np.asarray(t, dtype=np.float64).astype(H)


def same_bits(a, b):
    """equal binary16 values, NaN == NaN (sign and payload of a NaN are not compared: DESIGN.md §5)"""
    a, b = np.asarray(a, dtype=H), np.asarray(b, dtype=H)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def ulp32(t):
    """The Float32 ulp of the binade of |t| (float64 in, float64 out): 2^(e - 23), t = 1.m x 2^e; 2^-149 below floatmin."""
    t = np.abs(np.asarray(t, dtype=np.float64))
    with np.errstate(all="ignore"):
        _, e = np.frexp(np.where(np.isfinite(t), t, 1.0))
    return np.ldexp(1.0, np.where(t == 0, -149, np.maximum(e - 24, -149)))


def klass(v):
    """0 finite and not zero, 1 NaN, 2 +Inf, 3 -Inf, 4 +0, 5 -0."""
    v = np.asarray(v, dtype=H)
    neg = np.signbit(v)
    return np.where(np.isnan(v), 1, np.where(np.isinf(v), np.where(neg, 3, 2), np.where(v == 0, np.where(neg, 5, 4), 0)))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def all_patterns():
    """Every binary16 bit pattern, NaNs included: column u holds the value of bits u."""
    x = from_bits(np.arange(65536, dtype=np.uint16)).copy()
    x.setflags(write=False)
    return x


SPECIAL_BITS = (0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00)   # +-0, +-Inf, one NaN
GRID_MANTISSAS = (0x000, 0x001, 0x155, 0x200, 0x2AB, 0x3FE, 0x3FF)


def _grid(exponents, mantissas):
    u = [s | (e << 10) | m for s in (0, 0x8000) for e in exponents for m in mantissas]
    return np.array(sorted(set(u) | set(SPECIAL_BITS)), dtype=np.uint16)


def grid_values():
    """G: both signs, every exponent field 0..30, seven mantissas, and +-0, +-Inf, one NaN: 437 values."""
    return from_bits(_grid(range(31), GRID_MANTISSAS))


def subgrid_values():
    """Every third exponent field (0, 3 .. 30), the mantissas 0x000 0x001 0x3FF, both signs, the specials: 69 values."""
    return from_bits(_grid(range(0, 31, 3), (0x000, 0x001, 0x3FF)))


@functools.lru_cache(maxsize=None)
def binary_args():
    """All ordered pairs of G, then 20000 pairs of uniformly random bit patterns."""
    g = grid_values()
    x, y = np.repeat(g, len(g)), np.tile(g, len(g))
    rnd = _rng("f16", "binary", "random").integers(0, 65536, (2, 20000)).astype(np.uint16)
    out = (np.concatenate([x, from_bits(rnd[0])]), np.concatenate([y, from_bits(rnd[1])]))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ternary_args():
    """All triples of the sub-grid, then the cancelling family z = -r16(x y) +- k binary16 ulps, k = 0..3, over all pairs of the sub-grid
    and 4000 pairs of random bit patterns."""
    g = subgrid_values()
    n = len(g)
    x, y, z = np.repeat(g, n * n), np.tile(np.repeat(g, n), n), np.tile(g, n * n)
    rnd = from_bits(_rng("f16", "ternary", "random").integers(0, 65536, (2, 4000)).astype(np.uint16))
    px, py = np.concatenate([np.repeat(g, n), rnd[0]]), np.concatenate([np.tile(g, n), rnd[1]])
    with np.errstate(all="ignore"):
        p = r16(-(px.astype(np.float64) * py.astype(np.float64)))
    cx, cy, cz = [], [], []
    for k in range(-3, 4):
        o = ord16(p) + k                                       # k binary16 ulps away, across zero as ord16 counts
        zk = from_bits(np.where(o < 0, 0x8000 | np.minimum(-o, 0x7C00), np.minimum(o, 0x7C00)).astype(np.uint16))
        zk = np.where(np.isnan(p), p, np.where((o == 0) & np.signbit(p), H(-0.0), zk)).astype(H)
        cx.append(px), cy.append(py), cz.append(zk)
    out = (np.concatenate([x] + cx), np.concatenate([y] + cy), np.concatenate([z] + cz))
    for a in out:
        a.setflags(write=False)
    return out


def args_of(key):
    return ((all_patterns(),), binary_args(), ternary_args())[key[1] - 1]


def path_columns():
    """A few thousand columns of the exhaustive row: every 17th bit pattern (17 is prime to the mantissa count: every exponent, every
    mantissa residue), the specials, the largest and smallest finite values of both signs, two more NaNs."""
    u = set(range(0, 65536, 17)) | set(SPECIAL_BITS) | {0x7BFF, 0xFBFF, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x8400, 0x7C01, 0xFFFF, 0x3C00, 0xBC00}
    return np.array(sorted(u), dtype=np.uint16)


def direct_columns(n):
    """n columns of the exhaustive row that keep every exponent field of both signs and every special."""
    must = sorted({s | (e << 10) | m for s in (0, 0x8000) for e in range(32) for m in (0x000, 0x001, 0x2AB, 0x3FF)})
    rest = [u for u in range(0, 65536, 31) if u not in set(must)]
    u = np.array((must + rest)[:n], dtype=np.uint16)
    assert len(u) == n and len(must) <= n
    return u


# ---- truth ----------------------------------------------------------------------------------------------------------------------------
def _jl_max(x, y):
    return np.where(np.isnan(x), x, np.where(np.isnan(y), y, np.where((y > x) | (np.signbit(x) & ~np.signbit(y)), y, x)))


def _jl_min(x, y):
    return np.where(np.isnan(x), x, np.where(np.isnan(y), y, np.where((y < x) | (np.signbit(y) & ~np.signbit(x)), y, x)))


def _gamma64(x):
    """mpmath's gamma, rounded to float64; +-Inf at +-0, NaN at the negative integers and -Inf (C's tgamma; Julia throws there)."""
    import mpmath as mp
    out = np.full(len(x), np.nan)
    with mp.workprec(80):
        for i, v in enumerate(x):
            v = float(v)
            if np.isnan(v) or v == -np.inf or (v < 0 and v == np.floor(v)):
                continue
            if v == 0:
                out[i] = np.copysign(np.inf, v)
            elif v > 40:                                        # gamma(40) = 2e46: Inf in binary16 (and in Float32)
                out[i] = np.inf
            else:
                out[i] = float(mp.gamma(mp.mpf(v)))             # (underflows to a signed zero below -180: the sign of gamma)
                if out[i] == 0:
                    out[i] = np.copysign(0.0, -1.0 if int(np.floor(v)) % 2 else 1.0)
    return out


_LIBM = {"cbrt": np.cbrt, "exp": np.exp, "exp2": np.exp2, "log": np.log, "log2": np.log2, "log10": np.log10, "log1p": np.log1p, "sin": np.sin,
         "cos": np.cos, "tan": np.tan, "sinh": np.sinh, "cosh": np.cosh, "tanh": np.tanh, "asin": np.arcsin, "acos": np.arccos, "atan": np.arctan,
         "asinh": np.arcsinh, "acosh": np.arccosh, "atanh": np.arctanh, "sqrt": np.sqrt, "gamma": _gamma64}
_OUTSIDE = {"safe_log": lambda x: x <= 0, "safe_log2": lambda x: x <= 0, "safe_log10": lambda x: x <= 0, "safe_log1p": lambda x: x <= -1,
            "safe_sqrt": lambda x: x < 0, "safe_acosh": lambda x: x < 1}


def two_sum(a, b):
    """s = fl(a + b) and the exact error e: a + b = s + e (float64; no overflow at binary16 magnitudes)."""
    with np.errstate(all="ignore"):
        s = a + b
        bb = s - a
        e = (a - (s - bb)) + (b - bb)
    return s, e


def round_sum(s, e, R):
    """s + e (|e| <= half a float64 ulp of s) rounded ONCE to R (np.float32 / np.float16), nearest even: R(s), except where s is exactly
    the midpoint of two R values and e != 0 — then e decides."""
    with np.errstate(all="ignore"):
        v = s.astype(R)
        v64 = v.astype(np.float64)
        lo = np.where(v64 <= s, v, np.nextafter(v, R(-np.inf)))
        hi = np.nextafter(lo, R(np.inf))
        lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
        mid = np.isfinite(s) & np.isfinite(hi64) & np.isfinite(lo64) & (lo64 != s) & ((s - lo64) == (hi64 - s)) & (e != 0)
        return np.where(mid & (e > 0), hi, np.where(mid & (e < 0), lo, v)).astype(R)


def fma_exact(x, y, z):
    """(s, e): x y + z = s + e exactly, float64 (the product of two binary16 values is exact)."""
    with np.errstate(all="ignore"):
        return two_sum(x.astype(np.float64) * y.astype(np.float64), z.astype(np.float64))


def fma_fraction(x, y, z, single=False):
    """The contract in exact rational arithmetic, one point: the exact value rounded to Float32, then to binary16 (single: to binary16 at once)."""
    v = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))

    def rne(v, p, emin):                                        # p significant bits, exponent of the last place >= emin
        if v == 0:
            return v
        e = max(int(np.floor(np.log2(float(abs(v))))) - (p - 1), emin)
        while abs(v) >= Fraction(2) ** (e + p):
            e += 1
        while e > emin and abs(v) < Fraction(2) ** (e + p - 1):
            e -= 1
        q = v / Fraction(2) ** e
        n = q.numerator // q.denominator
        r = q - n
        n += 1 if (r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2)) else 0
        return n * Fraction(2) ** e
    w = v if single else rne(v, 24, -149)
    w = rne(w, 11, -24)
    if v == 0:
        return H(float(x) * float(y) + float(z))                # (an exact zero: the sign of the IEEE sum of the exact product and z)
    return H(np.copysign(np.inf if abs(w) >= 65520 else float(w), float(v)))


def truth(key, args):
    """The float64 true value t of a one-step opcode (NaN outside the domain), or the single-valued model's value for STEPS rows."""
    op, deg = key
    a = [np.asarray(v, dtype=H).astype(np.float64) for v in args]
    x = a[0]
    with np.errstate(all="ignore"):
        if deg == 1:
            if op in _OUTSIDE:
                return np.where(_OUTSIDE[op](x), np.nan, _LIBM[SAFE_OF[op]](x))
            if op in _LIBM:
                return _LIBM[op](x)
            return {"neg": lambda: -x, "abs": lambda: np.abs(x), "square": lambda: x * x, "relu": lambda: np.where(x < 0, 0.0, x),
                    "sign": lambda: np.where(x > 0, 1.0, np.where(x < 0, -1.0, x)), "round": lambda: np.rint(x), "floor": lambda: np.floor(x),
                    "ceil": lambda: np.ceil(x), "inv": lambda: 1 / x,
                    "cube": lambda: r16(r16(x * x).astype(np.float64) * x).astype(np.float64)}[op]()
        y = a[1]
        if deg == 2:
            if op == "mod":   # Base's float mod: rem is exact; a zero takes the divisor's sign; the one rounded step is r + y (exact in float64)
                r = np.fmod(x, y)
                return np.where(r == 0, np.copysign(r, y), np.where((r > 0) != (y > 0), r16(r + y).astype(np.float64), r))
            return {"+": lambda: x + y, "-": lambda: x - y, "*": lambda: x * y, "/": lambda: x / y, "^": lambda: np.power(x, y), "max": lambda: _jl_max(x, y),
                    "min": lambda: _jl_min(x, y), "rem": lambda: np.fmod(x, y), "greater": lambda: (x > y).astype(np.float64)}[op]()
        z = a[2]
        if op == "fma":
            return fma_exact(*[np.asarray(v, dtype=H) for v in args])[0]
        if op == "clamp":
            return np.where(x > z, z, np.where(x < y, y, x))
        if op == "+":
            return r16(r16(x + y).astype(np.float64) + z).astype(np.float64)
        return _jl_max(_jl_max(x, y), z)


Ref = namedtuple("Ref", "key args t lo hi")


def window(t, s):
    """(lo, hi): r16 of the two ends of t -+ (s + 2^-20) ulp32(t); NaN where t is."""
    w = (s + REF_SLACK) * ulp32(t)
    with np.errstate(all="ignore"):
        return r16(np.where(np.isinf(t), t, t - w)), r16(np.where(np.isinf(t), t, t + w))


def reference_at(key, args):
    """The reference of a one-step (or single-valued multi-step) opcode on `args`: t and the ends of the admissible set."""
    assert key not in COMPOSITE
    args = tuple(np.asarray(a, dtype=H) for a in args)
    t = truth(key, args)
    if key == ("fma", 3):
        s, e = fma_exact(*args)
        lo = hi = r16(round_sum(s, e, np.float32).astype(np.float64))
    elif key in EXACT or key in STEPS:
        lo = hi = r16(t)
        assert np.array_equal(lo.astype(np.float64)[np.isfinite(t)], t[np.isfinite(t)]), key   # every such result is a binary16 value
    elif key in ROUNDED:
        with np.errstate(all="ignore"):
            lo = hi = r16(t.astype(np.float32).astype(np.float64))
    else:
        lo, hi = window(t, S_LIBRARY)
    for a in (t, lo, hi):
        a.setflags(write=False)
    return Ref(key, args, t, lo, hi)


@functools.lru_cache(maxsize=None)
def reference(key):
    """The cached reference of an opcode on its own inputs (args_of)."""
    return reference_at(key, args_of(key))


def composite_accept(key, args, got):
    """custom_cos / pow_abs2 by their steps: `got` follows from SOME admissible value of every library step (the arithmetic steps are
    numpy binary16 operations, rounded once each)."""
    got = np.asarray(got, dtype=H)
    if key == ("custom_cos", 1):
        c = reference_at(("cos", 1), args)
        return same_bits(got, np_square(c.lo)) | same_bits(got, np_square(c.hi))
    assert key == ("pow_abs2", 2)
    l = reference_at(("log", 1), (np.abs(np.asarray(args[0], dtype=H)),))
    ok = np.zeros(len(got), dtype=bool)
    for lv in (l.lo, l.hi):
        ok |= accept(reference_at(("exp", 1), (np_mul(args[1], lv),)), got)
    return ok


def accept(ref, got):
    """Per point: `got` is admissible.  NaN truth: NaN.  Otherwise not NaN, between lo and hi in ord16, an infinity only with t's sign,
    and a zero with the sign of t."""
    got = np.asarray(got, dtype=H)
    o, tn = ord16(got), np.isnan(ref.t)
    inside = ~np.isnan(got) & (ord16(ref.lo) <= o) & (o <= ord16(ref.hi))
    zero_ok = (got != 0) | (np.signbit(got) == np.signbit(ref.t))
    return np.where(tn, np.isnan(got), inside & zero_ok)


def census(ref, got=None):
    """The conditions and the report figures of one opcode: points compared, finite-result points, those with a two-valued set, the widest
    set, and for `got`: points outside the rule, points that are not the correctly rounded value r16(t) (with the worst argument)."""
    tn = np.isnan(ref.t)
    width = np.where(tn, 0, ord16(ref.hi) - ord16(ref.lo))
    correct = ref.lo if slack(ref.key) != S_LIBRARY else r16(ref.t)
    finite_result = ~tn & np.isfinite(correct.astype(np.float32))
    finite_args = np.logical_and.reduce([np.isfinite(a.astype(np.float32)) for a in ref.args])
    out = dict(points=int(len(ref.t)), finite_argument_points=int(finite_args.sum()), finite_result_points=int(finite_result.sum()),
               two_valued=int((finite_result & (width == 1)).sum()), widest_set=int(width.max()) + 1)
    if got is not None:
        ok = accept(ref, got)
        off = ~tn & ~same_bits(got, correct) & ~((correct == 0) & (np.asarray(got, dtype=H) == 0))
        d = np.where(off, np.abs(ord16(got) - ord16(correct)), 0)
        i = int(np.argmax(d))
        out.update(compared=int(len(ok)), compared_finite_argument_points=int(finite_args.sum()), outside_rule=int((~ok).sum()),
                   not_correctly_rounded=int(off.sum()),
                   worst_argument=[float(a[i]) for a in ref.args] if off.any() else None,
                   worst_ulp16=int(d[i]) if off.any() else 0,
                   first_outside=([float(a[np.argmax(~ok)]) for a in ref.args] + [float(np.asarray(got, dtype=H)[np.argmax(~ok)]),
                                  float(ref.lo[np.argmax(~ok)]), float(ref.hi[np.argmax(~ok)])]) if (~ok).any() else None)
    return out


# ---- step models of the composites (host: from the oracle's single steps; numpy binary16 arithmetic rounds every operation) ------------
def np_square(x):
    with np.errstate(all="ignore"):
        return (np.asarray(x, dtype=H) * np.asarray(x, dtype=H)).astype(H)


def np_mul(x, y):
    with np.errstate(all="ignore"):
        return (np.asarray(x, dtype=H) * np.asarray(y, dtype=H)).astype(H)


def np_add(x, y):
    with np.errstate(all="ignore"):
        return (np.asarray(x, dtype=H) + np.asarray(y, dtype=H)).astype(H)


# ---- one-operator trees ---------------------------------------------------------------------------------------------------------------
def unary_enum(names=UNARY):
    return de.OperatorEnum(binary_operators=("+", "*"), unary_operators=tuple(names))


def binary_enum():
    return de.OperatorEnum(binary_operators=BINARY, unary_operators=("exp", "log", "abs"))


def ternary_enum():
    return de.OperatorEnum(binary_operators=("+",), ternary_operators=TERNARY)


def x(k):
    return de.Node(feature=k)


def unary_groups(size=13):
    """The unary opcodes in groups small enough for the fused forms (more than 15 operators of a degree switch fusion off)."""
    return [UNARY[i:i + size] for i in range(0, len(UNARY), size)]


def enum_of(degree):
    return (unary_enum(), binary_enum(), ternary_enum())[degree - 1]


def leaf_tree(key, ops=None):
    """op(x1), op(x1, x2), op(x1, x2, x3) under `ops` (default: the enum of all opcodes of that degree)."""
    ops = ops or enum_of(key[1])
    return de.Node(ops.index(key[0], key[1]), *[x(k + 1) for k in range(key[1])])


def feature_matrix(args):
    return np.asfortranarray(np.stack([np.asarray(a, dtype=H) for a in args]))


def oracle_row(f16o, key, args, options=6):
    """(values, element-wise flag) of the one-operator tree in the CPU Float16 oracle (options 6: no early exit, every column computed)."""
    ops = enum_of(key[1])
    tape, consts = de.flatten(leaf_tree(key, ops), ops, H)
    return f16o.eval_tree_array(tape, consts, feature_matrix(args), options=options, elementwise=True)


# ---- plausible wrong models (the discrimination checks of the host test) -------------------------------------------------------------
def wrong_cube_one_rounding(xv):
    v = np.asarray(xv, dtype=H).astype(np.float64)
    with np.errstate(all="ignore"):
        return r16(v * v * v)                                   # (exact in float64: 33 bits)


def wrong_custom_cos_one_rounding(xv):
    with np.errstate(all="ignore"):
        return r16(np.cos(np.asarray(xv, dtype=H).astype(np.float64)) ** 2)


def wrong_pow_abs2_no_middle_rounding(xv, yv):
    with np.errstate(all="ignore"):
        l = r16(np.log(np.abs(np.asarray(xv, dtype=H).astype(np.float64)))).astype(np.float64)
        return r16(np.exp(np.asarray(yv, dtype=H).astype(np.float64) * l))


def wrong_fma_rounded_once(xv, yv, zv):
    s, e = fma_exact(*[np.asarray(v, dtype=H) for v in (xv, yv, zv)])
    return round_sum(s, e, H)
