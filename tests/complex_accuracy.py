"""Inputs, reference and error measures of the complex accuracy tests (tests/test_complex_accuracy_host.py on the CPU oracle,
tests/test_gpu_complex_accuracy.py on the device).  A plain helper module: no fixtures, no collection hooks.

Inputs.  Every population is seeded (PCG64, seed = crc32 of its name), built in the COMPONENT type (float32 / float64) and only then
widened, so the reference sees exactly the bits the kernel sees.  A region has at most 1500 points; the regions of one (operator,
dtype) are concatenated into one population so that a test needs one device call and one oracle call.

Reference.  mpmath at 160 bits, kept per component as an unevaluated sum hi + lo of two Float64 values (106 bits), which makes the error
measures vectorised: (got - hi) - lo is exact wherever got is within a factor of two of the truth.

Error measures, R the component type:
    normwise       |got - true| / spacing_R(|true|)                 (complex modulus; every operator)
    componentwise  |got.re - true.re| / spacing_R(|true.re|), same for im   (only where the formula delivers it)
A point is KEPT when no component of the true result is at or above floatmax/2 and its modulus is at least 2 floatmin; every region
must keep >= 90 % of its points (asserted by both test files).  Componentwise, parts whose true value is below floatmin are skipped."""
import functools
import zlib
from collections import namedtuple

import numpy as np

import dynamicexpressions_jl_amd as de

CDTYPES = (np.complex64, np.complex128)
REAL_OF = {np.dtype(np.complex64): np.float32, np.dtype(np.complex128): np.float64}
NPTS = 1500
MP_PREC = 160
MIN_KEPT = 0.90

UNARY_REGIONS = {
    "sqrt": ("ordinary", "wide", "wide_eq", "circle", "ring"),
    "log": ("ordinary", "wide", "wide_eq", "circle", "ring"),
    "inv": ("ordinary", "wide", "wide_eq", "circle", "ring"),
    "exp": ("ordinary", "expz"),
    "sin": ("ordinary", "trigz", "trigbig"),
    "cos": ("ordinary", "trigz", "trigbig"),
    "sinh": ("ordinary", "expz"),
    "cosh": ("ordinary", "expz"),
    "tanh": ("ordinary", "guard", "poles"),
    "tan": ("ordinary", "guard_swapped", "poles_swapped"),
    "square": ("ordinary",),
    "cube": ("ordinary",),
    "custom_cos": ("ordinary",),
    "neg": ("ordinary",),
}
UNARY = tuple(UNARY_REGIONS)
# (class of a, class of b) per region of a binary operator
BINARY_REGIONS = {
    "/": (("ordinary", "ordinary"), ("huge", "huge"), ("tiny", "tiny"), ("huge", "ordinary"), ("ordinary", "tiny"), ("ordinary", "skewed"),
          ("skewed", "skewed")),
    "*": (("ordinary", "ordinary"), ("big", "big"), ("skewed", "skewed")),
}
# componentwise error is asserted for these; for tan / tanh outside the guard regions (behind the guard the small part is +-0)
COMPONENTWISE = ("sqrt", "exp", "sin", "cos", "sinh", "cosh", "inv", "tan", "tanh")
NO_COMPONENTWISE_REGIONS = ("guard", "guard_swapped")


def real_of(dtype):
    return REAL_OF[np.dtype(dtype)]


def _rng(*key):
    return np.random.Generator(np.random.PCG64(zlib.crc32("/".join(str(k) for k in key).encode())))


def _sign(rng, n):
    return rng.choice([-1.0, 1.0], n)


def _cx(re, im, dtype):
    """(re, im) computed in Float64 -> rounded to the component type -> one array of the complex dtype."""
    R = real_of(dtype)
    z = np.empty(len(re), dtype=dtype)
    with np.errstate(over="raise"):
        z.real = np.asarray(re, dtype=np.float64).astype(R)
        z.imag = np.asarray(im, dtype=np.float64).astype(R)
    return z


def asinh_omega(R):
    """asinh(prevfloat(floatmax(R))), the constant of csrc/de_complex_ops.h CR<T>::asinh_omega() (tanh's overflow guard)."""
    return R(89.415985) if R == np.float32 else R(710.4758600739439)


def _neighbours(x, R, k=2):
    """x and the k floats of R on either side of it."""
    out, lo, hi = [R(x)], R(x), R(x)
    for _ in range(k):
        lo, hi = np.nextafter(lo, R(-np.inf)), np.nextafter(hi, R(np.inf))
        out += [lo, hi]
    return out


def _ring_boundary(R):
    """Points on each clause of c_log's log1p condition `k == 0 && 0.5 < beta^2 && (beta <= 1.25 || rho < 3)` (beta = max(|x|, |y|),
    theta = min, rho = x^2 + y^2) and the floats next to it on either side, in both orientations and all four quadrants."""
    bt = []
    for b in _neighbours(np.sqrt(R(0.5)), R):          # 0.5 < beta^2
        bt += [(b, R(0.1)), (b, R(0.5)), (b, b)]
    for b in _neighbours(R(1.25), R):                  # beta <= 1.25, with rho >= 3 (theta = 1.2) and rho < 3 (theta = 0.3)
        bt += [(b, R(1.2)), (b, R(0.3))]
    for t in _neighbours(np.sqrt(R(0.75)), R):         # rho < 3 at beta = 1.5 > 1.25
        bt.append((R(1.5), t))
    for t in _neighbours(np.sqrt(R(0.11)), R):         # rho < 3 at beta = 1.7
        bt.append((R(1.7), t))
    re, im = [], []
    for b, t in bt:
        for sb in (1, -1):
            for st in (1, -1):
                re += [sb * b, st * t]
                im += [st * t, sb * b]
    return np.array(re, dtype=np.float64), np.array(im, dtype=np.float64)


def unary_region(region, dtype, n=NPTS):
    """The input region `region` in `dtype`: a complex array of at most n points."""
    R = real_of(dtype)
    fi = np.finfo(R)
    rng = _rng("unary", region, np.dtype(dtype).name)
    fmax, subn = float(fi.max), float(fi.smallest_subnormal)
    swapped = region.endswith("_swapped")
    base = region[:-len("_swapped")] if swapped else region
    if base == "ordinary":
        re, im = (_sign(rng, n) * 10.0 ** rng.uniform(-3, 1, n) for _ in range(2))
    elif base == "wide":
        lo, hi = np.log10(10 * subn), np.log10(fmax / 3)
        re, im = (_sign(rng, n) * 10.0 ** rng.uniform(lo, hi, n) for _ in range(2))
    elif base == "wide_eq":  # one magnitude, both parts within a factor of 2 of it
        lo, hi = np.log10(20 * subn), np.log10(fmax / 6)
        m = 10.0 ** rng.uniform(lo, hi, n)
        re, im = (_sign(rng, n) * m * 2.0 ** rng.uniform(-1, 1, n) for _ in range(2))
    elif base == "circle":
        r = 1 + _sign(rng, n) * 10.0 ** rng.uniform(np.log10(float(fi.eps)), -0.4, n)
        a = rng.uniform(-np.pi, np.pi, n)
        re, im = r * np.cos(a), r * np.sin(a)
    elif base == "ring":
        bre, bim = _ring_boundary(R)
        m = n - len(bre)
        r, a = rng.uniform(0.6, 1.9, m), rng.uniform(-np.pi, np.pi, m)
        re, im = np.concatenate([r * np.cos(a), bre]), np.concatenate([r * np.sin(a), bim])
    elif base == "expz":
        top = np.log(fmax) - 1
        re, im = rng.uniform(-top, top, n), rng.uniform(-20, 20, n)
    elif base == "trigz":
        top = np.log(fmax) - 1
        re, im = rng.uniform(-20, 20, n), rng.uniform(-top, top, n)
    elif base == "trigbig":
        re, im = rng.uniform(-1e4, 1e4, n), rng.uniform(-3, 3, n)
    elif base == "guard":  # tanh: |re| around omega / 4, the threshold of the overflow branch, and the floats on either side of it
        w4 = asinh_omega(R) / R(4)
        edge = np.array([s * float(v) for v in _neighbours(w4, R) for s in (1, -1)] * 3)
        eim = np.repeat([0.3, -2.0, 3.9], len(edge) // 3)
        m = n - len(edge)
        re = np.concatenate([_sign(rng, m) * float(w4) * rng.uniform(0.8, 1.2, m), edge])
        im = np.concatenate([rng.uniform(-4, 4, m), eim])
    elif base == "poles":  # tanh: im next to k pi / 2 (poles at odd k, zeros at even k when re is small)
        re = _sign(rng, n) * 10.0 ** rng.uniform(-6, 0.5, n)
        im = rng.integers(-5, 6, n) * (np.pi / 2) + _sign(rng, n) * 10.0 ** rng.uniform(-6, -1, n)
    else:
        raise KeyError(region)
    return _cx(im, re, dtype) if swapped else _cx(re, im, dtype)


def _magnitude(cls, rng, n, R):
    fi = np.finfo(R)
    if cls in ("ordinary", "skewed"):
        return 10.0 ** rng.uniform(-3, 1, n)
    if cls == "huge":   # within 10^3 of floatmax / 5
        return float(fi.max) / 5 * 10.0 ** -rng.uniform(0, 3, n)
    if cls == "tiny":   # with subnormals
        return float(fi.tiny) * 10.0 ** rng.uniform(-4, 2, n)
    if cls == "big":    # near sqrt(floatmax): the product of two stays below floatmax / 2
        return np.sqrt(float(fi.max)) * 10.0 ** rng.uniform(-3, -0.5, n)
    raise KeyError(cls)


def _spread(cls, R):
    return (30.0 if R == np.float32 else 250.0) if cls == "skewed" else 1.0


def binary_region(op, classes, dtype, const_side=None, n=NPTS, n_const=4):
    """(a, b) pairs of one region of `/` or `*`: an operand has one magnitude of its class, each part is magnitude x 10^U(-spread, 0)
    with a random sign.  const_side = "a" / "b": that operand takes n_const distinct values only, each repeated n / n_const times (the
    constant forms c op x and x op c: one tree per value).  For `/` the numerator's magnitude is capped at floatmax / 32 times the
    denominator's, so that huge / ordinary and ordinary / tiny stay finite (the cap binds in those two regions only)."""
    R = real_of(dtype)
    fi = np.finfo(R)
    rng = _rng("binary", op, classes[0], classes[1], np.dtype(dtype).name, const_side)
    rep = n // n_const

    def parts(mag, cls, count):
        return [_sign(rng, count) * mag * 10.0 ** -rng.uniform(0, _spread(cls, R), count) for _ in range(2)]

    def operand(cls, is_const, cap=None):
        count = n_const if is_const else n
        mag = _magnitude(cls, rng, count, R)
        if is_const:
            mag = np.repeat(mag, rep)
        if cap is not None:
            mag = np.minimum(mag, cap)
        if is_const:
            re, im = parts(mag[::rep], cls, n_const)
            if cls == "skewed":  # a skewed constant keeps one part at its magnitude: one that is tiny in both parts is a tiny constant
                full = _sign(rng, n_const) * mag[::rep]
                pick = rng.integers(0, 2, n_const) == 0
                re, im = np.where(pick, full, re), np.where(pick, im, full)
            re, im = np.repeat(re, rep), np.repeat(im, rep)
        else:
            re, im = parts(mag, cls, n)
        return mag, _cx(re, im, dtype)

    bmag, b = operand(classes[1], const_side == "b")
    with np.errstate(over="ignore"):
        cap = bmag * (float(fi.max) / 32) if op == "/" and const_side != "a" else None
    _, a = operand(classes[0], const_side == "a", cap=cap)
    if op == "/" and const_side == "a":
        # a constant numerator cannot be capped per sample: the denominators keep to magnitudes at which the quotient stays finite
        amag = np.maximum(np.abs(a.real.astype(np.float64)), np.abs(a.imag.astype(np.float64)))
        floor = amag / float(fi.max) * 64
        scale = np.maximum(1.0, floor / bmag)
        b = _cx(b.real.astype(np.float64) * scale, b.imag.astype(np.float64) * scale, dtype)  # (huge / ordinary and ordinary / tiny only)
    return a, b


def addsub_inputs(op, dtype, n=NPTS):
    """+ / -: ordinary pairs, and a cancelling half with b = -+a U(0.5, 2)."""
    rng = _rng("addsub", op, np.dtype(dtype).name)
    a = unary_region("ordinary", dtype, n)
    re, im = (_sign(rng, n) * 10.0 ** rng.uniform(-3, 1, n) for _ in range(2))
    h = n // 2
    s = -1.0 if op == "+" else 1.0
    re[h:] = s * a.real[h:].astype(np.float64) * rng.uniform(0.5, 2, n - h)
    im[h:] = s * a.imag[h:].astype(np.float64) * rng.uniform(0.5, 2, n - h)
    return a, _cx(re, im, dtype)


# ---- the reference --------------------------------------------------------------------------------------------------------------------
def _mp_functions():
    import mpmath as mp
    return {"sqrt": mp.sqrt, "log": mp.log, "inv": lambda z: 1 / z, "exp": mp.exp, "sin": mp.sin, "cos": mp.cos, "sinh": mp.sinh,
            "cosh": mp.cosh, "tanh": mp.tanh, "tan": mp.tan, "square": lambda z: z * z, "cube": lambda z: z * z * z,
            "custom_cos": lambda z: mp.cos(z) ** 2, "neg": lambda z: -z,
            "/": lambda a, b: a / b, "*": lambda a, b: a * b, "+": lambda a, b: a + b, "-": lambda a, b: a - b}


Ref = namedtuple("Ref", "re_hi re_lo im_hi im_lo")


def reference(op, *args):
    """mpmath's value of op at every point, each component as hi + lo in Float64 (inf where it overflows Float64)."""
    import mpmath as mp
    f = _mp_functions()[op]
    n = len(args[0])
    out = np.zeros((4, n))
    with mp.workprec(MP_PREC):
        cols = [[mp.mpc(float(v.real), float(v.imag)) for v in a] for a in args]
        for i in range(n):
            w = f(*[c[i] for c in cols])
            for k, part in ((0, w.real), (2, w.imag)):
                hi = float(part)
                out[k, i] = hi
                out[k + 1, i] = float(part - mp.mpf(hi)) if np.isfinite(hi) else 0.0
    return Ref(*out)


def kept(ref, dtype):
    """The points that count: no component at or above floatmax / 2, modulus at least 2 floatmin (of the component type)."""
    fi = np.finfo(real_of(dtype))
    with np.errstate(over="ignore"):
        mod = np.hypot(ref.re_hi, ref.im_hi)
    return (np.abs(ref.re_hi) < float(fi.max) / 2) & (np.abs(ref.im_hi) < float(fi.max) / 2) & (mod >= 2 * float(fi.tiny))


def _spacing(v, R):
    with np.errstate(over="ignore"):
        return np.spacing(np.abs(v).astype(R)).astype(np.float64)


def errors(got, ref, dtype):
    """(normwise, componentwise) error of `got` in ulps of the component type, per point.  Normwise is +inf where got is not finite;
    componentwise is the larger of the two parts' errors, a part whose true value is below floatmin skipped (0).  Points that are
    not kept() carry garbage: mask them."""
    R = real_of(dtype)
    tiny = float(np.finfo(R).tiny)
    g_re, g_im = got.real.astype(np.float64), got.imag.astype(np.float64)
    with np.errstate(all="ignore"):
        e_re, e_im = np.abs((g_re - ref.re_hi) - ref.re_lo), np.abs((g_im - ref.im_hi) - ref.im_lo)
        bad = ~(np.isfinite(g_re) & np.isfinite(g_im))
        norm = np.where(bad, np.inf, np.hypot(e_re, e_im) / _spacing(np.hypot(ref.re_hi, ref.im_hi), R))
        c_re = np.where(np.abs(ref.re_hi) >= tiny, e_re / _spacing(ref.re_hi, R), 0.0)
        c_im = np.where(np.abs(ref.im_hi) >= tiny, e_im / _spacing(ref.im_hi, R), 0.0)
        comp = np.where(bad, np.inf, np.maximum(c_re, c_im))
    return norm, comp


# ---- populations: the regions of one (operator, dtype, form) side by side -------------------------------------------------------------
Population = namedtuple("Population", "op dtype form args ref keep regions")  # regions: [(name, slice)]


@functools.lru_cache(maxsize=None)
def _population(op, dtype_name, form):
    dtype = np.dtype(dtype_name).type
    if op in UNARY_REGIONS:
        names = list(UNARY_REGIONS[op])
        chunks = [(unary_region(r, dtype),) for r in names]
    else:
        side = {"xx": None, "cx": "a", "xc": "b"}[form]
        names = ["%s/%s" % c for c in BINARY_REGIONS[op]]
        chunks = [binary_region(op, c, dtype, side) for c in BINARY_REGIONS[op]]
    regions, at = [], 0
    for name, ch in zip(names, chunks):
        regions.append((name, slice(at, at + len(ch[0]))))
        at += len(ch[0])
    args = tuple(np.concatenate([ch[k] for ch in chunks]) for k in range(len(chunks[0])))
    for a in args:
        a.setflags(write=False)
    ref = reference(op, *args)
    return Population(op, dtype, form, args, ref, kept(ref, dtype), regions)


def population(op, dtype, form="xx"):
    """The cached population of (operator, dtype, form); form is "xx" (every operand a feature), "cx" / "xc" (binary operators with a
    constant left / right operand: n_const distinct values, see binary_region)."""
    return _population(op, np.dtype(dtype).name, form)


def region_maxima(pop, got):
    """Per region: dict(share kept, max normwise error, its input, max componentwise error, its input)."""
    norm, comp = errors(got, pop.ref, pop.dtype)
    out = {}
    for name, sl in pop.regions:
        k = pop.keep[sl]
        nz = np.where(k, norm[sl], -1.0)
        cz = np.where(k, comp[sl], -1.0)
        i, j = int(np.argmax(nz)), int(np.argmax(cz))
        out[name] = dict(kept=float(k.mean()), points=int(k.sum()), norm=float(nz[i]), norm_at=[complex(a[sl][i]) for a in pop.args],
                         comp=float(cz[j]), comp_at=[complex(a[sl][j]) for a in pop.args])
    return out


def has_componentwise(op, region):
    return op in COMPONENTWISE and region not in NO_COMPONENTWISE_REGIONS


# ---- one-operator trees ---------------------------------------------------------------------------------------------------------------
def operator_enum(op):
    if op in UNARY_REGIONS:
        return de.OperatorEnum(binary_operators=("+",), unary_operators=(op,))
    return de.OperatorEnum(binary_operators=(op,))


def trees_and_X(pop):
    """The one-operator trees of a population and its feature matrix: (trees, X[F, N], rows) with rows[t] the slice-of-N list that
    tree t answers for (one tree, everything, unless the form has a constant operand: then one tree per distinct constant)."""
    n = len(pop.args[0])
    x1, x2 = de.Node(feature=1), de.Node(feature=2)
    if pop.op in UNARY_REGIONS:
        return [de.Node(1, x1)], np.asfortranarray(pop.args[0][None, :]), [np.arange(n)]
    a, b = pop.args
    if pop.form == "xx":
        return [de.Node(1, x1, x2)], np.asfortranarray(np.stack([a, b])), [np.arange(n)]
    c, x = (a, b) if pop.form == "cx" else (b, a)
    starts = np.concatenate([[0], np.nonzero(c[1:] != c[:-1])[0] + 1, [n]])
    trees, rows = [], []
    for s, e in zip(starts[:-1], starts[1:]):
        leaf = de.Node(val=complex(c[s]))
        trees.append(de.Node(1, leaf, x1) if pop.form == "cx" else de.Node(1, x1, leaf))
        rows.append(np.arange(s, e))
    return trees, np.asfortranarray(x[None, :]), rows


def gather(out_rows, rows, n, dtype):
    """out[t, :] of every tree -> one array over the population's points."""
    got = np.empty(n, dtype=dtype)
    for t, r in enumerate(rows):
        got[r] = out_rows[t][r]
    return got


def oracle_eval(co, pop, options=6):
    """The CPU oracle (tests/oracle_complex/) on the population's one-operator trees: (values, complete flag per tree)."""
    trees, X, rows = trees_and_X(pop)
    ops = operator_enum(pop.op)
    outs, oks = [], []
    for t in trees:
        tape, consts = de.flatten(t, ops, pop.dtype)
        y, ok = co.eval_tree_array(tape, consts, X, pop.dtype, options, elementwise=True)
        outs.append(y)
        oks.append(ok)
    return gather(outs, rows, X.shape[1], pop.dtype), oks


def special_grid(dtype):
    """{+-0, +-smallest subnormal, +-floatmin, +-1, +-floatmax, +-Inf, NaN}^2 as complex values of `dtype` (169 points)."""
    fi = np.finfo(real_of(dtype))
    v = []
    for m in (0.0, float(fi.smallest_subnormal), float(fi.tiny), 1.0, float(fi.max), np.inf):
        v += [m, -m]
    v.append(np.nan)
    re, im = np.meshgrid(v, v, indexing="ij")
    with np.errstate(over="ignore"):
        return _cx(re.ravel(), im.ravel(), dtype)


def guard_overflow_points(dtype):
    """tanh behind its overflow guard with an imaginary part past floatmax / 2 (2|im| overflows): the regression inputs of the zero's
    sign, tanh(floatmax + floatmax i) first."""
    fi = np.finfo(real_of(dtype))
    M = float(fi.max)
    re = [M, M, -M, 1e3, -1e3, 1e3, M, 1e3]
    im = [M, -M, M, M, 0.75 * M, -0.51 * M, 0.6 * M, 0.9 * M]
    return _cx(re, im, dtype)


def special_pairs(dtype):
    """A 7 x 7 subset of grid pairs for * and /: seven values that between them hold every class of the grid."""
    fi = np.finfo(real_of(dtype))
    t, s, M = float(fi.tiny), float(fi.smallest_subnormal), float(fi.max)
    vals = [complex(0.0, -0.0), complex(1.0, -1.0), complex(-s, t), complex(M, -M), complex(np.inf, 1.0), complex(-1.0, np.nan),
            complex(-np.inf, np.inf)]
    a, b = np.meshgrid(np.arange(7), np.arange(7), indexing="ij")
    z = _cx([v.real for v in vals], [v.imag for v in vals], dtype)
    return z[a.ravel()], z[b.ravel()]


if __name__ == "__main__":  # the oracle's figures, as tests/test_complex_accuracy_host.py's CAPS table records them
    import tempfile
    import complex_oracle
    co = complex_oracle.build(tempfile.mkdtemp())
    for op in list(UNARY) + list(BINARY_REGIONS):
        for dt in CDTYPES:
            p = population(op, dt)
            got, _ = oracle_eval(co, p)
            for name, m in region_maxima(p, got).items():
                print(f"{op:10s} {np.dtype(dt).name:10s} {name:16s} kept {m['kept']:.3f}  norm {m['norm']:7.3f} at {m['norm_at']}"
                      f"  comp {m['comp']:9.3f} at {m['comp_at']}")
