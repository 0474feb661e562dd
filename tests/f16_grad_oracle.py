"""References of the Float16 forward-mode gradients (DE_OPT_F16_GRAD, csrc/de_half_grad.hip).  A plain helper module:
no fixtures, no collection hooks.

* ``GradOracle``: de_oracle_grad_f16 / de_oracle_diff_f16 of the Float16 instantiation of the CPU oracle (tests/oracle_f16/: the shared
  oracle/de_oracle_impl.h with OT = _Float16 exports them), element-wise flags.
* ``np_dual``: a numpy binary16 dual-number interpreter of a tape over + - * / and the exact selectors.  numpy's float16 arithmetic rounds
  every operation to binary16, so this is Julia's Float16 grad_degn_eval for these operators independently of the C oracle and the device.
* the same interpreter with the unary library steps taken from 65536-entry tables, ``tables[name][bits(x)]``: the partial of sin is the
  cos table's entry, of cos the negated sin entry, of exp the exp entry (the contract: a library partial is the value table's own step)."""
import ctypes as C

import numpy as np

from dynamicexpressions_jl_amd.operators import OPCODE_NAMES

H = np.float16
VARIABLE, CONSTANT, BOTH = 0, 1, 2
LEAF_CONST, LEAF_FEATURE, LEAF_PARAM = 0, 1, 2


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class GradOracle:
    """eval_grad_tree_array / eval_diff_tree_array on Float16 data by the CPU oracle (an ``f16_oracle.F16Oracle``'s library)."""

    def __init__(self, f16o):
        self.lib = f16o.lib
        self.lib.de_oracle_grad_f16.restype = C.c_int
        self.lib.de_oracle_diff_f16.restype = C.c_int

    def grad(self, tape, consts, X, mode):
        """(out[N], grad[G, N], ok): rows ordered features, then constants in 'both' mode."""
        tape = np.ascontiguousarray(tape)
        consts = np.ascontiguousarray(consts, dtype=H)
        Xf = np.asfortranarray(np.asarray(X, dtype=H))
        F, N = Xf.shape
        nc = int(((tape["degree"] == 0) & (tape["op"] == LEAF_CONST)).sum())
        G = F if mode == VARIABLE else (nc if mode == CONSTANT else F + nc)
        out = np.empty(N, dtype=H)
        grad = np.zeros(max(G * N, 1), dtype=H)
        ok, ng = C.c_uint8(0), C.c_int64(0)
        rc = self.lib.de_oracle_grad_f16(_p(tape), C.c_int64(len(tape)), _p(consts), C.c_int64(len(consts)), _p(Xf), C.c_int32(F),
                                         C.c_int64(N), C.c_int64(F), C.c_int32(mode), C.c_int32(1), _p(out), _p(grad), C.byref(ok), C.byref(ng))
        if rc != 0:
            raise ValueError(f"oracle error {rc}")
        assert ng.value == G
        return out, grad[:G * N].reshape((G, N), order="F"), bool(ok.value)

    def diff(self, tape, consts, X, direction):
        """(out[N], dout[N], ok) for the 0-based feature `direction`."""
        tape = np.ascontiguousarray(tape)
        consts = np.ascontiguousarray(consts, dtype=H)
        Xf = np.asfortranarray(np.asarray(X, dtype=H))
        F, N = Xf.shape
        out, dout = np.empty(N, dtype=H), np.empty(N, dtype=H)
        ok = C.c_uint8(0)
        rc = self.lib.de_oracle_diff_f16(_p(tape), C.c_int64(len(tape)), _p(consts), C.c_int64(len(consts)), _p(Xf), C.c_int32(F),
                                         C.c_int64(N), C.c_int64(F), C.c_int32(direction), _p(out), _p(dout), C.byref(ok))
        if rc != 0:
            raise ValueError(f"oracle error {rc}")
        return out, dout, bool(ok.value)


def params_as_features(tape, X, params, classes, class_base=1):
    """The reference's own reduction of a parametric tree (src/ParametricExpression.jl:381-389): the parameters gathered by class into
    leading feature rows of a re-indexed tape.  Returns (tape', X'): parameter p is feature p, feature f is feature P + f."""
    params = np.asarray(params, dtype=H)
    P = params.shape[0]
    cls = np.clip(np.asarray(classes, dtype=np.int64) - class_base, 0, params.shape[1] - 1)
    t2 = np.array(tape, copy=True)
    leaf = t2["degree"] == 0
    feat, par = leaf & (t2["op"] == LEAF_FEATURE), leaf & (t2["op"] == LEAF_PARAM)
    t2["arg"][feat] += P
    t2["op"][par] = LEAF_FEATURE
    return t2, np.asfortranarray(np.concatenate([params[:, cls], np.asarray(X, dtype=H)], axis=0))


def _jl_max(x, y):
    return np.where(np.isnan(x), x, np.where(np.isnan(y), y, np.where((y > x) | (np.signbit(x) & ~np.signbit(y)), y, x)))


def _jl_min(x, y):
    return np.where(np.isnan(x), x, np.where(np.isnan(y), y, np.where((y < x) | (np.signbit(y) & ~np.signbit(x)), y, x)))


def _sign(x):
    return np.where(x > 0, H(1), np.where(x < 0, H(-1), x)).astype(H)


def _bits(a):
    return np.ascontiguousarray(a, dtype=H).view(np.uint16)


def np_dual(tape, consts, X, mode, tables=None, direction=None):
    """The dual-number evaluation of a tape in numpy binary16 arithmetic.  mode: VARIABLE / CONSTANT / BOTH, or `direction` (0-based
    feature) for eval_diff.  Returns (value[N], grad[G, N], flag): flag = every node's value and gradient finite on every sample, the
    reference's test after every node (eval_diff: always True).  `tables`: name -> 65536 binary16 values for cos / sin / exp."""
    X = np.asarray(X, dtype=H)
    F, N = X.shape
    consts = np.asarray(consts, dtype=H)
    nc = int(((tape["degree"] == 0) & (tape["op"] == LEAF_CONST)).sum())
    if direction is not None:
        G = 1
    else:
        G = F if mode == VARIABLE else (nc if mode == CONSTANT else F + nc)
    one, zero = H(1), H(0)
    ok = True
    stack = []

    def finite(v, d):
        return bool(np.all(np.isfinite(v)) and np.all(np.isfinite(d)))

    with np.errstate(all="ignore"):
        for nd in tape:
            deg, op, arg = int(nd["degree"]), int(nd["op"]), int(nd["arg"])
            if deg == 0:
                d = np.zeros((G, N), dtype=H)
                if op == LEAF_CONST:
                    v = np.full(N, consts[arg], dtype=H)
                    idx = arg if mode == CONSTANT else (F + arg if mode == BOTH else -1)
                    if direction is not None:
                        idx = -1
                else:
                    v = X[arg].copy()
                    idx = arg if mode in (VARIABLE, BOTH) else -1
                    if direction is not None:
                        idx = 0 if arg == direction else -1
                if idx >= 0:
                    d[idx] = one
            else:
                name = OPCODE_NAMES[op]
                kids = [stack.pop() for _ in range(deg)][::-1]
                if deg == 1:
                    (x, dx), = kids
                    if name == "neg":
                        v, g = -x, np.full(N, H(-1))
                    elif name == "abs":
                        v, g = np.abs(x), _sign(x)
                    elif name == "relu":
                        v, g = np.where(x < 0, zero, x).astype(H), np.where(x < 0, zero, one).astype(H)
                    elif name == "square":
                        v, g = (x * x).astype(H), (x + x).astype(H)
                    elif name in ("cos", "sin", "exp"):
                        b = _bits(x)
                        v = tables[name][b]
                        g = -tables["sin"][b] if name == "cos" else (tables["cos"][b] if name == "sin" else v)
                    else:
                        raise ValueError(f"np_dual: no model of the unary operator {name}")
                    d = (g[None, :] * dx).astype(H)
                elif deg == 2:
                    (x, dx), (y, dy) = kids
                    if name == "+":
                        v, gx, gy = (x + y).astype(H), np.full(N, one), np.full(N, one)
                    elif name == "-":
                        v, gx, gy = (x - y).astype(H), np.full(N, one), np.full(N, H(-1))
                    elif name == "*":
                        v, gx, gy = (x * y).astype(H), y, x
                    elif name == "/":
                        v = (x / y).astype(H)
                        gx, gy = (one / y).astype(H), (-((v / y).astype(H))).astype(H)
                    elif name in ("max", "min"):
                        gt = x > y
                        v = (_jl_max if name == "max" else _jl_min)(x, y).astype(H)
                        a, b = np.where(gt, one, zero).astype(H), np.where(gt, zero, one).astype(H)
                        gx, gy = (a, b) if name == "max" else (b, a)
                    elif name == "greater":
                        v, gx, gy = np.where(x > y, one, zero).astype(H), np.zeros(N, dtype=H), np.zeros(N, dtype=H)
                    else:
                        raise ValueError(f"np_dual: no model of the binary operator {name}")
                    d = ((gx[None, :] * dx).astype(H) + (gy[None, :] * dy).astype(H)).astype(H)
                else:
                    raise ValueError("np_dual: no ternary operators")
                v = np.asarray(v, dtype=H)
            if direction is None:
                ok = ok and finite(v, d)   # (after EVERY node, leaves included: src/EvaluateDerivative.jl:230-243)
            stack.append((v, d))
    (v, d), = stack
    return v, d, ok


# ---- partials with library steps, composed in numpy binary16 arithmetic from VALUE tables (the contract: a library partial is the value
# table's own step).  `tab`: unary operator name -> its 65536 values, tab[name][bits(x)] — the device's own one-step values in the GPU
# test, the oracle's in the host test.
LN2 = H(0.693147180559945309417232121458176568)
LIBRARY_UNARY = ("cbrt", "exp", "exp2", "sin", "cos", "tan", "sinh", "cosh", "tanh", "custom_cos")
LIBRARY_BINARY = ("^", "pow_abs2")
TABLE_OPS = ("cbrt", "exp", "exp2", "log", "sin", "cos", "tan", "sinh", "cosh", "tanh", "custom_cos")


def unary_partial_from_values(name, x, tab):
    x = np.asarray(x, dtype=H)
    b = _bits(x)
    one = H(1)
    with np.errstate(all="ignore"):
        o = tab[name][b]
        if name == "cbrt":
            return (one / (H(3) * (o * o).astype(H)).astype(H)).astype(H)
        if name == "exp":
            return o
        if name == "exp2":
            return (o * LN2).astype(H)
        if name == "sin":
            return tab["cos"][b]
        if name == "cos":
            return (-tab["sin"][b]).astype(H)
        if name == "tan":
            return (one + (o * o).astype(H)).astype(H)
        if name == "sinh":
            return tab["cosh"][b]
        if name == "cosh":
            return tab["sinh"][b]
        if name == "tanh":
            return (one - (o * o).astype(H)).astype(H)
        if name == "custom_cos":
            c, s = tab["cos"][b], tab["sin"][b]
            return ((H(2) * c).astype(H) * (-s)).astype(H)
    raise ValueError(name)


def binary_partials_from_values(name, x, y, o, tab):
    """(d/dx, d/dy) of ^ and pow_abs2 at (x, y) from the value row o = op(x, y) and the log table (ChainRules' real power rules)."""
    x, y, o = (np.asarray(v, dtype=H) for v in (x, y, o))
    one, zero = H(1), H(0)
    with np.errstate(all="ignore"):
        a = np.abs(x)
        l = tab["log"][_bits(a)]
        if name == "^":
            main = np.where(np.isinf(x) & (y == 1), one, ((o * y).astype(H) / x).astype(H))
            edge = np.where(y == 1, one, np.where((y == 0) | (y > 1), zero, H(np.inf)))
            gx = np.where((x != 0) | (y < 0), main, edge).astype(H)
            gy = np.where(x != 0, (o * l).astype(H), np.where(y > 0, zero, H(np.nan))).astype(H)
            return gx, gy
        if name == "pow_abs2":
            gx = (((o * y).astype(H) * (one / a).astype(H)).astype(H) * _sign(x)).astype(H)
            return gx, (o * l).astype(H)
    raise ValueError(name)


def one_hot_rows(partials):
    """The gradient rows of op(x1 .. xd) in variable mode from its partials: row k = sum_i g_i * (i == k), binary16 per operation, in the
    reference's association ((g0 s0 + g1 s1) + g2 s2) — Inf * 0 = NaN as in grad_degn_eval."""
    d = len(partials)
    rows = []
    with np.errstate(all="ignore"):
        for k in range(d):
            terms = [(g * (H(1) if i == k else H(0))).astype(H) for i, g in enumerate(partials)]
            acc = terms[0]
            for t in terms[1:]:
                acc = (acc + t).astype(H)
            rows.append(acc)
    return np.stack(rows)


def gamma_partial_reference(x):
    """t = gamma(x) digamma(x) by mpmath, rounded to float64: NaN at the poles 0, -1, -2 ... and at NaN / -Inf; +Inf at +Inf and wherever
    gamma overflows Float32; a zero carries the product's sign."""
    import mpmath as mp
    x = np.asarray(x, dtype=H).astype(np.float64)
    t = np.full(len(x), np.nan)
    with mp.workprec(64):
        for i, v in enumerate(x):
            if np.isnan(v) or v == -np.inf or (v <= 0 and v == np.floor(v)):
                continue
            if v > 36:    # gamma(36) = 1e40 overflows Float32; digamma > 0 there
                t[i] = np.inf
                continue
            m = mp.mpf(v)
            p = mp.gamma(m) * mp.digamma(m)
            t[i] = float(p)
            if t[i] == 0:
                t[i] = np.copysign(0.0, float(mp.sign(p)))
    return t


GAMMA_PARTIAL_MIN_SLACK = 2.5   # what gamma_partial_slack is at least: tgamma's slack (2) + the product's rounding (0.5)


def gamma_partial_slack(x):
    """The Float32 slack the Float32 partial of gamma is held to at the points x (tests/operator_accuracy.py: tgamma's slack, the
    product's rounding, and digamma's error as written over |digamma|) — per point by mpmath, so asked for few points only."""
    import mpmath as mp
    import operator_accuracy as oa
    assert oa.LIBRARY_ULP + 0.5 == GAMMA_PARTIAL_MIN_SLACK
    bound = oa._bounds(np.float32, oa.LIBRARY_ULP, 1.0)["gamma"]
    with mp.workprec(80):
        return np.array([float(bound(mp.mpf(float(v)))[0]) for v in np.asarray(x, dtype=H)])


# ---- the reference's own acceptance (test/test_derivatives.jl:40-144 runs it for Float16 too; equation 3 is skipped there as well) -------
def acceptance_cases():
    """[(name, tree, operators, mode, closed form X64 -> float64 gradient [G, N])]: equations 1 and 2 with respect to the variables,
    equations 4 and 5 with respect to the constants."""
    import dynamicexpressions_jl_amd as de
    ops = de.OperatorEnum(binary_operators=("+", "*", "-", "/", "pow_abs2"), unary_operators=("custom_cos", "exp", "sin"))
    x1, x2, x3 = (de.Node(feature=k) for k in (1, 2, 3))

    def b(name, l, r):
        return de.Node(ops.index(name, 2), l, r)

    def u(name, c):
        return de.Node(ops.index(name, 1), c)

    def c(v):
        return de.Node(val=v)

    eq1 = b("+", b("+", b("+", x1, x2), x3), c(3.2))
    eq2 = b("+", b("+", b("+", b("pow_abs2", x1, x2), x3), u("custom_cos", b("+", c(1.0), x3))), b("/", c(3.0), x1))
    eq4 = b("*", c(3.2), x1)
    eq5 = b("+", b("+", b("+", b("pow_abs2", x1, x2), x3), u("custom_cos", b("+", c(2.1), x3))), b("/", c(-3.2), x1))

    def g1(X):
        return np.ones_like(X)

    def g2(X):
        a, p, z = X
        return np.stack([p * np.abs(a) ** (p - 1) * np.sign(a) - 3.0 / a ** 2, np.abs(a) ** p * np.log(np.abs(a)),
                         1.0 - 2.0 * np.cos(1.0 + z) * np.sin(1.0 + z)])

    def g4(X):
        return X[:1].copy()

    def g5(X):
        a, _, z = X
        return np.stack([-2.0 * np.cos(2.1 + z) * np.sin(2.1 + z), 1.0 / a])

    return [("equation1", eq1, ops, VARIABLE, g1), ("equation2", eq2, ops, VARIABLE, g2),
            ("equation4", eq4, ops, CONSTANT, g4), ("equation5", eq5, ops, CONSTANT, g5)]


def acceptance_X(seed):
    """test_derivatives.jl:51, `rand(rng, type, nfeatures, N) * 5`, with numpy's PCG64 for the MersenneTwister."""
    return np.asfortranarray((np.random.Generator(np.random.PCG64(seed)).random((3, 100)).astype(H) * H(5)).astype(H))


def isapprox_norm(a, b, rtol=0.1):
    """Julia's isapprox(a, b; rtol) on arrays: norm(a - b) <= rtol * max(norm(a), norm(b)); returns (verdict, relative norm error)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    err, scale = np.linalg.norm(a - b), max(np.linalg.norm(a), np.linalg.norm(b))
    return bool(err <= rtol * scale), float(err / scale) if scale > 0 else 0.0
