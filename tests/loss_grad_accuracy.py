"""The vehicle of the fused loss-gradient accuracy tests (tests/test_loss_grad_accuracy_host.py on the CPU oracle,
tests/test_gpu_loss_grad_accuracy.py on the device).  A plain helper module: no fixtures, no collection hooks.

A fused loss gradient is a sum over samples, so a pointwise partial has to be isolated: loss="pullback" with y = dY = 1, N = 1,
variable=False and ONE TREE PER POINT of a population of tests/operator_accuracy.py, the point in the tree's constants.  Every feature
row holds -0.0: c + (-0.0) == c for every c (-0.0 included) and the partial of `+` is exactly 1, so entry k of a tree's dloss is the
kernel's partial k at that point with nothing else rounded, and its "loss" is the operator's value.

Forms (constants in depth-first order, so constant k is argument k):
    unary     acc          op(x1 + c)
    binary    slots        op(x1 + c1, x2 + c2)
              const-right  op(x1 + c1, c2)
              const-left   op(c1, x1 + c2)            (the reversed generic opcodes DOP_R* of the gradient kernels)
    ternary   slots        op(x1 + c1, x2 + c2, x3 + c3)
              two-consts   op(x1 + c1, c2, c3)

The acceptance rule is that of the eval_grad tests: E <= 1.01 B(x; s) + 2^-9 at every kept point of every region (oa.partial_maxima)."""
import math

import numpy as np

import dynamicexpressions_jl_amd as de
import operator_accuracy as oa

FORMS = {1: ("acc",), 2: ("slots", "const-right", "const-left"), 3: ("slots", "two-consts")}


def forms(key):
    return FORMS[key[1]]


def _plus(key):   # the index of `+` in oa.operator_enum(key)
    return 2 if key[1] == 2 and key[0] != "+" else 1


def form_features(key, form):
    return key[1] if form == "slots" else 1


def form_tree(key, form, consts):
    """The tree of one point: `consts` are the operator's arguments."""
    plus = _plus(key)
    xc = lambda i, c: de.Node(plus, de.Node(feature=i), de.Node(val=c))
    c = [float(v) for v in consts]
    if form == "acc":
        return de.Node(1, xc(1, c[0]))
    if form == "slots":
        return de.Node(1, *[xc(i + 1, v) for i, v in enumerate(c)])
    if form == "const-right":
        return de.Node(1, xc(1, c[0]), de.Node(val=c[1]))
    if form == "const-left":
        return de.Node(1, de.Node(val=c[0]), xc(1, c[1]))
    if form == "two-consts":
        return de.Node(1, xc(1, c[0]), de.Node(val=c[1]), de.Node(val=c[2]))
    raise KeyError(form)


def form_trees(key, form, args):
    """One tree per point of `args` (a tuple of arrays, one per argument)."""
    return [form_tree(key, form, point) for point in zip(*[a.tolist() for a in args])]


def neg_zero_X(n_features, N, dtype):
    return np.asfortranarray(np.full((n_features, N), -0.0, dtype=dtype))


def rows_of(dls, deg, dtype):
    """[dloss_t] of a population of one-point trees -> rows[k][t], the arrays oa.partial_maxima takes."""
    g = np.asarray([np.asarray(d, dtype=dtype) for d in dls], dtype=dtype).reshape(len(dls), deg)
    return tuple(np.ascontiguousarray(g[:, k]) for k in range(deg))


def oracle_form(oracle, key, form, args):
    """The CPU oracle through the vehicle: (values, rows, flags) of eval_grad_tree_array(GRAD_CONSTANT) at N = 1, one call per point
    (the tape is that of the form: only the constants change)."""
    R = args[0].dtype.type
    n, deg = len(args[0]), key[1]
    tape, _ = de.flatten(form_tree(key, form, [1.0] * deg), oa.operator_enum(key), R)
    X = neg_zero_X(form_features(key, form), 1, R)
    out, ok = np.empty(n, dtype=R), np.empty(n, dtype=bool)
    rows = np.empty((deg, n), dtype=R)
    consts = np.stack(args, axis=1).astype(R)
    for i in range(n):
        o, g, f = oracle.eval_grad_tree_array(tape, consts[i], X, oracle.GRAD_CONSTANT, elementwise=True)
        out[i], rows[:, i], ok[i] = o[0], g[:, 0], f
    return out, tuple(rows[k] for k in range(deg)), ok


def accept(pop, rows, bounds):
    """The acceptance rule over every partial and region: (failures, {(k, region): maxima})."""
    failures, maxima = [], {}
    for k in range(pop.key[1]):
        for r, m in oa.partial_maxima(pop, k, rows[k], bounds[k]).items():
            maxima[(k, r)] = m
            if m["kept"] < oa.MIN_KEPT:
                failures.append(f"d{k} {r}: kept {m['kept']:.3f} < {oa.MIN_KEPT}")
            if not m["worst_ratio"] <= 1.0:
                failures.append(f"d{k} {r}: E = {m['E_at_worst']:.3f} > B = {m['B_at_worst']:.3f} at {m['at']}")
    return failures, maxima


# ---- leaf operands, in sum form ---------------------------------------------------------------------------------------------------------
LEAF_N = 257   # across a 64-lane wave and a 256-sample tile


def gamma_k(k, R):
    """gamma_k = k u / (1 - k u), u = eps / 2: the relative error of a sum of k + 1 terms in any association (Higham, Lemma 3.1)."""
    u = oa.eps_of(R) / 2
    return k * u / (1 - k * u)


def leaf_sum_cases(key, dtype):
    """Per region of the operator's population: (region, args of the first LEAF_N points kept for every partial, per partial the exact
    terms p_j as (hi, lo) and the pointwise slack 1.01 B_j + 2^-9; an EXACT operator's partials are exact rows: no slack)."""
    if key in oa.EXACT:
        args, regions, want = oa.exact_population(key, dtype)
        keep = np.ones(len(args[0]), dtype=bool)
        for w in want:
            keep &= np.isfinite(w)
        parts = [(w.astype(np.float64), np.zeros(len(w)), np.zeros(len(w))) for w in want]
    else:
        pop = oa.partial_population(key, dtype)
        args, regions = pop.args, pop.regions
        keep = np.logical_and.reduce(pop.keep)
        parts = [(p.hi, p.lo, oa.SECOND_ORDER * b + oa.REF_ROUNDING) for p, b in zip(pop.partials, pop.b_dev)]
    out = []
    fmax = float(np.finfo(dtype).max)
    for name, sl in regions:
        idx = np.flatnonzero(keep[sl])[:LEAF_N] + sl.start
        case = (name, tuple(a[idx] for a in args), [(hi[idx], lo[idx], s[idx]) for hi, lo, s in parts])
        # conditions on the reference alone; what they leave out is written down in LEAF_SUM_LEFT_OUT
        if len(idx) == LEAF_N and all(float(np.sum(np.abs(p[0]))) <= fmax / 2 for p in case[2]):
            out.append(case)
    return out


# The regions that have no sum form: sum_j |p_j| of the 257 points is beyond floatmax / 2 of the dtype (a partial sum may overflow in
# some association), or the region has no finite partial at all (mod / rem at integer quotients: NaN by DESIGN.md §6).  The host test
# asserts that exactly these are left out.
LEAF_SUM_LEFT_OUT = {
    ("inv", 1, "float32"): {"wide"}, ("exp", 1, "float32"): {"wide"}, ("exp2", 1, "float32"): {"wide"}, ("sinh", 1, "float32"): {"wide"},
    ("gamma", 1, "float32"): {"top"},
    ("mod", 2, "float32"): {"integer"}, ("mod", 2, "float64"): {"integer"}, ("rem", 2, "float32"): {"integer"}, ("rem", 2, "float64"): {"integer"},
}


def leaf_sum_left_out(key, dtype):
    return LEAF_SUM_LEFT_OUT.get((key[0], key[1], np.dtype(dtype).name), set())


def leaf_sum_error(got, hi, lo, slack, R):
    """(|got - sum_j p_j|, the bound eps sum_j slack_j |p_j| + gamma_{N-1} sum_j |p_j|): the difference exactly (math.fsum of the hi
    and lo parts), the bound that of a sum in any association of terms that are each within their pointwise bound."""
    err = abs(math.fsum([float(got)] + [-v for v in hi] + [-v for v in lo]))
    mag = np.abs(hi)
    bound = oa.eps_of(R) * float(np.sum(slack * mag)) + gamma_k(len(hi) - 1, R) * float(np.sum(mag))
    return err, bound
