"""Float16 forward-mode gradients on the MI355X (csrc/de_half_grad.hip, DE_OPT_F16_GRAD): de_eval_grad in its three
modes and de_eval_diff of a DE_F16 program made with the bit.  Everything here fails with DE_ERR_UNSUPPORTED without the feature.

1. per operator, all 53 opcodes on the inputs of tests/f16_accuracy.py: partials of exact and correctly rounded steps against the Float16
   CPU oracle bit for bit, partials with library steps against the numpy composition of the DEVICE's own one-step values, gamma by the
   admissible-set rule; the value row carries de_eval's bits
2. constant operands and reversed forms, with a subnormal partial
3. random populations against the oracle (ieee, ternary) and the table interpreter (bench), every N / mode / option
4. windows and spills   5. parameters   6. buffers   7. program life cycle   8. scope of the bit   9. the reference's acceptance
Run with `pytest -m gpu`."""
import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import f16_accuracy as fa
import f16_grad_oracle as fg
import f16_oracle

pytestmark = pytest.mark.gpu
H = np.float16
_CACHE = {}

IEEE_OPS = de.OperatorEnum(binary_operators=("+", "-", "*", "/"))
BENCH_OPS = de.synth.BENCH_OPERATORS
TERN_OPS = de.OperatorEnum(binary_operators=("+", "-", "*", "/", "mod", "rem", "^"),
                           unary_operators=("log", "exp2", "tan", "sqrt", "cube", "sin", "inv", "atan"),
                           ternary_operators=("fma", "clamp", "+", "max"))
OPSETS = {"ieee": IEEE_OPS, "bench": BENCH_OPS, "ternary": TERN_OPS}
MODES = {"variable": (True, fg.VARIABLE), "constant": (False, fg.CONSTANT), "both": ("both", fg.BOTH)}
OPTIONS = {"early_exit": dict(), "no_early_exit": dict(early_exit=False), "full_eval": dict(full_eval=True)}
# partials made of exact and correctly rounded steps only: the oracle's bits
EXACT_PARTIALS = ([(n, 1) for n in ("neg", "abs", "square", "cube", "relu", "sign", "round", "floor", "ceil", "inv", "sqrt", "log", "log2", "log10",
                                    "log1p", "asin", "acos", "atan", "asinh", "acosh", "atanh") + tuple(fa.SAFE_OF)] +
                  [(n, 2) for n in ("+", "-", "*", "/", "max", "min", "mod", "rem", "greater")] + [(n, 3) for n in fa.TERNARY])
LIBRARY_PARTIALS = [(n, 1) for n in fg.LIBRARY_UNARY] + [(n, 2) for n in fg.LIBRARY_BINARY]
assert sorted(EXACT_PARTIALS + LIBRARY_PARTIALS + [("gamma", 1)]) == sorted(fa.OPS)


def _population(opset, n, seed):
    """The recipe of tests/test_gpu_f16.py: 12-node trees over 5 features; `ternary`: op3(tree, a smaller tree, a leaf)."""
    ops = OPSETS[opset]
    trees = de.synth.random_population(n, seed=seed, node_count=12, nfeatures=5, operators=ops)
    if opset == "ternary":
        small = de.synth.random_population(n, seed=seed + 1, node_count=4, nfeatures=5, operators=ops)
        names = ("fma", "clamp", "+", "max")
        leaves = [de.Node(feature=1 + t % 5) if t % 3 else de.Node(val=0.5 + 0.25 * (t % 7)) for t in range(n)]
        trees = [de.Node(ops.index(names[t % 4], 3), trees[t], small[t], leaves[t]) for t in range(n)]
    return trees, ops


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _api.library()
    return _api


@pytest.fixture(scope="module")
def f16o(tmp_path_factory):
    return f16_oracle.build(str(tmp_path_factory.mktemp("f16_oracle")))


@pytest.fixture(scope="module")
def gorc(f16o):
    return fg.GradOracle(f16o)


def same(a, b):
    return fa.same_bits(a, b)


def host(*xs):
    import torch
    torch.cuda.synchronize()
    out = [x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x) for x in xs]
    return out[0] if len(out) == 1 else out


def pop_of(api, trees, ops, F, n_params=0, half_grad=True, dtype=H, **kw):
    return api.Population(trees, ops, dtype, n_features=F, n_params=n_params, eval_context=api.EvalContext(half_grad=half_grad, **kw))


def first_diff(got, want, args):
    bad = ~same(got, want)
    i = int(np.argmax(bad))
    return f"{int(bad.sum())} of {bad.size} differ, first at {[float(np.asarray(a).reshape(-1)[i % np.asarray(a).size]) for a in args]}: {got.reshape(-1)[i]!r}, expected {want.reshape(-1)[i]!r}"


# ---- 1. per operator ------------------------------------------------------------------------------------------------------------------
def device_op_rows(api, degree):
    """Of every opcode of `degree` on its inputs (one population of one-operator trees, full_eval): the de_eval row, the de_eval_grad
    value row, the variable-mode gradient rows and the de_eval_diff row of every direction.  Cached for the module."""
    if degree not in _CACHE:
        names = (fa.UNARY, fa.BINARY, fa.TERNARY)[degree - 1]
        ops = fa.enum_of(degree)
        X = fa.feature_matrix(fa.args_of((names[0], degree)))
        pop = pop_of(api, [fa.leaf_tree((n, degree), ops) for n in names], ops, degree, full_eval=True)
        try:
            val, _ = pop.eval(X)
            out, grads, _ = pop.eval_grad(X, True)
            assert pop.ctx.last_kernel_name() == "de_grad_half_kernel"
            diffs = []
            for d in range(degree):
                o2, dout, okd = pop.eval_diff(X, d + 1)
                assert np.asarray(okd).all()
                assert same(o2, val).all(), f"de_eval_diff value rows, direction {d}"
                diffs.append(dout)
        finally:
            pop.close()
        _CACHE[degree] = dict(names=names, val=dict(zip(names, val)), out=dict(zip(names, out)), grad=dict(zip(names, grads)),
                              diff={n: np.stack([dd[t] for dd in diffs]) for t, n in enumerate(names)})
    return _CACHE[degree]


def oracle_partial_rows(gorc, key):
    """The rows of the one-operator tree by de_oracle_diff_f16 per direction (no validity test: every column is computed)."""
    ops = fa.enum_of(key[1])
    tape, consts = de.flatten(fa.leaf_tree(key, ops), ops, H)
    X = fa.feature_matrix(fa.args_of(key))
    return np.stack([gorc.diff(tape, consts, X, d)[1] for d in range(key[1])])


@pytest.mark.parametrize("key", fa.OPS, ids=[fa.key_name(k) for k in fa.OPS])
def test_value_row_carries_the_bits_of_de_eval(api, key):
    dev = device_op_rows(api, key[1])
    assert same(dev["out"][key[0]], dev["val"][key[0]]).all(), first_diff(dev["out"][key[0]], dev["val"][key[0]], fa.args_of(key))
    assert same(dev["grad"][key[0]], dev["diff"][key[0]]).all(), "de_eval_diff rows differ from the variable-mode gradient rows"


@pytest.mark.parametrize("key", EXACT_PARTIALS, ids=[fa.key_name(k) for k in EXACT_PARTIALS])
def test_exact_partials_equal_the_oracle_bit_for_bit(api, gorc, key):
    got = device_op_rows(api, key[1])["grad"][key[0]]
    want = oracle_partial_rows(gorc, key)
    assert got.shape == want.shape
    assert same(got, want).all(), first_diff(got, want, fa.args_of(key))


@pytest.mark.parametrize("key", LIBRARY_PARTIALS, ids=[fa.key_name(k) for k in LIBRARY_PARTIALS])
def test_library_partials_are_composed_of_the_device_value_steps(api, key):
    tab = {n: device_op_rows(api, 1)["val"][n] for n in fg.TABLE_OPS}   # (the unary rows ARE the tables: column u = bit pattern u)
    args = fa.args_of(key)
    if key[1] == 1:
        want = fg.one_hot_rows([fg.unary_partial_from_values(key[0], args[0], tab)])
    else:
        o = device_op_rows(api, 2)["val"][key[0]]
        want = fg.one_hot_rows(list(fg.binary_partials_from_values(key[0], args[0], args[1], o, tab)))
    got = device_op_rows(api, key[1])["grad"][key[0]]
    assert same(got, want).all(), first_diff(got, want, args)


def test_gamma_partial_within_the_rule(api):
    """r16 of the Float32 product tgamma(x) digamma(x): the admissible-set rule of f16_accuracy with t = mpmath's gamma digamma and the
    slack tests/operator_accuracy.py holds the Float32 partial to.  The window of the least slack (2.5 Float32 ulps) first; the few points
    outside it get their own slack, and count as two-valued sets."""
    x = fa.all_patterns()
    got = device_op_rows(api, 1)["grad"]["gamma"][0]
    t = fg.gamma_partial_reference(x)
    lo, hi = fa.window(t, fg.GAMMA_PARTIAL_MIN_SLACK)
    ok = fa.accept(fa.Ref(("gamma", 1), (x,), t, lo, hi), got)
    again = np.flatnonzero(~ok & ~np.isnan(t))
    if len(again):
        lo2, hi2 = fa.window(t[again], fg.gamma_partial_slack(x[again]))
        ok[again] = fa.accept(fa.Ref(("gamma", 1), (x[again],), t[again], lo2, hi2), got[again])
    finite = ~np.isnan(t) & np.isfinite(fa.r16(t).astype(np.float32))
    two = int((finite & (fa.ord16(hi) - fa.ord16(lo) == 1)).sum()) + len(again)
    print(f"[f16 grad] gamma partial: {len(x)} points, {int(finite.sum())} finite results, {two} two-valued sets ({len(again)} by their own slack), "
          f"{int((~ok).sum())} outside the rule")
    assert two <= fa.MAX_TWO_VALUED * finite.sum()
    assert ok.all(), f"{int((~ok).sum())} points outside the rule, first at x = {float(x[np.argmax(~ok)])!r}: {float(got[np.argmax(~ok)])!r}, t = {t[np.argmax(~ok)]!r}"


# ---- 2. constant operands and reversed forms ------------------------------------------------------------------------------------------
CONSTS = (float(fa.from_bits([0x0155])[0]), 0.5, -3.0, 65504.0)   # 341 * 2^-24 (a subnormal), 0.5, -3, floatmax


@pytest.mark.parametrize("c", CONSTS, ids=["subnormal", "0.5", "-3", "65504"])
def test_constant_operands_and_reversed_forms(api, c):
    """op(x1, c) and op(c, x1) in constant and both mode equal op(x1, x2) with x2 == c (op(x2, x1) for the reversed form), every binary
    opcode, on every 17th bit pattern and the edges."""
    ops = fa.binary_enum()
    x = fa.from_bits(fa.path_columns())
    N = len(x)
    X1 = np.asfortranarray(x.reshape(1, N))
    X2 = np.asfortranarray(np.stack([x, np.full(N, c, dtype=H)]))
    fwd = [de.Node(ops.index(n, 2), de.Node(feature=1), de.Node(val=c)) for n in fa.BINARY]
    rev = [de.Node(ops.index(n, 2), de.Node(val=c), de.Node(feature=1)) for n in fa.BINARY]
    ref_f = [de.Node(ops.index(n, 2), de.Node(feature=1), de.Node(feature=2)) for n in fa.BINARY]
    ref_r = [de.Node(ops.index(n, 2), de.Node(feature=2), de.Node(feature=1)) for n in fa.BINARY]
    pc, pr = pop_of(api, fwd + rev, ops, 1, full_eval=True), pop_of(api, ref_f + ref_r, ops, 2, full_eval=True)
    try:
        vo, vg, _ = pr.eval_grad(X2, True)               # rows (d/dx1, d/dx2) = (d/dx, d/dc)
        bo, bg, _ = pc.eval_grad(X1, "both")             # rows (d/dx, d/dc)
        co, cg, _ = pc.eval_grad(X1, False)              # row d/dc
    finally:
        pc.close(), pr.close()
    nb = len(fa.BINARY)
    for t in range(2 * nb):
        name = fa.BINARY[t % nb] + (" reversed" if t >= nb else "")
        assert same(bo[t], vo[t]).all() and same(co[t], vo[t]).all(), name
        assert same(bg[t], vg[t]).all(), f"{name}, both mode: " + first_diff(bg[t], vg[t], (x,))
        assert same(cg[t][0], vg[t][1]).all(), f"{name}, constant mode: " + first_diff(cg[t][0], vg[t][1], (x,))
    if c == 65504.0:   # subnormal partials: 1 / y, and -(o / y) at x = y = 65504 where o = 1
        div = fa.BINARY.index("/")
        fin = np.isfinite(x.astype(np.float32))                            # (a NaN or Inf x makes the other partial times its zero seed NaN)
        assert (fa.bits(bg[div][0])[fin] == 0x0100).all()                  # d(x / c)/dx = 1 / 65504 = 256 * 2^-24
        at = int(np.flatnonzero(fa.bits(x) == 0x7BFF)[0])
        assert fa.bits(bg[nb + div][0])[at] == 0x8100                      # d(c / x)/dx at x = 65504: -(1 / 65504)
        assert fa.bits(bg[div][1])[at] == 0x8100                           # d(x / c)/dc at x = 65504


# ---- 3. random populations ------------------------------------------------------------------------------------------------------------
def bench_tables(api):
    if "tab" not in _CACHE:
        ops = de.OperatorEnum(binary_operators=("+",), unary_operators=("cos", "sin", "exp"))
        pop = pop_of(api, [de.Node(k, de.Node(feature=1)) for k in (1, 2, 3)], ops, 1, early_exit=False)
        try:
            rows, _ = pop.eval(fa.feature_matrix((fa.all_patterns(),)))
        finally:
            pop.close()
        _CACHE["tab"] = dict(zip(("cos", "sin", "exp"), rows))
    return _CACHE["tab"]


def reference_of(gorc, tabs, opset, tape, consts, X, mode=None, direction=None):
    """(value, rows, flag) of one tree: the table interpreter for the bench operators, else the Float16 oracle."""
    if opset == "bench":
        v, g, ok = fg.np_dual(tape, consts, X, mode, tables=tabs, direction=direction)
        return v, g, ok
    if direction is not None:
        v, dv, ok = gorc.diff(tape, consts, X, direction)
        return v, dv[None, :], ok
    return gorc.grad(tape, consts, X, mode)


# The inputs.  The guard below (at least half of the trees complete, so that the comparison cannot go empty) is a property of the REFERENCE on
# the inputs: the gradient flag asks for every value and every partial to be finite on every sample, and with 2 randn features a third of
# the + - * / trees and one in twenty of the ternary set's (mod, rem, ^, log, sqrt of differences ...) are complete at N = 4099.  So the
# features are positive and of disjoint narrow ranges (feature k in 0.5 + 0.2 k + [0, 0.15)), N columns of one matrix (completeness can
# only fall with N), and the population seeds are ones at which the Float16 oracle alone finds enough complete trees at N = 4099 in
# every mode: 61 (ieee), 57 (bench), 33 (ternary; the best of 24 seeds) of 64.
X_FULL = np.asfortranarray((0.5 + 0.2 * np.arange(5)[:, None] + 0.15 * np.random.Generator(np.random.PCG64(1)).random((5, 4099))).astype(H))
SEEDS = {"ieee": 4, "bench": 5, "ternary": 6}


@pytest.mark.parametrize("N", [1, 255, 257, 1023, 1025, 4099])
@pytest.mark.parametrize("option", list(OPTIONS))
@pytest.mark.parametrize("opset", list(OPSETS))
def test_random_population(api, gorc, opset, option, N):
    trees, ops = _population(opset, 64, SEEDS[opset])
    X = np.asfortranarray(X_FULL[:, :N])
    tabs = bench_tables(api) if opset == "bench" else None
    tapes = [de.flatten(t, ops, H) for t in trees]
    pop = pop_of(api, trees, ops, 5, **OPTIONS[option])
    try:
        for mname, (variable, mode) in MODES.items():
            out, grads, ok = pop.eval_grad(X, variable)
            complete = 0
            for t, (tape, consts) in enumerate(tapes):
                v, g, rok = reference_of(gorc, tabs, opset, tape, consts, X, mode=mode)
                assert bool(ok[t]) == rok, f"{mname}: flag of tree {t} ({de.string_tree(trees[t], ops)}): device {bool(ok[t])}, reference {rok}"
                if not rok:
                    continue
                complete += 1
                assert same(out[t], v).all(), f"{mname}: values of tree {t} ({de.string_tree(trees[t], ops)}): " + first_diff(out[t], v, ())
                assert grads[t].shape == g.shape
                assert same(grads[t], g).all(), f"{mname}: gradient of tree {t} ({de.string_tree(trees[t], ops)}): " + first_diff(np.asarray(grads[t]), g, ())
            assert 2 * complete >= len(trees), f"{mname}: only {complete} of {len(trees)} trees complete"
        for d in range(5):
            out, dout, ok = pop.eval_diff(X, d + 1)
            assert np.asarray(ok).all()   # (de_eval_diff tests nothing)
            for t, (tape, consts) in enumerate(tapes):
                v, g, _ = reference_of(gorc, tabs, opset, tape, consts, X, mode=fg.VARIABLE, direction=d)
                assert same(out[t], v).all() and same(dout[t], g[0]).all(), f"de_eval_diff direction {d}, tree {t} ({de.string_tree(trees[t], ops)})"
    finally:
        pop.close()


@pytest.mark.parametrize("opset", ["ieee", "ternary"])
def test_flags_on_hostile_inputs(api, gorc, opset):
    """The same populations on 2 randn features, where most trees are incomplete (divisions by differences near zero, mod and rem at
    integer ratios, logarithms and roots of negative values): the flags of ALL trees equal the oracle's, the complete trees' rows its bits."""
    trees, ops = _population(opset, 64, 2000 + len(opset))
    X = np.asfortranarray(de.synth.random_X(5, 1025, seed=17).astype(H))
    pop = pop_of(api, trees, ops, 5)
    try:
        for mname, (variable, mode) in MODES.items():
            out, grads, ok = pop.eval_grad(X, variable)
            refs = [gorc.grad(*de.flatten(t, ops, H), X, mode) for t in trees]
            assert np.array_equal(np.asarray(ok, dtype=bool), np.array([r[2] for r in refs])), mname
            assert 0 < sum(r[2] for r in refs) < len(trees)
            for t, (v, g, rok) in enumerate(refs):
                if rok:
                    assert same(out[t], v).all() and same(grads[t], g).all(), (mname, t)
    finally:
        pop.close()


# ---- 4. windows and spills ------------------------------------------------------------------------------------------------------------
def chain_tree(k):
    """k constants: (((x1 * c1) + x2 * c2) - x3 * c3 ...), the products nested to the right so that the tree needs spill slots."""
    b = lambda name, l, r: de.Node(IEEE_OPS.index(name, 2), l, r)   # noqa: E731
    terms = [b("*", de.Node(feature=1 + i % 5), de.Node(val=0.25 + 0.125 * i)) for i in range(k)]
    t = terms[-1]
    for i in range(k - 2, -1, -1):
        t = b(("+", "-")[i % 2], terms[i], t)
    return t


def deep_tree():
    """((x1 c1 + x2 c2) * ((x3 c3 + x4 c4) - ((x5 c5 + x1 c6) / (x2 + c7)))): right-nested sums of products, two spill slots."""
    b = lambda name, l, r: de.Node(IEEE_OPS.index(name, 2), l, r)   # noqa: E731
    x, c = (lambda k: de.Node(feature=k)), (lambda v: de.Node(val=v))
    s = lambda i, j, ci, cj: b("+", b("*", x(i), c(ci)), b("*", x(j), c(cj)))   # noqa: E731
    return b("*", s(1, 2, 0.5, 1.5), b("-", s(3, 4, -0.75, 2.0), b("/", s(5, 1, 1.25, -0.5), b("+", x(2), c(7.0)))))


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 8, 9, 17, "deep"])
def test_windows_and_spills(api, gorc, k):
    """Constant mode with 1 .. 6, 8, 9 and 17 constants (every window width; one, two and three windows) and both mode with F = 5,
    one population per tree (the launch's window follows its widest tree); N = 300: a full tile and a ragged one."""
    tree = deep_tree() if k == "deep" else chain_tree(k)
    X = np.asfortranarray((1.0 + de.synth.random_X(5, 300, seed=11).astype(H) / H(4)).astype(H))
    tape, consts = de.flatten(tree, IEEE_OPS, H)
    pop = pop_of(api, [tree], IEEE_OPS, 5)
    try:
        if k == "deep":
            assert pop.meta(0)["n_slots"] >= 2
        for mname, (variable, mode) in MODES.items():
            out, grads, ok = pop.eval_grad(X, variable)
            v, g, rok = gorc.grad(tape, consts, X, mode)
            assert rok and bool(ok[0]), mname
            assert grads[0].shape == g.shape and (k == "deep" or mode == fg.VARIABLE or g.shape[0] == k + (5 if mode == fg.BOTH else 0))
            assert same(out[0], v).all(), mname
            assert same(grads[0], g).all(), f"{mname}: " + first_diff(np.asarray(grads[0]), g, ())
    finally:
        pop.close()


# ---- 5. parameters --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdtype", [np.int32, np.int64])
def test_parameters(api, gorc, cdtype):
    """P = 2 parameters, 3 classes, both mode: rows ordered parameters, features, constants; against the oracle on the reference's own
    reduction (the parameters gathered by class into leading feature rows)."""
    ops = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("square", "neg"))
    b = lambda name, l, r: de.Node(ops.index(name, 2), l, r)   # noqa: E731
    p, x, c = (lambda k: de.ParametricNode(parameter=k)), (lambda k: de.ParametricNode(feature=k)), (lambda v: de.ParametricNode(val=v))
    trees = [b("+", b("*", p(1), x(1)), b("/", x(2), b("+", p(2), c(3.0)))),
             de.ParametricNode(ops.index("square", 1), b("-", b("*", x(3), p(2)), b("*", c(0.5), p(1)))),
             b("*", p(1), p(1)), b("+", x(1), c(1.5))]
    N, F, P = 700, 3, 2
    X = np.asfortranarray(de.synth.random_X(F, N, seed=5).astype(H))
    params = np.asfortranarray(np.array([[0.5, -1.25, 2.0], [4.0, 5.5, 6.25]], dtype=H))
    classes = (1 + np.arange(N) % 3).astype(cdtype)
    pop = pop_of(api, trees, ops, F, n_params=P)
    try:
        out, grads, ok = pop.eval_grad(X, "both", params=params, classes=classes)
        outv, gradv, okv = pop.eval_grad(X, True, params=params, classes=classes)
    finally:
        pop.close()
    for t, tree in enumerate(trees):
        tape, consts = de.flatten(tree, ops, H)
        t2, X2 = fg.params_as_features(tape, X, params, classes)
        v, g, rok = gorc.grad(t2, consts, X2, fg.BOTH)
        assert rok and bool(ok[t]) and bool(okv[t]), t
        assert same(out[t], v).all(), t
        assert grads[t].shape == g.shape and same(grads[t], g).all(), f"tree {t}: " + first_diff(np.asarray(grads[t]), g, ())
        assert same(gradv[t], g[:P + F]).all(), t


# ---- 6. buffers -----------------------------------------------------------------------------------------------------------------------
def test_buffers_pointer_stride_and_device_tensors(api):
    """An X pointer that is 2 mod 4 with ldX == F = 3 (N = 2053), ldX > F, torch.float16 device buffers: the bits of host buffers."""
    import torch
    trees, ops = _population("bench", 24, 77)
    from dynamicexpressions_jl_amd.node import max_feature
    trees = [t for t in trees if max_feature(t) <= 3][:12]
    assert len(trees) >= 6
    F, N = 3, 2053
    Xh = np.asfortranarray(de.synth.random_X(F, N, seed=3).astype(H))
    flat = torch.zeros(1 + N * F + 7, dtype=torch.float16, device="cuda")
    flat[1:1 + N * F] = torch.from_numpy(np.ascontiguousarray(Xh.T).reshape(-1)).cuda()
    Xu = flat[1:1 + N * F].view(N, F).t()
    assert Xu.data_ptr() % 4 == 2 and Xu.stride(1) == F
    wide = torch.zeros((N, 8), dtype=torch.float16, device="cuda")
    wide[:, :F] = torch.from_numpy(np.ascontiguousarray(Xh.T)).cuda()
    Xw = wide.t()[:F]
    assert Xw.stride(1) == 8
    pop = pop_of(api, trees, ops, F, full_eval=True)
    try:
        want = pop.eval_grad(Xh, "both")
        wdiff = pop.eval_diff(Xh, 2)
        for name, Xd in (("2 mod 4", Xu), ("ldX > F", Xw)):
            out, grads, ok = pop.eval_grad(Xd, "both")
            assert out.dtype == torch.float16 and grads[0].dtype == torch.float16
            out, ok = host(out, ok)
            assert np.array_equal(ok, want[2]), name
            assert same(out, want[0]).all(), name
            for t in range(len(trees)):
                assert same(host(grads[t]), want[1][t]).all(), (name, t)
            o2, d2, _ = pop.eval_diff(Xd, 2)
            assert same(host(o2), wdiff[0]).all() and same(host(d2), wdiff[1]).all(), name
    finally:
        pop.close()


def test_buffers_offsets_null_out_and_no_samples(api):
    """Caller-supplied grad_offsets with odd element offsets, out == NULL, and N == 0: the host flags (a constant 1e5 is Inf in binary16)."""
    lib = api.library()
    trees, ops = _population("ieee", 8, 123)
    trees.append(de.Node(1, de.Node(feature=1), de.Node(val=1e5)))
    F, N = 5, 300
    X = np.asfortranarray(de.synth.random_X(F, N, seed=9).astype(H))
    pop = pop_of(api, trees, ops, F, full_eval=True)
    try:
        out, grads, ok = pop.eval_grad(X, "both")
        nt = len(trees)
        ng = np.array([pop.n_grad(t, fg.BOTH) for t in range(nt)], dtype=np.int64)
        offs = np.zeros(nt, dtype=np.int64)
        at = 1
        for t in range(nt):
            offs[t] = at
            at += int(ng[t]) * N + 2 * t + 1
            at += 1 - at % 2                       # keep every offset odd
        assert (offs % 2 == 1).all()
        buf = np.full(at + 8, 7.0, dtype=H)
        ok2 = np.zeros(nt, dtype=np.uint8)
        out2 = np.empty((nt, N), dtype=H)
        rc = lib.de_eval_grad(pop.ctx._h, pop._h, X.ctypes.data, N, F, None, fg.BOTH, out2.ctypes.data, N, buf.ctypes.data, offs.ctypes.data, ok2.ctypes.data)
        assert rc == 0, lib.de_last_error(pop.ctx._h).decode()
        ok3 = np.zeros(nt, dtype=np.uint8)
        buf3 = np.full(at + 8, 7.0, dtype=H)
        rc = lib.de_eval_grad(pop.ctx._h, pop._h, X.ctypes.data, N, F, None, fg.BOTH, None, N, buf3.ctypes.data, offs.ctypes.data, ok3.ctypes.data)   # out == NULL
        assert rc == 0, lib.de_last_error(pop.ctx._h).decode()
        assert np.array_equal(ok2.astype(bool), ok) and np.array_equal(ok3, ok2) and same(out2, out).all()
        used = np.zeros(len(buf), dtype=bool)
        for t in range(nt):
            sl = slice(int(offs[t]), int(offs[t]) + int(ng[t]) * N)
            used[sl] = True
            for b_ in (buf, buf3):
                assert same(b_[sl].reshape((int(ng[t]), N), order="F"), grads[t]).all(), t
        assert (buf[~used] == H(7)).all() and (buf3[~used] == H(7)).all(), "a gradient was written outside its block"
        assert not ok[-1] and ok[:-1].any()
        # N == 0: the flags alone, from the host side
        ok0 = np.full(nt, 7, dtype=np.uint8)
        rc = lib.de_eval_grad(pop.ctx._h, pop._h, None, 0, F, None, fg.CONSTANT, None, 0, None, None, ok0.ctypes.data)
        assert rc == 0, lib.de_last_error(pop.ctx._h).decode()
        assert ok0[-1] == 0 and (ok0[:-1] == 1).all()
    finally:
        pop.close()


# ---- 7. program life cycle ------------------------------------------------------------------------------------------------------------
def _grad_all(pop, X):
    res = {}
    for mname, (variable, _) in MODES.items():
        out, grads, ok = pop.eval_grad(X, variable)
        res[mname] = (host(out), [host(g) for g in grads], host(ok))
    return res


def _assert_same_results(a, b, what):
    for mname in MODES:
        assert np.array_equal(a[mname][2], b[mname][2]), (what, mname)
        assert same(a[mname][0], b[mname][0]).all(), (what, mname)
        for t, (ga, gb) in enumerate(zip(a[mname][1], b[mname][1])):
            assert ga.shape == gb.shape and same(ga, gb).all(), (what, mname, t)


def test_set_consts_set_consts_device_and_update_equal_a_fresh_program(api):
    import torch
    trees, ops = _population("bench", 32, 31)
    X = np.asfortranarray(de.synth.random_X(5, 600, seed=4).astype(H))
    pop = pop_of(api, trees, ops, 5, full_eval=True)
    try:
        _grad_all(pop, X)                                   # (the gradient program exists before the constants move)
        new = (pop.constants().astype(np.float32) * 0.75 + 0.125).astype(H)
        new[0] = H(np.inf)                                  # (what 1e5 is as a binary16: its tree's flag must clear)
        fresh_trees = [t.copy() for t in trees]
        at = 0
        for t in fresh_trees:
            vals, refs = de.get_scalar_constants(t)
            de.set_scalar_constants(t, new[at:at + len(refs)].astype(np.float64), refs)
            at += len(refs)
        fresh = pop_of(api, fresh_trees, ops, 5, full_eval=True)
        want = _grad_all(fresh, X)
        fresh.close()
        pop.set_constants(new)
        _assert_same_results(_grad_all(pop, X), want, "de_program_set_consts")
        pop.set_constants(np.zeros_like(new))               # move them away, then set them from the device
        pop.set_constants(torch.from_numpy(new).cuda())
        _assert_same_results(_grad_all(pop, X), want, "de_program_set_consts_device")
        # de_program_update: replace every third tree
        repl, _ = _population("bench", 11, 32)
        ids = list(range(0, len(trees), 3))
        pop.update(ids, repl[:len(ids)])
        for i, k in enumerate(ids):
            fresh_trees[k] = repl[i]
        fresh = pop_of(api, fresh_trees, ops, 5, full_eval=True)
        want = _grad_all(fresh, X)
        fresh.close()
        _assert_same_results(_grad_all(pop, X), want, "de_program_update")
    finally:
        pop.close()


def test_cse_program_equals_the_program_of_its_expanded_tapes(api):
    """GraphNode trees (de_program_create_cse): with the bit the gradient program is lowered from the expanded tape, so the rows are those
    of the expanded trees, every occurrence of a shared constant with its own partial (summed per shared constant by the caller)."""
    G = de.GraphNode
    ops = BENCH_OPS
    b = lambda name, l, r: G(ops.index(name, 2), l, r)   # noqa: E731
    trees = []
    for k in range(6):
        c = G(val=0.5 + 0.25 * k)
        shared = b("*", G(feature=1 + k % 5), c)
        inner = G(ops.index("cos", 1), b("+", shared, G(feature=2)))
        trees.append(b("-", b("*", inner, shared), b("/", c, b("+", G(feature=3), G(val=4.0)))))
    X = np.asfortranarray(de.synth.random_X(5, 500, seed=8).astype(H))
    pc = pop_of(api, trees, ops, 5, full_eval=True)
    pe = pop_of(api, [de.break_sharing(t) for t in trees], ops, 5, full_eval=True)
    try:
        assert pc._occ is not None
        for mname, (variable, mode) in MODES.items():
            oc, gc, okc = pc.eval_grad(X, variable)
            oe, ge, oke = pe.eval_grad(X, variable)
            assert np.array_equal(okc, oke) and same(oc, oe).all(), mname
            for t in range(len(trees)):
                want = pc._combine_rows(t, ge[t], mode)
                assert gc[t].shape == want.shape and same(gc[t], want).all(), (mname, t)
        assert same(pc.eval(X)[0], pe.eval(X)[0]).all()
    finally:
        pc.close(), pe.close()


# ---- 8. scope of the bit --------------------------------------------------------------------------------------------------------------
def test_scope_of_the_bit(api):
    lib = api.library()
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    tree = de.Node(1, de.Node(feature=1), de.Node(val=0.5))
    N = 16
    X = np.asfortranarray(np.ones((1, N), dtype=H))
    y = np.ones(N, dtype=H)
    off = np.zeros(1, dtype=np.int64)
    pop = pop_of(api, [tree], ops, 1)
    plain = pop_of(api, [tree], ops, 1, half_grad=False)
    try:
        ctx, p = pop.ctx._h, pop._h
        bufs = [np.full(64, 7, dtype=np.uint8) for _ in range(4)]
        ptr = [b_.ctypes.data for b_ in bufs]
        calls = {
            "de_eval_pullback_dX": lambda: lib.de_eval_pullback_dX(ctx, p, X.ctypes.data, N, 1, None, y.ctypes.data, ptr[0], None, ptr[2]),
            "de_eval_loss": lambda: lib.de_eval_loss(ctx, p, X.ctypes.data, N, 1, None, y.ctypes.data, None, 0, ptr[0], ptr[2]),
            "de_eval_loss_grad": lambda: lib.de_eval_loss_grad(ctx, p, X.ctypes.data, N, 1, None, 1, y.ctypes.data, None, 0, ptr[0], ptr[1], None, ptr[2]),
            "de_fit_consts_bfgs": lambda: lib.de_fit_consts_bfgs(ctx, p, X.ctypes.data, N, 1, None, y.ctypes.data, None, None, None, ptr[0], ptr[2],
                                                                 ptr[3], ptr[1]),
        }
        for name, call in calls.items():
            rc = call()
            assert rc == 7, (name, rc)
            assert "F16" in lib.de_last_error(ctx).decode(), name
            assert all((b_ == 7).all() for b_ in bufs), f"{name} wrote an output"
        for meth, args in (("eval_loss", (X, y)), ("eval_loss_grad", (X, y)), ("eval_pullback_dX", (X, y)), ("fit_constants_bfgs_device", (X, y))):
            with pytest.raises(api.DeviceError, match="DE_ERR_UNSUPPORTED"):
                getattr(pop, meth)(*args)
        # without the bit: as before
        rc = lib.de_eval_grad(plain.ctx._h, plain._h, X.ctypes.data, N, 1, None, 0, ptr[0], N, ptr[1], off.ctypes.data, ptr[2])
        assert rc == 7 and "no binary16 gradients" in lib.de_last_error(plain.ctx._h).decode()
        assert all((b_ == 7).all() for b_ in bufs)
        with pytest.raises(api.DeviceError, match="DE_ERR_UNSUPPORTED"):
            plain.eval_grad(X)
        # with it
        out, grads, ok = pop.eval_grad(X, "both")
        assert ok[0] and (out[0] == H(1.5)).all() and (np.asarray(grads[0]) == H(1)).all()
    finally:
        pop.close(), plain.close()
    # a Float32 program ignores the bit
    trees, bops = _population("bench", 16, 5)
    X32 = np.asfortranarray(de.synth.random_X(5, 500, seed=2).astype(np.float32))
    a = pop_of(api, trees, bops, 5, dtype=np.float32)
    b = pop_of(api, trees, bops, 5, dtype=np.float32, half_grad=False)
    try:
        ra, rb = a.eval_grad(X32, "both"), b.eval_grad(X32, "both")
        assert np.array_equal(ra[2], rb[2])
        for t in np.flatnonzero(ra[2]):
            assert np.array_equal(ra[0][t].view(np.uint32), rb[0][t].view(np.uint32))
            assert np.array_equal(np.ascontiguousarray(ra[1][t]).view(np.uint32), np.ascontiguousarray(rb[1][t]).view(np.uint32))
    finally:
        a.close(), b.close()


# ---- 9. the reference's acceptance on the device --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_reference_acceptance_on_the_device(api, seed):
    """test/test_derivatives.jl:40-144 for Float16: equations 1, 2 (variables; eval_grad and eval_diff per feature) and 4, 5 (constants)
    against the float64 closed forms, isapprox(rtol = 0.1) on the norm."""
    X = fg.acceptance_X(seed)
    X64 = X.astype(np.float64)
    for name, tree, ops, mode, closed in fg.acceptance_cases():
        pop = pop_of(api, [tree], ops, 3)
        try:
            _, grads, ok = pop.eval_grad(X, mode == fg.VARIABLE)
            assert ok[0], (name, seed)
            want = closed(X64)
            good, err = fg.isapprox_norm(grads[0], want)
            print(f"[f16 grad] device, {name} seed {seed}: relative norm error {err:.4f}")
            assert good, (name, seed, err)
            assert not fg.isapprox_norm(np.zeros_like(want), want)[0]
            if mode == fg.VARIABLE:
                rows = np.stack([pop.eval_diff(X, d + 1)[1][0] for d in range(3)])
                assert fg.isapprox_norm(rows, want)[0] and same(rows, grads[0]).all(), name
        finally:
            pop.close()
