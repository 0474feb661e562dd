"""DE_F16 (Float16) evaluation on the MI355X (csrc/de_half.hip): the reference's Float16 known answers, seeded random populations
against the Float16 CPU oracle (tests/oracle_f16/), the binary16 step semantics against the Float32 library, bit-equality across the
program's paths, the binary16 edges, the sum certificate and the entry points that refuse Float16.  Run with `pytest -m gpu`.
DESIGN.md §13."""
import json
import os

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
from helpers import case_tree
import f16_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_known_answers_f16.json")))["cases"]
H = np.float16

IEEE_OPS = de.OperatorEnum(binary_operators=("+", "-", "*", "/"))
BENCH_OPS = de.synth.BENCH_OPERATORS
WIDE_OPS = de.OperatorEnum(binary_operators=("+", "-", "*", "/", "max", "min", "pow_abs2", "greater"),
                           unary_operators=("cos", "sin", "exp", "safe_log", "safe_sqrt", "square", "cube", "abs", "neg", "tanh", "relu",
                                            "custom_cos"))
# the rest of the table: the ternary rows, mod / rem / ^, more one-rounding transcendentals, the composites cube and inv
TERN_OPS = de.OperatorEnum(binary_operators=("+", "-", "*", "/", "mod", "rem", "^"),
                           unary_operators=("log", "exp2", "tan", "sqrt", "cube", "sin", "inv", "atan"),
                           ternary_operators=("fma", "clamp", "+", "max"))
OPSETS = {"ieee": IEEE_OPS, "bench": BENCH_OPS, "wide": WIDE_OPS, "ternary": TERN_OPS}


def _population(opset, n, seed):
    ops = OPSETS[opset]
    trees = de.synth.random_population(n, seed=seed, node_count=12, nfeatures=5, operators=ops)
    if opset == "ternary":  # (the generator draws no ternary nodes: every tree becomes op3(tree, a smaller tree, a leaf))
        small = de.synth.random_population(n, seed=seed + 1, node_count=4, nfeatures=5, operators=ops)
        names = ("fma", "clamp", "+", "max")
        leaves = [de.Node(feature=1 + t % 5) if t % 3 else de.Node(val=0.5 + 0.25 * (t % 7)) for t in range(n)]
        trees = [de.Node(ops.index(names[t % 4], 3), trees[t], small[t], leaves[t]) for t in range(n)]
    return trees, ops


def f16_tolerance(tree, ops, X, options, draws=16, seed=0):
    """The tolerance model of helpers.parity_tolerance restated for binary16: the tree re-evaluated in float64 (tests/prog_interp.py)
    with every operator result perturbed by +-1 binary16 ulp (2^-10, random sign and a magnitude in [1/4, 1]) and overflowing at 65504 as
    binary16 does; tolerance = 1 binary16 ulp (2^-10 |y|) + 8 x the spread of the draws.  Samples whose selection operators (max, min,
    greater, clamp, abs at 0, ...) flip under the perturbations, whose float64 value is not finite, or whose spread exceeds |y| / 8
    (binary16's ulp is 1e-3 relative: helpers' 1e-3 |y| chaos bound would be one rounding) are ILL-CONDITIONED: +inf, compared on the
    flag only.  Returns (tolerance, ill-conditioned mask)."""
    from dynamicexpressions_jl_amd import api
    from helpers import unstable_selections
    import prog_interp
    tape, consts = de.flatten(tree, ops, H)
    words, _ = api.lower_tape(tape, consts.astype(np.float64), X.shape[0], 0, options, np.float64)
    X64 = np.asarray(X, dtype=np.float64)
    rng = np.random.Generator(np.random.PCG64(seed))
    with np.errstate(all="ignore"):
        sel_clean, sel_noisy = [], []
        clean, _ = prog_interp.run(words, X64, bool(options & 1), select_log=sel_clean, overflow_at=65504.0)
        spread = np.zeros(X64.shape[1])
        for _ in range(draws):
            sel_noisy.append([])
            noisy, _ = prog_interp.run(words, X64, bool(options & 1), noise_eps=2.0 ** -10, rng=rng, select_log=sel_noisy[-1], overflow_at=65504.0)
            d = np.abs(noisy - clean)
            spread = np.maximum(spread, np.where(np.isfinite(d), d, np.inf))
        ill = unstable_selections(sel_clean, sel_noisy, X64.shape[1]) | ~np.isfinite(clean) | ~(spread <= np.abs(clean) / 8)
        tol = 2.0 ** -10 * np.abs(clean) + 2.0 ** -24 + 8.0 * spread
    return np.where(ill, np.inf, tol), ill


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


def ord16(a):
    """binary16 bits -> integers that order like the values (ulp distance = difference)."""
    u = np.asarray(a, dtype=H).view(np.uint16).astype(np.int64)
    return np.where(u & 0x8000, -(u & 0x7FFF), u)


def same_bits(a, b):
    """equal binary16 values, NaN == NaN (sign and payload of a NaN are not compared: DESIGN.md §5)"""
    a, b = np.asarray(a, dtype=H), np.asarray(b, dtype=H)
    return (a.view(np.uint16) == b.view(np.uint16)) | (np.isnan(a) & np.isnan(b))


def ctx_of(api, case):
    o = case.get("options", {})
    return api.EvalContext(early_exit=o.get("early_exit", True), use_fused=o.get("use_fused", True), bumper=o.get("bumper", False))


# ---------------------------------------------------------------------------------------------------------------- golden Float16 cases
@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_golden_f16_on_gpu(api, case):
    tree, ops = case_tree(case)
    X = np.asfortranarray(np.asarray(case["X"], dtype=np.float64).astype(H))
    out, ok = api.eval_tree_array(tree, X, ops, eval_context=ctx_of(api, case))
    exp = case["expect"]
    assert out.dtype == H
    assert ok == exp["ok"], f"{case['name']} ({case['cite']})"
    if ok and "y" in exp:
        want = np.asarray(exp["y"], dtype=np.float64)
        got = out.astype(np.float64)
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), fin), case["name"]
        assert np.all(np.abs(got[fin] - want[fin]) <= exp.get("atol", 0) + exp.get("rtol", 0) * np.abs(want[fin])), case["name"]


# ---------------------------------------------------------------------------------------------------------------- random populations
MODES = {"early_exit": dict(), "no_early_exit": dict(early_exit=False), "full_eval": dict(full_eval=True)}


@pytest.mark.parametrize("N", [1, 63, 1000, 4097])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("opset", list(OPSETS))
def test_random_population_matches_f16_oracle(api, f16o, opset, mode, N):
    import torch
    seed = 1000 + 7 * N + len(mode) + len(opset)
    trees, ops = _population(opset, 48, seed)
    X = de.synth.random_X(5, N, seed=seed).astype(H)
    ectx = api.EvalContext(**MODES[mode])
    pop = api.Population(trees, ops, H, n_features=5, eval_context=ectx)
    out_h, ok_h = pop.eval(np.asfortranarray(X))
    # device buffers with ldX > F: [N, F + 3] storage viewed as [F + 3, N], the first F rows
    Xs = torch.zeros((N, 8), dtype=torch.float16, device="cuda")
    Xs[:, :5] = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    Xd = Xs.t()[:5]
    assert Xd.stride(1) == 8
    out_d, ok_d = pop.eval(Xd)
    torch.cuda.synchronize()
    out_d, ok_d = out_d.cpu().numpy(), ok_d.cpu().numpy()
    opts = ectx.option_bits(ops)
    n_cmp = n_ulp1 = n_far = n_ill = sum_flips = 0
    far_trees = []
    for t, tree in enumerate(trees):
        tape, consts = de.flatten(tree, ops, H)
        y, okr = f16o.eval_tree_array(tape, consts, X, opts, elementwise=True)
        _, oks = f16o.eval_tree_array(tape, consts, X, opts, elementwise=False)
        sum_flips += int(oks != okr)
        assert bool(ok_h[t]) == okr, f"{opset}/{mode}/N={N}: flag of tree {t} ({de.string_tree(tree, ops)})"
        assert bool(ok_d[t]) == okr
        if not okr:  # (the rows of an incomplete tree are unspecified, as the reference's buffer after its return: the oracle's stop
            continue  # where its exit did — with early_exit = false too, when a constant subtree failed — the device's full_eval rows go on)
        assert same_bits(out_h[t], out_d[t]).all(), f"tree {t}: host and device buffers differ"
        if opset == "ieee":
            assert same_bits(out_h[t], y).all(), f"tree {t} ({de.string_tree(tree, ops)}): + - * / rows must be bit-equal"
            n_cmp += N
            continue
        both = np.isfinite(y) & np.isfinite(out_h[t].astype(np.float32))
        d = np.abs(ord16(out_h[t]) - ord16(y))
        close = np.where(both, d <= 1, same_bits(out_h[t], y) | (np.isinf(y) & (out_h[t] == y)))
        n_cmp += N
        n_ulp1 += int(close.sum())
        n_far += int((~close).sum())
        if (~close).any():
            # the samples beyond 1 ulp: within the tolerance model (or ill-conditioned there, where only the flag is compared)
            far = np.nonzero(~close)[0]
            tol, ill = f16_tolerance(tree, ops, X[:, far], opts)
            err = np.abs(out_h[t][far].astype(np.float64) - y[far].astype(np.float64))
            bad = ~ill & ~(err <= tol)
            n_ill += int(ill.sum())
            assert not bad.any(), (f"tree {t} ({de.string_tree(tree, ops)}): samples {far[bad][:5].tolist()} outside the tolerance model: "
                                   f"device {out_h[t][far[bad][:5]]!r} oracle {y[far[bad][:5]]!r} tol {tol[bad][:5]!r}")
            if len(far_trees) < 3:
                j = int(far[0])
                far_trees.append(f"tree {t} {de.string_tree(tree, ops)}: sample {j} x={X[:, j].tolist()} device {out_h[t][j]!r} oracle {y[j]!r}")
    print(f"[f16 {opset}/{mode}/N={N}] {n_cmp} samples compared, {n_far} beyond 1 binary16 ulp ({n_ill} of them ill-conditioned), "
          f"{sum_flips} trees whose isfinite(sum) flag differs from the element-wise flag")
    if opset != "ieee" and n_cmp:
        assert n_ulp1 >= 0.999 * n_cmp, f"{n_far} of {n_cmp} samples beyond 1 binary16 ulp: " + "; ".join(far_trees)


# ---------------------------------------------------------------------------------------------------------------- steps vs the Float32 library
ONE_ROUNDING_UNARY = ["neg", "abs", "square", "relu", "sign", "round", "floor", "ceil", "inv", "sqrt", "cbrt", "exp", "exp2", "log", "log2",
                      "log10", "log1p", "sin", "cos", "tan", "sinh", "cosh", "tanh", "asin", "acos", "atan", "asinh", "acosh", "atanh",
                      "safe_log", "safe_log2", "safe_log10", "safe_log1p", "safe_sqrt", "safe_acosh", "gamma"]
ONE_ROUNDING_BINARY = ["+", "-", "*", "/", "^", "max", "min", "mod", "rem", "greater"]


def _xs16(n, seed):
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.standard_normal(n // 2) * 3, rng.uniform(-12, 12, n // 4), rng.uniform(0, 1.5, n - n // 2 - n // 4)])
    x[:10] = [0.0, -0.0, 1.0, -1.0, 0.5, 2.0 ** -24, 65504.0, -65504.0, 11.0, 1e-3]
    return x.astype(H)


@pytest.mark.parametrize("kind", ["unary", "binary"])
def test_one_rounding_opcodes_equal_round16_of_f32(api, kind):
    """An opcode that is one rounding in Julia's Float16 methods gives round16(the Float32 library's value) on the same binary16 inputs."""
    names = ONE_ROUNDING_UNARY if kind == "unary" else ONE_ROUNDING_BINARY
    ops = de.OperatorEnum(unary_operators=tuple(names)) if kind == "unary" else de.OperatorEnum(binary_operators=tuple(names))
    x1, x2 = de.Node(feature=1), de.Node(feature=2)
    trees = [de.Node(i + 1, x1) if kind == "unary" else de.Node(i + 1, x1, x2) for i in range(len(names))]
    X = np.stack([_xs16(4096, 1), _xs16(4096, 2)])
    ectx = api.EvalContext(early_exit=False)
    o16, _ = api.Population(trees, ops, H, n_features=2, eval_context=ectx).eval(np.asfortranarray(X))
    o32, _ = api.Population(trees, ops, np.float32, n_features=2, eval_context=ectx).eval(np.asfortranarray(X.astype(np.float32)))
    with np.errstate(over="ignore", invalid="ignore"):
        r32 = o32.astype(H)
    bad = {names[t]: int((~same_bits(o16[t], r32[t])).sum()) for t in range(len(names))}
    print(f"[f16 steps {kind}] mismatches against round16(Float32): {bad}")
    assert not any(bad.values()), bad


# ---------------------------------------------------------------------------------------------------------------- paths agree bit for bit
def _folding_population():
    ops = WIDE_OPS
    trees = de.synth.random_population(40, seed=77, node_count=14, nfeatures=3, operators=ops)
    x1, x2 = de.Node(feature=1), de.Node(feature=2)
    U, B = lambda n, a: de.Node(ops.index(n, 1), a), lambda n, a, b: de.Node(ops.index(n, 2), a, b)
    c = lambda v: de.Node(val=v)  # noqa: E731
    trees += [B("+", U("cos", B("*", c(2.0), c(3.1))), x1),                    # device-folded (auxiliary program): cos of a constant product
              B("*", B("/", c(1.0), c(3.0)), x2),                               # host-folded: + - * / only
              B("-", U("exp", B("pow_abs2", c(1.7), c(2.3))), U("square", x1)),
              B("*", B("*", c(300.0), c(300.0)), x1),                           # a folded subtree that is Inf in binary16
              U("custom_cos", B("+", U("cube", c(2.5)), x2))]
    return trees, ops


def test_set_consts_equals_fresh_create(api):
    trees, ops = _folding_population()
    X = np.asfortranarray(de.synth.random_X(3, 777, seed=5).astype(H))
    pop = api.Population(trees, ops, H, n_features=3)
    _, _, consts, _ = de.flatten_population(trees, ops, H)
    new = (consts.astype(np.float32) * 1.5 + 0.25).astype(H)
    pop.set_constants(new)
    o1, k1 = pop.eval(X)
    fresh = [t.copy() for t in trees]
    k = 0
    for t in fresh:
        _, refs = de.get_scalar_constants(t)
        for r in refs:
            r.val = float(new[k])
            k += 1
    assert k == len(new)
    o2, k2 = api.Population(fresh, ops, H, n_features=3).eval(X)
    assert np.array_equal(k1, k2)
    for t in range(len(trees)):
        if k1[t]:
            assert same_bits(o1[t], o2[t]).all(), t


def test_no_fold_equals_fold(api, monkeypatch):
    trees, ops = _folding_population()
    X = np.asfortranarray(de.synth.random_X(3, 1500, seed=6).astype(H))
    for ectx in (api.EvalContext(), api.EvalContext(early_exit=False)):
        o1, k1 = api.Population(trees, ops, H, n_features=3, eval_context=ectx).eval(X)
        monkeypatch.setenv("DE_NO_FOLD", "1")
        o2, k2 = api.Population(trees, ops, H, n_features=3, eval_context=ectx).eval(X)
        monkeypatch.delenv("DE_NO_FOLD")
        assert np.array_equal(k1, k2)
        for t in range(len(trees)):
            if k1[t]:
                assert same_bits(o1[t], o2[t]).all(), (t, de.string_tree(trees[t], ops))


def test_program_hooks_accept_f16(api):
    trees, ops = _folding_population()
    pop = api.Population(trees, ops, H, n_features=3)
    pop.verify()
    assert pop.stream_hash() != 0
    assert pop.dump(0).shape[0] > 0
    pl = pop.plan(10**6)  # de_half.hip's launch: 1024-sample tiles, chunks of <= 63 trees
    assert pl["tile"] == 1024 and pl["trees_per_chunk"] <= 63 and pl["n_chunks"] * pl["trees_per_chunk"] >= len(trees)
    assert api.library().de_program_dump(pop._h, 0, None, 0, 3) == 0  # no threaded (fused) form: F16 never runs that kernel


def test_cse_tape_equals_expanded_tape(api):
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))

    def build(cls):
        s = cls(1, cls(2, cls(feature=1), cls(val=0.75)))
        return cls(1, s, cls(2, s, s)), s

    dag, _ = build(de.GraphNode)
    expanded = de.Node(1, de.Node(1, de.Node(2, de.Node(feature=1), de.Node(val=0.75))),
                       de.Node(2, de.Node(1, de.Node(2, de.Node(feature=1), de.Node(val=0.75))),
                               de.Node(1, de.Node(2, de.Node(feature=1), de.Node(val=0.75)))))
    X = np.asfortranarray(np.linspace(-40, 40, 1029)[None, :].astype(H))
    ya, oka = api.eval_tree_array(dag, X, ops)
    yb, okb = api.eval_tree_array(expanded, X, ops)
    assert oka and okb
    assert same_bits(ya, yb).all()


def test_parametric_population_matches_oracle(api, f16o):
    ops = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
    P = de.ParametricNode
    p1, p2, x1, x2 = P(parameter=1), P(parameter=2), P(feature=1), P(feature=2)
    trees = [P(1, P(3, p1, x1), P(1, P(2, p2, x2))),                 # p1 * x1 + cos(p2 - x2)
             P(3, P(2, P(1, x1, p2), P(val=0.3)), p1),                # ((x1 + p2) - 0.3) * p1
             P(4, x2, P(2, P(3, p1, x1)))]                            # x2 / exp(p1 * x1)
    rng = np.random.default_rng(3)
    N = 2049
    X = (rng.standard_normal((2, N)) * 2).astype(H)
    params = (rng.standard_normal((2, 3)) * 1.5).astype(H)
    classes = rng.integers(1, 4, N)
    pop = api.Population(trees, ops, H, n_features=2, n_params=2)
    out, ok = pop.eval(np.asfortranarray(X), params=params, classes=classes)
    for t, tree in enumerate(trees):
        tape, consts = de.flatten(tree, ops, H)
        y, okr = f16o.eval_tree_array_parametric(tape, consts, X, params, classes, 1, 7, elementwise=True)
        assert bool(ok[t]) == okr, t
        if okr:
            d = np.abs(ord16(out[t]) - ord16(y))
            assert np.mean(d <= 1) >= 0.999 and (t != 1 or (d == 0).all()), (t, int(d.max()))


# ---------------------------------------------------------------------------------------------------------------- binary16 edges
def test_subnormals_and_overflow_edges(api):
    sub = 2.0 ** -24
    xs = np.array([sub, -sub, 3 * sub, 2.0 ** -14, 2.0 ** -15, 32752.0, 32760.0, 65504.0, -65504.0, 1.0], dtype=H)
    X = np.asfortranarray(xs[None, :])
    ops = de.OperatorEnum(binary_operators=("+", "*", "/", "-"))
    x1 = de.Node(feature=1)
    with np.errstate(over="ignore"):  # (32760 + 32760 = 65520 is Inf in binary16: expected)
        cases = [(x1, xs), (de.Node(2, x1, de.Node(val=0.5)), xs * H(0.5)), (de.Node(1, x1, x1), xs + xs),
                 (de.Node(3, x1, de.Node(val=1024.0)), xs / H(1024.0)), (de.Node(4, x1, de.Node(val=sub)), xs - H(sub))]
    for tree, want in cases:
        y, ok = api.eval_tree_array(tree, X, ops, eval_context=api.EvalContext(early_exit=False))
        with np.errstate(over="ignore"):
            want = np.asarray(want, dtype=H)
        assert same_bits(y, want).all(), (de.string_tree(tree, ops), y, want)
        _, ok_ee = api.eval_tree_array(tree, X, ops)
        assert ok_ee == bool(np.all(np.isfinite(want))), de.string_tree(tree, ops)
    # the largest finite sum: 32752 + 32752 = 65504 is finite; 32760 + 32760 = 65520 rounds to Inf and clears the flag
    _, ok = api.eval_tree_array(de.Node(1, x1, x1), np.asfortranarray(np.array([[32752.0]], dtype=H)), ops)
    assert ok
    y, ok = api.eval_tree_array(de.Node(1, x1, x1), np.asfortranarray(np.array([[32760.0]], dtype=H)), ops,
                                eval_context=api.EvalContext(early_exit=False))
    assert np.isposinf(y[0])
    _, ok = api.eval_tree_array(de.Node(1, x1, x1), np.asfortranarray(np.array([[32760.0]], dtype=H)), ops)
    assert not ok


# ---------------------------------------------------------------------------------------------------------------- certificate, refusals
def test_sum_certificate_flags_a_float16_sum_overflow(api):
    ops = de.OperatorEnum(binary_operators=("*",))
    x1 = de.Node(feature=1)
    trees = [x1, de.Node(1, x1, de.Node(val=0.001))]
    X = np.asfortranarray(np.full((1, 4), 30000.0, dtype=H))  # every element finite, their Float16 sum 120000 is not
    pop = api.Population(trees, ops, H, n_features=1)
    ok, cert, mx = pop.sum_certificate(X)
    assert ok.tolist() == [True, True]
    assert cert.tolist() == [False, True]
    assert mx[0] == 30000.0
    spop = api.Population(trees, ops, H, n_features=1, eval_context=api.EvalContext(strict_flags=True))
    out, ok = spop.eval(X)
    assert ok.all() and spop.uncertified.tolist() == [0]
    with pytest.raises(api.UncertifiedFlag):
        api.eval_tree_array(x1, X, ops, eval_context=api.EvalContext(strict_flags=True))


@pytest.mark.parametrize("N, v, certified", [(2049, 31.90625, False),   # N * max = 65375 < 65504, but every Float16 order of the sum is Inf
                                             (89243, 0.7, False),       # N * max = 0.954 * 65504: overflows in a pairwise Float16 sum
                                             (1024, 38.0, True)])       # N * max * (1 + 2^-11)^1032 = 64398 < 65504: provably finite
def test_sum_certificate_margin_is_a_binary16_one(api, N, v, certified):
    ops = de.OperatorEnum(binary_operators=("*",))
    tree = de.Node(1, de.Node(feature=1), de.Node(val=1.0))  # x1 * 1
    X = np.asfortranarray(np.full((1, N), v, dtype=H))
    # the sums themselves, in binary16: sequentially and pairwise in blocks of 1024 (Base.pairwise_blocksize)
    def pairwise(x):
        if len(x) <= 1024:
            s_ = H(0)
            for e in x:
                s_ = H(s_ + e)
            return s_
        h = len(x) // 2
        return H(pairwise(x[:h]) + pairwise(x[h:]))
    with np.errstate(over="ignore"):
        assert np.isfinite(pairwise(X[0])) == certified
    ok, cert, _ = api.Population([tree], ops, H, n_features=1).sum_certificate(X)
    assert ok[0]
    assert bool(cert[0]) == certified


def test_wide_feature_matrix_gathers_features(api, f16o):
    """40 features do not fit the LDS tile: the binary16 kernel gathers them from global memory (the Float32 flat kernel's `direct` case),
    constant subtrees through the auxiliary program included."""
    import torch
    ops = WIDE_OPS
    F, N = 40, 3000
    trees = de.synth.random_population(40, seed=91, node_count=14, nfeatures=F, operators=ops)
    x = lambda f: de.Node(feature=f)  # noqa: E731
    trees.append(de.Node(ops.index("+", 2), de.Node(ops.index("cos", 1), de.Node(ops.index("*", 2), de.Node(val=2.0), de.Node(val=3.1))), x(37)))
    X = de.synth.random_X(F, N, seed=92).astype(H)
    pop = api.Population(trees, ops, H, n_features=F)
    out, ok = pop.eval(np.asfortranarray(X))
    assert "direct" in pop.ctx.last_kernel_name()
    Xd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()
    out_d, ok_d = pop.eval(Xd)
    torch.cuda.synchronize()
    assert np.array_equal(ok, ok_d.cpu().numpy())
    n_far = n_cmp = 0
    for t, tree in enumerate(trees):
        tape, consts = de.flatten(tree, ops, H)
        y, okr = f16o.eval_tree_array(tape, consts, X, 7, elementwise=True)
        assert bool(ok[t]) == okr, t
        if okr:
            assert same_bits(out[t], out_d.cpu().numpy()[t]).all()
            d = np.abs(ord16(out[t]) - ord16(y))
            n_far += int((~((d <= 1) | same_bits(out[t], y))).sum())
            n_cmp += N
    assert n_cmp and n_far <= 0.001 * n_cmp, (n_far, n_cmp)


def test_unsupported_entry_points_return_7_and_leave_outputs_untouched(api):
    lib = api.library()
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    tree = de.Node(1, de.Node(feature=1), de.Node(val=0.5))
    pop = api.Population([tree], ops, H, n_features=1)
    N = 16
    X = np.asfortranarray(np.ones((1, N), dtype=H))
    y = np.ones(N, dtype=H)
    ctx, p = pop.ctx._h, pop._h
    bufs = [np.full(64, 7, dtype=np.uint8) for _ in range(5)]
    ptr = [b.ctypes.data for b in bufs]
    off = np.zeros(1, dtype=np.int64)
    starts = np.array([0, N], dtype=np.int64)
    calls = {
        "de_eval_grad": lambda: lib.de_eval_grad(ctx, p, X.ctypes.data, N, 1, None, 0, ptr[0], N, ptr[1], None, ptr[2]),
        "de_eval_diff": lambda: lib.de_eval_diff(ctx, p, X.ctypes.data, N, 1, 0, ptr[0], ptr[1], N, ptr[2]),
        "de_eval_pullback_dX": lambda: lib.de_eval_pullback_dX(ctx, p, X.ctypes.data, N, 1, None, y.ctypes.data, ptr[0], None, ptr[2]),
        "de_eval_loss": lambda: lib.de_eval_loss(ctx, p, X.ctypes.data, N, 1, None, y.ctypes.data, None, 0, ptr[0], ptr[2]),
        "de_eval_loss_grad": lambda: lib.de_eval_loss_grad(ctx, p, X.ctypes.data, N, 1, None, 1, y.ctypes.data, None, 0, ptr[0],
                                                            ptr[1], None, ptr[2]),
        "de_eval_loss_grad_by_class": lambda: lib.de_eval_loss_grad_by_class(ctx, p, X.ctypes.data, N, 1, None, 0, y.ctypes.data, None,
                                                                              0, starts.ctypes.data, ptr[0], ptr[1], off.ctypes.data,
                                                                              ptr[3], ptr[2]),
        "de_ctx_declare_dataset": lambda: lib.de_ctx_declare_dataset(ctx, 2, ptr[4], N, 1, 1),
    }
    for name, call in calls.items():
        rc = call()
        assert rc == 7, (name, rc)
        assert "F16" in lib.de_last_error(ctx).decode(), name
        assert all((b == 7).all() for b in bufs), f"{name} wrote an output"
    for meth, args in (("eval_grad", (X,)), ("eval_diff", (X, 1)), ("eval_loss", (X, y)), ("eval_loss_grad", (X, y)),
                       ("eval_pullback_dX", (X, y))):
        with pytest.raises(api.DeviceError, match="DE_ERR_UNSUPPORTED"):
            getattr(pop, meth)(*args)
    # the evaluation itself works on the same program
    out, ok = pop.eval(X)
    assert ok[0] and (out[0] == H(1.5)).all()
