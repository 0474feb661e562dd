"""GPU tests of the LOSS variant of the flat-switch interpreter (csrc/de_flat.h): de_eval_loss / de_eval_loss_ex for
Float32 / Float64 programs that do not run the threaded kernel (DE_EVAL_THREADED=0, a feature matrix too wide for its tile), and —
created with DE_OPT_TYPED_LOSS — for Float16 and complex programs.

In every comparison the reference (tests/typed_loss_reference.py) is formed from the DEVICE's own `Population.eval` rows of the same trees
and X — code the other test files hold to the oracles — so what is under test is the loss arithmetic and the reduction: the design of
tests/test_gpu_loss_kinds.py, whose tolerance model is used here too (eps = the element type's, or the component type's):
  real      64 eps sum_j w_j (l_j + |l'_j z_j|) + tiny        z = e, the margin a for the margin kinds (derived in test_gpu_loss_kinds.py)
  complex   64 eps sum_j w_j (l_j + |e_j| |dl/d|e_j||) + tiny  the same model: each component of e is rounded once in T
  binary16  64 * 2^-23 * sum of the kept terms                 every term is >= 0 and exact in binary16 (it is formed with the steps of
                                                              the reference helper, bit for bit), so the only error is the Float32
                                                              accumulation: 4 + 6 + 2 additions at most on any path, in double beyond"""
import ctypes as C

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import typed_loss_reference as ref
from loss_reference import KINDS, MARGIN, PARAMS

pytestmark = pytest.mark.gpu
H = np.float16
ALL_KINDS = ["L2", "L1"] + sorted(KINDS)
REAL_OF = {np.dtype(np.complex64): np.float32, np.dtype(np.complex128): np.float64}
FLAT_TILE = {np.dtype(np.float32): 1024, np.dtype(np.float64): 512, np.dtype(H): 1024, np.dtype(np.complex64): 512, np.dtype(np.complex128): 256}
CBENCH = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
F16_WIDE_OPS = de.OperatorEnum(binary_operators=("+", "-", "*", "/", "max", "min", "pow_abs2", "greater"),
                               unary_operators=("cos", "sin", "exp", "safe_log", "safe_sqrt", "square", "cube", "abs", "neg", "tanh", "relu",
                                                "custom_cos"))


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _api.library()
    return _api


def targets(kind, N, dtype, seed):
    """tests/test_gpu_loss_kinds.py `targets`: continuous random targets; the margin kinds get labels of either sign with |y| in [1, 1.5)."""
    g = np.random.Generator(np.random.PCG64(seed))
    y = g.standard_normal(N)
    if kind in MARGIN:
        y = np.where(y > 0, 1.0, -1.0) * (1.0 + 0.5 * g.random(N))
    return y.astype(dtype)


def weights_with_zeros(N, dtype, seed):
    w = np.random.Generator(np.random.PCG64(seed)).uniform(0, 2, N).astype(dtype)
    w[::7] = 0
    return w


def kernel_name(pop):
    return pop.ctx.last_kernel_name()


# ---- 1 / 2: Float32 and Float64 on the flat-switch interpreter ------------------------------------------------------------------------
def check_real(pop, X, out, ok_eval, y, w, kind, dtype, min_ok, **kw):
    """tests/test_gpu_loss_kinds.py check_kind_losses, with L2 and L1 among the kinds."""
    p = PARAMS.get(kind, 0.0)
    loss, ok = pop.eval_loss(X, y, weights=w, loss=kind, loss_param=p, **kw)
    assert "loss" in kernel_name(pop), kernel_name(pop)
    assert np.array_equal(ok, ok_eval), "fused loss and plain eval disagree on the completion flags"
    assert loss.dtype == np.dtype(dtype)
    eps, fmax, tiny = np.finfo(dtype).eps, float(np.finfo(dtype).max), float(np.finfo(dtype).tiny) * X.shape[1]
    n_ok, worst = 0, 0.0
    for t in range(len(ok)):
        if not ok[t]:
            assert np.isnan(loss[t]), f"tree {t}: incomplete evaluation must give a NaN loss"
            continue
        n_ok += 1
        want, mag, big = ref.real_loss(kind, out[t].astype(np.float64), y, w, p)
        if np.isnan(want):  # complete does not promise finite values (untested leaves)
            assert np.isnan(loss[t])
            continue
        assert loss[t] >= 0 or np.isnan(loss[t])
        if not np.isfinite(mag) or max(want, big, mag) > 0.25 * fmax:  # a term or the sum overflows T
            assert np.isposinf(loss[t]) or abs(float(loss[t]) - want) <= 64 * eps * mag
            continue
        err = abs(float(loss[t]) - want)
        worst = max(worst, err / (eps * mag + tiny))
        assert err <= 64 * eps * mag + tiny, (kind, t, loss[t], want, err / (eps * mag + tiny))
    assert n_ok >= min_ok, (n_ok, min_ok)
    return worst


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_real_flat_kernel_loss(api, monkeypatch, kind, dtype):
    """DE_EVAL_THREADED=0: every kind x {Float32, Float64} x {no weights, weights with zeros} x N in {1, 63, tile, tile + 1, 4099}.
    (Status 7, "de_eval_loss needs the LDS-tiled kernel", before the flat-switch interpreter had a loss variant.)"""
    monkeypatch.setenv("DE_EVAL_THREADED", "0")
    ops = de.synth.BENCH_OPERATORS
    trees = de.synth.random_population(150, seed=0xDE02, dtype=dtype)
    pop = api.Population(trees, ops, dtype, n_features=5)
    tile = FLAT_TILE[np.dtype(dtype)]
    worst = 0.0
    for N in (1, 63, tile, tile + 1, 4099):
        X = de.synth.random_X(5, N, seed=1, dtype=dtype)
        out, ok_eval = pop.eval(X)
        assert kernel_name(pop) == "de_eval_tape_kernel"
        y = targets(kind, N, dtype, seed=N)
        w = weights_with_zeros(N, dtype, N + 1)
        for weights in (None, w):
            worst = max(worst, check_real(pop, X, out, ok_eval, y, weights, kind, dtype, min_ok=15 if N > 1 else 5))
            assert kernel_name(pop) == "de_eval_tape_kernel<loss>"
    print(f"[flat loss {kind} {np.dtype(dtype).name}] worst error {worst:.2f} eps sum w (l + |l' e|) (bound 64)")
    pop.close()


WIDE_F = 200  # 200 feature rows fit neither kernel's LDS tile: `eval` runs de_eval_tape_kernel<direct> (asserted below)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_real_gather_variant_loss(api, dtype):
    """A feature matrix too wide for the threaded kernel — what a user with 200 features gets from the call the README advertises first."""
    trees = de.synth.random_population(40, seed=7, node_count=14, nfeatures=WIDE_F, operators=de.synth.BENCH_OPERATORS, dtype=dtype)
    pop = api.Population(trees, de.synth.BENCH_OPERATORS, dtype, n_features=WIDE_F)
    N = 1500
    X = de.synth.random_X(WIDE_F, N, seed=3, dtype=dtype)
    out, ok_eval = pop.eval(X)
    assert kernel_name(pop) == "de_eval_tape_kernel<direct>"
    assert ok_eval.sum() >= 10
    w = weights_with_zeros(N, dtype, 5)
    for kind in ("L2", "huber"):
        check_real(pop, X, out, ok_eval, targets(kind, N, dtype, seed=2), w, kind, dtype, min_ok=10)
        name = kernel_name(pop)
        assert "direct" in name and "loss" in name, name
    pop.close()


def test_real_parametric_population_loss(api, monkeypatch):
    """The shape of test_fused_loss_kinds_parametric_population_and_compacted_launch on the flat-switch interpreter."""
    monkeypatch.setenv("DE_EVAL_THREADED", "0")
    ops = de.OperatorEnum(binary_operators=("+", "*", "-"), unary_operators=("cos", "exp"))
    rng = de.synth.Xoshiro256ss(21)
    trees = [de.synth.gen_random_tree_fixed_size(9 + i % 8, ops, 2, rng, np.float32, de.ParametricNode, 2) for i in range(40)]
    N, P, Cn = 1500, 2, 4
    g = np.random.Generator(np.random.PCG64(5))
    X = np.asfortranarray(g.standard_normal((2, N)).astype(np.float32))
    params = np.asfortranarray(g.standard_normal((P, Cn)).astype(np.float32))
    classes = g.integers(1, Cn + 1, N)
    pop = api.Population(trees, ops, np.float32, n_features=2, n_params=P)
    out, ok_e = pop.eval(X, params=params, classes=classes)
    assert ok_e.any()
    for kind in ("L2", "l1_hinge"):
        check_real(pop, X, out, ok_e, targets(kind, N, np.float32, 3), None, kind, np.float32, min_ok=1, params=params, classes=classes)
        assert kernel_name(pop) == "de_eval_tape_kernel<loss>"
    pop.close()


# ---- 3: Float16 ------------------------------------------------------------------------------------------------------------------
def check_f16(pop, X, out, ok_eval, y, w, kind, **kw):
    """-> the number of complete trees with a finite reference loss.  The terms come from the device's rows in numpy float16 steps; where
    one is +Inf (|e| >= 256 under L2) the loss must be +Inf with ok still 1."""
    loss, ok = pop.eval_loss(X, y, weights=w, loss=kind, **kw)
    assert "half" in kernel_name(pop) and "loss" in kernel_name(pop), kernel_name(pop)
    assert loss.dtype == np.float32
    assert np.array_equal(ok, ok_eval), "fused loss and plain eval disagree on the completion flags"
    n_fin, worst = 0, 0.0
    for t in range(len(ok)):
        if not ok[t]:
            assert np.isnan(loss[t]), t
            continue
        terms = ref.f16_terms(kind, out[t], y, w).astype(np.float64)
        if np.isnan(terms).any():
            assert np.isnan(loss[t]), t
            continue
        if np.isposinf(terms).any():
            assert np.isposinf(loss[t]), (t, loss[t])
            continue
        assert (terms >= 0).all()
        want = terms.sum()
        if want > 0.25 * float(np.finfo(np.float32).max):
            continue
        n_fin += 1
        err = abs(float(loss[t]) - want)
        worst = max(worst, err / (2.0 ** -23 * want) if want > 0 else (0.0 if err == 0 else np.inf))
        assert err <= 64 * 2.0 ** -23 * want, (kind, t, loss[t], want)
    return n_fin, worst


def test_f16_loss(api):
    """L2 and L1 x {no weights, binary16 weights in [0, 2) with zeros} x N in {1, 63, 1024, 1025, 4099}.
    (Status 7 without EvalContext(typed_loss=True), and before the option existed.)"""
    ops = de.synth.BENCH_OPERATORS
    trees = de.synth.random_population(150, seed=0xDE02, node_count=12, nfeatures=5, operators=ops)
    pop = api.Population(trees, ops, H, n_features=5, eval_context=api.EvalContext(typed_loss=True))
    worst = 0.0
    for N in (1, 63, 1024, 1025, 4099):
        X = np.asfortranarray(de.synth.random_X(5, N, seed=N).astype(H))
        y = np.random.Generator(np.random.PCG64(N)).standard_normal(N).astype(H)
        w = weights_with_zeros(N, H, N + 1)
        out, ok_eval = pop.eval(X)
        for kind in ("L2", "L1"):
            for weights in (None, w):
                n_fin, wr = check_f16(pop, X, out, ok_eval, y, weights, kind)
                worst = max(worst, wr)
                print(f"[f16 loss {kind} N={N} weights={weights is not None}] {n_fin} complete trees with a finite reference loss")
                assert n_fin >= (60 if N > 1 else 100), (N, kind, n_fin)
    print(f"[f16 loss] worst error {worst:.2f} x 2^-23 x sum of the terms (bound 64)")
    pop.close()


def test_f16_gather_variant_loss(api):
    """40 features: the population of test_wide_feature_matrix_gathers_features."""
    ops = F16_WIDE_OPS
    F, N = 40, 3000
    trees = de.synth.random_population(40, seed=91, node_count=14, nfeatures=F, operators=ops)
    X = np.asfortranarray(de.synth.random_X(F, N, seed=92).astype(H))
    y = np.random.Generator(np.random.PCG64(1)).standard_normal(N).astype(H)
    pop = api.Population(trees, ops, H, n_features=F, eval_context=api.EvalContext(typed_loss=True))
    out, ok_eval = pop.eval(X)
    assert "direct" in kernel_name(pop)
    n = 0
    for kind in ("L2", "L1"):
        n_fin, _ = check_f16(pop, X, out, ok_eval, y, weights_with_zeros(N, H, 2), kind)
        assert "direct" in kernel_name(pop)
        n += n_fin
    assert n >= 10, n
    pop.close()


def test_f16_parametric_population_loss(api):
    """The shape of test_parametric_population_matches_oracle."""
    ops = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
    P = de.ParametricNode
    p1, p2, x1, x2 = P(parameter=1), P(parameter=2), P(feature=1), P(feature=2)
    trees = [P(1, P(3, p1, x1), P(1, P(2, p2, x2))), P(3, P(2, P(1, x1, p2), P(val=0.3)), p1), P(4, x2, P(2, P(3, p1, x1)))]
    rng = np.random.default_rng(3)
    N = 2049
    X = np.asfortranarray((rng.standard_normal((2, N)) * 2).astype(H))
    params = (rng.standard_normal((2, 3)) * 1.5).astype(H)
    classes = rng.integers(1, 4, N)
    y = rng.standard_normal(N).astype(H)
    pop = api.Population(trees, ops, H, n_features=2, n_params=2, eval_context=api.EvalContext(typed_loss=True))
    out, ok_eval = pop.eval(X, params=params, classes=classes)
    for kind in ("L2", "L1"):
        n_fin, _ = check_f16(pop, X, out, ok_eval, y, weights_with_zeros(N, H, 4), kind, params=params, classes=classes)
        assert n_fin >= 1
    pop.close()


def test_f16_known_answers(api):
    """x1 at 255 against 0: 255^2 = 65025 rounds to the binary16 65024; at 300 the term overflows binary16: +Inf, and the tree is complete."""
    ops = de.synth.BENCH_OPERATORS
    pop = api.Population([de.Node(feature=1)], ops, H, n_features=1, eval_context=api.EvalContext(typed_loss=True))
    loss, ok = pop.eval_loss(np.array([[255]], dtype=H), np.zeros(1, H))
    assert ok[0] and loss.dtype == np.float32 and loss[0] == np.float32(65024.0)
    loss, ok = pop.eval_loss(np.array([[300]], dtype=H), np.zeros(1, H))
    assert ok[0] and np.isposinf(loss[0])
    loss, ok = pop.eval_loss(np.array([[300]], dtype=H), np.zeros(1, H), loss="L1")
    assert ok[0] and loss[0] == 300.0
    pop.close()


# ---- 4: complex --------------------------------------------------------------------------------------------------------------------
def complex_population(n, seed, nfeatures=5):
    """tests/test_gpu_complex.py `_population("bench", n, seed)`: random real trees whose constants get a random imaginary part."""
    trees = de.synth.random_population(n, seed=seed, node_count=12, nfeatures=5, operators=CBENCH)
    rng = np.random.default_rng(seed + 11)
    for t in trees:
        for node in t:
            if node.degree == 0 and node.constant:
                node.val = complex(node.val, float(rng.standard_normal()))
    if nfeatures != 5:
        rng = np.random.default_rng(5)
        for t in trees:
            for node in t:
                if node.degree == 0 and not node.constant:
                    node.feature = int(rng.integers(1, nfeatures + 1))
    return trees


def complex_normals(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


def check_complex(pop, X, out, ok_eval, y, w, kind, dtype):
    rt = REAL_OF[np.dtype(dtype)]
    loss, ok = pop.eval_loss(X, y, weights=w, loss=kind)
    assert "complex" in kernel_name(pop) and "loss" in kernel_name(pop), kernel_name(pop)
    assert loss.dtype == np.dtype(rt)
    assert np.array_equal(ok, ok_eval), "fused loss and plain eval disagree on the completion flags"
    eps, fmax, tiny = np.finfo(rt).eps, float(np.finfo(rt).max), float(np.finfo(rt).tiny) * X.shape[1]
    n_ok, worst = 0, 0.0
    for t in range(len(ok)):
        if not ok[t]:
            assert np.isnan(loss[t]), t
            continue
        n_ok += 1
        want, mag = ref.complex_loss(kind, out[t], y, w)
        if np.isnan(want):
            assert np.isnan(loss[t])
            continue
        if not np.isfinite(mag) or mag > 0.25 * fmax:
            assert np.isposinf(loss[t]) or abs(float(loss[t]) - want) <= 64 * eps * mag
            continue
        err = abs(float(loss[t]) - want)
        worst = max(worst, err / (eps * mag + tiny))
        assert err <= 64 * eps * mag + tiny, (kind, t, loss[t], want, err / (eps * mag + tiny))
    return n_ok, worst


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128], ids=["cf32", "cf64"])
def test_complex_loss(api, dtype):
    """L2 and L1 x {no weights, real weights with zeros} x N in {1, 63, tile, tile + 1, 4 tile + 3}; complex constants, X and y."""
    trees = complex_population(48, 0)
    pop = api.Population(trees, CBENCH, dtype, n_features=5, eval_context=api.EvalContext(typed_loss=True))
    tile = FLAT_TILE[np.dtype(dtype)]
    worst = 0.0
    for N in (1, 63, tile, tile + 1, 4 * tile + 3):
        X = np.asfortranarray(complex_normals((5, N), dtype, N))
        y = complex_normals(N, dtype, N + 1)
        w = weights_with_zeros(N, REAL_OF[np.dtype(dtype)], N + 2)
        out, ok_eval = pop.eval(X)
        for kind in ("L2", "L1"):
            for weights in (None, w):
                n_ok, wr = check_complex(pop, X, out, ok_eval, y, weights, kind, dtype)
                worst = max(worst, wr)
                assert N == 1 or n_ok >= 24, (N, n_ok)
        print(f"[complex loss {np.dtype(dtype).name} N={N}] {n_ok} complete trees of 48")
    print(f"[complex loss {np.dtype(dtype).name}] worst error {worst:.2f} eps sum w (l + |e| |dl/d|e||) (bound 64)")
    pop.close()


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128], ids=["cf32", "cf64"])
def test_complex_gather_variant_loss(api, dtype):
    F, N = 17, 1500  # 17 feature rows of 4096 B are past the 64 KB tile
    trees = complex_population(24, 31, nfeatures=F)
    pop = api.Population(trees, CBENCH, dtype, n_features=F, eval_context=api.EvalContext(typed_loss=True))
    X = np.asfortranarray(complex_normals((F, N), dtype, 17))
    y = complex_normals(N, dtype, 18)
    out, ok_eval = pop.eval(X)
    assert "direct" in kernel_name(pop)
    for kind in ("L2", "L1"):
        n_ok, _ = check_complex(pop, X, out, ok_eval, y, weights_with_zeros(N, REAL_OF[np.dtype(dtype)], 19), kind, dtype)
        assert "direct" in kernel_name(pop) and n_ok >= 6
    pop.close()


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128], ids=["cf32", "cf64"])
def test_complex_known_answers(api, dtype):
    pop = api.Population([de.Node(feature=1)], CBENCH, dtype, n_features=1, eval_context=api.EvalContext(typed_loss=True))
    X, y = np.array([[3 + 4j]], dtype=dtype), np.zeros(1, dtype)
    l1, ok1 = pop.eval_loss(X, y, loss="L1")
    l2, ok2 = pop.eval_loss(X, y, loss="L2")
    assert ok1[0] and ok2[0] and l1[0] == 5.0 and l2[0] == 25.0 and l1.dtype == REAL_OF[np.dtype(dtype)]
    pop.close()


# ---- 5: the contract, for each of the five element types -------------------------------------------------------------------------------
TYPES = {"f32": np.float32, "f64": np.float64, "f16": H, "cf32": np.complex64, "cf64": np.complex128}


def setup_type(api, monkeypatch, name, N, **ctx_kw):
    """(population, X, y, w) of an element type on the flat-switch interpreter; a population whose random trees partly go non-finite."""
    dtype = TYPES[name]
    if name in ("f32", "f64"):
        monkeypatch.setenv("DE_EVAL_THREADED", "0")
    ectx = api.EvalContext(typed_loss=True, **ctx_kw)
    if name in ("cf32", "cf64"):
        trees, ops = complex_population(48, 0), CBENCH
        X = np.asfortranarray(complex_normals((5, N), dtype, 3))
        y = complex_normals(N, dtype, 4)
        w = weights_with_zeros(N, REAL_OF[np.dtype(dtype)], 5)
    else:
        ops = de.synth.BENCH_OPERATORS
        kw = dict(dtype=dtype) if name != "f16" else {}
        trees = de.synth.random_population(96, seed=0xDE02, node_count=12, nfeatures=5, operators=ops, **kw)
        X = np.asfortranarray(de.synth.random_X(5, N, seed=3).astype(dtype))
        y = np.random.Generator(np.random.PCG64(4)).standard_normal(N).astype(dtype)
        w = weights_with_zeros(N, dtype, 5)
    return api.Population(trees, ops, dtype, n_features=5, eval_context=ectx), X, y, w


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


@pytest.mark.parametrize("name", list(TYPES))
def test_contract_reproducible_host_and_device_and_strided(api, monkeypatch, name):
    """Two identical calls give identical bits; host buffers and torch device buffers give identical bits and flags; an ld-strided X
    (ldX > F) equals the contiguous call; NaN exactly where a tree is incomplete."""
    import torch
    N = 2 * FLAT_TILE[np.dtype(TYPES[name])] + 77
    pop, X, y, w = setup_type(api, monkeypatch, name, N)
    Xd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()
    wide = torch.zeros((N, 8), dtype=Xd.dtype, device="cuda")
    wide[:, :5] = Xd.t()
    Xs = wide.t()[:5]
    assert Xs.stride() == (1, 8)
    yd, wd = torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda()
    _, ok_eval = pop.eval(X)
    assert ok_eval.any() and (~ok_eval).any()
    for kind in ("L2", "L1"):
        for wh, wdev in ((None, None), (w, wd)):
            a, ok_a = pop.eval_loss(X, y, weights=wh, loss=kind)
            b, ok_b = pop.eval_loss(X, y, weights=wh, loss=kind)
            c, ok_c = pop.eval_loss(Xd, yd, weights=wdev, loss=kind)
            s, ok_s = pop.eval_loss(Xs, yd, weights=wdev, loss=kind)
            torch.cuda.synchronize()
            assert np.array_equal(ok_a, ok_eval) and np.array_equal(ok_a, ok_b)
            assert np.array_equal(ok_a, ok_c.cpu().numpy()) and np.array_equal(ok_a, ok_s.cpu().numpy())
            assert np.array_equal(np.isnan(a), ~ok_a), "NaN exactly where the evaluation was incomplete"
            assert np.array_equal(bits(a), bits(b)), "two identical calls differ"
            assert np.array_equal(bits(a)[ok_a], bits(c.cpu().numpy())[ok_a]), "host and device buffers differ"
            assert np.array_equal(bits(a)[ok_a], bits(s.cpu().numpy())[ok_a]), "strided X differs"
            assert bool(torch.isnan(c[~ok_c]).all()) and bool(torch.isnan(s[~ok_s]).all())
    pop.close()


@pytest.mark.parametrize("ctx_kw", [dict(full_eval=True), dict(early_exit=False)], ids=["full_eval", "no_early_exit"])
@pytest.mark.parametrize("name", list(TYPES))
def test_contract_flags_follow_eval(api, monkeypatch, name, ctx_kw):
    """DE_OPT_FULL_EVAL and early_exit = False populations give the flags of their `eval` and NaN at ~ok; a DE_OPT_FULL_EVAL population
    gives the flags and — the same program over the same samples in the same order — the loss bits of the default one."""
    N = FLAT_TILE[np.dtype(TYPES[name])] + 5
    pop, X, y, w = setup_type(api, monkeypatch, name, N, **ctx_kw)
    ref_pop, _, _, _ = setup_type(api, monkeypatch, name, N)
    _, ok_eval = pop.eval(X)
    loss, ok = pop.eval_loss(X, y, weights=w)
    want, ok_w = ref_pop.eval_loss(X, y, weights=w)
    assert ok.any() and np.array_equal(ok, ok_eval) and np.isnan(loss[~ok]).all()
    if "full_eval" in ctx_kw:
        assert np.array_equal(ok, ok_w) and np.array_equal(np.isnan(loss), ~ok)
        assert np.array_equal(bits(loss)[ok], bits(want)[ok])
    pop.close()
    ref_pop.close()


@pytest.mark.parametrize("name", list(TYPES))
def test_contract_no_samples(api, monkeypatch, name):
    """N = 0: the empty sum is 0; NaN where a constant already failed the flag (1 / 0 folds to Inf)."""
    dtype = TYPES[name]
    if name in ("f32", "f64"):
        monkeypatch.setenv("DE_EVAL_THREADED", "0")
    ops = CBENCH
    one, zero = (1.0 + 0j, 0j) if name.startswith("cf") else (1.0, 0.0)
    trees = [de.Node(1, de.Node(feature=1), de.Node(val=one)),
             de.Node(1, de.Node(feature=1), de.Node(4, de.Node(val=one), de.Node(val=zero)))]
    pop = api.Population(trees, ops, dtype, n_features=1, eval_context=api.EvalContext(typed_loss=True))
    X = np.zeros((1, 0), dtype=dtype, order="F")
    _, ok_eval = pop.eval(X)
    loss, ok = pop.eval_loss(X, np.zeros(0, dtype))
    assert list(ok_eval) == [True, False] and np.array_equal(ok, ok_eval)
    assert loss[0] == 0 and np.isnan(loss[1])
    pop.close()


# ---- 6: the scope of the bit ----------------------------------------------------------------------------------------------------------
SCOPE = [(H, 0.5, "F16", "DE_F16", 4.0), (np.complex64, 0.5 + 0.5j, "complex", "DE_CF32", 8.0), (np.complex128, 0.5 + 0.5j, "complex", "DE_CF64", 8.0)]


@pytest.mark.parametrize("dt, val, word, tname, want", SCOPE, ids=["f16", "cf32", "cf64"])
def test_scope_of_the_bit(api, dt, val, word, tname, want):
    """The 16-sample programs of the existing refusal tests (x1 + c on X = 1 against y = 1), created with DE_OPT_TYPED_LOSS."""
    lib = api.library()
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    N = 16
    out_t = np.float32 if dt in (H, np.complex64) else np.float64
    X, y = np.asfortranarray(np.ones((1, N), dtype=dt)), np.ones(N, dtype=dt)
    tree = de.Node(1, de.Node(feature=1), de.Node(val=val))
    # without the bit: refused as before, no output touched
    plain = api.Population([tree], ops, dt, n_features=1)
    buf = np.full(64, 7, dtype=np.uint8)
    okb = np.full(8, 7, dtype=np.uint8)
    assert lib.de_eval_loss(plain.ctx._h, plain._h, X.ctypes.data, N, 1, None, y.ctypes.data, None, 0, buf.ctypes.data, okb.ctypes.data) == 7
    assert word in lib.de_last_error(plain.ctx._h).decode() and (buf == 7).all() and (okb == 7).all()
    with pytest.raises(api.DeviceError, match="DE_ERR_UNSUPPORTED"):
        plain.eval_loss(X, y)
    plain.close()
    # with it: status 0 and the closed form — e = 0.5 (binary16: 16 x 0.25) or 0.5 + 0.5i (16 x 0.5)
    pop = api.Population([tree], ops, dt, n_features=1, eval_context=api.EvalContext(typed_loss=True))
    h, ph = pop.ctx._h, pop._h
    loss = np.full(1, -1, dtype=out_t)
    ok = np.zeros(1, np.uint8)
    assert lib.de_eval_loss(h, ph, X.ctypes.data, N, 1, None, y.ctypes.data, None, 0, loss.ctypes.data, ok.ctypes.data) == 0
    assert ok[0] == 1 and loss[0] == want
    l1, _ = pop.eval_loss(X, y, loss="L1")
    want1 = 16 * (0.5 if dt == H else np.sqrt(0.5))  # (|0.5 + 0.5i|: the device's hypot, a 1-ulp function)
    assert abs(float(l1[0]) - want1) <= 4 * np.finfo(out_t).eps * want1
    # another kind: status 7, the kind and the element type named, every output untouched
    bufs = [np.full(512, 7, dtype=np.uint8) for _ in range(4)]
    ptr = [b.ctypes.data for b in bufs]
    spec = api.LossSpec(16, 0, 1.0)
    assert lib.de_eval_loss_ex(h, ph, X.ctypes.data, N, 1, None, y.ctypes.data, None, C.byref(spec), ptr[0], ptr[2]) == 7
    msg = lib.de_last_error(h).decode()
    assert "16" in msg and tname in msg, msg
    with pytest.raises(api.DeviceError, match="DE_ERR_UNSUPPORTED"):
        pop.eval_loss(X, y, loss="huber", loss_param=1.0)
    # every other entry point that refuses these programs keeps refusing them
    off = np.zeros(1, dtype=np.int64)
    l2 = api.LossSpec(0, 0, 0.0)
    calls = {
        "de_eval_loss_grad": lambda: lib.de_eval_loss_grad(h, ph, X.ctypes.data, N, 1, None, 1, y.ctypes.data, None, 0, ptr[0], ptr[1], None, ptr[2]),
        "de_eval_pullback_dX": lambda: lib.de_eval_pullback_dX(h, ph, X.ctypes.data, N, 1, None, y.ctypes.data, ptr[0], None, ptr[2]),
        "de_eval_fit_stats": lambda: lib.de_eval_fit_stats(h, ph, X.ctypes.data, N, 1, None, y.ctypes.data, None, ptr[0], ptr[1], ptr[2]),
        "de_fit_consts_bfgs": lambda: lib.de_fit_consts_bfgs(h, ph, X.ctypes.data, N, 1, None, y.ctypes.data, None, C.byref(l2), None, ptr[0], ptr[2],
                                                            None, None),
        "de_eval_loss_tree_params": lambda: lib.de_eval_loss_tree_params(h, ph, X.ctypes.data, N, 1, None, y.ctypes.data, None, C.byref(l2), ptr[0],
                                                                        ptr[2]),
        "de_ctx_declare_dataset": lambda: lib.de_ctx_declare_dataset(h, api._dtype_code(dt), ptr[3], N, 1, 1),
    }
    for name, call in calls.items():
        assert call() == 7, name
    assert all((b == 7).all() for b in bufs), "a refused call wrote an output"
    for meth, args in (("eval_loss_grad", (X, y)), ("eval_fit_stats", (X, y)), ("eval_pullback_dX", (X, y))):
        with pytest.raises(api.DeviceError, match="DE_ERR_UNSUPPORTED"):
            getattr(pop, meth)(*args)
    pop.close()


@pytest.mark.parametrize("threaded", ["1", "0"], ids=["threaded", "flat"])
def test_float32_ignores_the_bit(api, monkeypatch, threaded):
    monkeypatch.setenv("DE_EVAL_THREADED", threaded)
    ops = de.synth.BENCH_OPERATORS
    trees = de.synth.random_population(60, seed=0xDE02)
    N = 3000
    X = de.synth.random_X(5, N, seed=1)
    y = targets("L2", N, np.float32, 2)
    got = []
    for typed in (False, True):
        pop = api.Population(trees, ops, np.float32, n_features=5, eval_context=api.EvalContext(typed_loss=typed))
        got.append(pop.eval_loss(X, y, weights=weights_with_zeros(N, np.float32, 3), loss="huber", loss_param=1.3))
        pop.close()
    assert np.array_equal(got[0][1], got[1][1]) and got[0][1].any()
    assert np.array_equal(bits(got[0][0]), bits(got[1][0]))
