"""GPU tests of the parameterised loss kinds of the fused reductions (include/de_hip.h de_loss_kind_t values >= 16: Huber, log-cosh,
the two epsilon-insensitive kinds, quantile, Lp, the logistic distance, and the logistic / hinge margins), modelled on check_losses and
check_loss_grads of tests/test_gpu_loss.py — the same populations and seeds.

The reference is tests/loss_reference.py (float64, written from the header's table) over the DEVICE's own `Population.eval` rows and
`eval_grad` Jacobians — existing code that the other test files hold to the oracle — so what is tested here is the loss arithmetic and
the reductions.  Tolerances (eps = the element type's):
  value     64 eps sum_j w_j (l_j + |l'_j e_j|) + tiny     e is rounded once in T, which moves l by |l' e| eps; the forms of
                                                           csrc/de_loss_kinds.h keep l's own arithmetic within a few eps l; 64 is the
                                                           factor test_gpu_loss.py grants the summation (a_j for e_j in the margin kinds)
  gradient  64 eps sum_j w_j (|l'_j| + |l''_j e_j|) gabs_kj + tiny    gabs = helpers.path_abs_jacobian (any association of the products);
                                                           the l'' e term is the rounding of e inside l'
  kinks     a sample whose e (a) lies within 4 eps max(|yhat|, |y|) of a jump of l' may take either side: it adds w_j jump gabs_kj,
            and such samples must stay below 1 % of the samples of every compared tree."""
import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
from helpers import path_abs_jacobian
from loss_reference import KINDS, MARGIN, PARAMS, kink_samples, loss_terms
from oracle import oracle

pytestmark = pytest.mark.gpu
ALL_KINDS = sorted(KINDS)


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _api.library()
    return _api


def targets(kind, N, dtype, seed):
    """Continuous random targets; the margin kinds get labels of either sign with |y| in [1, 1.5)."""
    g = np.random.Generator(np.random.PCG64(seed))
    y = g.standard_normal(N)
    if kind in MARGIN:
        y = np.where(y > 0, 1.0, -1.0) * (1.0 + 0.5 * g.random(N))
    return y.astype(dtype)


def ref_loss(kind, p, out64, y, w):
    """(sum_j w_j l_j, the tolerance's magnitude sum_j w_j (l_j + |l'_j z_j|), largest term) — z = e, or a for a margin kind."""
    y64 = y.astype(np.float64)
    with np.errstate(all="ignore"):
        l, lp, _ = loss_terms(kind, out64, y64, p)
        z = y64 * out64 if kind in MARGIN else out64 - y64
        ww = np.ones_like(y64) if w is None else w.astype(np.float64)
        keep = ww != 0
        return (ww * l)[keep].sum(), (ww * (l + np.abs(lp * z)))[keep].sum(), (ww * l)[keep].max(initial=0.0)


def check_kind_losses(api, pop, trees, X, out, ok_eval, y, w, kind, p, dtype, min_ok):
    loss, ok = pop.eval_loss(X, y, weights=w, loss=kind, loss_param=p)
    assert np.array_equal(ok, ok_eval), "fused loss and plain eval disagree on the completion flags"
    eps, fmax, tiny = np.finfo(dtype).eps, float(np.finfo(dtype).max), float(np.finfo(dtype).tiny) * X.shape[1]
    n_ok, worst = 0, 0.0
    for t in range(len(trees)):
        if not ok[t]:
            assert np.isnan(loss[t]), f"tree {t}: incomplete evaluation must give a NaN loss"
            continue
        n_ok += 1
        want, mag, big = ref_loss(kind, p, out[t].astype(np.float64), y, w)
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
    assert n_ok >= min_ok
    return worst


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_fused_loss_kinds_values(api, kind, dtype):
    """Every kind x {Float32, Float64} x {no weights, weights with zeros} x N in {1, 63, 1024, 4099}."""
    ops = de.synth.BENCH_OPERATORS
    trees = de.synth.random_population(150, seed=0xDE02, dtype=dtype)
    pop = api.Population(trees, ops, dtype, n_features=5)
    worst = 0.0
    for N in (1, 63, 1024, 4099):
        X = de.synth.random_X(5, N, seed=1, dtype=dtype)
        out, ok_eval = pop.eval(X)
        y = targets(kind, N, dtype, seed=N)
        g = np.random.Generator(np.random.PCG64(N + 1))
        w = g.uniform(0, 2, N).astype(dtype)
        w[::7] = 0
        for weights in (None, w):
            worst = max(worst, check_kind_losses(api, pop, trees, X, out, ok_eval, y, weights, kind, PARAMS[kind], dtype, min_ok=15 if N > 1 else 5))
    print(f"[loss kind {kind} {np.dtype(dtype).name}] worst error {worst:.2f} eps sum w (l + |l' e|) (bound 64)")
    pop.close()


def test_fused_loss_kinds_parametric_population_and_compacted_launch(api):
    """The loss launch of a parametric population, and one large enough for the probe launch + compaction of the live trees (the
    compacted stream names the out-of-line end directly): kind and parameter travel as in the plain launch."""
    import torch
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
    for kind in ("huber", "logcosh", "l1_hinge"):
        y = targets(kind, N, np.float32, 3)
        loss, ok = pop.eval_loss(X, y, params=params, classes=classes, loss=kind, loss_param=PARAMS[kind])
        assert np.array_equal(ok, ok_e) and ok.any()
        for t in np.nonzero(ok)[0]:
            want, mag, _ = ref_loss(kind, PARAMS[kind], out[t].astype(np.float64), y, None)
            assert abs(float(loss[t]) - want) <= 64 * np.finfo(np.float32).eps * mag + 1e-30
    pop.close()
    trees = de.synth.random_population(300, seed=0xDE02)
    pop = api.Population(trees, de.synth.BENCH_OPERATORS, np.float32, n_features=5)
    gen = torch.Generator(device="cuda").manual_seed(4)
    Nd = 400_000 + 37
    Xd = torch.randn((Nd, 5), generator=gen, device="cuda").t()
    yd = torch.randn(Nd, generator=gen, device="cuda")
    out, ok_e = pop.eval(Xd)
    for kind in ("huber", "lp", "logit_dist"):
        loss, ok = pop.eval_loss(Xd, yd, loss=kind, loss_param=PARAMS[kind])
        torch.cuda.synchronize()
        assert torch.equal(ok, ok_e)
        # the call DID compact (else this block would pass without LossEnds ever carrying one of the new kinds): the trees behind the
        # probe launch were counted, every complete tree is among them, and the probe dropped some of this population's failing trees
        live = pop.last_live_trees()
        assert int(ok.sum()) <= live < len(trees), (kind, live, int(ok.sum()), "the loss launch did not compact its live trees")
        o64, y64 = out[ok].double().cpu().numpy(), yd.double().cpu().numpy()
        got = loss[ok].double().cpu().numpy()
        for k in range(min(len(o64), 40)):
            l, lp, _ = loss_terms(kind, o64[k], y64, PARAMS[kind])
            mag = (l + np.abs(lp * (o64[k] - y64))).sum()
            if np.isfinite(mag) and mag < 0.25 * np.finfo(np.float32).max:
                assert abs(got[k] - l.sum()) <= 64 * np.finfo(np.float32).eps * mag
        assert bool(torch.isnan(loss[~ok]).all())
    pop.close()


# ---- fused loss + gradient ---------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["forward", "forward-2-per-lane", "reverse"])
def accumulation(request, monkeypatch):
    """The three kernels that carry a gradient epilogue (tests/test_gpu_loss.py `accumulation`)."""
    monkeypatch.setenv("DE_LOSS_GRAD_REVERSE", "1" if request.param == "reverse" else "0")
    monkeypatch.setenv("DE_GRAD_VS2_MIN_N", "0" if request.param == "forward-2-per-lane" else "1000000000000")
    return request.param


MODES = {"variable": (True, oracle.GRAD_VARIABLE), "constant": (False, oracle.GRAD_CONSTANT), "both": ("both", oracle.GRAD_BOTH)}
_ANCHORS = {}  # (dtype, mode) -> per tree: the oracle's (values, Jacobian) and the path-absolute Jacobian (the same for every kind)


def ref_loss_grad(kind, p, o64, g64, gabs, y, w, eps):
    """(loss, its magnitude, dloss[k], magnitude[k] with the kink slack, share of samples on a kink)."""
    y64 = y.astype(np.float64)
    ww = np.ones_like(y64) if w is None else w.astype(np.float64)
    keep = ww != 0
    with np.errstate(all="ignore"):
        l, lp, lpp = loss_terms(kind, o64, y64, p)
        z = y64 * o64 if kind in MARGIN else o64 - y64
        near, jump = kink_samples(kind, o64, y64, p, eps)
        ga = np.abs(g64) if gabs is None else np.maximum(np.abs(g64), np.nan_to_num(gabs, nan=np.inf, posinf=np.inf))
        terms = (ww * lp)[None, keep] * g64[:, keep]
        mag = ((ww * (np.abs(lp) + np.abs(lpp * z)))[None, keep] * ga[:, keep]).sum(axis=1)
        slack = ((ww * jump * near)[None, keep] * ga[:, keep]).sum(axis=1)
        return (ww * l)[keep].sum(), (ww * (l + np.abs(lp * z)))[keep].sum(), terms.sum(axis=1), mag, slack, near[keep].mean() if keep.any() else 0.0


def check_kind_loss_grads(api, trees, ops, X, y, w, kind, p, dtype, mode_name, min_ok):
    variable, omode = MODES[mode_name]
    pop = api.Population(trees, ops, dtype, n_features=X.shape[0])
    loss, dls, ok = pop.eval_loss_grad(X, y, weights=w, loss=kind, variable=variable, loss_param=p)
    out, grads, ok_g = pop.eval_grad(X, variable)
    assert np.array_equal(ok, ok_g)
    eps, fmax = np.finfo(dtype).eps, float(np.finfo(dtype).max)
    tiny = float(np.finfo(dtype).tiny) * X.shape[1]
    key = (np.dtype(dtype).name, mode_name)
    if key not in _ANCHORS:
        anchors = []
        for tree in trees:
            tape, consts = de.flatten(tree, ops, dtype)
            yo, go, ok_o = oracle.eval_grad_tree_array(tape, consts, X, omode, elementwise=True)
            anchors.append((yo.astype(np.float64), go.astype(np.float64), ok_o, path_abs_jacobian(tree, ops, X, mode_name)))
        _ANCHORS[key] = anchors
    n_ok, worst = 0, 0.0
    for t in range(len(trees)):
        assert dls[t].shape == (grads[t].shape[0],)
        if not ok[t]:
            assert np.isnan(loss[t]) and np.all(np.isnan(dls[t]))
            continue
        yo, go, ok_o, gabs = _ANCHORS[key][t]
        assert ok_o  # IEEE-exact operators: the oracle's Jacobian is a second anchor (oracle_exact=True of test_gpu_loss.py)
        for o64, g64 in ((out[t].astype(np.float64), np.asarray(grads[t], dtype=np.float64)), (yo, go)):
            want_l, mag_l, want_g, mag, slack, kink_share = ref_loss_grad(kind, p, o64, g64, gabs, y, w, eps)
            if not np.all(np.isfinite(want_g)) or not np.all(np.isfinite(mag)) or max(abs(want_l), mag_l, mag.max(initial=0)) > 0.05 * fmax:
                continue  # a term overflows T
            assert kink_share < 0.01, (kind, t, kink_share)
            assert abs(float(loss[t]) - want_l) <= 64 * eps * mag_l + tiny, (kind, t, loss[t], want_l)
            err = np.abs(dls[t].astype(np.float64) - want_g)
            worst = max(worst, float((err / (eps * mag + slack + tiny)).max(initial=0)))
            assert np.all(err <= 64 * eps * mag + slack + tiny), (kind, t, mode_name, de.string_tree(trees[t], ops), dls[t], want_g, mag)
        n_ok += 1
    assert n_ok >= min_ok
    pop.close()
    return worst


@pytest.mark.parametrize("mode", ["constant", "variable", "both"])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_fused_loss_kinds_gradients_exact_operators(api, accumulation, mode, kind):
    """Every kind x constant / variable / both x the three accumulation modes, Float32 and Float64, weights with zeros, against the
    device's own Jacobian and the oracle's (an IEEE-exact operator set)."""
    ops = de.OperatorEnum(binary_operators=("+", "-", "/", "*"), unary_operators=("neg", "square", "abs"))
    rng = de.synth.Xoshiro256ss(17)
    worst = 0.0
    for dtype in (np.float32, np.float64):
        trees = [de.synth.gen_random_tree_fixed_size(3 + i % 26, ops, 4, rng, dtype) for i in range(60)]
        N = 777
        X = de.synth.random_X(4, N, seed=12, dtype=dtype)
        g = np.random.Generator(np.random.PCG64(2))
        y = targets(kind, N, dtype, seed=2)
        w = g.uniform(0, 2, N).astype(dtype)
        w[::5] = 0
        worst = max(worst, check_kind_loss_grads(api, trees, ops, X, y, w, kind, PARAMS[kind], dtype, mode, min_ok=10))
    print(f"[loss kind gradient {kind} {mode} {accumulation}] worst error {worst:.2f} eps sum w (|l'| + |l'' e|) gabs (bound 64)")


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_fused_loss_kinds_by_class_matches_scatter_of_jacobian(api, accumulation, kind):
    """A parametric population through eval_loss_grad_by_class: dparams[t][p, c] == sum over the samples of class c of w l' J[p, j], the
    dloss rows the sum over all classes; `grouped` both ways gives the same bits."""
    dtype = np.float32
    ops = de.OperatorEnum(binary_operators=("+", "*", "-", "/"), unary_operators=("cos", "exp"))
    rng = de.synth.Xoshiro256ss(33)
    P, Cn, N = 3, 7, 2500
    trees = [de.synth.gen_random_tree_fixed_size(7 + i % 12, ops, 2, rng, dtype, de.ParametricNode, P) for i in range(60)]
    g = np.random.Generator(np.random.PCG64(9))
    X = np.asfortranarray(g.standard_normal((2, N)).astype(dtype))
    params = np.asfortranarray(g.standard_normal((P, Cn)).astype(dtype))
    classes = g.choice([1, 2, 4, 5, 7], N)  # classes 3 and 6 have no sample
    y = targets(kind, N, dtype, seed=9)
    w = (g.random(N) > 0.2).astype(dtype) * g.random(N).astype(dtype)
    p = PARAMS[kind]
    pop = api.Population(trees, ops, dtype, n_features=2, n_params=P)
    loss, dls, dp, ok = pop.eval_loss_grad_by_class(X, y, params, classes, weights=w, loss=kind, variable="both", loss_param=p)
    loss1, dls1, ok1 = pop.eval_loss_grad(X, y, weights=w, loss=kind, variable="both", params=params, classes=classes, loss_param=p)
    out, grads, okg = pop.eval_grad(X, "both", params=params, classes=classes)
    assert np.array_equal(ok, okg) and np.array_equal(ok, ok1) and ok.sum() > 10 and dp.shape == (len(trees), P, Cn)
    eps, fmax = float(np.finfo(dtype).eps), float(np.finfo(dtype).max)
    w64 = w.astype(np.float64)
    for t in range(len(trees)):
        if not ok[t]:
            assert np.isnan(loss[t]) and np.isnan(dls[t]).all() and np.isnan(dp[t]).all()
            continue
        o64, g64 = out[t].astype(np.float64), np.asarray(grads[t], dtype=np.float64)
        gabs = path_abs_jacobian(trees[t], ops, X, "both", params, classes)
        with np.errstate(all="ignore"):
            l, lp, lpp = loss_terms(kind, o64, y.astype(np.float64), p)
            z = y * o64 if kind in MARGIN else o64 - y
            near, jump = kink_samples(kind, o64, y, p, eps)
            ga = np.abs(g64) if gabs is None else np.maximum(np.abs(g64), np.nan_to_num(gabs, nan=np.inf, posinf=np.inf))
            terms = (w64 * lp)[None, :] * g64
            aterms = (w64 * (np.abs(lp) + np.abs(lpp * z)))[None, :] * ga
            kterms = (w64 * jump * near)[None, :] * ga
        assert near[w64 != 0].mean() < 0.01
        for c in range(Cn):
            sel = classes == c + 1
            want, mag, slack = terms[:P, sel].sum(axis=1), aterms[:P, sel].sum(axis=1), kterms[:P, sel].sum(axis=1)
            big = ~np.isfinite(mag) | (mag > 0.25 * fmax)
            assert np.all((np.abs(dp[t][:, c] - want) <= 64 * eps * mag + slack + 1e-300) | big), (kind, t, c)
            if not sel.any():
                assert np.all(dp[t][:, c] == 0)
        want, mag, slack = terms.sum(axis=1), aterms.sum(axis=1), kterms.sum(axis=1)
        assert np.all((np.abs(dls[t] - want) <= 64 * eps * mag + slack + 1e-300) | ~np.isfinite(mag) | (mag > 0.25 * fmax)), (kind, t)
        mag_l = (w64 * (l + np.abs(lp * z))).sum()
        # (the same loss from the by-class and the plain reduction: equal — both +Inf where the sum overflows T — or within the bound)
        assert loss[t] == loss1[t] or abs(float(loss[t]) - float(loss1[t])) <= 64 * eps * mag_l + 1e-300 or not np.isfinite(mag_l)
    order = np.argsort(classes, kind="stable")
    b = pop.eval_loss_grad_by_class(np.asfortranarray(X[:, order]), y[order], params, classes[order], weights=w[order], loss=kind,
                                    variable="both", grouped=True, loss_param=p)
    assert np.array_equal(dp, b[2], equal_nan=True) and np.array_equal(loss, b[0], equal_nan=True)
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(dls, b[1])) and np.array_equal(ok, b[3])
    pop.close()


# ---- properties ----------------------------------------------------------------------------------------------------------------------
def test_fused_loss_kinds_exact_properties(api):
    """loss(tree_t, y = tree_t(X)) == 0 exactly for the kinds that vanish at e = 0; doubling the weights doubles every loss bit for bit;
    two runs are bit-identical; log-cosh stays finite at |e| ~ 10^4."""
    import torch
    ops = de.synth.BENCH_OPERATORS
    trees = de.synth.random_population(200, seed=0xDE02)
    N = 10**5 + 37
    pop = api.Population(trees, ops, np.float32, n_features=5)
    g = torch.Generator(device="cuda").manual_seed(4)
    X = torch.randn((N, 5), generator=g, device="cuda").t()
    out, ok = pop.eval(X)
    t_ok = [int(t) for t in torch.nonzero(ok).flatten()[:2]]
    assert t_ok
    for kind in ("huber", "l1_eps", "l2_eps", "quantile", "lp"):
        for t in t_ok:
            loss, ok2 = pop.eval_loss(X, out[t], loss=kind, loss_param=PARAMS[kind])
            assert torch.equal(ok, ok2)
            assert float(loss[t]) == 0.0, kind
            assert bool((loss[ok] >= 0).all()) and bool(torch.isnan(loss[~ok]).all())
    y = torch.randn(N, generator=g, device="cuda")
    w = torch.rand(N, generator=g, device="cuda")
    for kind in ALL_KINDS:
        l1, _ = pop.eval_loss(X, y, weights=w, loss=kind, loss_param=PARAMS[kind])
        l1b, _ = pop.eval_loss(X, y, weights=w, loss=kind, loss_param=PARAMS[kind])
        l2, _ = pop.eval_loss(X, y, weights=2 * w, loss=kind, loss_param=PARAMS[kind])
        torch.cuda.synchronize()
        assert torch.equal(l1[ok], l1b[ok]), kind
        assert torch.equal(2 * l1[ok], l2[ok]), kind
    # |e| ~ 10^4: log cosh(10^4) = 9999.3069 in Float32, no overflow of cosh
    far = torch.full((N,), 1.0e4, device="cuda") + out[t_ok[0]]
    lc, _ = pop.eval_loss(X, far, loss="logcosh")
    ld, _ = pop.eval_loss(X, far, loss="logit_dist")
    assert np.isfinite(float(lc[t_ok[0]])) and abs(float(lc[t_ok[0]]) / N - 9999.3069) < 0.01
    assert np.isfinite(float(ld[t_ok[0]])) and abs(float(ld[t_ok[0]]) / N - (1.0e4 - 2 * np.log(2.0))) < 0.01
    pop.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_fused_loss_kinds_reduce_to_l2_and_l1(api, dtype):
    """huber with delta above every |e| = L2 / 2, l1_eps with eps = 0 = L1, lp with p = 2 = L2 — within the summation tolerance
    (64 eps sum of the terms), values and gradients."""
    ops = de.OperatorEnum(binary_operators=("+", "-", "*"), unary_operators=("cos", "neg", "square"))
    rng = de.synth.Xoshiro256ss(5)
    trees = [de.synth.gen_random_tree_fixed_size(3 + i % 14, ops, 3, rng, dtype) for i in range(60)]
    N = 3001
    X = de.synth.random_X(3, N, seed=4, dtype=dtype)
    g = np.random.Generator(np.random.PCG64(11))
    y = g.standard_normal(N).astype(dtype)
    w = g.uniform(0, 2, N).astype(dtype)
    w[::9] = 0
    pop = api.Population(trees, ops, dtype, n_features=3)
    eps = np.finfo(dtype).eps
    out, ok = pop.eval(X)
    assert ok.sum() >= 20
    emax = float(np.abs(out[ok].astype(np.float64) - y).max())
    assert np.isfinite(emax)
    l2, _ = pop.eval_loss(X, y, weights=w, loss="L2")
    l1, _ = pop.eval_loss(X, y, weights=w, loss="L1")
    hub, _ = pop.eval_loss(X, y, weights=w, loss="huber", loss_param=2.0 * emax + 1.0)
    e0, _ = pop.eval_loss(X, y, weights=w, loss="l1_eps", loss_param=0.0)
    p2, _ = pop.eval_loss(X, y, weights=w, loss="lp", loss_param=2.0)
    for t in np.nonzero(ok)[0]:
        assert abs(float(hub[t]) - 0.5 * float(l2[t])) <= 64 * eps * float(l2[t]) + 1e-300
        assert abs(float(e0[t]) - float(l1[t])) <= 64 * eps * float(l1[t]) + 1e-300
        # (pow rounds each |e|^2 once more than e * e does: within the same bound)
        assert abs(float(p2[t]) - float(l2[t])) <= 64 * eps * float(l2[t]) + 1e-300
    gl2 = pop.eval_loss_grad(X, y, weights=w, loss="L2")
    ghub = pop.eval_loss_grad(X, y, weights=w, loss="huber", loss_param=2.0 * emax + 1.0)
    outg, grads, _ = pop.eval_grad(X, False)
    for t in np.nonzero(ok)[0]:
        mag = (np.abs(w.astype(np.float64) * 2 * (outg[t].astype(np.float64) - y))[None, :] * np.abs(np.asarray(grads[t], dtype=np.float64))).sum(axis=1)
        assert np.all(np.abs(ghub[1][t].astype(np.float64) - 0.5 * gl2[1][t].astype(np.float64)) <= 64 * eps * mag + 1e-300)
    pop.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_fused_loss_kinds_errors(api):
    ops = de.synth.BENCH_OPERATORS
    trees = de.synth.random_population(5, seed=1)
    pop = api.Population(trees, ops, np.float32, n_features=5)
    X = de.synth.random_X(5, 10, seed=1)
    y = np.zeros(10, np.float32)
    for kind, bad in (("huber", 0.0), ("huber", float("nan")), ("l1_eps", -1.0), ("l2_eps", float("inf")), ("quantile", 1.5), ("lp", 0.5)):
        with pytest.raises(ValueError):
            pop.eval_loss(X, y, loss=kind, loss_param=bad)
        with pytest.raises(ValueError):
            pop.eval_loss_grad(X, y, loss=kind, loss_param=bad)
    with pytest.raises(KeyError):
        pop.eval_loss(X, y, loss="hubert")
    with pytest.raises(KeyError):
        pop.eval_loss(X, y, loss="pullback")
    # the C entry points: a bad spec is DE_ERR_INVALID_ARG and de_last_error names the kind; the old ones still refuse the new values
    import ctypes as C
    lib = api.library()
    okb, lossb = np.zeros(5, np.uint8), np.zeros(5, np.float32)
    spec = api.LossSpec(16, 0, -1.0)
    rc = lib.de_eval_loss_ex(pop.ctx._h, pop._h, X.ctypes.data, 10, 5, None, y.ctypes.data, None, C.byref(spec), lossb.ctypes.data, okb.ctypes.data)
    assert rc == 1 and b"DE_LOSS_HUBER" in lib.de_last_error(pop.ctx._h)
    spec = api.LossSpec(2, 0, 0.0)
    rc = lib.de_eval_loss_ex(pop.ctx._h, pop._h, X.ctypes.data, 10, 5, None, y.ctypes.data, None, C.byref(spec), lossb.ctypes.data, okb.ctypes.data)
    assert rc == 1 and b"loss_kind" in lib.de_last_error(pop.ctx._h)
    rc = lib.de_eval_loss(pop.ctx._h, pop._h, X.ctypes.data, 10, 5, None, y.ctypes.data, None, 16, lossb.ctypes.data, okb.ctypes.data)
    assert rc == 1 and b"loss_kind" in lib.de_last_error(pop.ctx._h)
    dl = np.zeros(64, np.float32)
    rc = lib.de_eval_loss_grad(pop.ctx._h, pop._h, X.ctypes.data, 10, 5, None, 1, y.ctypes.data, None, 17, lossb.ctypes.data, dl.ctypes.data, None, okb.ctypes.data)
    assert rc == 1 and b"loss_kind" in lib.de_last_error(pop.ctx._h)
    spec = api.LossSpec(20, 0, 0.25)
    rc = lib.de_eval_loss_ex(pop.ctx._h, pop._h, X.ctypes.data, 10, 5, None, y.ctypes.data, None, C.byref(spec), lossb.ctypes.data, okb.ctypes.data)
    assert rc == 0
    pop.close()
    # Float16 and complex populations evaluate only: DE_ERR_UNSUPPORTED from the new entry points as from the old ones, outputs untouched
    ops1 = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    N = 16
    starts, off = np.array([0, N], dtype=np.int64), np.zeros(1, dtype=np.int64)
    for dt, val, word in ((np.float16, 0.5, "F16"), (np.complex64, 0.5 + 0.5j, "complex"), (np.complex128, 0.5 + 0.5j, "complex")):
        popx = api.Population([de.Node(1, de.Node(feature=1), de.Node(val=val))], ops1, dt, n_features=1)
        Xx, yx = np.asfortranarray(np.ones((1, N), dtype=dt)), np.ones(N, dtype=dt)
        for meth in ("eval_loss", "eval_loss_grad"):
            with pytest.raises(api.DeviceError, match="DE_ERR_UNSUPPORTED"):
                getattr(popx, meth)(Xx, yx, loss="huber", loss_param=1.0)
        spec = api.LossSpec(16, 0, 1.0)
        bufs = [np.full(512, 7, dtype=np.uint8) for _ in range(4)]
        ptr = [b.ctypes.data for b in bufs]
        h, ph = popx.ctx._h, popx._h
        rcs = [lib.de_eval_loss_ex(h, ph, Xx.ctypes.data, N, 1, None, yx.ctypes.data, None, C.byref(spec), ptr[0], ptr[2]),
               lib.de_eval_loss_grad_ex(h, ph, Xx.ctypes.data, N, 1, None, 1, yx.ctypes.data, None, C.byref(spec), ptr[0], ptr[1], None, ptr[2]),
               lib.de_eval_loss_grad_by_class_ex(h, ph, Xx.ctypes.data, N, 1, None, 0, yx.ctypes.data, None, C.byref(spec), starts.ctypes.data,
                                                 ptr[0], ptr[1], off.ctypes.data, ptr[3], ptr[2])]
        assert rcs == [7, 7, 7] and word in lib.de_last_error(h).decode()
        assert all((b == 7).all() for b in bufs)
        popx.close()


@pytest.mark.parametrize("one_pass", ["1", "0"])
def test_by_class_checks_the_spec_first_on_every_path(api, monkeypatch, one_pass):
    """The by-class entry points check the spec before anything else, whichever reduction follows (one pass over class-aligned tiles, or
    one call per class: DE_BY_CLASS_ONE_PASS=0) and also when there is no sample: the OLD entry point keeps refusing every kind but L2 /
    L1 / PULLBACK, the new one a bad parameter and a non-zero `reserved`; the outputs stay untouched."""
    import ctypes as C
    monkeypatch.setenv("DE_BY_CLASS_ONE_PASS", one_pass)
    lib = api.library()
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    rng = de.synth.Xoshiro256ss(7)
    P, Cn, N = 2, 3, 96
    trees = [de.synth.gen_random_tree_fixed_size(7, ops, 2, rng, np.float32, de.ParametricNode, P) for _ in range(4)]
    pop = api.Population(trees, ops, np.float32, n_features=2, n_params=P)
    g = np.random.Generator(np.random.PCG64(2))
    X = np.asfortranarray(g.standard_normal((2, N)).astype(np.float32))
    params = np.asfortranarray(g.standard_normal((P, Cn)).astype(np.float32))
    classes = np.sort(g.integers(1, Cn + 1, N))
    y = g.standard_normal(N).astype(np.float32)
    starts = np.concatenate([[0], np.cumsum(np.bincount(classes - 1, minlength=Cn))]).astype(np.int64)
    h, ph, mode = pop.ctx._h, pop._h, oracle.GRAD_BOTH
    for n, st in ((N, starts), (0, np.zeros(Cn + 1, dtype=np.int64))):
        keep = []
        pa = pop._param_args(params, classes[:n], 1, n, keep)
        bufs = [np.full(4096, 7, dtype=np.uint8) for _ in range(4)]
        lo, dl, dp, ok = (b.ctypes.data for b in bufs)

        def old(kind):
            return lib.de_eval_loss_grad_by_class(h, ph, X.ctypes.data, n, 2, C.byref(pa), mode, y.ctypes.data, None, kind, st.ctypes.data, lo, dl, None, dp, ok)

        def new(spec):
            return lib.de_eval_loss_grad_by_class_ex(h, ph, X.ctypes.data, n, 2, C.byref(pa), mode, y.ctypes.data, None, C.byref(spec), st.ctypes.data, lo, dl, None, dp, ok)

        for kind in (17, 16, 7):
            assert old(kind) == 1 and b"loss_kind" in lib.de_last_error(h), (n, kind)
        assert new(api.LossSpec(16, 0, -1.0)) == 1 and b"DE_LOSS_HUBER" in lib.de_last_error(h)
        assert new(api.LossSpec(17, 1, 0.0)) == 1 and b"reserved" in lib.de_last_error(h)
        assert new(api.LossSpec(99, 0, 0.0)) == 1 and b"loss_kind" in lib.de_last_error(h)
        assert all((b == 7).all() for b in bufs)
        if n:
            assert old(0) == 0 and new(api.LossSpec(17, 0, 0.0)) == 0  # (and the good ones pass)
    pop.close()
