"""CPU tests of the host half of the fit statistics with gradients (include/de_hip.h de_eval_fit_stats_grad): what
`FitStatsGrad` derives in float64 from the moments D, P, Q and H — the gradients of m2_p, cov, scaled_sse and r^2 against central
differences, the projected Gauss-Newton matrix against b^2 J^T W P_perp J formed with a weighted QR of [1, yhat], the rules for a tree
without variance, the refusal of a scaled fit under another kind than L2, the scaled Levenberg-Marquardt loop on the recovery case in
a numpy emulation, and the C prototype against the ctypes signature."""
import os
import re

import numpy as np
import pytest

from dynamicexpressions_jl_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def model(theta, x):
    """yhat = cos(t1 x1) + t2 x2 and its Jacobian [2, N] — the tree of the recovery case: no constant absorbs scale or offset"""
    yh = np.cos(theta[0] * x[0]) + theta[1] * x[1]
    return yh, np.stack([-x[0] * np.sin(theta[0] * x[0]), x[1]])


def moments(yh, J, y, w):
    """FitStatsGrad of ONE tree from its values and Jacobian, every sum in float64"""
    yh, J, y, w = (np.asarray(v, dtype=np.float64) for v in (yh, J, y, w))
    W = w.sum()
    mp, my = (w * yh).sum() / W, (w * y).sum() / W
    pc, yc = yh - mp, y - my
    st = api.FitStats([mp], [(w * pc * pc).sum()], [(w * pc * yc).sum()], W, my, (w * yc * yc).sum())
    H = (J * w) @ J.T
    H = np.tril(H) + np.tril(H, -1).T  # both triangles present, exactly symmetric (as the library writes them)
    return api.FitStatsGrad(st, [J @ w], [J @ (w * pc)], [J @ (w * yc)], [H], np.ones(1, dtype=bool))


def data(seed=5, n=400):
    g = np.random.default_rng(seed)
    x = g.uniform(-2.0, 2.0, (2, n))
    w = g.uniform(0.5, 1.5, n)
    w[-37:] = 0.0
    y = 2.0 - 3.0 * model(np.array([1.3, 0.7]), x)[0] + 0.3 * g.standard_normal(n)
    return x, y, w


def test_gradients_against_central_differences():
    x, y, w = data()
    theta, h = np.array([1.1, 0.9]), 1e-6
    fg = moments(*model(theta, x), y, w)
    st = fg.stats
    b, C, M, My = st.slope[0], st.cov[0], st.m2_p[0], st.m2_y
    D, P, Q = fg._dpq(0)

    def at(th):
        return moments(*model(th, x), y, w).stats

    def cd(f):
        out = np.zeros(2)
        for k in range(2):
            e = np.zeros(2)
            e[k] = h
            out[k] = (f(at(theta + e)) - f(at(theta - e))) / (2 * h)
        return out

    cases = [
        ("m2", fg.m2_grad()[0], cd(lambda s: s.m2_p[0]), np.abs(2 * P)),
        ("cov", fg.cov_grad()[0], cd(lambda s: s.cov[0]), np.abs(Q)),
        ("mean", fg.mean_grad()[0], cd(lambda s: s.mean_p[0]), np.abs(D / st.W)),
        ("scaled_sse", fg.scaled_sse_grad()[0], cd(lambda s: s.scaled_sse[0]), np.abs(2 * b * b * P) + np.abs(2 * b * Q)),
        ("r2", fg.pearson_r2_grad()[0], cd(lambda s: s.pearson_r[0] ** 2),
         np.abs(2 * C * Q / (M * My)) + np.abs(2 * C * C * P / (M * M * My))),
        ("sse", fg.sse_grad()[0], cd(lambda s: s.sse[0]), np.abs(2 * P) + np.abs(2 * Q) + np.abs(2 * (st.mean_p[0] - st.mean_y) * D)),
    ]
    for name, got, want, terms in cases:
        ratio = np.max(np.abs(got - want) / (1e-7 * (np.abs(want) + terms)))
        print(f"{name}: worst error / bound = {ratio:.3g}")
        assert ratio <= 1.0, (name, got, want)
    # the L2 gradient from the moments is the plain one
    yh, J = model(theta, x)
    assert np.allclose(fg.sse_grad()[0], J @ (2 * w * (yh - y)), rtol=1e-12, atol=0)


def test_projected_matrix_against_weighted_qr():
    x, y, w = data(seed=6)
    for theta in (np.array([1.1, 0.9]), np.array([0.4, -1.7])):
        yh, J = model(theta, x)
        fg = moments(yh, J, y, w)
        gn = fg.projected()
        sw = np.sqrt(w)
        A = np.stack([sw, sw * yh], axis=1)  # W^(1/2) [1, yhat]
        Qm, _ = np.linalg.qr(A)
        Jw = (J * sw).T
        Jp = Jw - Qm @ (Qm.T @ Jw)  # P_perp W^(1/2) J^T
        b = fg.stats.slope[0]
        want = b * b * (Jp.T @ Jp)
        H = (J * w) @ J.T
        err = np.max(np.abs(gn.jtj[0] - want)) / (b * b * np.linalg.norm(H))
        print(f"projected: error / ||b^2 H|| = {err:.3g}")
        assert err <= 1e-10
        assert np.array_equal(gn.jtj[0], gn.jtj[0].T)
        assert np.array_equal(gn.grad[0], fg.scaled_sse_grad()[0]) and np.array_equal(gn.loss, fg.stats.scaled_sse)
        assert gn.has_jtj.all()
        # the step of the projected system is a descent direction of scaled_sse
        step = gn.lm_step(1e-3, tree=0)
        assert step @ gn.grad[0] < 0
        # and the gradient is J_perp^T r with the scaled residual r = a + b yhat - y
        a = fg.stats.intercept[0]
        r = sw * (a + b * yh - y)
        assert np.allclose(gn.grad[0], 2 * b * (Jp.T @ r), rtol=1e-9, atol=1e-9 * np.linalg.norm(gn.grad[0]))


def test_degenerate_trees():
    # m2_p == 0 (a tree constant over the samples): zero gradients of the scaled quantities, zero projected matrix, zero step
    st = api.FitStats([3.0, 1.0, np.nan], [0.0, 2.0, np.nan], [0.0, 1.0, np.nan], 10.0, 0.5, 4.0)
    d = [np.array([1.0, 2.0]), np.array([0.5]), np.array([np.nan])]
    H = [np.array([[1.0, 0.0], [0.0, 0.0]]), np.array([[3.0]]), np.array([[np.nan]])]
    fg = api.FitStatsGrad(st, d, d, d, H, np.array([True, True, False]))
    assert np.array_equal(fg.has_jtj, [True, True, False]) and len(fg) == 3
    assert np.array_equal(fg.scaled_sse_grad()[0], [0.0, 0.0]) and np.array_equal(fg.pearson_r2_grad()[0], [0.0, 0.0])
    gn = fg.projected()
    assert np.array_equal(gn.jtj[0], np.zeros((2, 2))) and np.array_equal(gn.lm_step(1e-3, tree=0), [0.0, 0.0])
    assert gn.loss[0] == 4.0  # scaled_sse of a constant tree: m2_y
    # a regular tree next to it: b = 1/2, grad = 2 b (b P - Q) = -0.25, H~ = b^2 (3 - 0.25 / 10 - 0.25 / 2)
    assert np.allclose(gn.grad[1], [2 * 0.5 * (0.5 * 0.5 - 0.5)]) and np.allclose(gn.jtj[1], [[0.25 * (3.0 - 0.025 - 0.125)]])
    # an incomplete tree: NaN in, NaN out, no step
    assert np.isnan(gn.grad[2]).all() and np.isnan(gn.jtj[2]).all() and not gn.has_jtj[2]
    assert np.array_equal(gn.lm_step(1e-3, tree=2), [0.0])
    # W == 0: every moment is 0, the means NaN
    z = api.FitStatsGrad(api.FitStats([np.nan], [0.0], [0.0], 0.0, np.nan, 0.0), [np.zeros(2)], [np.zeros(2)], [np.zeros(2)],
                         [np.zeros((2, 2))], np.array([True]))
    assert np.array_equal(z.mean_grad()[0], [0.0, 0.0]) and np.array_equal(z.sse_grad()[0], [0.0, 0.0])
    assert np.array_equal(z.projected().jtj[0], np.zeros((2, 2)))
    with pytest.raises(ValueError):
        api.FitStatsGrad(st, d[:2], d, d, H, np.array([True, True, False]))


def test_scaled_fit_takes_l2_only():
    class Touched(Exception):
        pass

    class Dummy:  # any attribute access would mean the population was looked at before the refusal
        def __getattr__(self, name):
            raise Touched(name)

    for loss in ("L1", "huber", "logcosh", "pullback"):
        with pytest.raises(ValueError, match="scaled"):
            api.Population.fit_constants_lm(Dummy(), None, None, np.zeros(2), loss=loss, scaled=True)
    with pytest.raises(Touched):  # L2 goes on (and scaled=False never reaches the check)
        api.Population.fit_constants_lm(Dummy(), None, None, np.zeros(2), loss="L2", scaled=True)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_scaled_lm_loop_emulation_recovers(dtype):
    """`fit_constants_lm(scaled=True)` in numpy: values and Jacobian in `dtype`, moments in float64, the loop's own accept rule"""
    g = np.random.default_rng(11)
    N = 513
    x = g.uniform(-2.0, 2.0, (2, N)).astype(dtype)
    w = g.uniform(0.5, 1.5, N).astype(dtype)
    w[-37:] = 0
    star = np.array([1.3, 0.7])
    y = (2.0 - 3.0 * model(star, x.astype(np.float64))[0]).astype(dtype)
    u = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53
    signs = [(1, 1), (1, -1), (-1, 1), (-1, -1)]

    def ev(th):
        yh, J = model(th.astype(dtype), x)
        return moments(yh.astype(dtype), J.astype(dtype), y, w)

    worst = 0.0
    for s in signs:
        th = (star * (1.0 + 0.3 * np.array(s))).astype(dtype)
        fg = ev(th)
        gn, lam = fg.projected(), 1e-3
        first = loss = gn.loss[0]
        m2y = fg.stats.m2_y
        assert first >= 5e-3 * m2y
        for _ in range(10):
            trial = (th.astype(np.float64) + gn.lm_step(lam, tree=0)).astype(dtype)
            gt = ev(trial).projected()
            if gt.loss[0] < loss:
                th, gn, loss, lam = trial, gt, gt.loss[0], max(lam * 0.1, 1e-12)
            else:
                lam *= 10.0
        bound = max(1e-9 * first, 4 * 1024 * u * m2y)
        worst = max(worst, loss / bound)
        assert loss <= bound, (s, loss, bound)
        st = ev(th).stats
        # sqrt(final / m2_y), with final no smaller than what scaled_sse = m2_y - cov^2 / m2_p resolves (1024 u m2_y: below it the
        # computed value, which may even be 0, says nothing about the true residual)
        tol = np.sqrt(max(loss, 1024 * u * m2y) / m2y)
        assert abs(st.slope[0] + 3.0) <= 3.0 * tol and abs(st.intercept[0] - 2.0) <= 2.0 * tol
    print(f"{np.dtype(dtype).name}: worst final scaled_sse / bound = {worst:.3g}")


def test_prototype_and_exports():
    src = open(os.path.join(ROOT, "include", "de_hip.h")).read()
    m = re.search(r"\bint\s+de_eval_fit_stats_grad\s*\(([^;]*?)\)\s*;", src)
    assert m, "include/de_hip.h declares de_eval_fit_stats_grad"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 16
    assert [("*" in p) for p in params] == [True, True, True, False, False, True, False, True, True, True, True, True, True, True, True, True]
    assert "double *stats" in params[9] and "double *ystats" in params[10] and "double *dmom" in params[11]
    fn = api.library().de_eval_fit_stats_grad
    assert len(fn.argtypes) == 16
    assert "de_eval_fit_stats_grad" in api.EXPORTS and api.ABI_VERSION == 3 and re.search(r"#define\s+DE_HIP_ABI_VERSION\s+3\b", src)
    # null handles are refused before anything is touched
    assert fn(None, None, None, 0, 0, None, 1, None, None, None, None, None, None, None, None, None) == 1
