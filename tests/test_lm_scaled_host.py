"""CPU tests of the arithmetic of the device-side Levenberg-Marquardt step under linear scaling (include/de_hip.h de_lm_project_host,
DESIGN.md §4.4.8): the host-only hook runs csrc/de_lm_project.h, the code de_lm_step_scaled_kernel runs.

The header writes `FitStats.scaled_sse`, `FitStatsGrad.scaled_sse_grad` and `FitStatsGrad.projected()` out in their own association, in
float64 and without contraction, so the hook equals numpy BIT FOR BIT (both triangles).  The step `lm_solve_host(Ht, g, lam)` is held to
tests/test_lm_host.py's forward bound against numpy's solve of the same system,
    |delta - delta_np| <= 8 G^2 u cond_2(A) |delta_np|,   u = 2^-53,   A = Ht + lam diag(diag Ht);
random J with N >= 64 samples keeps the projected matrix regular, so no system is exempt."""
import os
import re

import numpy as np
import pytest

from dynamicexpressions_jl_amd import api
import test_fit_stats_grad_host as FSG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53


def damped(H, lam):
    A = np.array(H, dtype=np.float64)
    for j in range(A.shape[0]):
        A[j, j] = A[j, j] + np.float64(lam) * A[j, j]
    return A


def draw(seed):
    """(G, N, dtype, FitStatsGrad of one tree) over G = 1 .. 8, N in {64, 300}: rows scaled by exp(U(-3, 3)), weights with some zeros,
    moments and H in float64, H rounded through float32 or float64"""
    g = np.random.default_rng(seed)
    for G in range(1, 9):
        for N in (64, 300):
            for dtype in (np.float32, np.float64):
                J = g.standard_normal((G, N)) * np.exp(g.uniform(-3.0, 3.0, (G, 1)))
                yh, y = g.standard_normal(N) * 1.5 + 0.3, g.standard_normal(N) - 0.7
                w = g.uniform(0.25, 2.0, N)
                w[g.integers(0, N, N // 8)] = 0.0
                fg = FSG.moments(yh, J, y, w)
                H = fg.jtj[0].astype(dtype).astype(np.float64)
                fg.jtj[0] = np.tril(H) + np.tril(H, -1).T
                yield G, N, dtype, fg


def hook(fg, t=0):
    st = fg.stats
    D, P, Q = fg._dpq(t)
    return api.lm_project_host([st.mean_p[t], st.m2_p[t], st.cov[t]], [st.W, st.mean_y, st.m2_y], D, P, Q, fg.jtj[t])


@pytest.mark.parametrize("seed", range(3))
def test_bit_equal_to_numpy_and_forward_bound(seed):
    worst, n = 0.0, 0
    for G, N, dtype, fg in draw(seed):
        gn = fg.projected()
        sse, g, Ht, formed = hook(fg)
        assert formed, (G, N, dtype)
        assert np.float64(sse).tobytes() == np.float64(fg.stats.scaled_sse[0]).tobytes() == np.float64(gn.loss[0]).tobytes()
        assert g.tobytes() == fg.scaled_sse_grad()[0].tobytes() == np.asarray(gn.grad[0]).tobytes(), (G, N, dtype)
        assert np.ascontiguousarray(Ht).tobytes() == np.ascontiguousarray(gn.jtj[0]).tobytes(), (G, N, dtype)  # both triangles
        assert np.array_equal(Ht, Ht.T)
        for lam in (1e-3, 1.0, 1e3):
            step, produced = api.lm_solve_host(Ht, g, lam)
            assert produced, (G, N, dtype, lam)  # no system is exempt
            ref = gn.lm_step(lam, tree=0)
            cond = np.linalg.cond(damped(Ht, lam), 2)
            err, bound = np.linalg.norm(step - ref), 8 * G * G * U64 * cond * np.linalg.norm(ref)
            assert np.isfinite(cond) and ref.any() and err <= bound, (G, N, dtype, lam, err, bound)
            worst, n = max(worst, err / bound), n + 1
    assert n == 8 * 2 * 2 * 3
    print(f"[lm scaled host] seed {seed}: {n} systems bit-equal to projected(); worst forward error {worst:.3g} of the bound")


def test_not_formed_rules():
    D, P, Q = np.array([1.0, 2.0]), np.array([0.5, 0.2]), np.array([0.3, 0.1])
    H = np.array([[2.0, 0.5], [0.5, 3.0]])
    ys = [10.0, 0.5, 4.0]
    # a regular tree is formed, and its step is produced
    sse, g, Ht, formed = api.lm_project_host([0.1, 2.0, 1.0], ys, D, P, Q, H)
    assert formed and sse == 4.0 - 1.0 / 2.0 and g.any() and api.lm_solve_host(Ht, g, 1e-3)[1]
    # M2_p == 0 (a tree constant over the samples) and W == 0: not formed, zeros, sse = M2_y — or NaN where C is NaN
    for st, y3, want in (([3.0, 0.0, 0.0], ys, 4.0), ([3.0, 0.0, np.nan], ys, np.nan), ([np.nan, 0.0, 0.0], [0.0, np.nan, 0.0], 0.0),
                         ([np.nan, 2.0, 1.0], [0.0, np.nan, 4.0], 4.0)):
        sse, g, Ht, formed = api.lm_project_host(st, y3, D, P, Q, H)
        assert not formed and not g.any() and not Ht.any() and (sse == want or (np.isnan(want) and np.isnan(sse))), (st, y3)
        step, produced = api.lm_solve_host(Ht, g, 1e-3)
        assert not produced and not step.any()
    # ... as FitStats / projected() have it
    fg = api.FitStatsGrad(api.FitStats([3.0], [0.0], [0.0], *ys), [D], [P], [Q], [H], np.ones(1, dtype=bool))
    gn = fg.projected()
    assert gn.loss[0] == 4.0 and not gn.grad[0].any() and not gn.jtj[0].any()
    # NaN statistics (an incomplete tree) propagate, and the solve answers the zero step
    nan = np.nan
    sse, g, Ht, formed = api.lm_project_host([nan, nan, nan], ys, D * nan, P * nan, Q * nan, H * nan)
    assert np.isnan(sse) and np.isnan(g).all() and np.isnan(Ht).all()
    step, produced = api.lm_solve_host(Ht, g, 1e-3)
    assert not produced and step.tolist() == [0.0, 0.0]
    sse, g, Ht, formed = api.lm_project_host([0.1, 2.0, 1.0], ys, D, [nan, 0.2], Q, H)
    assert formed and not api.lm_solve_host(Ht, g, 1e-3)[1]
    # G = 0 and G = 9: not formed; the wide system's g and Ht are zero-filled
    lib = api.library()
    st3, ys3, one = np.array([0.1, 2.0, 1.0]), np.array(ys), np.full(1, 7.0)
    sse = np.full(1, 7.0)
    assert lib.de_lm_project_host(0, st3.ctypes.data, ys3.ctypes.data, one.ctypes.data, one.ctypes.data, sse.ctypes.data, one.ctypes.data,
                                  one.ctypes.data) == 0 and one[0] == 7.0 and sse[0] == 3.5
    sse, g, Ht, formed = api.lm_project_host([0.1, 2.0, 1.0], ys, np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((0, 0)))
    assert not formed and g.size == 0 and sse == 3.5
    sse, g, Ht, formed = api.lm_project_host([0.1, 2.0, 1.0], ys, np.ones(9), np.ones(9), np.ones(9), np.eye(9))
    assert not formed and g.shape == (9,) and Ht.shape == (9, 9) and not g.any() and not Ht.any() and sse == 3.5
    assert lib.de_lm_project_host(2, None, None, None, None, None, None, None) == 0


def test_prototypes_and_null_contexts():
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "de_hip.h")).read(), flags=re.S)
    lib = api.library()
    for name, n_args in (("de_lm_project_host", 8), ("de_fit_stats_lm_step", 14), ("de_fit_consts_lm_scaled", 15)):
        m = re.search(r"^int %s\(([^;]*)\);" % name, src, re.M)
        assert m, f"include/de_hip.h declares {name}"
        assert len(m.group(1).split(",")) == n_args == len(getattr(lib, name).argtypes)
        assert name in api.EXPORTS
    assert api.ABI_VERSION == 3 == lib.de_abi_version() and re.search(r"#define\s+DE_HIP_ABI_VERSION\s+3\b", src)
    assert re.search(r"\(l\) de_fit_stats_lm_step", open(os.path.join(ROOT, "include", "de_hip.h")).read())
    # null contexts are refused without a device
    assert lib.de_fit_stats_lm_step(None, 0, 1, None, None, None, None, None, None, None, None, None, None, None) == 1
    assert lib.de_fit_consts_lm_scaled(None, None, None, 0, 0, None, None, None, None, None, None, None, None, None, None) == 1


def test_scaled_device_fit_takes_l2_and_narrow_trees_only():
    class Touched(Exception):
        pass

    class Dummy:  # any attribute access would mean the population was looked at before the refusal
        def __getattr__(self, name):
            raise Touched(name)

    for kw in (dict(wide=True), dict(loss="huber"), dict(loss="L1"), dict(loss="huber", wide=True)):
        with pytest.raises(ValueError, match="scaled"):
            api.Population.fit_constants_lm_device(Dummy(), None, None, np.zeros(2), scaled=True, **kw)
    with pytest.raises(Touched):  # L2 and narrow goes on
        api.Population.fit_constants_lm_device(Dummy(), None, None, np.zeros(2), scaled=True)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_scaled_loop_emulation_driven_by_the_hook_recovers(dtype):
    """tests/test_fit_stats_grad_host.py's recovery case, cos(c1 x1) + c2 x2 against 2 - 3 (...), with the step and the objective taken
    from the hook (what the device loop runs) instead of projected() / lm_step: the same bound,
    final scaled_sse <= max(1e-9 initial, 4 * 1024 u m2_y)."""
    g = np.random.default_rng(11)
    N = 513
    x = g.uniform(-2.0, 2.0, (2, N)).astype(dtype)
    w = g.uniform(0.5, 1.5, N).astype(dtype)
    w[-37:] = 0
    star = np.array([1.3, 0.7])
    y = (2.0 - 3.0 * FSG.model(star, x.astype(np.float64))[0]).astype(dtype)
    u = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53

    def ev(th):
        yh, J = FSG.model(th.astype(dtype), x)
        fg = FSG.moments(yh.astype(dtype), J.astype(dtype), y, w)
        fg.jtj[0] = fg.jtj[0].astype(dtype).astype(np.float64)  # (the matrix has the population's element type)
        sse, gr, Ht, formed = hook(fg)
        assert formed
        return fg, sse, gr, Ht

    worst = 0.0
    for s in [(1, 1), (1, -1), (-1, 1), (-1, -1)]:
        th = (star * (1.0 + 0.3 * np.array(s))).astype(dtype)
        fg, loss, gr, Ht = ev(th)
        first, lam, m2y = loss, 1e-3, fg.stats.m2_y
        assert first >= 5e-3 * m2y
        for _ in range(10):
            step, produced = api.lm_solve_host(Ht, gr, lam)
            trial = (th.astype(np.float64) + step).astype(dtype) if produced else th
            fgt, loss_t, gr_t, Ht_t = ev(trial)
            if loss_t < loss:
                th, fg, loss, gr, Ht, lam = trial, fgt, loss_t, gr_t, Ht_t, max(lam * 0.1, 1e-12)
            else:
                lam *= 10.0
        bound = max(1e-9 * first, 4 * 1024 * u * m2y)
        worst = max(worst, loss / bound)
        assert loss <= bound, (s, loss, bound)
        tol = np.sqrt(max(loss, 1024 * u * m2y) / m2y)
        assert abs(fg.stats.slope[0] + 3.0) <= 3.0 * tol and abs(fg.stats.intercept[0] - 2.0) <= 2.0 * tol
    print(f"{np.dtype(dtype).name}: worst final scaled_sse / bound = {worst:.3g}")
