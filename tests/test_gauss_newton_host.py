"""CPU tests of the host half of the Gauss-Newton entry point (include/de_hip.h de_eval_loss_gn): the
Levenberg-Marquardt step `GaussNewton.lm_step` forms in float64 against numpy.linalg.solve, its zero step for singular, non-finite
and matrix-less trees, the S H S^T combination of a GraphNode's shared constants, the offsets `Population.eval_gauss_newton` hands
the library, and the C prototype against the ctypes signature."""
import os
import re

import numpy as np
import pytest

from dynamicexpressions_jl_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spd(g, n, scale=1.0):
    a = g.standard_normal((n + 3, n)) * scale
    return a.T @ a


def make(mats, grads, ok=None, has=None):
    n = len(mats)
    ok = np.ones(n, dtype=bool) if ok is None else np.asarray(ok, dtype=bool)
    return api.GaussNewton(np.zeros(n), grads, mats, ok, has)


def test_lm_step_against_numpy_solve():
    g = np.random.default_rng(3)
    mats = [spd(g, n) for n in (1, 2, 3, 5, 8)]
    grads = [g.standard_normal(h.shape[0]) for h in mats]
    gn = make(mats, grads)
    assert gn.has_jtj.all() and len(gn) == 5
    for lam in (0.0, 1e-3, 2.5):
        steps = gn.lm_step(lam)
        for h, d, s in zip(mats, grads, steps):
            want = np.linalg.solve(h + lam * np.diag(np.diag(h)), -0.5 * d)
            assert s.dtype == np.float64 and np.array_equal(s, want)
    # float32 inputs are solved in float64
    gn32 = make([h.astype(np.float32) for h in mats], [d.astype(np.float32) for d in grads])
    for h, d, s in zip(mats, grads, gn32.lm_step(0.5)):
        h32, d32 = h.astype(np.float32).astype(np.float64), d.astype(np.float32).astype(np.float64)
        assert s.dtype == np.float64 and np.array_equal(s, np.linalg.solve(h32 + 0.5 * np.diag(np.diag(h32)), -0.5 * d32))


def test_lm_step_scalar_and_per_tree_lambda_and_single_tree():
    g = np.random.default_rng(4)
    mats = [spd(g, 3) for _ in range(4)]
    grads = [g.standard_normal(3) for _ in range(4)]
    gn = make(mats, grads)
    lam = np.array([0.0, 1e-3, 1.0, 10.0])
    per_tree = gn.lm_step(lam)
    for t in range(4):
        assert np.array_equal(per_tree[t], make([mats[t]], [grads[t]]).lm_step(float(lam[t]))[0])
        assert np.array_equal(per_tree[t], gn.lm_step(lam, tree=t))
    same = gn.lm_step(0.25)
    assert all(np.array_equal(a, b) for a, b in zip(same, gn.lm_step(np.full(4, 0.25))))
    # Marquardt's scaling: lam multiplies diag(H), so a larger lam shortens the step
    assert np.linalg.norm(gn.lm_step(10.0, tree=0)) < np.linalg.norm(gn.lm_step(0.0, tree=0))


def test_lm_step_is_zero_where_there_is_nothing_to_solve():
    g = np.random.default_rng(5)
    good = spd(g, 2)
    singular = np.array([[1.0, 1.0], [1.0, 1.0]])
    zero_row = np.array([[2.0, 0.0], [0.0, 0.0]])
    nan_mat = np.array([[1.0, np.nan], [np.nan, 1.0]])
    wide = np.full((9, 9), np.nan)
    mats = [good, singular, zero_row, nan_mat, good, good, wide, np.zeros((0, 0))]
    grads = [np.ones(2), np.ones(2), np.ones(2), np.ones(2), np.array([1.0, np.inf]), np.ones(2), np.ones(9), np.zeros(0)]
    ok = [1, 1, 1, 1, 1, 0, 1, 1]
    gn = make(mats, grads, ok)
    assert gn.has_jtj.tolist() == [True, True, True, True, True, False, False, True]  # incomplete; wider than GN_MAX_ROWS
    steps = gn.lm_step(0.0)
    assert np.array_equal(steps[0], np.linalg.solve(good, -0.5 * np.ones(2)))
    for t in (1, 2, 3, 4, 5, 6):
        assert steps[t].shape == grads[t].shape and not steps[t].any(), t
    assert steps[7].shape == (0,)
    assert not gn.lm_step(1.0, tree=2).any()  # lam * diag(H) leaves the zero row singular
    # an explicit has_jtj wins over the one derived from ok and the width
    assert not make([good], [np.ones(2)], has=np.array([False])).lm_step(0.0)[0].any()
    with pytest.raises(ValueError):
        api.GaussNewton(np.zeros(2), [np.ones(1)], [np.ones((1, 1))], np.ones(2, dtype=bool))


def test_shared_constants_combine_on_both_sides():
    # occurrence rows (c0, c1, c0, c2) behind two feature rows: S sums occurrence 0 and 2
    o = np.array([0, 1, 0, 2])
    g = np.random.default_rng(6)
    J = g.standard_normal((6, 50))
    H = J @ J.T
    S = np.zeros((5, 6))
    S[0, 0] = S[1, 1] = 1
    for k, u in enumerate(o):
        S[2 + u, 2 + k] = 1
    got = api.gn_combine(H, o)
    assert got.shape == (5, 5) and np.allclose(got, S @ H @ S.T, rtol=1e-13, atol=0)
    Jc = S @ J  # the matrix of the combined Jacobian rows is the same thing
    assert np.allclose(got, Jc @ Jc.T, rtol=1e-12, atol=1e-12)
    assert api.gn_combine(H, None) is H
    # constants only (no leading rows), and an exact small case
    H3 = np.array([[1.0, 2.0, 3.0], [2.0, 5.0, 7.0], [3.0, 7.0, 11.0]])
    assert np.array_equal(api.gn_combine(H3, np.array([0, 1, 0])), np.array([[1 + 3 + 3 + 11.0, 2 + 7.0], [2 + 7.0, 5.0]]))
    torch = pytest.importorskip("torch")
    assert np.array_equal(api.gn_combine(torch.from_numpy(H3), np.array([0, 1, 0])).numpy(), api.gn_combine(H3, np.array([0, 1, 0])))


def test_offsets_of_a_mixed_width_population():
    doff, joff = api.gn_offsets([0, 3, 1, 9, 8, 0, 2])
    assert doff.dtype == np.int64 and joff.dtype == np.int64
    assert doff.tolist() == [0, 0, 3, 4, 13, 21, 21, 23]
    assert joff.tolist() == [0, 0, 9, 10, 91, 155, 155, 159]  # a wide tree keeps its (NaN) block: G^2 entries whatever G is
    d0, j0 = api.gn_offsets([])
    assert d0.tolist() == [0] and j0.tolist() == [0]
    assert api.GN_MAX_ROWS == 8


def test_c_prototype_matches_ctypes():
    import ctypes as C
    src = open(os.path.join(ROOT, "include", "de_hip.h")).read()
    m = re.search(r"\bint\s+de_eval_loss_gn\s*\(([^;]*?)\)\s*;", src)
    assert m, "include/de_hip.h declares de_eval_loss_gn"
    params = [p.strip() for p in " ".join(m.group(1).split()).split(",")]
    assert len(params) == 15
    lib = api.library()
    fn = lib.de_eval_loss_gn
    assert len(fn.argtypes) == 15
    for prm, at in zip(params, fn.argtypes):
        if "*" in prm:
            assert at in (C.c_void_p,) or issubclass(at, C._Pointer), prm
        elif prm.startswith("int64_t"):
            assert at is C.c_int64, prm
        else:
            assert at is C.c_int, prm
    assert re.search(r"\bint\s+de_gn_max_rows\s*\(\s*void\s*\)\s*;", src)
    assert lib.de_gn_max_rows() == api.GN_MAX_ROWS == 8
    assert {"de_eval_loss_gn", "de_gn_max_rows"} <= set(api.EXPORTS)
    assert api.ABI_VERSION == 3 and re.search(r"#define\s+DE_HIP_ABI_VERSION\s+3\b", src)
    # null context / program: refused without touching anything (no device needed)
    assert fn(None, None, None, 0, 0, None, 1, None, None, None, None, None, None, None, None) == 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_lm_loop_emulated_in_numpy_reaches_the_floor(dtype):
    """The basis of the GPU test's 1e-9: the algorithm of Population.fit_constants_lm on c0 cos(c1 x) + c2 with the model, its
    Jacobian and the sums formed in numpy in the element type, the steps by GaussNewton.lm_step."""
    g = np.random.default_rng(0)
    x = g.uniform(-2, 2, 1000).astype(dtype)
    y = (2.0 * np.cos(1.5 * x.astype(np.float64)) - 0.5).astype(dtype)

    def normal_equations(c):
        c = c.astype(dtype)
        u = c[1] * x
        e = (c[0] * np.cos(u) + c[2]) - y
        J = np.stack([np.cos(u), -c[0] * np.sin(u) * x, np.ones_like(x)]).astype(dtype)
        return float((e * e).sum(dtype=dtype)), (2 * e * J).sum(axis=1, dtype=dtype), (J[:, None, :] * J[None, :, :]).sum(axis=2, dtype=dtype)

    c = np.array([1.7, 1.4, 0.0], dtype=dtype)
    loss, grad, H = normal_equations(c)
    first, lam, hist = loss, 1e-3, [loss]
    for _ in range(10):
        step = api.GaussNewton(np.array([loss]), [grad], [H], np.array([True])).lm_step(lam, tree=0)
        trial = (c.astype(np.float64) + step).astype(dtype)
        lt, gt, Ht = normal_equations(trial)
        if lt < loss:
            c, loss, grad, H, lam = trial, lt, gt, Ht, max(lam * 0.1, 1e-12)
        else:
            lam *= 10.0
        hist.append(loss)
    assert all(b <= a for a, b in zip(hist, hist[1:]))
    assert hist[4] <= 1e-9 * first and loss <= 1e-12 * first, hist
    assert np.allclose(c, [2.0, 1.5, -0.5], atol=1e-5)
    # the linear model of the GPU test: cond(J J^T) ~ 1.17
    X = np.random.default_rng(1).standard_normal((2, 1000)).astype(np.float32)
    J = np.stack([X[0], X[1], np.ones(1000)]).astype(np.float64)
    assert abs(np.linalg.cond(J @ J.T) - 1.17) < 0.01
