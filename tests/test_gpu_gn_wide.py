"""GPU tests of the wide Gauss-Newton route (include/de_hip.h de_eval_loss_gn_wide / de_gn_lm_step_wide / de_fit_consts_lm_wide,
DESIGN.md §4.4.7): the matrices, steps and fits of trees of 9 to 32 gradient rows, and the bits of everything else.

The population is tests/test_gpu_lm.py's narrow one (63 trees of 0 .. 8 constants), then chain(k) for k in 9, 12, 16, 17, 31, 32, 33 — linear
in their constants, so every Jacobian over X in [-2, 2) is finite and no wide tree is exempt from the bound — then the two incomplete
trees.  chain(32) and chain(33) pass the gradient kernels' LDS check at 3 features (test_the_widest_chains_fit_the_gradient_kernels).

The matrix bound is the derived one of tests/test_gpu_gauss_newton.py, unchanged:  |H - H_ref| <= 256 u A  entrywise, H_ref and A from
`GN.reference` over the device's own `eval_grad` Jacobian; for another loss kind the weight is w c, c from tests/gn_kinds_reference.py as
tests/test_gpu_gn_kinds.py forms it.  The step and loop bounds are those of tests/test_gpu_lm.py.  Every case prints the worst ratio it saw
("[gauss-newton wide ...]" lines of the parity report)."""
import ctypes as C

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import test_gpu_gauss_newton as GN
import test_gpu_gn_kinds as GK
from test_gpu_lm import U64, bad_trees, chain, damped, dev_X, offsets

pytestmark = pytest.mark.gpu
OPS = GN.OPS
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
WIDTHS = (9, 12, 16, 17, 31, 32, 33)
N_GOOD = 63
WIDE = list(range(N_GOOD, N_GOOD + len(WIDTHS) - 1))  # the trees of 9 .. 32 constants
TOO_WIDE = N_GOOD + len(WIDTHS) - 1
BAD = [TOO_WIDE + 1, TOO_WIDE + 2]


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _api.library()
    return _api


@pytest.fixture(scope="module")
def torch():
    import torch as _torch
    return _torch


def trees_of(dtype):
    good = GN.population_trees(31, range(9), dtype)
    assert len(good) == N_GOOD
    return good + [chain(k) for k in WIDTHS] + list(bad_trees())


_POPS = {}


def population(api, dtype):
    """One population per element type, shared by the cases that do not change its constants."""
    key = np.dtype(dtype)
    if key not in _POPS:
        _POPS[key] = api.Population(trees_of(dtype), OPS, dtype, n_features=3)
    return _POPS[key]


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def narrow_and_common_bits(gw, gn, ng):
    """wide=True against wide=False: every tree's loss / grad / ok, and the blocks of the trees of at most 8 rows."""
    assert np.array_equal(gw.ok, gn.ok) and same_bits(gw.loss, gn.loss)
    for t in range(len(gn)):
        assert same_bits(gw.grad[t], gn.grad[t]), t
        if ng[t] <= 8:
            assert same_bits(gw.jtj[t], gn.jtj[t]), t
            assert bool(np.asarray(gw.has_jtj)[t]) == bool(np.asarray(gn.has_jtj)[t])


def none_exempt(grads, w, dtype, which):
    fmax = float(np.finfo(dtype).max)
    for t in which:
        _, A = GN.reference(grads[t], w)
        assert np.isfinite(np.asarray(grads[t])).all() and np.isfinite(A).all() and A.max() <= 0.25 * fmax, t


def test_the_widest_chains_fit_the_gradient_kernels(api):
    for dtype in (np.float32, np.float64):
        pop = api.Population([chain(32), chain(33)], OPS, dtype, n_features=3)
        X, _, _ = GN.data(64, 3, dtype, 1)
        _, grads, ok = pop.eval_grad(X)  # (an LDS footprint beyond the kernels' is a DeviceError here)
        assert ok.all() and [g.shape[0] for g in grads] == [32, 33] and all(np.isfinite(g).all() for g in grads)
        pop.close()


@DTYPES
@pytest.mark.parametrize("N", [1, 64, 257])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_wide_matrices(api, dtype, N, weighted):
    pop = population(api, dtype)
    ng = pop._n_grad_all(api._grad_mode(False))
    assert ng[WIDE].tolist() == list(WIDTHS[:-1]) and ng[TOO_WIDE] == 33
    X, y, w = GN.data(N, 3, dtype, 40 + N, weighted)
    gw = pop.eval_gauss_newton(X, y, weights=w, wide=True)  # (without the feature: no such keyword, no such symbol)
    kernel = pop.ctx.last_kernel_name()
    gn = pop.eval_gauss_newton(X, y, weights=w)
    ok, has = np.asarray(gw.ok), np.asarray(gw.has_jtj)
    assert np.array_equal(has, ok & (ng <= 32)) and has[WIDE].all() and ok[TOO_WIDE] and not has[TOO_WIDE] and not ok[BAD].any()
    for t in [TOO_WIDE] + BAD:
        assert gw.jtj[t].size > 0 and np.isnan(gw.jtj[t]).all()
    narrow_and_common_bits(gw, gn, ng)
    for t in WIDE:
        assert np.isnan(gn.jtj[t]).all() and np.isfinite(gw.jtj[t]).all()
    _, grads, okg = pop.eval_grad(X)
    assert np.array_equal(okg, ok)
    none_exempt(grads, w, dtype, WIDE)
    worst_all, share = GN.check_bound(gw, grads, w, dtype, min_checked=40, label=f"wide N={N} w={weighted}")  # every tree with has_jtj, symmetry included
    worst = 0.0
    for t in WIDE:
        Href, A = GN.reference(grads[t], w)
        err = np.abs(np.asarray(gw.jtj[t]).astype(np.float64) - Href)
        worst = max(worst, float((err[A > 0] / (GN.unit(dtype) * A[A > 0])).max()) if (A > 0).any() else 0.0)
    print(f"[gauss-newton wide] {np.dtype(dtype).name} N={N} {'weighted' if weighted else 'unweighted'}: worst |H - H_ref| = {worst:.2f} u A over the "
          f"{len(WIDE)} wide trees ({worst_all:.2f} over all, bound {GN.K:.0f}), exempt share {100 * share:.1f} %, kernel {kernel}")


@DTYPES
def test_three_chunks_the_last_one_ragged(api, dtype, monkeypatch):
    monkeypatch.setenv("DE_GN_WIDE_CHUNK", "128")
    pop = population(api, dtype)
    X, y, w = GN.data(300, 3, dtype, 77)
    gw = pop.eval_gauss_newton(X, y, weights=w, wide=True)
    again = pop.eval_gauss_newton(X, y, weights=w, wide=True)
    assert all(same_bits(a, b) for a, b in zip(gw.jtj, again.jtj))  # run to run
    _, grads, _ = pop.eval_grad(X)
    none_exempt(grads, w, dtype, WIDE)
    worst, _ = GN.check_bound(gw, grads, w, dtype, min_checked=40, label="chunks")
    print(f"[gauss-newton wide chunks] {np.dtype(dtype).name} N=300 in chunks of 128: worst |H - H_ref| = {worst:.2f} u A (bound {GN.K:.0f})")


@DTYPES
@pytest.mark.parametrize("kind,param", [("huber", 1.3), ("L1", 0.0)])
def test_other_loss_kinds(api, dtype, kind, param):
    pop = population(api, dtype)
    ng = pop._n_grad_all(api._grad_mode(False))
    X, y, w = GN.data(257, 3, dtype, 58)
    gw = pop.eval_gauss_newton(X, y, weights=w, loss=kind, loss_param=param, e_floor=GK.FLOOR, wide=True)
    gn = pop.eval_gauss_newton(X, y, weights=w, loss=kind, loss_param=param, e_floor=GK.FLOOR)
    narrow_and_common_bits(gw, gn, ng)
    lo, dl, okl = pop.eval_loss_grad(X, y, weights=w, loss=kind, loss_param=param)
    assert same_bits(lo, gw.loss) and all(same_bits(a, b) for a, b in zip(dl, gw.grad))
    out, grads, _ = pop.eval_grad(X)
    u, worst = GN.unit(dtype), 0.0
    for t in WIDE:
        assert np.asarray(gw.has_jtj)[t]
        H, J = np.asarray(gw.jtj[t]).astype(np.float64), np.asarray(grads[t])
        wc, keep = GK.weights_c(kind, param, np.asarray(out[t]), y, w, dtype)
        Jl, wk = J.astype(np.longdouble)[:, keep], wc[keep]
        Href = ((Jl * wk) @ Jl.T).astype(np.float64)
        A = ((np.abs(Jl) * wk) @ np.abs(Jl).T).astype(np.float64)
        assert np.isfinite(J).all() and np.isfinite(A).all() and np.array_equal(H, H.T)
        err = np.abs(H - Href)
        assert (err <= GN.K * u * A).all(), (kind, t, (err / (u * np.maximum(A, np.finfo(np.float64).tiny))).max())
        worst = max(worst, float((err[A > 0] / (u * A[A > 0])).max()))
    print(f"[gauss-newton wide kinds] {np.dtype(dtype).name} {kind}: worst |M - M_ref| = {worst:.2f} u A with w c as the weight (bound {GN.K:.0f})")


@DTYPES
def test_mode_both_reaches_wide_trees_with_few_constants(api, dtype):
    trees = GN.population_trees(11, range(9), dtype)  # <= 8 constants and 3 features: G = 3 .. 11
    pop = api.Population(trees, OPS, dtype, n_features=3)
    ng = pop._n_grad_all(api._grad_mode("both"))
    wide = np.flatnonzero(ng > 8)
    assert sorted(set(ng[wide].tolist())) == [9, 10, 11] and max(pop.n_consts) == 8
    X, y, w = GN.data(257, 3, dtype, 61)
    gw = pop.eval_gauss_newton(X, y, weights=w, variable="both", wide=True)
    gn = pop.eval_gauss_newton(X, y, weights=w, variable="both")
    narrow_and_common_bits(gw, gn, ng)
    assert np.array_equal(np.asarray(gw.has_jtj), np.asarray(gw.ok)) and np.asarray(gw.has_jtj)[wide].sum() >= 5
    _, grads, _ = pop.eval_grad(X, variable="both")
    worst, share = GN.check_bound(gw, grads, w, dtype, min_checked=40, label="both")
    print(f"[gauss-newton wide both] {np.dtype(dtype).name}: worst |H - H_ref| = {worst:.2f} u A over {int(np.asarray(gw.has_jtj).sum())} trees, "
          f"{len(wide)} of them wide; exempt share {100 * share:.1f} %")
    pop.close()


@DTYPES
def test_device_tensors_with_a_padded_X(api, torch, dtype):
    pop = population(api, dtype)
    X, y, w = GN.data(257, 3, dtype, 63)
    host = pop.eval_gauss_newton(X, y, weights=w, wide=True)
    buf = torch.zeros((257, 5), dtype=torch.from_numpy(X).dtype, device="cuda")
    buf[:, :3] = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    Xd = buf[:, :3].t()  # [3, N] with ldX = 5
    assert Xd.stride() == (1, 5)
    dev = pop.eval_gauss_newton(Xd, torch.from_numpy(y).cuda(), weights=torch.from_numpy(w).cuda(), wide=True)
    torch.cuda.synchronize()
    assert all(torch.is_tensor(h) and h.is_cuda for h in dev.jtj) and torch.is_tensor(dev.loss)
    assert np.array_equal(api._host(dev.has_jtj), np.asarray(host.has_jtj)) and same_bits(api._host(dev.loss), host.loss)
    for t in range(len(host)):
        assert same_bits(api._host(dev.jtj[t]), host.jtj[t]) and same_bits(api._host(dev.grad[t]), host.grad[t]), t


@DTYPES
def test_a_population_without_a_wide_tree(api, dtype):
    pop = api.Population(GN.population_trees(31, range(9), dtype), OPS, dtype, n_features=3)
    X, y, w = GN.data(257, 3, dtype, 64)
    gw, gn = pop.eval_gauss_newton(X, y, weights=w, wide=True), pop.eval_gauss_newton(X, y, weights=w)
    assert pop.ctx.last_kernel_name() != "de_gnw_gram_kernel"
    assert same_bits(gw._packed["jtj"], gn._packed["jtj"]) and same_bits(gw._packed["dloss"], gn._packed["dloss"])
    assert same_bits(gw.loss, gn.loss) and np.array_equal(gw.ok, gn.ok) and np.array_equal(gw.has_jtj, gn.has_jtj)
    pop.close()


def test_a_program_with_shared_subtrees_is_refused_with_its_outputs_untouched(api):
    Gn = de.GraphNode
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    x1, c, c2 = Gn(feature=1), Gn(val=0.75), Gn(val=-0.4)
    sh = Gn(1, Gn(2, x1, c))
    dag = Gn(1, Gn(1, sh, Gn(2, sh, Gn(2, c, x1))), c2)  # a shared subtree: a CSE tape
    lib = api.library()
    for dtype in (np.float32, np.float64):
        pop = api.Population([dag], ops, dtype, n_features=1)
        X, y = np.asfortranarray(np.linspace(-1, 1, 64)[None, :].astype(dtype)), np.zeros(64, dtype=dtype)
        G = pop.n_grad(0, 1)
        lo, dl, jt = np.full(1, 7, dtype=dtype), np.full(G, 7, dtype=dtype), np.full(G * G, 7, dtype=dtype)
        okb = np.full(1, 9, dtype=np.uint8)
        spec = api.gn_loss_spec("L2", 0.0, 1e-4)
        rc = lib.de_eval_loss_gn_wide(pop.ctx._h, pop._h, X.ctypes.data, 64, 1, None, 1, y.ctypes.data, None, C.byref(spec), 0.0, lo.ctypes.data,
                                      dl.ctypes.data, None, jt.ctypes.data, None, okb.ctypes.data)
        assert rc == 7 and (lo == 7).all() and (dl == 7).all() and (jt == 7).all() and okb[0] == 9
        with pytest.raises(api.DeviceError, match="de_program_create_cse"):
            pop.eval_gauss_newton(X, y, wide=True)
        hist, acc = np.full(4, 7.0), np.full(1, 9, dtype=np.int32)
        rc = lib.de_fit_consts_lm_wide(pop.ctx._h, pop._h, X.ctypes.data, 64, 1, None, y.ctypes.data, None, C.byref(spec), 0.0, None, lo.ctypes.data,
                                       okb.ctypes.data, hist.ctypes.data, acc.ctypes.data)
        assert rc == 7 and (lo == 7).all() and okb[0] == 9 and (hist == 7).all() and acc[0] == 9
        pop.close()


@DTYPES
def test_wide_step_kernel(api, torch, dtype):
    pop = population(api, dtype)
    n = pop.n_trees
    X, y, w = GN.data(257, 3, dtype, 66)
    lam = np.array([(0.0, 1e-3, 1.0, 1e3)[t % 4] for t in range(n)])
    lam[WIDE] = [1e-3, 1.0, 1e3, 1e-3, 1.0, 0.0]
    gw, gn = pop.eval_gauss_newton(X, y, weights=w, wide=True), pop.eval_gauss_newton(X, y, weights=w)
    ng = gw._packed["n_grad"].astype(np.int64)
    off = offsets(ng)
    step, narrow_step = gw.lm_step_device(lam), gn.lm_step_device(lam)
    has = np.asarray(gw.has_jtj)
    host_steps = gw.lm_step(lam)
    worst, n_fwd, n_wide_nonzero = 0.0, 0, 0
    for t in range(n):
        G, mine = int(ng[t]), step[off[t]:off[t + 1]]
        if G <= 8:
            assert mine.tobytes() == narrow_step[off[t]:off[t + 1]].tobytes(), t  # de_gn_lm_step's bytes
        if not has[t] or G == 0:
            assert not mine.any(), t  # 33 rows, incomplete and constant-free trees: exactly zero
            continue
        H, g = np.asarray(gw.jtj[t]).astype(np.float64), np.asarray(gw.grad[t]).astype(np.float64)
        want, produced = api.lm_solve_host_wide(H, g, lam[t])
        assert mine.tobytes() == want.tobytes(), (t, G, mine, want)  # one header on both sides: the same bits
        n_wide_nonzero += int(G > 8 and produced and mine.any())
        if not (np.isfinite(H).all() and np.isfinite(g).all()):
            continue
        cond = np.linalg.cond(damped(H, lam[t]), 2)
        if lam[t] >= 1e-3 and cond < 1e12:
            ref = host_steps[t]
            err, bound = np.linalg.norm(mine - ref), 8 * G * G * U64 * cond * np.linalg.norm(ref)
            assert err <= bound, (t, G, lam[t], err / bound)
            worst, n_fwd = max(worst, err / bound if bound else 0.0), n_fwd + 1
    assert n_fwd >= 25 and n_wide_nonzero >= 5, (n_fwd, n_wide_nonzero)
    assert not narrow_step[off[WIDE[0]]:off[TOO_WIDE + 1]].any()  # (the narrow call leaves every wide tree the zero step)
    # device tensors: the same bits
    Xd, yd, wd = dev_X(torch, X), torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda()
    gd = pop.eval_gauss_newton(Xd, yd, weights=wd, wide=True)
    sd = gd.lm_step_device(torch.from_numpy(lam).cuda())
    assert torch.is_tensor(sd) and sd.is_cuda and sd.cpu().numpy().tobytes() == step.tobytes()
    # caller-chosen offsets with gaps: entries no tree owns keep the sentinel
    lib = api.library()
    off2 = (off[:-1] + 2 * np.arange(n)).astype(np.int64)
    span2 = int(off2[-1] + ng[-1]) + 3
    dl2, owned = np.full(span2, np.nan, dtype=dtype), np.zeros(span2, dtype=bool)
    for t in range(n):
        dl2[off2[t]:off2[t] + ng[t]] = gw._packed["dloss"][off[t]:off[t + 1]]
        owned[off2[t]:off2[t] + ng[t]] = True
    hasb, st2 = has.astype(np.uint8), np.full(span2, 7.0)
    pop.ctx.check(lib.de_gn_lm_step_wide(pop.ctx._h, api._dtype_code(dtype), n, gw._packed["n_grad"].ctypes.data, dl2.ctypes.data, off2.ctypes.data,
                                         gw._packed["jtj"].ctypes.data, None, hasb.ctypes.data, lam.ctypes.data, st2.ctypes.data))
    assert (st2[~owned] == 7.0).all() and st2[owned].tobytes() == step.tobytes()
    print(f"[gauss-newton wide step] {np.dtype(dtype).name}: {n_wide_nonzero} wide steps equal de_lm_solve_host_wide bit for bit; against lm_step worst "
          f"{worst:.3g} of the forward bound over {n_fwd} trees")


@DTYPES
def test_wide_fit_on_the_device(api, dtype):
    trees = trees_of(dtype)
    pop = api.Population(trees, OPS, dtype, n_features=3)  # (its own population: the fit changes the constants)
    X, _, w = GN.data(257, 3, dtype, 67)
    at = offsets(pop.n_consts)
    cstar = pop.constants().copy()
    out, ok_e = pop.eval(X)
    i32 = N_GOOD + WIDTHS.index(32)
    assert ok_e[i32]
    y = np.ascontiguousarray(out[i32]).astype(dtype)  # chain(32)(X; c*): every chain of at least three constants can reach it
    xi = np.random.default_rng(5).standard_normal(cstar.size)
    consts0 = (cstar.astype(np.float64) * (1 + 0.05 * xi)).astype(dtype)
    hn, hw = [], []
    cn, ln, okn = pop.fit_constants_lm_device(X, y, consts0, weights=w, iters=6, history=hn)
    accn = np.asarray(pop.lm_accepts).copy()
    cw, lw, okw = pop.fit_constants_lm_device(X, y, consts0, weights=w, iters=6, history=hw, wide=True)
    accw = np.asarray(pop.lm_accepts).copy()
    assert np.array_equal(okn, okw) and len(hw) == 7
    ng = np.asarray(pop.n_consts)
    for t in range(pop.n_trees):
        a, b = at[t], at[t + 1]
        if ng[t] <= 8:  # the narrow trees: the trajectory of the default call, bit for bit
            assert cw[a:b].tobytes() == cn[a:b].tobytes() and same_bits(lw[t:t + 1], ln[t:t + 1]) and accw[t] == accn[t], t
            assert all(same_bits(r1[t:t + 1], r2[t:t + 1]) for r1, r2 in zip(hw, hn)), t
    for t in WIDE:
        a, b = at[t], at[t + 1]
        assert okw[t] and accn[t] == 0 and cn[a:b].tobytes() == consts0[a:b].tobytes()  # (the default call leaves a wide tree alone)
        col = np.array([r[t] for r in hw])
        assert accw[t] >= 1 and (col[1:] <= col[:-1]).all() and col[-1] < col[0], (t, accw[t], col)
        assert float(lw[t]) == col[-1]
    for t in [TOO_WIDE] + BAD:  # 33 rows, incomplete: the constants' bits stay
        assert cw[at[t]:at[t + 1]].tobytes() == consts0[at[t]:at[t + 1]].tobytes() and accw[t] == 0
    assert pop.constants().tobytes() == cw.tobytes()
    lo, _, okl = pop.eval_loss_grad(X, y, weights=w)  # at the returned constants
    assert np.array_equal(okl, okw) and same_bits(lo, lw)
    ratio = max(float(hw[-1][t] / hw[0][t]) for t in WIDE)
    # the first iteration against the host rule of tests/test_gpu_lm.py
    pop.set_constants(consts0)
    g0 = pop.eval_gauss_newton(X, y, weights=w, wide=True)
    steps = g0.lm_step(1e-3)
    c1, _, _ = pop.fit_constants_lm_device(X, y, consts0, weights=w, iters=1, wide=True)
    acc1, moved = np.asarray(pop.lm_accepts), 0
    for t in WIDE:
        a, b = at[t], at[t + 1]
        if c1[a:b].tobytes() == consts0[a:b].tobytes():
            assert acc1[t] == 0
            continue
        G = b - a
        want = (consts0[a:b].astype(np.float64) + steps[t]).astype(dtype)
        cond = np.linalg.cond(damped(np.asarray(g0.jtj[t]).astype(np.float64), 1e-3), 2)
        tol = np.spacing(np.abs(want)).astype(np.float64) + 8 * G * G * U64 * cond * np.abs(steps[t]).max()
        assert acc1[t] == 1 and (np.abs(c1[a:b].astype(np.float64) - want.astype(np.float64)) <= tol).all(), (t, c1[a:b], want, tol)
        moved += 1
    assert moved >= 4, moved
    print(f"[gauss-newton wide fit] {np.dtype(dtype).name}: accepted steps of the wide trees {accw[WIDE].tolist()}, worst loss_final / loss_initial "
          f"{ratio:.3g}; first iteration: {moved} of {len(WIDE)} moved to T(c0 + lm_step(1e-3))")
    pop.close()
