"""GPU tests of Levenberg-Marquardt on the constants on the device (include/de_hip.h de_gn_lm_step / de_fit_consts_lm).

The step kernel runs csrc/de_lm_solve.h, the code behind the host hook de_lm_solve_host: the two agree BIT FOR BIT on the same buffers.
Against the host's `GaussNewton.lm_step` (numpy's LU) the forward bound of tests/test_lm_host.py applies,
    |delta - delta_np| <= 8 G^2 u cond_2(A) |delta_np|,   u = 2^-53,
for trees with has_jtj, cond_2(A) < 10^12 and lam >= 1e-3.  One iteration of the loop is held to the host rule: a tree's constants
afterwards are its consts0 bits, or T(c0 + lm_step(lam0)) within 1 ulp_T + 8 G^2 u cond_2(A) |delta|_inf.  The loop scenarios are those of
tests/test_gpu_gauss_newton.py (a linear model, 30 jittered copies of c0 cos(c1 x) + c2) with those tests' own bounds."""
import ctypes as C

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import test_gpu_gauss_newton as GN

pytestmark = pytest.mark.gpu
OPS = GN.OPS
U64 = 2.0 ** -53
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


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


def chain(k):  # x1 * c1 + x2 * c2 + ... : k constants, every one with a non-trivial row
    t = de.Node(3, de.Node(feature=1), de.Node(val=0.5))
    for i in range(1, k):
        t = de.Node(1, t, de.Node(3, de.Node(feature=1 + i % 3), de.Node(val=0.25 * (i + 1))))
    return t


def bad_trees():
    x1, x2 = de.Node(feature=1), de.Node(feature=2)
    div0 = de.Node(1, de.Node(4, de.Node(val=1.5), de.Node(2, x1, x1)), de.Node(val=0.5))       # 1.5 / (x1 - x1) + 0.5
    big = de.Node(3, de.Node(val=2.0), de.Node(2, de.Node(2, de.Node(3, de.Node(val=60.0), x2))))  # 2 * exp(exp(60 * x2))
    return div0, big


def dev_X(torch, X):
    return torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()


def damped(H, lam):
    A = np.array(H, dtype=np.float64)
    for j in range(A.shape[0]):
        A[j, j] = A[j, j] + lam * A[j, j]
    return A


def offsets(ng):
    off = np.zeros(len(ng) + 1, dtype=np.int64)
    np.cumsum(ng, out=off[1:])
    return off


# ---- 1. the step kernel --------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("N", [64, 257])
def test_step_kernel_against_the_host_hook_and_lm_step(api, torch, dtype, N):
    good = GN.population_trees(31, range(9), dtype)
    div0, big = bad_trees()
    trees = good + [chain(9), chain(12), div0, big]
    wide, bad = [len(good), len(good) + 1], [len(good) + 2, len(good) + 3]
    pop, alone = api.Population(trees, OPS, dtype, n_features=3), api.Population(good, OPS, dtype, n_features=3)
    X, y, w = GN.data(N, 3, dtype, 40 + N)
    lam = np.array([(0.0, 1e-3, 1.0, 1e3)[t % 4] for t in range(len(trees))])
    gn = pop.eval_gauss_newton(X, y, weights=w)
    ng = gn._packed["n_grad"].astype(np.int64)
    off = offsets(ng)
    assert sorted(set(ng[:len(good)].tolist())) == list(range(9)) and ng[wide].tolist() == [9, 12]
    step = gn.lm_step_device(lam)
    assert step.dtype == np.float64 and step.shape == (int(off[-1]),)
    has = np.asarray(gn.has_jtj)
    assert not has[wide].any() and not has[bad].any() and has.sum() >= 40
    host_steps = gn.lm_step(lam)
    worst, n_fwd, n_nonzero = 0.0, 0, 0
    for t in range(len(trees)):
        G, mine = int(ng[t]), step[off[t]:off[t + 1]]
        if not has[t] or G == 0:
            assert not mine.any(), t  # wide, incomplete and constant-free trees: exactly zero
            continue
        H, g = np.asarray(gn.jtj[t]).astype(np.float64), np.asarray(gn.grad[t]).astype(np.float64)
        want, produced = api.lm_solve_host(H, g, lam[t])
        assert mine.tobytes() == want.tobytes(), (t, mine, want)  # the same header on both sides: the same bits
        n_nonzero += int(produced and mine.any())
        if not (np.isfinite(H).all() and np.isfinite(g).all()):
            continue
        cond = np.linalg.cond(damped(H, lam[t]), 2)
        if lam[t] >= 1e-3 and cond < 1e12:
            ref = host_steps[t]
            err, bound = np.linalg.norm(mine - ref), 8 * G * G * U64 * cond * np.linalg.norm(ref)
            assert err <= bound, (t, G, lam[t], err / bound)
            worst, n_fwd = max(worst, err / bound if bound else 0.0), n_fwd + 1
    assert n_fwd >= 20 and n_nonzero >= 30, (n_fwd, n_nonzero)
    # neighbours: the population without the wide and incomplete trees gives the same bytes
    ga = alone.eval_gauss_newton(X, y, weights=w)
    assert ga.lm_step_device(lam[:len(good)]).tobytes() == step[:off[len(good)]].tobytes()
    # device tensors: the same bits, nothing copied
    Xd, yd, wd = dev_X(torch, X), torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda()
    gd = pop.eval_gauss_newton(Xd, yd, weights=wd)
    sd = gd.lm_step_device(torch.from_numpy(lam).cuda())
    assert torch.is_tensor(sd) and sd.is_cuda and sd.dtype == torch.float64
    assert sd.cpu().numpy().tobytes() == step.tobytes()
    # caller-chosen offsets with gaps: entries no tree owns keep the sentinel (host buffers, then device buffers)
    lib = api.library()
    off2 = (off[:-1] + 2 * np.arange(len(trees))).astype(np.int64)
    span2 = int(off2[-1] + ng[-1]) + 3
    dl2 = np.full(span2, np.nan, dtype=dtype)
    owned = np.zeros(span2, dtype=bool)
    for t in range(len(trees)):
        dl2[off2[t]:off2[t] + ng[t]] = gn._packed["dloss"][off[t]:off[t + 1]]
        owned[off2[t]:off2[t] + ng[t]] = True
    hasb, ng32 = has.astype(np.uint8), gn._packed["n_grad"]
    st2 = np.full(span2, 7.0)
    pop.ctx.check(lib.de_gn_lm_step(pop.ctx._h, api._dtype_code(dtype), len(trees), ng32.ctypes.data, dl2.ctypes.data, off2.ctypes.data,
                                    gn._packed["jtj"].ctypes.data, None, hasb.ctypes.data, lam.ctypes.data, st2.ctypes.data))
    assert (st2[~owned] == 7.0).all() and st2[owned].tobytes() == step.tobytes()
    d_dl2, d_jt, d_has, d_lam = (torch.from_numpy(v).cuda() for v in (dl2, gn._packed["jtj"], hasb, lam))
    d_st2 = torch.full((span2,), 7.0, dtype=torch.float64, device="cuda")
    pop.ctx.use_torch_stream()
    pop.ctx.check(lib.de_gn_lm_step(pop.ctx._h, api._dtype_code(dtype), len(trees), ng32.ctypes.data, d_dl2.data_ptr(), off2.ctypes.data,
                                    d_jt.data_ptr(), None, d_has.data_ptr(), d_lam.data_ptr(), d_st2.data_ptr()))
    assert d_st2.cpu().numpy().tobytes() == st2.tobytes()
    print(f"[lm step kernel] {np.dtype(dtype).name} N={N}: {n_nonzero} steps equal de_lm_solve_host bit for bit; against lm_step worst "
          f"{worst:.3g} of the forward bound over {n_fwd} trees")
    pop.close()
    alone.close()


# ---- 2. one iteration against the host rule --------------------------------------------------------------------------------------------
@DTYPES
def test_one_iteration_follows_the_host_rule(api, dtype):
    trees = GN.population_trees(32, (1, 2, 3, 4, 5, 6), dtype, per_width=5)
    assert len(trees) == 30
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = GN.data(300, 3, dtype, 17)
    c0 = pop.constants().copy()
    at = offsets(pop.n_consts)
    gn0 = pop.eval_gauss_newton(X, y, weights=w)
    steps = gn0.lm_step(1e-3)
    loss0, _ = pop.eval_loss(X, y, weights=w)
    consts, loss, ok = pop.fit_constants_lm_device(X, y, weights=w, iters=1)
    acc = np.asarray(pop.lm_accepts)
    assert consts.dtype == dtype and loss.dtype == dtype and set(acc.tolist()) <= {0, 1}
    loss1, _ = pop.eval_loss(X, y, weights=w)  # at the returned constants: the population holds them
    with np.errstate(invalid="ignore"):
        below = loss1.astype(np.float64) < loss0.astype(np.float64)
    assert np.array_equal(acc == 1, below), (acc, loss0, loss1)
    moved = 0
    for t in range(30):
        a, b = at[t], at[t + 1]
        if consts[a:b].tobytes() == c0[a:b].tobytes():
            assert acc[t] == 0
            continue
        assert acc[t] == 1 and np.asarray(gn0.has_jtj)[t]
        G = b - a
        want = (c0[a:b].astype(np.float64) + steps[t]).astype(dtype)
        cond = np.linalg.cond(damped(np.asarray(gn0.jtj[t]).astype(np.float64), 1e-3), 2)
        tol = np.spacing(np.abs(want)).astype(np.float64) + 8 * G * G * U64 * cond * np.abs(steps[t]).max()
        assert (np.abs(consts[a:b].astype(np.float64) - want.astype(np.float64)) <= tol).all(), (t, consts[a:b], want, tol)
        moved += 1
    assert moved >= 10, moved
    print(f"[lm one iteration] {np.dtype(dtype).name}: {moved} of 30 trees moved to T(c0 + lm_step(1e-3))")
    pop.close()


# ---- 3. the loop -------------------------------------------------------------------------------------------------------------------------
def holds_the_result(api, pop, X, y, consts, loss, w=None):
    lo, _, _ = pop.eval_loss_grad(X, y, weights=w)
    assert api._host(lo).tobytes() == api._host(loss).tobytes()  # bit for bit
    assert pop.constants().tobytes() == api._host(consts).tobytes()


@DTYPES
@pytest.mark.parametrize("where", ["numpy", "torch"])
def test_loop_fits_a_linear_model(api, torch, dtype, where):
    g = np.random.default_rng(1)
    N = 1000
    X = np.asfortranarray(g.standard_normal((2, N)).astype(dtype))
    truth = np.array([1.5, -0.7, 0.3])
    y = (truth[0] * X[0] + truth[1] * X[1] + truth[2]).astype(dtype) + (0.1 * g.standard_normal(N)).astype(dtype)
    x1, x2 = de.Node(feature=1), de.Node(feature=2)
    c0 = np.array([0.3, 2.0, -1.0], dtype=dtype)
    tree = de.Node(1, de.Node(1, de.Node(3, de.Node(val=c0[0]), x1), de.Node(3, de.Node(val=c0[1]), x2)), de.Node(val=c0[2]))
    pop = api.Population([tree], OPS, dtype, n_features=2)
    Jd = np.stack([X[0], X[1], np.ones(N, dtype=dtype)]).astype(np.float64)
    cond = np.linalg.cond(Jd @ Jd.T)
    want = np.linalg.lstsq(Jd.T, y.astype(np.float64), rcond=None)[0]
    hist = []
    if where == "torch":
        Xa, ya, ca = dev_X(torch, X), torch.from_numpy(y).cuda(), torch.from_numpy(c0).cuda()
    else:
        Xa, ya, ca = X, y, c0
    consts, loss, ok = pop.fit_constants_lm_device(Xa, ya, ca, iters=10, history=hist)
    if where == "torch":
        assert all(torch.is_tensor(v) and v.is_cuda for v in (consts, loss, ok)) and pop.consts_on_device_path
    got = api._host(consts).astype(np.float64)
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"[lm device loop, linear model] {np.dtype(dtype).name} {where}: |c - lstsq| / |lstsq| = {rel / GN.unit(dtype):.2f} u "
          f"(bound {4 * GN.K * cond:.0f} u)")
    assert bool(api._host(ok).all()) and len(hist) == 11
    assert rel <= 4 * GN.K * GN.unit(dtype) * cond
    hs = [api._host(h) for h in hist]
    assert all((b <= a).all() for a, b in zip(hs, hs[1:]))
    holds_the_result(api, pop, X, y, consts, loss)
    pop.close()


@DTYPES
@pytest.mark.parametrize("where", ["numpy", "torch"])
def test_loop_recovers_the_constants(api, torch, dtype, where):
    g = np.random.default_rng(0)
    N = 1000
    x = g.uniform(-2, 2, N)
    X = np.asfortranarray(x[None, :].astype(dtype))
    y = (2.0 * np.cos(1.5 * X[0].astype(np.float64)) - 0.5).astype(dtype)
    start = np.array([1.7, 1.4, 0.0])
    starts = start[None, :] * np.concatenate([[np.ones(3)], 1 + g.uniform(-0.05, 0.05, (29, 3))])

    def make(c):  # c0 * cos(c1 * x1) + c2
        return de.Node(1, de.Node(3, de.Node(val=c[0]), de.Node(1, de.Node(3, de.Node(val=c[1]), de.Node(feature=1)))), de.Node(val=c[2]))

    trees = [make(c) for c in starts]
    pop = api.Population(trees, OPS, dtype, n_features=1)
    consts0 = np.concatenate([de.get_scalar_constants(t)[0] for t in trees]).astype(dtype)
    hist = []
    if where == "torch":
        Xa, ya, ca = dev_X(torch, X), torch.from_numpy(y).cuda(), torch.from_numpy(consts0).cuda()
    else:
        Xa, ya, ca = X, y, consts0
    consts, loss, ok = pop.fit_constants_lm_device(Xa, ya, ca, iters=10, history=hist)
    if where == "torch":
        assert all(torch.is_tensor(v) and v.is_cuda for v in (consts, loss, ok)) and pop.consts_on_device_path
    hs = [api._host(h) for h in hist]
    assert bool(api._host(ok).all()) and len(hs) == 11 and hs[0].dtype == np.float64
    for a, b in zip(hs, hs[1:]):
        assert (b <= a).all()  # the accepted losses never increase
    ratio = api._host(loss).astype(np.float64) / hs[0]
    print(f"[lm device loop] {np.dtype(dtype).name} {where}: worst loss_final / loss_initial = {ratio.max():.3g} (bound 1e-9), "
          f"accepted steps per tree {np.asarray(api._host(pop.lm_accepts)).min()} .. {np.asarray(api._host(pop.lm_accepts)).max()}")
    assert (ratio <= 1e-9).all(), ratio
    assert np.allclose(api._host(consts).reshape(30, 3), [2.0, 1.5, -0.5], atol=1e-3)
    assert np.array_equal(hs[-1], api._host(loss).astype(np.float64))
    holds_the_result(api, pop, X, y, consts, loss)
    pop.close()


# ---- 4. a mixed population -------------------------------------------------------------------------------------------------------------
@DTYPES
def test_mixed_population(api, dtype):
    good = GN.population_trees(33, (1, 2, 3, 5, 8), dtype, per_width=3)
    div0, big = bad_trees()
    none = de.Node(1, de.Node(feature=1), de.Node(2, de.Node(feature=2)))  # x1 + exp(x2): no constant
    trees = good[:4] + [div0] + good[4:9] + [none, chain(9)] + good[9:] + [big]
    i_div0, i_none, i_wide, i_big = 4, 10, 11, len(trees) - 1
    keep = [t for t in range(len(trees)) if t not in (i_div0, i_none, i_wide, i_big)]
    pop, alone = api.Population(trees, OPS, dtype, n_features=3), api.Population(good, OPS, dtype, n_features=3)
    X, y, w = GN.data(257, 3, dtype, 23)
    c0 = pop.constants().copy()
    at = offsets(pop.n_consts)
    lo0, _, ok0 = pop.eval_loss_grad(X, y, weights=w)
    h1, h2 = [], []
    consts, loss, ok = pop.fit_constants_lm_device(X, y, weights=w, iters=6, history=h1)
    ca, la, oka = alone.fit_constants_lm_device(X, y, weights=w, iters=6, history=h2)
    for t in (i_div0, i_big):  # incomplete at the start: constants kept bit for bit, NaN loss
        assert not ok[t] and np.isnan(loss[t]) and consts[at[t]:at[t + 1]].tobytes() == c0[at[t]:at[t + 1]].tobytes()
    for t in (i_none, i_wide):  # no constant / wider than the matrix: constants kept, the plain loss
        assert ok[t] and consts[at[t]:at[t + 1]].tobytes() == c0[at[t]:at[t + 1]].tobytes()
        assert loss[t:t + 1].tobytes() == lo0[t:t + 1].tobytes() and np.isfinite(loss[t])
        assert pop.lm_accepts[t] == 0
    assert at[i_wide + 1] - at[i_wide] == 9 and at[i_none + 1] == at[i_none]
    ata = offsets(alone.n_consts)
    for i, t in enumerate(keep):  # the good trees: byte for byte what a population of them alone gives
        assert consts[at[t]:at[t + 1]].tobytes() == ca[ata[i]:ata[i + 1]].tobytes(), t
        assert loss[t:t + 1].tobytes() == la[i:i + 1].tobytes() and ok[t] == oka[i]
        assert all(a[t:t + 1].tobytes() == b[i:i + 1].tobytes() for a, b in zip(h1, h2))
        assert pop.lm_accepts[t] == alone.lm_accepts[i]
    assert np.asarray(alone.lm_accepts).sum() >= len(good)  # the fit did something
    holds_the_result(api, pop, X, y, consts, loss, w)
    pop.close()
    alone.close()


# ---- 5. a parametric program -------------------------------------------------------------------------------------------------------------
@DTYPES
def test_parametric_program(api, dtype):
    P, Cn, N = 3, 4, 300
    trees = GN.population_trees(34, (1, 2, 3), dtype, nfeatures=2, per_width=4, node_type=de.ParametricNode, nparams=P)
    pop = api.Population(trees, OPS, dtype, n_features=2, n_params=P)
    X, y, w = GN.data(N, 2, dtype, 12)
    g = np.random.Generator(np.random.PCG64(5))
    params = np.asfortranarray(g.uniform(-1.5, 1.5, (P, Cn)).astype(dtype))
    classes = g.integers(1, Cn + 1, N)
    hist = []
    consts, loss, ok = pop.fit_constants_lm_device(X, y, weights=w, iters=5, history=hist, params=params, classes=classes)
    assert len(hist) == 6 and ok.sum() >= 8
    for a, b in zip(hist, hist[1:]):
        assert (b[ok] <= a[ok]).all()
    assert (hist[-1][ok] < hist[0][ok]).sum() >= 4
    lo, _, ok2 = pop.eval_loss_grad(X, y, weights=w, params=params, classes=classes)  # at the returned constants, the parameters fixed
    assert np.array_equal(ok, ok2) and lo[ok].tobytes() == loss[ok].tobytes() and np.isnan(loss[~ok]).all()
    assert pop.constants().tobytes() == consts.tobytes()
    pop.close()


# ---- 6. edges and refusals ---------------------------------------------------------------------------------------------------------------
def test_edges(api, torch):
    dtype = np.float32
    trees = GN.population_trees(35, (0, 2, 3), dtype, per_width=2) + [de.Node(1, de.Node(feature=1), de.Node(val=float("inf")))]
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = GN.data(129, 3, dtype, 5)
    c0 = pop.constants().copy()
    # iters = 0: de_eval_loss_gn's loss and flags, the constants unchanged
    hist = []
    consts, loss, ok = pop.fit_constants_lm_device(X, y, weights=w, iters=0, history=hist)
    gn = pop.eval_gauss_newton(X, y, weights=w)
    assert len(hist) == 1 and consts.tobytes() == c0.tobytes() and pop.constants().tobytes() == c0.tobytes()
    assert loss.tobytes() == np.asarray(gn.loss).tobytes() and np.array_equal(ok, gn.ok) and not ok[-1] and ok[:-1].all()
    assert np.array_equal(hist[0], loss.astype(np.float64), equal_nan=True) and not np.asarray(pop.lm_accepts).any()
    # N = 0: losses 0, NaN where a constant already fails the flag; every row of the history the same; the constants unchanged
    hist = []
    consts, loss, ok = pop.fit_constants_lm_device(np.zeros((3, 0), dtype=dtype, order="F"), np.zeros(0, dtype=dtype), iters=3, history=hist)
    assert ok.tolist() == [True] * 6 + [False] and not loss[:6].any() and np.isnan(loss[6]) and len(hist) == 4
    assert all(np.array_equal(h, loss.astype(np.float64), equal_nan=True) for h in hist)
    assert consts.tobytes() == c0.tobytes() and pop.constants().tobytes() == c0.tobytes()
    pop.close()
    # an empty population
    empty = api.Population([], OPS, dtype, n_features=3)
    consts, loss, ok = empty.fit_constants_lm_device(X, y, iters=2)
    assert consts.size == 0 and loss.size == 0 and ok.size == 0
    consts, loss, ok = empty.fit_constants_lm_device(dev_X(torch, X), torch.from_numpy(y).cuda(), iters=2)
    assert consts.numel() == 0 and loss.numel() == 0 and ok.numel() == 0
    empty.close()


def test_refusals(api):
    lib = api.library()
    cos1 = de.OperatorEnum(binary_operators=("+",), unary_operators=("cos",))
    tree = de.Node(1, de.Node(1, de.Node(feature=1)), de.Node(val=0.5))
    X = np.asfortranarray(np.linspace(-1, 1, 64)[None, :])

    def raw(pop, Xa, ya, opts=None, yp=True, okp=True, n=1):
        """de_fit_consts_lm itself on sentinel-filled outputs: (status, every output still the sentinel)."""
        lo, ok = np.full(2 * n, 7, dtype=np.float64), np.full(n, 9, dtype=np.uint8)
        hist, acc = np.full(16 * n, 7.0), np.full(n, 9, dtype=np.int32)
        rc = lib.de_fit_consts_lm(pop.ctx._h, pop._h, Xa.ctypes.data, Xa.shape[1], Xa.shape[0], None, ya.ctypes.data if yp else None, None,
                                  C.byref(opts) if opts is not None else None, lo.ctypes.data, ok.ctypes.data if okp else None,
                                  hist.ctypes.data, acc.ctypes.data)
        return rc, bool((lo == 7).all() and (ok == 9).all() and (hist == 7).all() and (acc == 9).all())

    for dtype in (np.float16, np.complex64):  # evaluation-only populations
        pop = api.Population([tree], cos1, dtype, n_features=1)
        before = pop.constants().copy()
        with pytest.raises(api.DeviceError, match="DE_ERR_UNSUPPORTED"):
            pop.fit_constants_lm_device(X.astype(dtype), np.zeros(64, dtype=dtype))
        Xc = np.asfortranarray(X.astype(dtype))
        assert raw(pop, Xc, Xc) == (7, True) and pop.constants().tobytes() == before.tobytes()
        pop.close()
    # a GraphNode population with a shared constant: the host loop serves it
    Gn = de.GraphNode
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    x1, c, c2 = Gn(feature=1), Gn(val=0.75), Gn(val=-0.4)
    sh = Gn(1, Gn(2, x1, c))                              # cos(x1 * c), c is ONE node
    dag = Gn(1, Gn(1, sh, Gn(2, sh, Gn(2, c, x1))), c2)   # sh + sh * (c * x1) + c2: a shared subtree (a CSE tape), c occurs three times
    for dtype in (np.float32, np.float64):
        pop = api.Population([dag], ops, dtype, n_features=1)
        before = pop.constants().copy()
        Xf, y = np.asfortranarray(X.astype(dtype)), np.zeros(64, dtype=dtype)
        with pytest.raises(ValueError, match="fit_constants_lm"):
            pop.fit_constants_lm_device(Xf, y)
        with pytest.raises(ValueError, match="lm_step"):
            pop.eval_gauss_newton(Xf, y).lm_step_device(1e-3)
        assert raw(pop, Xf, y) == (7, True) and pop.constants().tobytes() == before.tobytes()
        pop.close()
    # bad options, a null y, a null ok
    dtype = np.float32
    pop = api.Population([tree, de.Node(1, de.Node(feature=1), de.Node(val=2.0))], cos1, dtype, n_features=1)
    Xf, y = np.asfortranarray(X.astype(dtype)), np.cos(X[0]).astype(dtype)
    before = pop.constants().copy()
    O = api.LmOpts
    for opts in (O(-1, 0, 1e-3, 10, 0.1, 1e-12), O(3, 1, 1e-3, 10, 0.1, 1e-12), O(3, 0, 0.0, 10, 0.1, 1e-12), O(3, 0, -1e-3, 10, 0.1, 1e-12),
                 O(3, 0, 1e-3, float("inf"), 0.1, 1e-12), O(3, 0, 1e-3, 10, float("nan"), 1e-12), O(3, 0, 1e-3, 10, 0.1, 0.0),
                 O(3, 0, float("nan"), 10, 0.1, 1e-12), O(3, 0, 1e-3, 0.0, 0.1, 1e-12), O(3, 0, 1e-3, 10, 0.1, float("inf"))):
        assert raw(pop, Xf, y, opts, n=2) == (1, True), list(getattr(opts, n) for n, _ in O._fields_)
        assert pop.constants().tobytes() == before.tobytes()
    assert raw(pop, Xf, y, yp=False, n=2) == (1, True) and raw(pop, Xf, y, okp=False, n=2) == (1, True)
    assert pop.constants().tobytes() == before.tobytes()
    for kw in (dict(iters=-1), dict(lam0=0.0), dict(up=float("inf")), dict(down=float("nan"))):
        with pytest.raises(ValueError):
            pop.fit_constants_lm_device(Xf, y, **kw)
    with pytest.raises(ValueError):
        pop.fit_constants_lm_device(Xf, y[:-1])
    with pytest.raises(ValueError):
        pop.fit_constants_lm_device(Xf, y, consts0=before[:-1])
    assert pop.constants().tobytes() == before.tobytes()
    # ... and the same call with good arguments runs (null options: the defaults)
    rc, untouched = raw(pop, Xf, y, None, n=2)
    assert rc == 0 and not untouched and pop.constants().tobytes() != before.tobytes()
    pop.close()


# ---- 7. ordering -------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_stream_order_without_synchronisation(api, torch, dtype):
    trees = GN.population_trees(36, (1, 2, 3, 4), dtype, per_width=5)
    X, y, w = GN.data(513, 3, dtype, 9)
    Xd, yd, wd = dev_X(torch, X), torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda()
    got = []
    for sync in (False, True):
        pop = api.Population(trees, OPS, dtype, n_features=3)
        c0 = pop.constants()
        start, other = torch.from_numpy((c0 * dtype(1.25)).astype(dtype)).cuda(), torch.from_numpy((c0 * dtype(0.5)).astype(dtype)).cuda()
        wait = torch.cuda.synchronize if sync else (lambda: None)
        wait()
        consts, loss, ok = pop.fit_constants_lm_device(Xd, yd, start, weights=wd, iters=4)
        wait()
        pop.set_constants(other)
        wait()
        lo, oke = pop.eval_loss(Xd, yd, weights=wd)
        torch.cuda.synchronize()
        got.append([api._host(v).tobytes() for v in (consts, loss, ok, lo, oke)])
        assert pop.consts_on_device_path
        ref = api.Population(trees, OPS, dtype, n_features=3)  # the last evaluation saw `other`, not the fitted constants
        ref.set_constants(api._host(other))
        rl, rk = ref.eval_loss(X, y, weights=w)
        assert rl.tobytes() == api._host(lo).tobytes()
        ref.close()
        pop.close()
    assert got[0] == got[1]
