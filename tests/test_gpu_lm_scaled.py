"""GPU tests of Levenberg-Marquardt on the constants under linear scaling, on the device (include/de_hip.h de_fit_stats_lm_step /
de_fit_consts_lm_scaled).

The step kernel runs csrc/de_lm_project.h and csrc/de_lm_solve.h, the code behind the host hooks de_lm_project_host and
de_lm_solve_host: on the same buffers the two agree BIT FOR BIT, for every tree, and so does the scaled_sse the kernel returns.  The
loop is held to a host emulation that takes every evaluation from `eval_fit_stats_grad` (deterministic: the same bits for the same
constants), every step from the hooks and applies the accept rule of `fit_constants_lm(scaled=True)`: constants, scaled_sse, history
and n_accept are equal bit for bit.  The end-to-end scenario and its bounds are those of
tests/test_gpu_fit_stats_grad.py::test_scaled_fit_recovers_the_constants:
    final scaled_sse <= max(1e-9 initial, 4 * 1024 u M2_y),   |slope + 3| <= 3 tol, |intercept - 2| <= 2 tol,
    tol = sqrt(max(final, 1024 u M2_y) / M2_y),   u = 2^-24 / 2^-53.
Trees and data are those of tests/test_gpu_gauss_newton.py, the helpers those of tests/test_gpu_lm.py."""
import ctypes as C

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import test_gpu_gauss_newton as GN
import test_gpu_lm as LM

pytestmark = pytest.mark.gpu
OPS = GN.OPS
DTYPES = LM.DTYPES
api = LM.api
torch = LM.torch
chain, bad_trees, dev_X, offsets = LM.chain, LM.bad_trees, LM.dev_X, LM.offsets


def cos_sum(k, dtype):
    """cos(c_1 x_1) + cos(c_2 x_2) + ...: k independent non-linear constants, no row in the span of [1, yhat]"""
    t = None
    for i in range(k):
        term = de.Node(1, de.Node(3, de.Node(val=float(dtype(0.6 + 0.17 * i))), de.Node(feature=1 + i % 3)))
        t = term if t is None else de.Node(1, t, term)
    return t


def flat_tree():  # 0 * 0.75: constant over the samples and exactly 0, so mean_p = M2_p = C = 0 exactly; two constant rows
    return de.Node(3, de.Node(val=0.0), de.Node(val=0.75))


def no_const():  # x1 + exp(x2)
    return de.Node(1, de.Node(feature=1), de.Node(2, de.Node(feature=2)))


def hooks(api, fg, lam):
    """Per tree of a numpy FitStatsGrad: (step[G] or zeros, scaled_sse, produced) from de_lm_project_host + de_lm_solve_host"""
    st, has = fg.stats, np.asarray(fg.has_jtj)
    lams = np.broadcast_to(np.asarray(lam, dtype=np.float64), (len(fg),))
    steps, sses, made = [], np.empty(len(fg)), np.zeros(len(fg), dtype=bool)
    for t in range(len(fg)):
        D, P, Q = fg._dpq(t)
        G = D.size
        if G == 0 or G > 8:  # (the objective needs no matrix)
            sses[t] = api.lm_project_host([st.mean_p[t], st.m2_p[t], st.cov[t]], [st.W, st.mean_y, st.m2_y], [], [], [], np.zeros((0, 0)))[0]
            steps.append(np.zeros(G))
            continue
        sse, g, Ht, formed = api.lm_project_host([st.mean_p[t], st.m2_p[t], st.cov[t]], [st.W, st.mean_y, st.m2_y], D, P, Q,
                                                 np.asarray(fg.jtj[t]).astype(np.float64))
        sses[t] = sse
        step, produced = api.lm_solve_host(Ht, g, lams[t]) if has[t] else (np.zeros(G), False)
        made[t] = bool(has[t] and formed and produced)
        steps.append(step if made[t] else np.zeros(G))
    return steps, sses, made


def emulate(api, ref, X, y, w, c0, iters, lam0=1e-3, up=10.0, down=0.1, **kw):
    """fit_constants_lm(scaled=True) on the host with the hooks' steps, on the population `ref`: (consts, sse, history, n_accept, stats)"""
    dtype, at = c0.dtype.type, offsets(ref.n_consts)
    nt = ref.n_trees

    def ev(c):
        ref.set_constants(c)
        return ref.eval_fit_stats_grad(X, y, weights=w, **kw)

    consts, fg = c0.copy(), ev(c0)
    _, sse, _ = hooks(api, fg, lam0)
    lam, acc, hist = np.full(nt, lam0), np.zeros(nt, dtype=np.int32), [sse.copy()]
    if X.shape[1] == 0 or consts.size == 0:
        iters, hist = 0, [sse.copy() for _ in range(iters + 1)]
    for _ in range(iters):
        steps, _, made = hooks(api, fg, lam)
        trial = consts.copy()
        for t in np.flatnonzero(made):
            trial[at[t]:at[t + 1]] = (consts[at[t]:at[t + 1]].astype(np.float64) + steps[t]).astype(dtype)
        ft = ev(trial)
        _, sse_t, _ = hooks(api, ft, lam)
        with np.errstate(invalid="ignore"):
            accept = np.asarray(fg.has_jtj) & np.asarray(ft.has_jtj) & (sse_t < sse)
        for t in np.flatnonzero(accept):
            consts[at[t]:at[t + 1]] = trial[at[t]:at[t + 1]]
            sse[t] = sse_t[t]
            for name in ("d_sum", "d_pred", "d_targ", "jtj"):
                getattr(fg, name)[t] = getattr(ft, name)[t]
            for name in ("mean_p", "m2_p", "cov"):
                getattr(fg.stats, name)[t] = getattr(ft.stats, name)[t]
            fg.ok[t], fg.has_jtj[t] = ft.ok[t], ft.has_jtj[t]
        lam = np.where(accept, np.maximum(lam * down, 1e-12), lam * up)
        acc += accept
        hist.append(sse.copy())
    return consts, sse, hist, acc, fg.stats


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def post_conditions(api, pop, fresh, X, y, w, c0, consts, sse, hist, **kw):
    """What holds after every fit: the program holds the constants, eval_fit_stats_grad reproduces the statistics, the history's rows"""
    hs = np.stack([api._host(h) for h in hist])
    acc = api._host(pop.lm_accepts)
    assert same(pop.constants(), api._host(consts))
    fg = pop.eval_fit_stats_grad(X, y, weights=w, **kw)
    st = pop.lm_fit_stats
    for name in ("mean_p", "m2_p", "cov"):
        assert same(getattr(fg.stats, name), getattr(st, name)), name  # bit for bit
    assert (fg.stats.W, fg.stats.m2_y) == (st.W, st.m2_y) and same(np.float64(fg.stats.mean_y), np.float64(st.mean_y))
    assert same(hooks(api, fg, 1.0)[1], api._host(sse)) and same(hs[-1], api._host(sse))
    fresh.set_constants(c0)
    assert same(hooks(api, fresh.eval_fit_stats_grad(X, y, weights=w, **kw), 1.0)[1], hs[0])
    with np.errstate(invalid="ignore"):
        assert not (hs[1:] > hs[:-1]).any()  # never increases
        assert np.array_equal(acc, (hs[1:] < hs[:-1]).sum(axis=0))  # the accepted steps are the strict decreases
    return fg


# ---- 1. the step kernel --------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("N", [64, 257])
def test_step_kernel_against_the_host_hooks(api, torch, dtype, N):
    good = GN.population_trees(31, range(9), dtype)
    div0, big = bad_trees()
    built = [cos_sum(k, dtype) for k in range(1, 9)]
    trees = good + [chain(9), chain(12), div0, big, flat_tree(), no_const()] + built
    n0 = len(good)
    wide, bad, flat, none, mine = [n0, n0 + 1], [n0 + 2, n0 + 3], n0 + 4, n0 + 5, list(range(n0 + 6, n0 + 14))
    assert len(trees) <= 80
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = GN.data(N, 3, dtype, 40 + N)
    lam = np.array([(0.0, 1e-3, 1.0, 1e3)[t % 4] for t in range(len(trees))])
    lam[mine] = 1.0
    fg = pop.eval_fit_stats_grad(X, y, weights=w)
    ng = fg._packed["n_grad"].astype(np.int64)
    off = offsets(ng)
    assert sorted(set(ng[:n0].tolist())) == list(range(9)) and ng[wide].tolist() == [9, 12] and ng[mine].tolist() == list(range(1, 9))
    assert ng[flat] == 2 and fg.stats.m2_p[flat] == 0.0 and fg.stats.cov[flat] == 0.0 and ng[none] == 0
    step, sse = fg.lm_step_device(lam, return_sse=True)
    assert step.dtype == np.float64 and step.shape == (int(off[-1]),) and sse.dtype == np.float64 and sse.shape == (len(trees),)
    has = np.asarray(fg.has_jtj)
    assert not has[wide].any() and not has[bad].any() and has[mine].all() and has[flat] and has.sum() >= 48
    want, want_sse, made = hooks(api, fg, lam)
    differ = [(t, sse[t:t + 1].tobytes().hex(), want_sse[t:t + 1].tobytes().hex()) for t in range(len(trees)) if not same(sse[t:t + 1], want_sse[t:t + 1])]
    assert not differ, differ  # every tree, the NaN of the incomplete ones included
    assert np.array_equal(sse, fg.stats.scaled_sse, equal_nan=True)
    for t in range(len(trees)):
        assert same(step[off[t]:off[t + 1]], want[t]), (t, step[off[t]:off[t + 1]], want[t])  # no exemption
    for t in wide + bad + [flat, none]:
        assert not step[off[t]:off[t + 1]].any() and not made[t], t
    assert np.isnan(sse[bad]).all() and sse[flat] == fg.stats.m2_y
    for t in mine:  # the purpose-built trees produce a step at lam = 1
        assert made[t] and step[off[t]:off[t + 1]].all(), t
    n_nonzero = int(sum(made[t] and step[off[t]:off[t + 1]].any() for t in range(len(trees))))
    assert n_nonzero >= len(mine), n_nonzero  # (the purpose-built trees; a random tree's rows may lie in the span of [1, yhat])
    # against projected().lm_step (numpy's LU on the same projected system): test_lm_host.py's forward bound
    ref, worst, n_fwd = fg.projected().lm_step(lam), 0.0, 0
    for t in np.flatnonzero(made):
        G = int(ng[t])
        _, g, Ht, _ = api.lm_project_host([fg.stats.mean_p[t], fg.stats.m2_p[t], fg.stats.cov[t]], [fg.stats.W, fg.stats.mean_y, fg.stats.m2_y],
                                          *fg._dpq(t), np.asarray(fg.jtj[t]).astype(np.float64))
        cond = np.linalg.cond(LM.damped(Ht, lam[t]), 2)
        if lam[t] >= 1e-3 and cond < 1e12:
            err, bound = np.linalg.norm(step[off[t]:off[t + 1]] - ref[t]), 8 * G * G * LM.U64 * cond * np.linalg.norm(ref[t])
            assert err <= bound, (t, G, lam[t], err / bound)
            worst, n_fwd = max(worst, err / bound if bound else 0.0), n_fwd + 1
    assert n_fwd >= len(mine), n_fwd
    # device tensors: the same bits, nothing copied
    Xd, yd, wd = dev_X(torch, X), torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda()
    fd = pop.eval_fit_stats_grad(Xd, yd, weights=wd)
    sd, ed = fd.lm_step_device(torch.from_numpy(lam).cuda(), return_sse=True)
    assert all(torch.is_tensor(v) and v.is_cuda and v.dtype == torch.float64 for v in (sd, ed))
    assert same(sd.cpu().numpy(), step) and same(ed.cpu().numpy(), sse)
    # the C call itself: caller-chosen dmom and jtj offsets with gaps, sentinels around the packed step (host, then device buffers)
    lib, pk, nt = api.library(), fg._packed, len(trees)
    moff = (3 * off[:-1] + 2 * np.arange(nt)).astype(np.int64)
    joff_p = offsets(ng * ng)
    joff = (joff_p[:-1] + 3 * np.arange(nt)).astype(np.int64)
    dm2, jt2 = np.full(int(moff[-1] + 3 * ng[-1]) + 3, np.nan), np.full(int(joff[-1] + ng[-1] ** 2) + 3, np.nan, dtype=dtype)
    for t in range(nt):
        dm2[moff[t]:moff[t] + 3 * ng[t]] = pk["dmom"][3 * off[t]:3 * off[t + 1]]
        jt2[joff[t]:joff[t] + ng[t] ** 2] = pk["jtj"][joff_p[t]:joff_p[t + 1]]
    hasb, total = has.astype(np.uint8), int(off[-1])
    st2, se2 = np.full(total + 8, 7.0), np.full(nt + 8, 7.0)
    args = (api._dtype_code(dtype), nt, pk["n_grad"].ctypes.data)
    pop.ctx.check(lib.de_fit_stats_lm_step(pop.ctx._h, *args, pk["stats"].ctypes.data, pk["stats"].ctypes.data + 24 * nt, dm2.ctypes.data,
                                           moff.ctypes.data, jt2.ctypes.data, joff.ctypes.data, hasb.ctypes.data, lam.ctypes.data,
                                           st2[4:].ctypes.data, se2[4:].ctypes.data))
    assert (st2[:4] == 7).all() and (st2[4 + total:] == 7).all() and same(st2[4:4 + total], step)
    assert (se2[:4] == 7).all() and (se2[4 + nt:] == 7).all() and same(se2[4:4 + nt], sse)
    d_st, d_dm, d_jt, d_has, d_lam = (torch.from_numpy(v).cuda() for v in (pk["stats"], dm2, jt2, hasb, lam))
    d_st2 = torch.full((total + 8,), 7.0, dtype=torch.float64, device="cuda")
    pop.ctx.use_torch_stream()
    pop.ctx.check(lib.de_fit_stats_lm_step(pop.ctx._h, *args, d_st.data_ptr(), d_st.data_ptr() + 24 * nt, d_dm.data_ptr(), moff.ctypes.data,
                                           d_jt.data_ptr(), joff.ctypes.data, d_has.data_ptr(), d_lam.data_ptr(), d_st2.data_ptr() + 32, None))
    assert same(d_st2.cpu().numpy(), st2)
    print(f"[lm scaled step kernel] {np.dtype(dtype).name} N={N}: {n_nonzero} steps and {nt} scaled_sse equal the host hooks bit for bit; "
          f"against projected().lm_step worst {worst:.3g} of the forward bound over {n_fwd} trees")
    pop.close()


# ---- 2. two iterations against the host rule -------------------------------------------------------------------------------------------
@DTYPES
def test_iterations_follow_the_host_rule(api, dtype):
    trees = GN.population_trees(32, (1, 2, 3, 4, 5, 6), dtype, per_width=5) + [cos_sum(k, dtype) for k in (2, 5, 8)]
    pop, ref = api.Population(trees, OPS, dtype, n_features=3), api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = GN.data(300, 3, dtype, 17)
    c0, at = pop.constants().copy(), offsets(pop.n_consts)
    moved = {}
    for iters in (1, 2):  # (the second iteration's step shows the lam the first left: down on accept, up otherwise)
        pop.set_constants(c0)
        hist = []
        consts, sse, ok = pop.fit_constants_lm_device(X, y, weights=w, iters=iters, history=hist, scaled=True)
        acc = np.asarray(pop.lm_accepts)
        assert consts.dtype == dtype and sse.dtype == np.float64 and len(hist) == iters + 1
        ce, se, he, ae, _ = emulate(api, ref, X, y, w, c0, iters)
        assert same(consts, ce) and same(sse, se) and same(np.stack(hist), np.stack(he)) and np.array_equal(acc, ae), (iters, acc, ae)
        moved[iters] = sum(not same(consts[at[t]:at[t + 1]], c0[at[t]:at[t + 1]]) for t in range(len(trees)))
        assert set(acc.tolist()) <= set(range(iters + 1))
    # one iteration: a tree's constants are its consts0 bits or T(c0 + the hooks' step at lam0), exactly
    ref.set_constants(c0)
    steps, _, made = hooks(api, ref.eval_fit_stats_grad(X, y, weights=w), 1e-3)
    pop.set_constants(c0)
    consts, _, _ = pop.fit_constants_lm_device(X, y, weights=w, iters=1, scaled=True)
    for t in range(len(trees)):
        a, b = at[t], at[t + 1]
        if not same(consts[a:b], c0[a:b]):
            assert made[t] and pop.lm_accepts[t] == 1 and same(consts[a:b], (c0[a:b].astype(np.float64) + steps[t]).astype(dtype)), t
        else:
            assert pop.lm_accepts[t] == 0, t
    assert moved[1] >= 1 and moved[2] >= moved[1], moved  # (the exact-trial branch above was taken)
    print(f"[lm scaled iterations] {np.dtype(dtype).name}: {moved[1]} / {moved[2]} of {len(trees)} trees moved after 1 / 2 iterations, as the host rule has it")
    pop.close()
    ref.close()


# ---- 3. the end-to-end fit, 4. its post-conditions -------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("where", ["numpy", "torch"])
def test_scaled_fit_recovers_the_constants_on_the_device(api, torch, dtype, where):
    u = GN.unit(dtype)
    g = np.random.default_rng(0)
    N = 513
    X = np.asfortranarray(g.uniform(-2, 2, (2, N)).astype(dtype))
    w = g.uniform(0.5, 1.5, N).astype(dtype)
    w[-37:] = 0
    star = np.array([1.3, 0.7])
    X64 = X.astype(np.float64)
    y = (2.0 - 3.0 * (np.cos(star[0] * X64[0]) + star[1] * X64[1])).astype(dtype)
    signs = [(1, 1), (1, -1), (-1, 1), (-1, -1)]
    starts = np.array([star * (1.0 + 0.3 * np.array(signs[i % 4])) for i in range(28)])

    def make(c):  # cos(c1 * x1) + c2 * x2
        return de.Node(1, de.Node(1, de.Node(3, de.Node(val=c[0]), de.Node(feature=1))), de.Node(3, de.Node(val=c[1]), de.Node(feature=2)))

    trees = [make(c) for c in starts]
    pop, fresh = api.Population(trees, OPS, dtype, n_features=2), api.Population(trees, OPS, dtype, n_features=2)
    consts0 = np.concatenate([de.get_scalar_constants(t)[0] for t in trees]).astype(dtype)
    if where == "torch":
        Xa, ya, wa, ca = dev_X(torch, X), torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(consts0).cuda()
    else:
        Xa, ya, wa, ca = X, y, w, consts0
    hist = []
    consts, sse, ok = pop.fit_constants_lm_device(Xa, ya, ca, weights=wa, iters=10, history=hist, scaled=True)
    if where == "torch":
        assert all(torch.is_tensor(v) and v.is_cuda for v in (consts, sse, ok)) and pop.consts_on_device_path and sse.dtype == torch.float64
    loss, h0 = api._host(sse), api._host(hist[0])
    assert bool(api._host(ok).all()) and len(hist) == 11 and loss.dtype == np.float64
    fs = pop.lm_fit_stats
    m2y = fs.m2_y
    assert (h0 >= 5e-3 * m2y).all()
    bound = np.maximum(1e-9 * h0, 4 * 1024 * u * m2y)
    print(f"[lm scaled device fit] {np.dtype(dtype).name} {where}: worst final / bound = {(loss / bound).max():.3g}, final / initial = "
          f"{(loss / h0).max():.3g}, slope {fs.slope[0]:.9g}, intercept {fs.intercept[0]:.9g}, accepted steps per tree "
          f"{api._host(pop.lm_accepts).min()} .. {api._host(pop.lm_accepts).max()}")
    assert (loss <= bound).all(), loss / bound
    tol = np.sqrt(np.maximum(loss, 1024 * u * m2y) / m2y)
    assert (np.abs(fs.slope + 3.0) <= 3.0 * tol).all() and (np.abs(fs.intercept - 2.0) <= 2.0 * tol).all(), (fs.slope, fs.intercept, tol)
    assert same(fs.scaled_sse, loss)
    post_conditions(api, pop, fresh, X, y, w, consts0, consts, sse, hist)
    pop.close()
    fresh.close()


# ---- 5. an exact property: samples of weight zero change nothing ------------------------------------------------------------------------
@DTYPES
def test_zero_weight_padding_gives_the_same_bits(api, dtype):
    trees = GN.population_trees(37, (1, 2, 3, 5, 8), dtype, per_width=3) + [cos_sum(k, dtype) for k in (3, 6)]
    X, y, w = GN.data(300, 3, dtype, 29)
    Xp, yp, wp = GN.data(512, 3, dtype, 30)
    Xp[:, :300], yp[:300], wp[:300], wp[300:] = X, y, w, 0
    out = []
    for Xa, ya, wa in ((X, y, w), (np.asfortranarray(Xp), yp, wp)):
        pop = api.Population(trees, OPS, dtype, n_features=3)
        hist = []
        consts, sse, ok = pop.fit_constants_lm_device(Xa, ya, weights=wa, iters=5, history=hist, scaled=True)
        out.append((consts, sse, ok, np.stack(hist), np.asarray(pop.lm_accepts)))
        pop.close()
    assert all(same(a, b) for a, b in zip(*out))
    assert out[0][4].sum() >= len(trees) // 2  # the fit did something


# ---- 6. other populations and shapes ---------------------------------------------------------------------------------------------------
@DTYPES
def test_mixed_population(api, dtype):
    good = GN.population_trees(33, (1, 2, 3, 5, 8), dtype, per_width=3) + [cos_sum(4, dtype)]
    div0, big = bad_trees()
    trees = good[:4] + [div0] + good[4:9] + [no_const(), chain(9)] + good[9:] + [big]
    i_div0, i_none, i_wide, i_big = 4, 10, 11, len(trees) - 1
    keep = [t for t in range(len(trees)) if t not in (i_div0, i_none, i_wide, i_big)]
    pop, alone = api.Population(trees, OPS, dtype, n_features=3), api.Population(good, OPS, dtype, n_features=3)
    fresh = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = GN.data(257, 3, dtype, 23)
    c0, at = pop.constants().copy(), offsets(pop.n_consts)
    c0[at[i_div0 + 1] - 1], c0[at[i_wide] + 3] = -0.0, -0.0  # (the bits are kept: -0 stays -0)
    pop.set_constants(c0)
    fg0 = pop.eval_fit_stats_grad(X, y, weights=w)
    h1, h2 = [], []
    consts, sse, ok = pop.fit_constants_lm_device(X, y, weights=w, iters=6, history=h1, scaled=True)
    ca, sa, oka = alone.fit_constants_lm_device(X, y, weights=w, iters=6, history=h2, scaled=True)
    assert np.signbit(consts[at[i_div0 + 1] - 1]) and np.signbit(consts[at[i_wide] + 3])
    for t in (i_div0, i_big):  # incomplete at the start: constants kept bit for bit, NaN objective
        assert not ok[t] and np.isnan(sse[t]) and same(consts[at[t]:at[t + 1]], c0[at[t]:at[t + 1]]) and pop.lm_accepts[t] == 0
    for t in (i_none, i_wide):  # no constant / wider than the matrix: constants kept, the objective of the first evaluation
        assert ok[t] and same(consts[at[t]:at[t + 1]], c0[at[t]:at[t + 1]]) and pop.lm_accepts[t] == 0
        assert same(sse[t:t + 1], fg0.stats.scaled_sse[t:t + 1]) and np.isfinite(sse[t])
    assert at[i_wide + 1] - at[i_wide] == 9 and at[i_none + 1] == at[i_none]
    ata = offsets(alone.n_consts)
    for i, t in enumerate(keep):  # the good trees: byte for byte what a population of them alone gives
        assert same(consts[at[t]:at[t + 1]], ca[ata[i]:ata[i + 1]]), t
        assert same(sse[t:t + 1], sa[i:i + 1]) and ok[t] == oka[i] and pop.lm_accepts[t] == alone.lm_accepts[i]
        assert all(same(a[t:t + 1], b[i:i + 1]) for a, b in zip(h1, h2))
    assert np.asarray(alone.lm_accepts).any() and alone.lm_accepts[len(good) - 1] >= 1  # the fit did something (cos_sum(4) moved)
    post_conditions(api, pop, fresh, X, y, w, c0, consts, sse, h1)
    for p in (pop, alone, fresh):
        p.close()


@DTYPES
def test_parametric_program(api, dtype):
    P, Cn, N = 3, 4, 300
    trees = GN.population_trees(34, (1, 2, 3), dtype, nfeatures=2, per_width=4, node_type=de.ParametricNode, nparams=P)
    pop = api.Population(trees, OPS, dtype, n_features=2, n_params=P)
    fresh = api.Population(trees, OPS, dtype, n_features=2, n_params=P)
    X, y, w = GN.data(N, 2, dtype, 12)
    g = np.random.Generator(np.random.PCG64(5))
    params = np.asfortranarray(g.uniform(-1.5, 1.5, (P, Cn)).astype(dtype))
    classes = g.integers(1, Cn + 1, N)
    c0, hist = pop.constants().copy(), []
    consts, sse, ok = pop.fit_constants_lm_device(X, y, weights=w, iters=5, history=hist, params=params, classes=classes, scaled=True)
    assert len(hist) == 6 and ok.sum() >= 8 and np.isnan(sse[~ok]).all()
    assert (hist[-1][ok] < hist[0][ok]).any()
    fg = post_conditions(api, pop, fresh, X, y, w, c0, consts, sse, hist, params=params, classes=classes)
    assert np.array_equal(np.asarray(fg.ok), ok)
    ce, se, he, ae, _ = emulate(api, fresh, X, y, w, c0, 5, params=params, classes=classes)
    assert same(consts, ce) and same(sse, se) and np.array_equal(np.asarray(pop.lm_accepts), ae)
    pop.close()
    fresh.close()


def test_edges(api, torch):
    dtype = np.float32
    trees = GN.population_trees(35, (0, 2, 3), dtype, per_width=2) + [de.Node(1, de.Node(feature=1), de.Node(val=float("inf")))]
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = GN.data(129, 3, dtype, 5)
    c0 = pop.constants().copy()
    # iters = 0: the first evaluation's values, the constants unchanged
    hist = []
    consts, sse, ok = pop.fit_constants_lm_device(X, y, weights=w, iters=0, history=hist, scaled=True)
    fg = pop.eval_fit_stats_grad(X, y, weights=w)
    assert len(hist) == 1 and same(consts, c0) and same(pop.constants(), c0)
    assert np.array_equal(sse, fg.stats.scaled_sse, equal_nan=True) and np.array_equal(ok, fg.ok) and not ok[-1] and ok[:-1].all() and np.isnan(sse[-1])
    assert same(hist[0], sse) and not np.asarray(pop.lm_accepts).any()
    assert same(pop.lm_fit_stats.m2_p, fg.stats.m2_p) and same(pop.lm_fit_stats.cov, fg.stats.cov) and pop.lm_fit_stats.W == fg.stats.W
    # N = 0: M2_y = 0 for every complete tree, NaN where a constant already fails the flag; every row of the history the same
    hist = []
    consts, sse, ok = pop.fit_constants_lm_device(np.zeros((3, 0), dtype=dtype, order="F"), np.zeros(0, dtype=dtype), iters=3, history=hist, scaled=True)
    assert ok.tolist() == [True] * 6 + [False] and not sse[:6].any() and np.isnan(sse[6]) and len(hist) == 4
    assert all(same(h, sse) for h in hist) and pop.lm_fit_stats.W == 0.0
    assert same(consts, c0) and same(pop.constants(), c0) and not np.asarray(pop.lm_accepts).any()
    pop.close()
    # a population without a constant: nothing to fit, every row the first
    pop = api.Population([no_const(), no_const()], OPS, dtype, n_features=3)
    hist = []
    consts, sse, ok = pop.fit_constants_lm_device(X, y, weights=w, iters=2, history=hist, scaled=True)
    assert consts.size == 0 and ok.all() and len(hist) == 3 and all(same(h, sse) for h in hist) and np.isfinite(sse).all()
    pop.close()
    # an empty population
    empty = api.Population([], OPS, dtype, n_features=3)
    consts, sse, ok = empty.fit_constants_lm_device(X, y, iters=2, scaled=True)
    assert consts.size == 0 and sse.size == 0 and ok.size == 0
    consts, sse, ok = empty.fit_constants_lm_device(dev_X(torch, X), torch.from_numpy(y).cuda(), iters=2, scaled=True)
    assert consts.numel() == 0 and sse.numel() == 0 and ok.numel() == 0
    empty.close()


def test_refusals(api):
    lib = api.library()
    cos1 = de.OperatorEnum(binary_operators=("+",), unary_operators=("cos",))
    tree = de.Node(1, de.Node(1, de.Node(feature=1)), de.Node(val=0.5))
    X = np.asfortranarray(np.linspace(-1, 1, 64)[None, :])

    def raw(pop, Xa, ya, opts=None, yp=True, okp=True, ssep=True, n=1):
        """de_fit_consts_lm_scaled itself on sentinel-filled outputs: (status, every output still the sentinel)."""
        se, st, ys, ok = np.full(n, 7.0), np.full(3 * n, 7.0), np.full(3, 7.0), np.full(n, 9, dtype=np.uint8)
        hist, acc = np.full(16 * n, 7.0), np.full(n, 9, dtype=np.int32)
        rc = lib.de_fit_consts_lm_scaled(pop.ctx._h, pop._h, Xa.ctypes.data, Xa.shape[1], Xa.shape[0], None, ya.ctypes.data if yp else None, None,
                                         C.byref(opts) if opts is not None else None, se.ctypes.data if ssep else None, st.ctypes.data,
                                         ys.ctypes.data, ok.ctypes.data if okp else None, hist.ctypes.data, acc.ctypes.data)
        return rc, bool((se == 7).all() and (st == 7).all() and (ys == 7).all() and (ok == 9).all() and (hist == 7).all() and (acc == 9).all())

    for dtype in (np.float16, np.complex64):  # evaluation-only populations
        pop = api.Population([tree], cos1, dtype, n_features=1)
        before = pop.constants().copy()
        with pytest.raises(api.DeviceError, match="DE_ERR_UNSUPPORTED"):
            pop.fit_constants_lm_device(X.astype(dtype), np.zeros(64, dtype=dtype), scaled=True)
        Xc = np.asfortranarray(X.astype(dtype))
        assert raw(pop, Xc, Xc) == (7, True) and same(pop.constants(), before)
        pop.close()
    # a GraphNode population with a shared constant: the host loop serves it
    Gn = de.GraphNode
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    x1, c, c2 = Gn(feature=1), Gn(val=0.75), Gn(val=-0.4)
    sh = Gn(1, Gn(2, x1, c))
    dag = Gn(1, Gn(1, sh, Gn(2, sh, Gn(2, c, x1))), c2)
    for dtype in (np.float32, np.float64):
        pop = api.Population([dag], ops, dtype, n_features=1)
        before = pop.constants().copy()
        Xf, y = np.asfortranarray(X.astype(dtype)), np.zeros(64, dtype=dtype)
        with pytest.raises(ValueError, match="fit_constants_lm"):
            pop.fit_constants_lm_device(Xf, y, scaled=True)
        with pytest.raises(ValueError, match="lm_step"):
            pop.eval_fit_stats_grad(Xf, y).lm_step_device(1e-3)
        assert raw(pop, Xf, y) == (7, True) and same(pop.constants(), before)
        pop.close()
    # the Python refusals of scaled=True, bad options, a null y / ok / sse
    dtype = np.float32
    # (under scaling an additive constant has a zero projected gradient: the second tree, cos(x1 + 0.3), is the one that moves)
    pop = api.Population([tree, de.Node(1, de.Node(1, de.Node(feature=1), de.Node(val=0.3)))], cos1, dtype, n_features=1)
    Xf, y = np.asfortranarray(X.astype(dtype)), np.cos(X[0]).astype(dtype)
    before = pop.constants().copy()
    for kw in (dict(wide=True), dict(loss="huber", loss_param=1.0), dict(loss="L1")):
        with pytest.raises(ValueError, match="scaled"):
            pop.fit_constants_lm_device(Xf, y, consts0=before * 2, scaled=True, **kw)
    assert same(pop.constants(), before)
    O = api.LmOpts
    for opts in (O(-1, 0, 1e-3, 10, 0.1, 1e-12), O(3, 1, 1e-3, 10, 0.1, 1e-12), O(3, 0, 0.0, 10, 0.1, 1e-12), O(3, 0, -1e-3, 10, 0.1, 1e-12),
                 O(3, 0, 1e-3, float("inf"), 0.1, 1e-12), O(3, 0, 1e-3, 10, float("nan"), 1e-12), O(3, 0, 1e-3, 10, 0.1, 0.0),
                 O(3, 0, float("nan"), 10, 0.1, 1e-12), O(3, 0, 1e-3, 0.0, 0.1, 1e-12), O(3, 0, 1e-3, 10, 0.1, float("inf"))):
        assert raw(pop, Xf, y, opts, n=2) == (1, True), list(getattr(opts, n) for n, _ in O._fields_)
        assert same(pop.constants(), before)
    assert raw(pop, Xf, y, yp=False, n=2) == (1, True) and raw(pop, Xf, y, okp=False, n=2) == (1, True)
    assert raw(pop, Xf, y, ssep=False, n=2) == (1, True) and same(pop.constants(), before)
    for kw in (dict(iters=-1), dict(lam0=0.0), dict(up=float("inf")), dict(down=float("nan"))):
        with pytest.raises(ValueError):
            pop.fit_constants_lm_device(Xf, y, scaled=True, **kw)
    with pytest.raises(ValueError):
        pop.fit_constants_lm_device(Xf, y[:-1], scaled=True)
    with pytest.raises(ValueError):
        pop.fit_constants_lm_device(Xf, y, consts0=before[:-1], scaled=True)
    assert same(pop.constants(), before)
    # de_fit_stats_lm_step: a bad dtype, a negative offset, a null buffer
    one, z8 = np.zeros(16), np.zeros(16, dtype=np.uint8)
    ng1, neg = np.array([1], dtype=np.int32), np.array([-1], dtype=np.int64)
    p = [v.ctypes.data for v in (one, one, one)]
    h = pop.ctx._h
    assert lib.de_fit_stats_lm_step(h, 99, 1, ng1.ctypes.data, *p, None, one.ctypes.data, None, z8.ctypes.data, one.ctypes.data, one.ctypes.data, None) == 1
    assert lib.de_fit_stats_lm_step(h, 1, 1, ng1.ctypes.data, *p, neg.ctypes.data, one.ctypes.data, None, z8.ctypes.data, one.ctypes.data, one.ctypes.data, None) == 1
    assert lib.de_fit_stats_lm_step(h, 1, 1, ng1.ctypes.data, *p, None, None, None, z8.ctypes.data, one.ctypes.data, one.ctypes.data, None) == 1
    assert lib.de_fit_stats_lm_step(h, 1, 0, None, None, None, None, None, None, None, None, None, None, None) == 0
    # ... and the fit with good arguments runs (null options: the defaults; stats / ystats / history / n_accept may be null)
    rc, untouched = raw(pop, Xf, y, None, n=2)
    assert rc == 0 and not untouched and not same(pop.constants(), before)
    se, ok = np.full(2, 7.0), np.full(2, 9, dtype=np.uint8)
    assert lib.de_fit_consts_lm_scaled(h, pop._h, Xf.ctypes.data, 64, 1, None, y.ctypes.data, None, None, se.ctypes.data, None, None, ok.ctypes.data,
                                       None, None) == 0 and ok.tolist() == [1, 1] and np.isfinite(se).all()
    pop.close()


# ---- 7. ordering -------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_stream_order_without_synchronisation(api, torch, dtype):
    trees = GN.population_trees(36, (1, 2, 3, 4), dtype, per_width=5)
    X, y, w = GN.data(513, 3, dtype, 9)
    Xd, yd, wd = dev_X(torch, X), torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda()
    busy = torch.randn(2048, 2048, device="cuda")
    got = []
    for sync in (False, True):
        pop = api.Population(trees, OPS, dtype, n_features=3)
        c0 = pop.constants()
        start, other = torch.from_numpy((c0 * dtype(1.25)).astype(dtype)).cuda(), torch.from_numpy((c0 * dtype(0.5)).astype(dtype)).cuda()
        wait = torch.cuda.synchronize if sync else (lambda: None)
        wait()
        for _ in range(8):  # a long kernel ahead of the fit on the stream
            busy = torch.tanh(busy @ busy) if not sync else busy
        consts, sse, ok = pop.fit_constants_lm_device(Xd, yd, start, weights=wd, iters=4, scaled=True)
        step = pop.eval_fit_stats_grad(Xd, yd, weights=wd).lm_step_device(1e-3)
        wait()
        pop.set_constants(other)
        wait()
        lo, oke = pop.eval_loss(Xd, yd, weights=wd)
        torch.cuda.synchronize()
        got.append([api._host(v).tobytes() for v in (consts, sse, ok, step, lo, oke, pop.lm_accepts)])
        assert pop.consts_on_device_path
        ref = api.Population(trees, OPS, dtype, n_features=3)  # the last evaluation saw `other`, not the fitted constants
        ref.set_constants(api._host(other))
        rl, rk = ref.eval_loss(X, y, weights=w)
        assert same(rl, api._host(lo))
        ref.close()
        pop.close()
    assert got[0] == got[1]
