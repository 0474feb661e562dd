"""GPU tests of the scaled Levenberg-Marquardt fit for trees of 9 to 32 constants (include/de_hip.h de_eval_fit_stats_grad_wide /
de_fit_stats_lm_step_wide / de_fit_consts_lm_scaled_wide): the wide route (§4.4.7) and the scaled fit (§4.4.8) joined.

The population: tests/test_gpu_lm.py's narrow one (63 trees of 0 .. 8 constants), cos_sum(k) and chain(k) for k in 9, 12, 16, 17, 31, 32,
chain(33), the two incomplete trees and the flat tree 0 * 0.75; 3 features, X in [-2, 2).  cos_sum(32) and cos_sum(31) are used as they are
if test_the_widest_trees_fit_the_gradient_kernels passes (it asserts that eval_grad accepts them).

    matrices   stats / ystats / D / P / Q / ok and the narrow blocks: the bits of eval_fit_stats_grad; the wide blocks: the bits of
               eval_gauss_newton(wide=True) under L2 and, independently, |H - H_ref| <= 256 u A entrywise over the device's own eval_grad
               rows (tests/test_gpu_gauss_newton.py's derived bound, none exempt)
    steps      G <= 8: de_fit_stats_lm_step's bytes; 8 < G <= 32: de_lm_solve_host_wide of de_lm_project_host_wide's system bit for bit,
               and |delta - delta_np| <= 8 G^2 u cond_2(A) |delta_np| against projected().lm_step where cond_2(A) < 10^12, lam >= 1e-3
    loop       a host emulation that takes every evaluation from eval_fit_stats_grad(wide=True) and every step from the wide hooks:
               constants, scaled_sse, history, n_accept and stats bit for bit
    recovery   the scenario tests/test_lm_scaled_wide_host.py fixed on the CPU (c0 = c* + PERTURB, ITERS iterations):
               final scaled_sse <= max(1e-9 initial, 4 * 1024 u M2_y)"""
import ctypes as C

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import test_gpu_gauss_newton as GN
import test_gpu_lm as LM
import test_gpu_lm_scaled as LS
import test_lm_scaled_wide_host as WH

pytestmark = pytest.mark.gpu
OPS = GN.OPS
DTYPES = LM.DTYPES
api = LM.api
torch = LM.torch
chain, bad_trees, dev_X, offsets, cos_sum, same = LM.chain, LM.bad_trees, LM.dev_X, LM.offsets, LS.cos_sum, LS.same

WIDTHS = (9, 12, 16, 17, 31, 32)
N_GOOD = 63
COS = list(range(N_GOOD, N_GOOD + 6))
CHAIN = list(range(N_GOOD + 6, N_GOOD + 12))
WIDE = COS + CHAIN
TOO_WIDE = N_GOOD + 12
BAD = [TOO_WIDE + 1, TOO_WIDE + 2]
FLAT = TOO_WIDE + 3
N_TREES = FLAT + 1


def trees_of(dtype):
    good = GN.population_trees(31, range(9), dtype)
    assert len(good) == N_GOOD
    return good + [cos_sum(k, dtype) for k in WIDTHS] + [chain(k) for k in WIDTHS] + [chain(33)] + list(bad_trees()) + [LS.flat_tree()]


_POPS = {}


def population(api, dtype):
    """One population per element type, shared by the cases that do not change its constants."""
    key = np.dtype(dtype)
    if key not in _POPS:
        _POPS[key] = api.Population(trees_of(dtype), OPS, dtype, n_features=3)
    return _POPS[key]


def stats3(fg, t):
    st = fg.stats
    return [st.mean_p[t], st.m2_p[t], st.cov[t]], [st.W, st.mean_y, st.m2_y]


def hooks_wide(api, fg, lam):
    """tests/test_gpu_lm_scaled.py's `hooks` for trees of up to 32 rows: per tree of a numpy FitStatsGrad (step[G] or zeros, scaled_sse,
    produced) from de_lm_project_host_wide + de_lm_solve_host_wide"""
    has = np.asarray(fg.has_jtj)
    lams = np.broadcast_to(np.asarray(lam, dtype=np.float64), (len(fg),))
    steps, sses, made = [], np.empty(len(fg)), np.zeros(len(fg), dtype=bool)
    for t in range(len(fg)):
        D, P, Q = fg._dpq(t)
        G = D.size
        if G == 0 or G > 32:  # (the objective needs no matrix)
            sses[t] = api.lm_project_host_wide(*stats3(fg, t), [], [], [], np.zeros((0, 0)))[0]
            steps.append(np.zeros(G))
            continue
        sse, g, Ht, formed = api.lm_project_host_wide(*stats3(fg, t), D, P, Q, np.asarray(fg.jtj[t]).astype(np.float64))
        sses[t] = sse
        step, produced = api.lm_solve_host_wide(Ht, g, lams[t]) if has[t] else (np.zeros(G), False)
        made[t] = bool(has[t] and formed and produced)
        steps.append(step if made[t] else np.zeros(G))
    return steps, sses, made


def emulate_wide(api, ref, X, y, w, c0, iters, lam0=1e-3, up=10.0, down=0.1, **kw):
    """tests/test_gpu_lm_scaled.py's `emulate` with every evaluation eval_fit_stats_grad(wide=True) and the wide hooks' steps"""
    dtype, at, nt = c0.dtype.type, offsets(ref.n_consts), ref.n_trees

    def ev(c):
        ref.set_constants(c)
        return ref.eval_fit_stats_grad(X, y, weights=w, wide=True, **kw)

    consts, fg = c0.copy(), ev(c0)
    _, sse, _ = hooks_wide(api, fg, lam0)
    lam, acc, hist = np.full(nt, lam0), np.zeros(nt, dtype=np.int32), [sse.copy()]
    for _ in range(iters):
        steps, _, made = hooks_wide(api, fg, lam)
        trial = consts.copy()
        for t in np.flatnonzero(made):
            trial[at[t]:at[t + 1]] = (consts[at[t]:at[t + 1]].astype(np.float64) + steps[t]).astype(dtype)
        ft = ev(trial)
        _, sse_t, _ = hooks_wide(api, ft, lam)
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


def test_the_widest_trees_fit_the_gradient_kernels(api):
    for dtype in (np.float32, np.float64):
        pop = api.Population([cos_sum(31, dtype), cos_sum(32, dtype), chain(32), chain(33)], OPS, dtype, n_features=3)
        X, _, _ = GN.data(64, 3, dtype, 1)
        _, grads, ok = pop.eval_grad(X)  # (an LDS footprint beyond the kernels' is a DeviceError here)
        assert ok.all() and [g.shape[0] for g in grads] == [31, 32, 32, 33] and all(np.isfinite(g).all() for g in grads)
        pop.close()


# ---- 1. matrices ---------------------------------------------------------------------------------------------------------------------------
def check_matrices(api, pop, X, y, w, dtype, label):
    ng = pop._n_grad_all(api._grad_mode(False))
    assert ng[COS].tolist() == list(WIDTHS) and ng[CHAIN].tolist() == list(WIDTHS) and ng[TOO_WIDE] == 33 and ng[FLAT] == 2
    fw = pop.eval_fit_stats_grad(X, y, weights=w, wide=True)  # (without the feature: no such keyword, no such symbol)
    kernel = pop.ctx.last_kernel_name()
    fn = pop.eval_fit_stats_grad(X, y, weights=w)
    again = pop.eval_fit_stats_grad(X, y, weights=w, wide=True)
    gw = pop.eval_gauss_newton(X, y, weights=w, wide=True)
    ok, has = np.asarray(fw.ok), np.asarray(fw.has_jtj)
    assert np.array_equal(has, ok & (ng <= 32)) and has[WIDE].all() and ok[TOO_WIDE] and not has[TOO_WIDE] and not ok[BAD].any()
    assert np.array_equal(ok, np.asarray(fn.ok)) and np.array_equal(ok, np.asarray(gw.ok)) and fw._packed["wide"] and not fn._packed["wide"]
    assert same(fw._packed["stats"], fn._packed["stats"]) and same(fw._packed["dmom"], fn._packed["dmom"])  # stats, ystats, D | P | Q: every tree
    assert same(fw._packed["jtj"], again._packed["jtj"]) and same(fw._packed["dmom"], again._packed["dmom"])  # run to run
    for t in range(N_TREES):
        if ng[t] <= 8:
            assert same(fw.jtj[t], fn.jtj[t]) and bool(has[t]) == bool(np.asarray(fn.has_jtj)[t]), t
    for t in [TOO_WIDE] + BAD:
        assert fw.jtj[t].size > 0 and np.isnan(fw.jtj[t]).all()
    _, grads, okg = pop.eval_grad(X)
    assert np.array_equal(okg, ok)
    u, fmax, worst = GN.unit(dtype), float(np.finfo(dtype).max), 0.0
    for t in WIDE:
        assert np.isnan(fn.jtj[t]).all() and np.isfinite(fw.jtj[t]).all(), t
        assert same(fw.jtj[t], gw.jtj[t]), t  # de_eval_loss_gn_wide's block under {DE_LOSS_L2, 0, 0}, bit for bit
        H = np.asarray(fw.jtj[t]).astype(np.float64)
        Href, A = GN.reference(grads[t], w)
        assert np.isfinite(np.asarray(grads[t])).all() and np.isfinite(A).all() and A.max() <= 0.25 * fmax, t  # none exempt
        assert np.array_equal(H, H.T), t
        err = np.abs(H - Href)
        assert (err <= GN.K * u * A).all(), (label, t, (err / (u * np.maximum(A, np.finfo(np.float64).tiny))).max())
        worst = max(worst, float((err[A > 0] / (u * A[A > 0])).max()) if (A > 0).any() else 0.0)
    print(f"[lm scaled wide matrices] {np.dtype(dtype).name} {label}: {len(WIDE)} wide blocks equal eval_gauss_newton(wide=True) bit for bit, "
          f"worst |H - H_ref| = {worst:.2f} u A (bound {GN.K:.0f}), kernel {kernel}")
    return fw, ng


@DTYPES
@pytest.mark.parametrize("N", [1, 64, 257])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_wide_matrices(api, dtype, N, weighted):
    X, y, w = GN.data(N, 3, dtype, 40 + N, weighted)
    check_matrices(api, population(api, dtype), X, y, w, dtype, f"N={N} {'weighted' if weighted else 'unweighted'}")


# ---- 2. three chunks, the last one ragged --------------------------------------------------------------------------------------------------
@DTYPES
def test_three_chunks_the_last_one_ragged(api, torch, dtype, monkeypatch):
    monkeypatch.setenv("DE_GN_WIDE_CHUNK", "128")
    pop = population(api, dtype)
    X, y, w = GN.data(300, 3, dtype, 77)
    fw, ng = check_matrices(api, pop, X, y, w, dtype, "N=300 in chunks of 128")
    # device buffers: the same bytes
    fd = pop.eval_fit_stats_grad(dev_X(torch, X), torch.from_numpy(y).cuda(), weights=torch.from_numpy(w).cuda(), wide=True)
    torch.cuda.synchronize()
    assert same(api._host(fd._packed["stats"]), fw._packed["stats"]) and same(api._host(fd._packed["dmom"]), fw._packed["dmom"])
    assert same(api._host(fd._packed["jtj"]), fw._packed["jtj"]) and np.array_equal(api._host(fd.has_jtj), np.asarray(fw.has_jtj))
    # the C call itself: caller-chosen offsets with gaps, sentinels around dmom and jtj
    lib, nt = api.library(), N_TREES
    off, joff_p = offsets(ng), offsets(ng * ng)
    moff = (3 * off[:-1] + 2 * np.arange(nt) + 4).astype(np.int64)
    joff = (joff_p[:-1] + 3 * np.arange(nt) + 4).astype(np.int64)
    dm2 = np.full(int(moff[-1] + 3 * ng[-1]) + 4, 7.0)
    jt2 = np.full(int(joff[-1] + ng[-1] ** 2) + 4, 7, dtype=dtype)
    st2, ok2 = np.full(3 * nt + 3, 7.0), np.full(nt, 9, dtype=np.uint8)
    pop.ctx.check(lib.de_eval_fit_stats_grad_wide(pop.ctx._h, pop._h, X.ctypes.data, 300, 3, None, 1, y.ctypes.data, w.ctypes.data, st2.ctypes.data,
                                                  st2.ctypes.data + 24 * nt, dm2.ctypes.data, moff.ctypes.data, jt2.ctypes.data, joff.ctypes.data,
                                                  ok2.ctypes.data))
    own_m, own_j = np.zeros(dm2.size, dtype=bool), np.zeros(jt2.size, dtype=bool)
    for t in range(nt):
        own_m[moff[t]:moff[t] + 3 * ng[t]] = True
        own_j[joff[t]:joff[t] + ng[t] ** 2] = True
        assert same(dm2[moff[t]:moff[t] + 3 * ng[t]], fw._packed["dmom"][3 * off[t]:3 * off[t + 1]]), t
        assert same(jt2[joff[t]:joff[t] + ng[t] ** 2], fw._packed["jtj"][joff_p[t]:joff_p[t + 1]]), t
    assert (dm2[~own_m] == 7).all() and (jt2[~own_j] == 7).all() and same(st2, fw._packed["stats"])
    assert np.array_equal(ok2.astype(bool), np.asarray(fw.ok))


# ---- 3. the step kernel ----------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("N", [64, 257])
def test_wide_step_kernel_against_the_host_hooks(api, torch, dtype, N):
    pop = population(api, dtype)
    nt = N_TREES
    X, y, w = GN.data(N, 3, dtype, 40 + N)
    lam = np.array([(0.0, 1e-3, 1.0, 1e3)[t % 4] for t in range(nt)])
    lam[COS] = [1e-3, 1.0, 1e3, 1e-3, 1.0, 1e3]
    fw, fn = pop.eval_fit_stats_grad(X, y, weights=w, wide=True), pop.eval_fit_stats_grad(X, y, weights=w)
    ng = fw._packed["n_grad"].astype(np.int64)
    off = offsets(ng)
    step, sse = fw.lm_step_device(lam, return_sse=True)
    nstep, nsse = fn.lm_step_device(lam, return_sse=True)  # de_fit_stats_lm_step
    assert step.dtype == np.float64 and step.shape == (int(off[-1]),) and sse.shape == (nt,)
    has = np.asarray(fw.has_jtj)
    want, want_sse, made = hooks_wide(api, fw, lam)
    assert same(sse, nsse) and same(sse, want_sse)  # every tree, the NaN of the incomplete ones included
    n_wide_nonzero = 0
    for t in range(nt):
        mine = step[off[t]:off[t + 1]]
        if ng[t] <= 8:
            assert same(mine, nstep[off[t]:off[t + 1]]), t  # de_fit_stats_lm_step's bytes
        assert same(mine, want[t]), (t, ng[t], lam[t], mine, want[t])  # the hooks' bits: no exemption
        n_wide_nonzero += int(ng[t] > 8 and made[t] and mine.any())
    assert not nstep[off[WIDE[0]]:off[TOO_WIDE + 1]].any()  # (the narrow call leaves every wide tree the zero step)
    for t in [TOO_WIDE, FLAT] + BAD:
        assert not step[off[t]:off[t + 1]].any() and not made[t], t
    for t in COS:  # lam > 0: the purpose-built trees produce a step
        assert made[t] and step[off[t]:off[t + 1]].any(), (t, ng[t], lam[t])
    assert n_wide_nonzero >= len(COS), n_wide_nonzero
    # against projected().lm_step (numpy's LU on the same projected system): the forward bound
    ref, worst, n_fwd = fw.projected().lm_step(lam), 0.0, 0
    for t in np.flatnonzero(made):
        G = int(ng[t])
        _, g, Ht, _ = api.lm_project_host_wide(*stats3(fw, t), *fw._dpq(t), np.asarray(fw.jtj[t]).astype(np.float64))
        cond = np.linalg.cond(LM.damped(Ht, lam[t]), 2)
        if lam[t] >= 1e-3 and cond < 1e12:
            err, bound = np.linalg.norm(step[off[t]:off[t + 1]] - ref[t]), 8 * G * G * LM.U64 * cond * np.linalg.norm(ref[t])
            assert err <= bound, (t, G, lam[t], err / bound)
            worst, n_fwd = max(worst, err / bound if bound else 0.0), n_fwd + 1
    assert n_fwd >= len(COS), n_fwd  # (the purpose-built trees; a random tree's rows may lie in the span of [1, yhat])
    # device tensors: the same bits, nothing copied
    fd = pop.eval_fit_stats_grad(dev_X(torch, X), torch.from_numpy(y).cuda(), weights=torch.from_numpy(w).cuda(), wide=True)
    sd, ed = fd.lm_step_device(torch.from_numpy(lam).cuda(), return_sse=True)
    assert all(torch.is_tensor(v) and v.is_cuda and v.dtype == torch.float64 for v in (sd, ed))
    assert same(sd.cpu().numpy(), step) and same(ed.cpu().numpy(), sse)
    # the C call itself: has == 0 for one wide tree, sentinels around the packed step and sse (host, then device buffers)
    lib, pk = api.library(), fw._packed
    hasb, total = has.astype(np.uint8), int(off[-1])
    hasb[COS[1]] = 0
    st2, se2 = np.full(total + 8, 7.0), np.full(nt + 8, 7.0)
    args = (api._dtype_code(dtype), nt, pk["n_grad"].ctypes.data)
    pop.ctx.check(lib.de_fit_stats_lm_step_wide(pop.ctx._h, *args, pk["stats"].ctypes.data, pk["stats"].ctypes.data + 24 * nt, pk["dmom"].ctypes.data,
                                                None, pk["jtj"].ctypes.data, None, hasb.ctypes.data, lam.ctypes.data, st2[4:].ctypes.data,
                                                se2[4:].ctypes.data))
    expect = step.copy()
    expect[off[COS[1]]:off[COS[1] + 1]] = 0.0
    assert (st2[:4] == 7).all() and (st2[4 + total:] == 7).all() and same(st2[4:4 + total], expect)
    assert (se2[:4] == 7).all() and (se2[4 + nt:] == 7).all() and same(se2[4:4 + nt], sse)
    d_st, d_dm, d_jt, d_has, d_lam = (torch.from_numpy(v).cuda() for v in (pk["stats"], pk["dmom"], pk["jtj"], hasb, lam))
    d_st2 = torch.full((total + 8,), 7.0, dtype=torch.float64, device="cuda")
    pop.ctx.use_torch_stream()
    pop.ctx.check(lib.de_fit_stats_lm_step_wide(pop.ctx._h, *args, d_st.data_ptr(), d_st.data_ptr() + 24 * nt, d_dm.data_ptr(), None, d_jt.data_ptr(),
                                                None, d_has.data_ptr(), d_lam.data_ptr(), d_st2.data_ptr() + 32, None))
    assert same(d_st2.cpu().numpy(), st2)
    print(f"[lm scaled wide step] {np.dtype(dtype).name} N={N}: {n_wide_nonzero} non-zero wide steps and {nt} scaled_sse equal the wide hooks bit for "
          f"bit; against projected().lm_step worst {worst:.3g} of the forward bound over {n_fwd} trees")


# ---- 4. the loop against a host emulation ----------------------------------------------------------------------------------------------------
@DTYPES
def test_iterations_follow_the_host_rule(api, dtype):
    trees = trees_of(dtype)
    pop, ref = api.Population(trees, OPS, dtype, n_features=3), api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = GN.data(257, 3, dtype, 17)
    c0, at, ng = pop.constants().copy(), offsets(pop.n_consts), np.asarray(pop.n_consts)
    moved = {}
    for iters in (1, 2):  # (the second iteration's step shows the lam the first left: down on accept, up otherwise)
        hist, hn = [], []
        consts, sse, ok = pop.fit_constants_lm_scaled_device(X, y, c0, weights=w, iters=iters, history=hist, wide=True)
        acc, st = np.asarray(pop.lm_accepts).copy(), pop.lm_fit_stats
        assert consts.dtype == dtype and sse.dtype == np.float64 and len(hist) == iters + 1
        ce, se, he, ae, ste = emulate_wide(api, ref, X, y, w, c0, iters)
        assert same(consts, ce) and same(sse, se) and same(np.stack(hist), np.stack(he)) and np.array_equal(acc, ae), (iters, acc, ae)
        for name in ("mean_p", "m2_p", "cov"):
            assert same(getattr(st, name), getattr(ste, name)), name
        moved[iters] = [t for t in WIDE if not same(consts[at[t]:at[t + 1]], c0[at[t]:at[t + 1]])]
        # the narrow trees: de_fit_consts_lm_scaled's trajectory on the same population
        cn, sn, okn = pop.fit_constants_lm_device(X, y, c0, weights=w, iters=iters, history=hn, scaled=True)
        accn, stn = np.asarray(pop.lm_accepts), pop.lm_fit_stats
        assert np.array_equal(ok, okn)
        for t in range(N_TREES):
            a, b = at[t], at[t + 1]
            if ng[t] <= 8:
                assert same(consts[a:b], cn[a:b]) and same(sse[t:t + 1], sn[t:t + 1]) and acc[t] == accn[t], t
                assert all(same(r1[t:t + 1], r2[t:t + 1]) for r1, r2 in zip(hist, hn)), t
                assert all(same(getattr(st, n)[t:t + 1], getattr(stn, n)[t:t + 1]) for n in ("mean_p", "m2_p", "cov")), t
            else:
                assert same(cn[a:b], c0[a:b]) and accn[t] == 0, t  # (the narrow call leaves a wide tree alone)
        for t in [TOO_WIDE] + BAD:
            assert same(consts[at[t]:at[t + 1]], c0[at[t]:at[t + 1]]) and acc[t] == 0, t
    assert len(moved[2]) >= 1 and set(moved[1]) <= set(moved[2]), moved  # (an accepted tree never returns to c0)
    print(f"[lm scaled wide iterations] {np.dtype(dtype).name}: {len(moved[1])} / {len(moved[2])} of {len(WIDE)} wide trees moved after 1 / 2 "
          f"iterations, as the host rule has it")
    pop.close()
    ref.close()


# ---- 5. recovery -----------------------------------------------------------------------------------------------------------------------------
def narrow_tree(c):  # cos(c1 * x1) + c2 * x2
    return de.Node(1, de.Node(1, de.Node(3, de.Node(val=c[0]), de.Node(feature=1))), de.Node(3, de.Node(val=c[1]), de.Node(feature=2)))


@DTYPES
@pytest.mark.parametrize("where", ["numpy", "torch"])
def test_scaled_fit_of_cos_sum_12_on_the_device(api, torch, dtype, where):
    u = GN.unit(dtype)
    x, y, w = WH.recovery_data(dtype)
    X = np.asfortranarray(x)
    n_copies = 28
    trees = [cos_sum(WH.K, dtype) for _ in range(n_copies)] + [narrow_tree(c) for c in ((1.3, 0.7), (0.9, -0.4), (1.7, 0.2), (0.5, 1.1))]
    pop, fresh = api.Population(trees, OPS, dtype, n_features=3), api.Population(trees, OPS, dtype, n_features=3)
    consts0 = pop.constants().copy()
    assert np.array_equal(consts0[:WH.K], WH.C_STAR.astype(dtype))  # cos_sum's own constants are c*
    for i in range(n_copies):
        consts0[i * WH.K:(i + 1) * WH.K] = (WH.C_STAR + WH.PERTURB).astype(dtype)
    if where == "torch":
        Xa, ya, wa, ca = dev_X(torch, X), torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(consts0).cuda()
    else:
        Xa, ya, wa, ca = X, y, w, consts0
    hist = []
    consts, sse, ok = pop.fit_constants_lm_scaled_device(Xa, ya, ca, weights=wa, iters=WH.ITERS, history=hist, wide=True)
    if where == "torch":
        assert all(torch.is_tensor(v) and v.is_cuda for v in (consts, sse, ok)) and pop.consts_on_device_path and sse.dtype == torch.float64
    loss, h0 = api._host(sse), api._host(hist[0])
    assert bool(api._host(ok).all()) and len(hist) == WH.ITERS + 1 and loss.dtype == np.float64
    m2y = pop.lm_fit_stats.m2_y
    bound = np.maximum(1e-9 * h0, 4 * 1024 * u * m2y)
    wide = slice(0, n_copies)
    assert (h0[wide] >= 10 * bound[wide]).all()
    acc = api._host(pop.lm_accepts)
    print(f"[lm scaled wide device fit] {np.dtype(dtype).name} {where}: worst final / bound = {(loss[wide] / bound[wide]).max():.3g}, initial / bound = "
          f"{(h0[wide] / bound[wide]).min():.3g}, accepted steps per copy {acc[wide].min()} .. {acc[wide].max()}")
    assert (loss[wide] <= bound[wide]).all(), loss[wide] / bound[wide]  # every copy
    assert same(pop.lm_fit_stats.scaled_sse, loss)
    LS.post_conditions(api, pop, fresh, X, y, w, consts0, consts, sse, hist)
    if where == "numpy":  # the host loop on the same data (one copy and the narrow trees: one evaluation per iteration on the host)
        few = api.Population(trees[n_copies - 1:], OPS, dtype, n_features=3)
        ch, lh, okh = few.fit_constants_lm(X, y, consts0[(n_copies - 1) * WH.K:], weights=w, iters=WH.ITERS, scaled=True, wide=True)
        print(f"[lm scaled wide host loop] {np.dtype(dtype).name}: final / bound = {lh[0] / bound[0]:.3g}")
        assert okh.all() and lh[0] <= bound[0], (lh[0], bound[0])
        few.close()
    pop.close()
    fresh.close()


# ---- 6. zero-weight padding ----------------------------------------------------------------------------------------------------------------
@DTYPES
def test_zero_weight_padding_gives_the_same_bits(api, dtype):
    trees = GN.population_trees(37, (1, 3, 8), dtype, per_width=2) + [cos_sum(k, dtype) for k in (9, 12, 17)] + [chain(16)]
    X, y, w = GN.data(300, 3, dtype, 29)
    Xp, yp, wp = GN.data(512, 3, dtype, 30)
    Xp[:, :300], yp[:300], wp[:300], wp[300:] = X, y, w, 0
    out = []
    for Xa, ya, wa in ((X, y, w), (np.asfortranarray(Xp), yp, wp)):
        pop = api.Population(trees, OPS, dtype, n_features=3)
        hist = []
        consts, sse, ok = pop.fit_constants_lm_scaled_device(Xa, ya, weights=wa, iters=5, history=hist, wide=True)
        out.append((consts, sse, ok, np.stack(hist), np.asarray(pop.lm_accepts)))
        pop.close()
    assert all(same(a, b) for a, b in zip(*out))
    assert out[0][4][6:9].all()  # the fit did something for the wide cos_sum trees


# ---- 7. edges and refusals -------------------------------------------------------------------------------------------------------------------
def test_edges(api, torch):
    dtype = np.float32
    trees = GN.population_trees(35, (0, 2, 3), dtype, per_width=2) + [cos_sum(12, dtype), chain(33),
                                                                      de.Node(1, de.Node(feature=1), de.Node(val=float("inf")))]
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = GN.data(129, 3, dtype, 5)
    c0 = pop.constants().copy()
    i_wide, i_33, i_inf = 6, 7, 8
    # iters = 0: the first evaluation's values, the constants unchanged
    hist = []
    consts, sse, ok = pop.fit_constants_lm_scaled_device(X, y, weights=w, iters=0, history=hist, wide=True)
    fg = pop.eval_fit_stats_grad(X, y, weights=w, wide=True)
    assert len(hist) == 1 and same(consts, c0) and same(pop.constants(), c0)
    assert np.array_equal(sse, fg.stats.scaled_sse, equal_nan=True) and np.array_equal(ok, fg.ok) and not ok[i_inf] and ok[:i_inf].all()
    assert same(hist[0], sse) and not np.asarray(pop.lm_accepts).any() and same(pop.lm_fit_stats.m2_p, fg.stats.m2_p)
    # N = 0: blocks of 0 up to 32 rows, NaN beyond and where a constant already fails the flag; every row of the history the same
    X0, y0 = np.zeros((3, 0), dtype=dtype, order="F"), np.zeros(0, dtype=dtype)
    f0 = pop.eval_fit_stats_grad(X0, y0, wide=True)
    assert not f0.jtj[i_wide].any() and f0.jtj[i_wide].shape == (12, 12) and np.isnan(f0.jtj[i_33]).all() and np.isnan(f0.jtj[i_inf]).all()
    assert np.isnan(pop.eval_fit_stats_grad(X0, y0).jtj[i_wide]).all()  # (the narrow call keeps its NaN block)
    assert np.asarray(f0.has_jtj).tolist() == [True] * 7 + [False, False]
    hist = []
    consts, sse, ok = pop.fit_constants_lm_scaled_device(X0, y0, iters=3, history=hist, wide=True)
    assert ok.tolist() == [True] * 8 + [False] and not sse[:8].any() and np.isnan(sse[8]) and len(hist) == 4
    assert all(same(h, sse) for h in hist) and pop.lm_fit_stats.W == 0.0 and same(consts, c0) and not np.asarray(pop.lm_accepts).any()
    # all-zero weights at N > 0: wide blocks of exact 0 (the Gram kernel's select excludes every sample), nothing accepted
    fz = pop.eval_fit_stats_grad(X, y, weights=np.zeros_like(w), wide=True)
    assert fz.stats.W == 0.0 and not np.asarray(fz.jtj[i_wide]).any() and np.isnan(fz.jtj[i_33]).all()
    consts, sse, ok = pop.fit_constants_lm_scaled_device(X, y, weights=np.zeros_like(w), iters=2, wide=True)
    assert same(consts, c0) and not np.asarray(pop.lm_accepts).any()
    pop.close()
    # a population without a constant, and the empty population
    pop = api.Population([LS.no_const(), LS.no_const()], OPS, dtype, n_features=3)
    hist = []
    consts, sse, ok = pop.fit_constants_lm_scaled_device(X, y, weights=w, iters=2, history=hist, wide=True)
    assert consts.size == 0 and ok.all() and len(hist) == 3 and all(same(h, sse) for h in hist) and np.isfinite(sse).all()
    pop.close()
    empty = api.Population([], OPS, dtype, n_features=3)
    consts, sse, ok = empty.fit_constants_lm_scaled_device(X, y, iters=2, wide=True)
    assert consts.size == 0 and sse.size == 0 and ok.size == 0
    consts, sse, ok = empty.fit_constants_lm_scaled_device(dev_X(torch, X), torch.from_numpy(y).cuda(), iters=2, wide=True)
    assert consts.numel() == 0 and sse.numel() == 0 and ok.numel() == 0
    empty.close()


@DTYPES
def test_parametric_program_with_a_wide_tree(api, dtype):
    P, Cn, N = 3, 4, 300
    PN = de.ParametricNode
    t = PN(3, PN(parameter=1), PN(feature=2))  # p1 * x2 + sum_i cos(c_i x_{1 + i mod 2}): 10 constants
    for i in range(10):
        t = PN(1, t, PN(1, PN(3, PN(val=float(dtype(0.6 + 0.17 * i))), PN(feature=1 + i % 2))))
    trees = GN.population_trees(34, (1, 2, 3), dtype, nfeatures=2, per_width=2, node_type=PN, nparams=P) + [t]
    pop, fresh = api.Population(trees, OPS, dtype, n_features=2, n_params=P), api.Population(trees, OPS, dtype, n_features=2, n_params=P)
    X, y, w = GN.data(N, 2, dtype, 12)
    g = np.random.Generator(np.random.PCG64(5))
    params = np.asfortranarray(g.uniform(-1.5, 1.5, (P, Cn)).astype(dtype))
    classes = g.integers(1, Cn + 1, N)
    c0, hist = pop.constants().copy(), []
    assert pop.n_consts[-1] == 10
    consts, sse, ok = pop.fit_constants_lm_scaled_device(X, y, weights=w, iters=4, history=hist, wide=True, params=params, classes=classes)
    assert len(hist) == 5 and ok[-1] and hist[-1][-1] < hist[0][-1] and pop.lm_accepts[-1] >= 1  # the wide tree moved
    LS.post_conditions(api, pop, fresh, X, y, w, c0, consts, sse, hist, params=params, classes=classes)
    ce, se, he, ae, _ = emulate_wide(api, fresh, X, y, w, c0, 4, params=params, classes=classes)
    assert same(consts, ce) and same(sse, se) and np.array_equal(np.asarray(pop.lm_accepts), ae)
    pop.close()
    fresh.close()


def test_refusals(api):
    lib = api.library()
    cos1 = de.OperatorEnum(binary_operators=("+",), unary_operators=("cos",))
    tree = de.Node(1, de.Node(1, de.Node(feature=1)), de.Node(val=0.5))
    X = np.asfortranarray(np.linspace(-1, 1, 64)[None, :])

    def raw_fit(pop, Xa, ya, opts=None, yp=True, okp=True, ssep=True, n=1):
        """de_fit_consts_lm_scaled_wide itself on sentinel-filled outputs: (status, every output still the sentinel)."""
        se, st, ys, ok = np.full(n, 7.0), np.full(3 * n, 7.0), np.full(3, 7.0), np.full(n, 9, dtype=np.uint8)
        hist, acc = np.full(16 * n, 7.0), np.full(n, 9, dtype=np.int32)
        rc = lib.de_fit_consts_lm_scaled_wide(pop.ctx._h, pop._h, Xa.ctypes.data, Xa.shape[1], Xa.shape[0], None, ya.ctypes.data if yp else None, None,
                                              C.byref(opts) if opts is not None else None, se.ctypes.data if ssep else None, st.ctypes.data,
                                              ys.ctypes.data, ok.ctypes.data if okp else None, hist.ctypes.data, acc.ctypes.data)
        return rc, bool((se == 7).all() and (st == 7).all() and (ys == 7).all() and (ok == 9).all() and (hist == 7).all() and (acc == 9).all())

    def raw_eval(pop, Xa, ya, G):
        """de_eval_fit_stats_grad_wide on sentinel-filled outputs"""
        st, ys, dm, jt, ok = np.full(3, 7.0), np.full(3, 7.0), np.full(3 * G, 7.0), np.full(G * G, 7, dtype=Xa.dtype), np.full(1, 9, dtype=np.uint8)
        rc = lib.de_eval_fit_stats_grad_wide(pop.ctx._h, pop._h, Xa.ctypes.data, Xa.shape[1], Xa.shape[0], None, 1, ya.ctypes.data, None, st.ctypes.data,
                                             ys.ctypes.data, dm.ctypes.data, None, jt.ctypes.data, None, ok.ctypes.data)
        return rc, bool((st == 7).all() and (ys == 7).all() and (dm == 7).all() and (jt == 7).all() and ok[0] == 9)

    for dtype in (np.float16, np.complex64):  # evaluation-only populations
        pop = api.Population([tree], cos1, dtype, n_features=1)
        before = pop.constants().copy()
        Xc = np.asfortranarray(X.astype(dtype))
        with pytest.raises(api.DeviceError, match="DE_ERR_UNSUPPORTED"):
            pop.fit_constants_lm_scaled_device(Xc, np.zeros(64, dtype=dtype), wide=True)
        assert raw_fit(pop, Xc, Xc) == (7, True) and raw_eval(pop, Xc, Xc, 1) == (7, True) and same(pop.constants(), before)
        pop.close()
    # a program made by de_program_create_cse: DE_ERR_UNSUPPORTED, sentinels and constants untouched (the narrow evaluation serves it)
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
            pop.fit_constants_lm_scaled_device(Xf, y, wide=True)
        with pytest.raises(api.DeviceError, match="de_program_create_cse"):
            pop.eval_fit_stats_grad(Xf, y, wide=True)
        assert raw_fit(pop, Xf, y) == (7, True) and raw_eval(pop, Xf, y, pop.n_grad(0, 1)) == (7, True) and same(pop.constants(), before)
        assert len(pop.eval_fit_stats_grad(Xf, y)) == 1
        pop.close()
    # bad options, a null y / ok / sse: DE_ERR_INVALID_ARG before anything is touched
    dtype = np.float32
    pop = api.Population([tree, cos_sum(10, dtype)], OPS, dtype, n_features=3)
    Xf = np.asfortranarray(np.random.default_rng(1).uniform(-2, 2, (3, 64)).astype(dtype))
    y = np.cos(Xf[0]).astype(dtype)
    before = pop.constants().copy()
    O = api.LmOpts
    for opts in (O(-1, 0, 1e-3, 10, 0.1, 1e-12), O(3, 1, 1e-3, 10, 0.1, 1e-12), O(3, 0, 0.0, 10, 0.1, 1e-12), O(3, 0, 1e-3, float("inf"), 0.1, 1e-12),
                 O(3, 0, 1e-3, 10, float("nan"), 1e-12), O(3, 0, 1e-3, 10, 0.1, 0.0)):
        assert raw_fit(pop, Xf, y, opts, n=2) == (1, True), list(getattr(opts, n) for n, _ in O._fields_)
    assert raw_fit(pop, Xf, y, yp=False, n=2) == (1, True) and raw_fit(pop, Xf, y, okp=False, n=2) == (1, True)
    assert raw_fit(pop, Xf, y, ssep=False, n=2) == (1, True) and same(pop.constants(), before)
    for kw in (dict(iters=-1), dict(lam0=0.0), dict(up=float("inf")), dict(down=float("nan")), dict(lam_min=0.0)):
        with pytest.raises(ValueError):
            pop.fit_constants_lm_scaled_device(Xf, y, wide=True, **kw)
    with pytest.raises(ValueError, match="scaled"):
        pop.fit_constants_lm_device(Xf, y, consts0=before * 2, scaled=True, wide=True)
    assert same(pop.constants(), before)
    # de_eval_fit_stats_grad_wide: a bad mode, a null buffer and a negative offset are de_eval_fit_stats_grad's refusals
    st, dm, jt, ok = np.full(9, 7.0), np.full(33, 7.0), np.full(101, 7, dtype=dtype), np.full(2, 9, dtype=np.uint8)
    neg = np.array([0, -1], dtype=np.int64)
    h, a = pop.ctx._h, (Xf.ctypes.data, 64, 3, None)
    assert lib.de_eval_fit_stats_grad_wide(h, pop._h, *a, 9, y.ctypes.data, None, st.ctypes.data, st.ctypes.data + 48, dm.ctypes.data, None, jt.ctypes.data, None, ok.ctypes.data) == 1
    assert lib.de_eval_fit_stats_grad_wide(h, pop._h, *a, 1, None, None, st.ctypes.data, st.ctypes.data + 48, dm.ctypes.data, None, jt.ctypes.data, None, ok.ctypes.data) == 1
    assert lib.de_eval_fit_stats_grad_wide(h, pop._h, *a, 1, y.ctypes.data, None, st.ctypes.data, st.ctypes.data + 48, dm.ctypes.data, None, jt.ctypes.data, neg.ctypes.data, ok.ctypes.data) == 1
    assert (st == 7).all() and (dm == 7).all() and (jt == 7).all() and (ok == 9).all()
    # ... and the fit with good arguments runs (null options: the defaults; stats / ystats / history / n_accept may be null)
    rc, untouched = raw_fit(pop, Xf, y, None, n=2)
    assert rc == 0 and not untouched and not same(pop.constants()[1:], before[1:])  # the wide tree moved
    pop.close()


# ---- stream order ------------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_stream_order_without_synchronisation(api, torch, dtype):
    trees = GN.population_trees(36, (1, 2, 3, 4), dtype, per_width=3) + [cos_sum(9, dtype), cos_sum(16, dtype)]
    X, y, w = GN.data(513, 3, dtype, 9)
    Xd, yd, wd = dev_X(torch, X), torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda()
    busy = torch.randn(2048, 2048, device="cuda")
    got = []
    for sync in (False, True):
        pop = api.Population(trees, OPS, dtype, n_features=3)
        c0 = pop.constants()
        start, other = torch.from_numpy((c0 * dtype(1.05)).astype(dtype)).cuda(), torch.from_numpy((c0 * dtype(0.5)).astype(dtype)).cuda()
        wait = torch.cuda.synchronize if sync else (lambda: None)
        wait()
        for _ in range(8):  # a long kernel ahead of the fit on the stream
            busy = torch.tanh(busy @ busy) if not sync else busy
        consts, sse, ok = pop.fit_constants_lm_scaled_device(Xd, yd, start, weights=wd, iters=4, wide=True)
        step = pop.eval_fit_stats_grad(Xd, yd, weights=wd, wide=True).lm_step_device(1e-3)
        wait()
        pop.set_constants(other)
        wait()
        lo, oke = pop.eval_loss(Xd, yd, weights=wd)
        torch.cuda.synchronize()
        got.append([api._host(v).tobytes() for v in (consts, sse, ok, step, lo, oke, pop.lm_accepts)])
        assert pop.consts_on_device_path and api._host(pop.lm_accepts)[-2:].any()
        ref = api.Population(trees, OPS, dtype, n_features=3)  # the last evaluation saw `other`, not the fitted constants
        ref.set_constants(api._host(other))
        rl, rk = ref.eval_loss(X, y, weights=w)
        assert same(rl, api._host(lo))
        ref.close()
        pop.close()
    assert got[0] == got[1]
