"""GPU tests of the fit statistics with gradients (include/de_hip.h de_eval_fit_stats_grad): per tree the statistics of
de_eval_fit_stats, the gradient moments D = sum w d, P = sum w (yhat - mean_p) d, Q = sum w (y - mean_y) d over the gradient rows of the
mode, and de_eval_loss_gn's matrix sum w d d^T — without the [n_grad, N] Jacobian.

The reference is numpy in long double over the DEVICE's own `Population.eval_grad` values and Jacobian (same handlers, same dual rows),
rounded to float64.  Bounds for complete trees, u = 2^-24 (Float32) / 2^-53 (Float64) — worst cases from the operation counts, not fits:
    stats / ystats   the bounds of tests/test_gpu_fit_stats.py: 1024 u x magnitude, 16 * 2^-53 for ystats
    |dD_k| <= 256 u sum w |d_k|                                   (a wave sum of at most 128 terms, two roundings per term, FMA or not)
    |dQ_k| <= 1024 u sum w |y - mean_y| |d_k|                     (four roundings per term, the shift of y)
    |dP_k| <= 1024 u (sum w |yhat - mean_p| |d_k| + (sum w |yhat| / W) sum w |d_k|)      (the second term: the allowed error of mean_p)
    jtj    <= 256 u sum w |d_i d_k|, and the bits of eval_gauss_newton's block for the same call
Trees whose Jacobian has a non-finite entry, or whose magnitudes are beyond a quarter of the type's largest finite value, are compared
on finiteness only; at most 5 % of a case's complete trees may be.  Every parity case prints the worst ratio it saw.

The tree generator and its seeds are those of tests/test_gpu_gauss_newton.py."""
import ctypes as C

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de

pytestmark = pytest.mark.gpu
KD, KP, KS = 256.0, 1024.0, 1024.0
U64 = 2.0 ** -53
OPS = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
MODES = {"constant": False, "variable": True, "both": "both"}
L = np.longdouble


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _api.library()
    return _api


def unit(dtype):
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def leaves_of(tree):
    return [n for n in de.postorder(tree) if n.degree == 0]


def tree_with_consts(rng, k, nodes, nfeatures, dtype, node_type=de.Node, nparams=0):
    """A random tree of `nodes` nodes whose leaves are exactly k constants (+-[0.5, 1.5)) and otherwise features (parameters keep their place)."""
    need = min(k + 1, 8)  # one feature leaf besides the constants, where 15 nodes leave room for it
    while True:
        t = de.synth.gen_random_tree_fixed_size(nodes, OPS, nfeatures, rng, dtype, node_type, nparams)
        lv = [n for n in leaves_of(t) if not getattr(n, "is_parameter", False)]
        if len(lv) >= need:
            break
    for i, n in enumerate(lv):
        if i < k:
            n.constant, n.val, n.feature = True, float(np.dtype(dtype).type(0.5 + rng.rand()) * (1 if rng.randbool() else -1)), 0
        else:
            n.constant, n.val, n.feature = False, 0.0, rng.randint(nfeatures)
    return t


def population_trees(seed, widths, dtype, nfeatures=3, per_width=7, node_type=de.Node, nparams=0):
    """per_width trees of at most 15 nodes for every number of constants in `widths`."""
    rng = de.synth.Xoshiro256ss(seed)
    trees = []
    for i in range(per_width):
        for k in widths:
            nodes = min(15, 2 * k + 1 + 2 * (i % 3))  # k + 1 leaves need 2 k + 1 nodes
            trees.append(tree_with_consts(rng, k, nodes, nfeatures, dtype, node_type, nparams))
    return trees


def data(N, nfeatures, dtype, seed, weights=True):
    g = np.random.Generator(np.random.PCG64(seed))
    X = np.asfortranarray(g.uniform(-2.0, 2.0, (nfeatures, N)).astype(dtype))
    y = g.standard_normal(N).astype(dtype)
    w = None
    if weights:
        w = g.uniform(0.25, 2, N).astype(dtype)
        w[::5] = 0
        w[-(N // 4 + 1)::2] = 0
        if N == 1:
            w[:] = 1.5
    return X, y, w


def chain(k):  # x1 * c1 + x2 * c2 + ... : k constants, every one with a non-trivial row
    t = de.Node(3, de.Node(feature=1), de.Node(val=0.5))
    for i in range(1, k):
        t = de.Node(1, t, de.Node(3, de.Node(feature=1 + i % 3), de.Node(val=0.25 * (i + 1))))
    return t


def reference(yh, J, y, w):
    """The statistics, the moments and the magnitudes of their bounds for ONE tree, in long double -> float64."""
    yh, J, yl = np.asarray(yh).astype(L), np.asarray(J).astype(L), np.asarray(y).astype(L)
    ww = np.ones_like(yl) if w is None else np.asarray(w).astype(L)
    keep = ww != 0
    yh, J, yl, ww = yh[keep], J[:, keep], yl[keep], ww[keep]
    G = J.shape[0]
    f = float
    with np.errstate(all="ignore"):
        W = ww.sum()
        my, mp = (ww * yl).sum() / W, (ww * yh).sum() / W
        pc, yc = yh - mp, yl - my
        r = dict(W=f(W), mean_y=f(my), m2_y=f((ww * yc * yc).sum()), mean_p=f(mp), m2_p=f((ww * pc * pc).sum()), cov=f((ww * pc * yc).sum()),
                 abs1=f((ww * np.abs(yh)).sum() / W), sq=f((ww * yh * yh).sum()), ysq=f((ww * yl * yl).sum()))
        r["D"] = np.array([f((ww * J[k]).sum()) for k in range(G)])
        r["P"] = np.array([f((ww * pc * J[k]).sum()) for k in range(G)])
        r["Q"] = np.array([f((ww * yc * J[k]).sum()) for k in range(G)])
        r["AD"] = np.array([f((ww * np.abs(J[k])).sum()) for k in range(G)])
        r["AP"] = np.array([f((ww * np.abs(pc) * np.abs(J[k])).sum()) for k in range(G)]) + r["abs1"] * r["AD"]
        r["AQ"] = np.array([f((ww * np.abs(yc) * np.abs(J[k])).sum()) for k in range(G)])
        r["E"] = np.array([f((ww * np.abs(2 * (yh - yl)) * np.abs(J[k])).sum()) for k in range(G)])  # the L2 gradient's magnitude
        H, A = np.zeros((G, G)), np.zeros((G, G))
        for i in range(G):
            for k in range(i, G):
                p = (ww * J[i]) * J[k]
                H[i, k] = H[k, i] = f(p.sum())
                A[i, k] = A[k, i] = f(np.abs(p).sum())
        r["H"], r["A"] = H, A
    return r


def stat_tolerances(r, dtype, constant_rule=True, factor=1.0):
    u = unit(dtype)
    with np.errstate(all="ignore"):
        t_m2, t_c = KS * u * r["m2_p"], KS * u * np.sqrt(r["m2_p"] * r["m2_y"])
        if constant_rule:
            t_m2 = max(t_m2, (KS * u) ** 2 * r["sq"])
            t_c = max(t_c, (KS * u) ** 2 * np.sqrt(r["sq"] * r["ysq"]))
    return factor * KS * u * r["abs1"], factor * t_m2, factor * t_c


def ratio(err, tol):
    err, tol = np.atleast_1d(np.asarray(err, dtype=np.float64)), np.atleast_1d(np.asarray(tol, dtype=np.float64))
    with np.errstate(all="ignore"):
        q = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(q.max()) if q.size else 0.0


def check_ystats(st, y, w):
    yl = np.asarray(y).astype(L)
    wl = np.ones_like(yl) if w is None else np.asarray(w).astype(L)
    W = wl.sum()
    my = (wl * yl).sum() / W
    m2y, amag = float((wl * (yl - my) ** 2).sum()), float((wl * np.abs(yl)).sum() / W)
    assert abs(st.W - float(W)) <= 16 * U64 * float(W)
    assert abs(st.mean_y - float(my)) <= 16 * U64 * amag
    assert abs(st.m2_y - m2y) <= 16 * U64 * m2y


def check(fg, out, grads, ok_g, y, w, dtype, gn=None, min_checked=1, constant_rule=True, label=""):
    """Every bound of the module docstring for every complete tree; returns the worst ratios (stats, D, P, Q, jtj) and the exempt share."""
    u, fmax = unit(dtype), float(np.finfo(dtype).max)
    ok, has = np.asarray(fg.ok, dtype=bool), np.asarray(fg.has_jtj, dtype=bool)
    assert np.array_equal(ok, np.asarray(ok_g, dtype=bool)), label
    st = fg.stats
    worst = dict(stats=0.0, D=0.0, P=0.0, Q=0.0, jtj=0.0)
    checked = exempt = complete = 0
    for t in range(len(fg)):
        D, P, Q = (np.asarray(v[t], dtype=np.float64) for v in (fg.d_sum, fg.d_pred, fg.d_targ))
        H = np.asarray(fg.jtj[t]).astype(np.float64)
        G = np.asarray(grads[t]).shape[0]
        assert D.shape == P.shape == Q.shape == (G,) and H.shape == (G, G), (label, t)
        if not ok[t]:
            assert np.isnan(st.mean_p[t]) and np.isnan(st.m2_p[t]) and np.isnan(st.cov[t]), (label, t)
            assert np.isnan(D).all() and np.isnan(P).all() and np.isnan(Q).all() and np.isnan(H).all(), (label, t)
            continue
        complete += 1
        if gn is not None:  # the same code, the same column order: eval_gauss_newton's bits (NaN block of a wide tree included)
            assert np.asarray(fg.jtj[t]).tobytes() == np.asarray(gn.jtj[t]).tobytes(), (label, t)
        if not has[t]:
            assert np.isnan(H).all() and (G > 8 or gn is None), (label, t)
        r = reference(out[t], grads[t], y, w)
        mags = [r["sq"], r["m2_p"], r["ysq"]] + [np.max(r[k], initial=0.0) for k in ("AD", "AP", "AQ", "A")]
        if not np.isfinite(np.asarray(grads[t])).all() or not np.isfinite(np.asarray(out[t])).all() or not np.isfinite(mags).all() \
                or max(mags) > 0.25 * fmax:
            exempt += 1
            continue
        t_mean, t_m2, t_c = stat_tolerances(r, dtype, constant_rule)
        assert st.m2_p[t] >= 0
        rs = max(ratio(abs(st.mean_p[t] - r["mean_p"]), t_mean), ratio(abs(st.m2_p[t] - r["m2_p"]), t_m2), ratio(abs(st.cov[t] - r["cov"]), t_c))
        rd, rp, rq = ratio(np.abs(D - r["D"]), KD * u * r["AD"]), ratio(np.abs(P - r["P"]), KP * u * r["AP"]), ratio(np.abs(Q - r["Q"]), KP * u * r["AQ"])
        rj = 0.0
        if has[t] and G:
            assert np.array_equal(H, H.T), f"{label} tree {t}: not symmetric"
            rj = ratio(np.abs(H - r["H"]), KD * u * r["A"])
        assert max(rs, rd, rp, rq, rj) <= 1.0, (label, t, dict(stats=rs, D=rd, P=rp, Q=rq, jtj=rj))
        for k, v in zip(("stats", "D", "P", "Q", "jtj"), (rs, rd, rp, rq, rj)):
            worst[k] = max(worst[k], v)
        checked += 1
    share = exempt / max(complete, 1)
    assert share <= 0.05, (label, exempt, complete)
    assert checked >= min_checked, (label, checked)
    return worst, share


def fmt(worst):
    return ", ".join(f"{k} {v * (KD if k in ('D', 'jtj') else KP):.2f} u" for k, v in worst.items())


def merge(a, b):
    return {k: max(a[k], b[k]) for k in a}


ZERO = dict(stats=0.0, D=0.0, P=0.0, Q=0.0, jtj=0.0)


@pytest.mark.parametrize("dtype,sizes", [(np.float32, (1, 63, 64, 65, 255, 256, 257, 513, 1000)), (np.float64, (1, 127, 128, 129, 513))],
                         ids=["f32", "f64"])
@pytest.mark.parametrize("mode", list(MODES))
def test_fit_stats_grad_parity(api, dtype, sizes, mode):
    # 63 trees of <= 15 nodes, every number of constants 0 ... 8; 3 features: G = 3 (variable), 0 ... 8 (constant), 3 ... 11 (both: some wide)
    trees = population_trees(11, range(9), dtype)
    pop = api.Population(trees, OPS, dtype, n_features=3)
    ng = pop._n_grad_all(api._grad_mode(MODES[mode]))
    worst, share_max = dict(ZERO), 0.0
    for N in sizes:
        for weighted in (False, True):
            X, y, w = data(N, 3, dtype, 100 + N, weighted)
            fg = pop.eval_fit_stats_grad(X, y, weights=w, variable=MODES[mode])
            kernel = pop.ctx.last_kernel_name()
            gn = pop.eval_gauss_newton(X, y, weights=w, variable=MODES[mode])
            out, grads, ok_g = pop.eval_grad(X, variable=MODES[mode])
            assert np.array_equal(np.asarray(fg.has_jtj), np.asarray(fg.ok) & (ng <= 8))
            if N > 1:
                check_ystats(fg.stats, y, w)
            wst, share = check(fg, out, grads, ok_g, y, w, dtype, gn=gn, min_checked=20, label=f"{mode} N={N} w={weighted}")
            worst, share_max = merge(worst, wst), max(share_max, share)
    assert "FIT" in kernel
    print(f"[fit-stats-grad parity] {np.dtype(dtype).name} {mode}: worst error / magnitude: {fmt(worst)} (bounds 1024 / 256 / 1024 / 1024 / 256 u), "
          f"exempt share <= {100 * share_max:.1f} %, kernel {kernel}")
    pop.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_offset_data(api, dtype):
    """yhat = c + s cos(theta x1) with |c| >> s: what a P' that is not centred inside the data misses.  Held to the centred bounds alone."""
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    N_ = de.Node
    trees = [N_(1, N_(val=dtype(c)), N_(2, N_(val=dtype(s)), N_(1, N_(2, N_(val=dtype(1.3)), N_(feature=1))))) for c, s in ((1000.0, 0.1), (-1.0e4, 1.0))]
    pop = api.Population(trees, ops, dtype, n_features=2)
    N = 4099
    X = de.synth.random_X(2, N, seed=7, dtype=dtype)
    y = (1000.0 + 0.5 * np.cos(X[0].astype(np.float64)) + 0.1 * X[1].astype(np.float64)).astype(dtype)
    out, grads, ok_g = pop.eval_grad(X)
    assert ok_g.all() and all(g.shape[0] == 3 for g in grads)
    worst = dict(ZERO)
    g = np.random.Generator(np.random.PCG64(3))
    wt = g.uniform(0.25, 2, N).astype(dtype)
    wt[::7] = 0
    for w in (None, wt):
        fg = pop.eval_fit_stats_grad(X, y, weights=w)
        gn = pop.eval_gauss_newton(X, y, weights=w)
        check_ystats(fg.stats, y, w)
        wst, _ = check(fg, out, grads, ok_g, y, w, dtype, gn=gn, min_checked=2, constant_rule=False, label="offsets")
        worst = merge(worst, wst)
    print(f"[fit-stats-grad offsets] {np.dtype(dtype).name}: worst error / magnitude: {fmt(worst)}")
    pop.close()


def all_bits(api, fg):
    import torch
    torch.cuda.synchronize()
    st = fg.stats
    parts = [st.mean_p.tobytes(), st.m2_p.tobytes(), st.cov.tobytes(), np.array([st.W, st.mean_y, st.m2_y]).tobytes()]
    for grp in (fg.d_sum, fg.d_pred, fg.d_targ):
        parts += [np.ascontiguousarray(api._host(v)).tobytes() for v in grp]
    return parts, [np.ascontiguousarray(api._host(h)).tobytes() for h in fg.jtj]


def test_exact_properties_on_device_tensors(api):
    import torch
    dtype = np.float32
    trees = population_trees(14, range(9), dtype, per_width=5)
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = data(300, 3, dtype, 9)
    w[256:] = 0
    Xd, yd, wd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t(), torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda()
    a = pop.eval_fit_stats_grad(Xd, yd, weights=wd)
    assert all(torch.is_tensor(h) and h.is_cuda for h in a.jtj) and all(torch.is_tensor(v) and v.is_cuda and v.dtype == torch.float64 for v in a.d_pred)
    assert a.has_jtj.dtype == torch.bool and a.has_jtj.sum().item() >= 30
    ba, ja = all_bits(api, a)
    for h in a.jtj:
        assert torch.equal(h, h.t()) or torch.isnan(h).all()  # exactly symmetric
    assert all_bits(api, pop.eval_fit_stats_grad(Xd, yd, weights=wd)) == (ba, ja)  # run to run
    hst = pop.eval_fit_stats_grad(X, y, weights=w)  # host buffers
    assert all_bits(api, hst) == (ba, ja) and np.array_equal(api._host(a.ok), hst.ok)
    # without the matrix: the same statistics and moments
    nj = pop.eval_fit_stats_grad(Xd, yd, weights=wd, want_jtj=False)
    assert all_bits(api, nj)[0] == ba and not nj.has_jtj.any() and all(torch.isnan(h).all() for h in nj.jtj)
    # doubling every weight doubles every sum exactly and leaves the means alone
    dbl = pop.eval_fit_stats_grad(Xd, yd, weights=wd * 2)
    okh = api._host(a.ok)
    s1, s2 = a.stats, dbl.stats
    assert s2.W == 2 * s1.W and s2.m2_y == 2 * s1.m2_y and s2.mean_y == s1.mean_y
    assert np.array_equal(s2.mean_p[okh], s1.mean_p[okh]) and np.array_equal(s2.m2_p[okh], 2 * s1.m2_p[okh]) and np.array_equal(s2.cov[okh], 2 * s1.cov[okh])
    n_dbl = 0
    for t in np.flatnonzero(okh):
        for grp1, grp2 in ((a.d_sum, dbl.d_sum), (a.d_pred, dbl.d_pred), (a.d_targ, dbl.d_targ)):
            assert torch.equal(grp2[t], grp1[t] * 2)
        if api._host(a.has_jtj)[t] and a.jtj[t].numel() and torch.isfinite(a.jtj[t] * 2).all():
            assert torch.equal(dbl.jtj[t], a.jtj[t] * 2)
            n_dbl += 1
    assert n_dbl >= 25
    # zero weights behind sample 256 == the 256 leading samples alone
    lead = pop.eval_fit_stats_grad(Xd[:, :256], yd[:256], weights=wd[:256])
    assert all_bits(api, lead) == (ba, ja)
    pop.close()


def test_two_samples_per_lane(api, monkeypatch):
    monkeypatch.setenv("DE_GRAD_VS2_MIN_N", "0")  # before the population's first gradient call
    dtype = np.float32
    trees = population_trees(12, range(6), dtype, per_width=6)  # windows <= 6: the widths that have two-sample modules
    pop = api.Population(trees, OPS, dtype, n_features=3)
    vs = []
    for t in trees:
        tape, consts = de.flatten(t, OPS, dtype)
        _, meta = api.lower_tape_grad(tape, consts, 3, 1, 1, dtype=dtype)
        vs.append(int(meta[1]))
    assert vs.count(2) >= len(trees) // 2, vs
    worst = dict(ZERO)
    for N in (513, 1000):
        X, y, w = data(N, 3, dtype, 7 + N)
        fg = pop.eval_fit_stats_grad(X, y, weights=w)
        assert pop.ctx.last_kernel_name() == "de_grad_threaded_kernel<FIT>"
        gn = pop.eval_gauss_newton(X, y, weights=w)
        out, grads, ok_g = pop.eval_grad(X)
        wst, _ = check(fg, out, grads, ok_g, y, w, dtype, gn=gn, min_checked=20, label=f"vs2 N={N}")
        worst = merge(worst, wst)
    print(f"[fit-stats-grad two samples per lane] {vs.count(2)} of {len(trees)} trees in two-sample buckets: {fmt(worst)}")
    pop.close()


def test_shared_leaf_rows_give_the_same_bits(api, monkeypatch):
    dtype = np.float32
    trees = population_trees(20, range(9), dtype, nfeatures=20, per_width=4)
    got = {}
    for share in ("0", "1"):
        monkeypatch.setenv("DE_GRAD_SHARE", share)
        pop = api.Population(trees, OPS, dtype, n_features=20)
        for N in (321, 64, 1000):
            X, y, w = data(N, 20, dtype, 30 + N)
            fg = pop.eval_fit_stats_grad(X, y, weights=w)
            got[share, N] = all_bits(api, fg)
            if share == "1" and N == 321:
                out, grads, ok_g = pop.eval_grad(X)
                check(fg, out, grads, ok_g, y, w, dtype, gn=pop.eval_gauss_newton(X, y, weights=w), min_checked=15, label="shared rows")
        pop.close()
    for N in (321, 64, 1000):
        assert got["0", N] == got["1", N], N


def test_float64_on_the_flat_and_on_the_threaded_kernels(api):
    dtype = np.float64
    X, y, w = data(515, 3, dtype, 6)
    worst = {}
    for name, widths, kernel in (("flat", (6, 7, 8, 2), "de_grad_tape_kernel<FIT>"), ("threaded", (0, 1, 2, 3, 4, 5), "de_grad_threaded_kernel<FIT>")):
        trees = population_trees(18, widths, dtype, per_width=4)
        pop = api.Population(trees, OPS, dtype, n_features=3)
        fg = pop.eval_fit_stats_grad(X, y, weights=w)
        assert pop.ctx.last_kernel_name() == kernel
        gn = pop.eval_gauss_newton(X, y, weights=w)
        out, grads, ok_g = pop.eval_grad(X)
        worst[name], _ = check(fg, out, grads, ok_g, y, w, dtype, gn=gn, min_checked=10, label=name)
        pop.close()
    print(f"[fit-stats-grad f64] flat kernel: {fmt(worst['flat'])}; threaded modules: {fmt(worst['threaded'])}")


def test_flat_kernel_float32(api, monkeypatch):
    monkeypatch.setenv("DE_GRAD_THREADED", "0")
    dtype = np.float32
    trees = population_trees(19, range(9), dtype, per_width=3) + [de.Node(1, de.Node(feature=1), de.Node(val=1.0)), chain(9), chain(12)]
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = data(300, 3, dtype, 8)
    fg = pop.eval_fit_stats_grad(X, y, weights=w)
    assert pop.ctx.last_kernel_name() == "de_grad_tape_kernel<FIT>"
    gn = pop.eval_gauss_newton(X, y, weights=w)
    out, grads, ok_g = pop.eval_grad(X)
    worst, _ = check(fg, out, grads, ok_g, y, w, dtype, gn=gn, min_checked=15, label="flat f32")
    print(f"[fit-stats-grad flat f32] {fmt(worst)}")
    pop.close()


def test_parametric_population(api):
    dtype, P, Cn, N = np.float32, 3, 4, 700
    trees = population_trees(21, (0, 1, 2, 3), dtype, nfeatures=2, per_width=6, node_type=de.ParametricNode, nparams=P)
    pop = api.Population(trees, OPS, dtype, n_features=2, n_params=P)
    X, y, w = data(N, 2, dtype, 12)
    g = np.random.Generator(np.random.PCG64(5))
    params = np.asfortranarray(g.uniform(-1.5, 1.5, (P, Cn)).astype(dtype))
    classes = g.integers(1, Cn + 1, N)
    kw = dict(variable="both", params=params, classes=classes)
    fg = pop.eval_fit_stats_grad(X, y, weights=w, **kw)
    gn = pop.eval_gauss_newton(X, y, weights=w, **kw)
    out, grads, ok_g = pop.eval_grad(X, **kw)
    assert all(h.shape[0] >= P + 2 for h in fg.jtj)
    worst, _ = check(fg, out, grads, ok_g, y, w, dtype, gn=gn, min_checked=12, label="parametric")
    print(f"[fit-stats-grad parametric] {fmt(worst)}")
    pop.close()


def test_graphnode_shared_constant(api):
    G = de.GraphNode
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    x1, c, c2 = G(feature=1), G(val=0.75), G(val=-0.4)
    s = G(1, G(2, x1, c))                              # cos(x1 * c), c is ONE node
    dag = G(1, G(1, s, G(2, s, G(2, c, x1))), c2)      # s + s * (c * x1) + c2: c occurs three times
    plain = de.Node(1, de.Node(2, de.Node(feature=1), de.Node(val=0.3)), de.Node(val=1.0))
    for dtype in (np.float32, np.float64):
        pop = api.Population([dag, plain], ops, dtype, n_features=1)
        assert list(pop.n_consts) == [2, 2] and pop.n_grad(0, 1) == 4  # the library's rows: one per occurrence
        X, y, w = data(513, 1, dtype, 14)
        fg = pop.eval_fit_stats_grad(X, y, weights=w)
        out, grads, ok_g = pop.eval_grad(X)  # combined rows: [2, N]
        assert fg.jtj[0].shape == (2, 2) and fg.d_pred[0].shape == (2,) and grads[0].shape[0] == 2 and fg.has_jtj.all()
        # the summed occurrence rows against the reference formed from the COMBINED Jacobian rows (the bounds are linear in the rows)
        check(fg, out, grads, ok_g, y, w, dtype, gn=None, min_checked=2, label="graphnode")
        gn = pop.eval_gauss_newton(X, y, weights=w)
        assert all(np.array_equal(a, b) for a, b in zip(fg.jtj, gn.jtj))
        # the scaled gradient of the combined rows is what central differences of the device's own scaled_sse see
        pr = fg.projected()
        assert pr.jtj[0].shape == (2, 2) and np.isfinite(pr.grad[0]).all()
        pop.close()


def test_wide_trees_get_dmom_and_a_nan_matrix(api):
    dtype = np.float32
    trees = population_trees(16, range(9), dtype, per_width=2) + [chain(9), chain(12)] + population_trees(17, (1, 4, 8), dtype, per_width=2)
    wide = [18, 19]
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = data(600, 3, dtype, 4)
    fg = pop.eval_fit_stats_grad(X, y, weights=w)
    gn = pop.eval_gauss_newton(X, y, weights=w)
    out, grads, ok_g = pop.eval_grad(X)
    for t in wide:
        G = pop.n_grad(t, 1)
        assert G in (9, 12) and fg.ok[t] and not fg.has_jtj[t]
        assert fg.jtj[t].shape == (G, G) and np.isnan(fg.jtj[t]).all()
        assert all(np.isfinite(v[t]).all() and v[t].shape == (G,) for v in (fg.d_sum, fg.d_pred, fg.d_targ)) and np.abs(fg.d_sum[t]).min() > 0
    worst, _ = check(fg, out, grads, ok_g, y, w, dtype, gn=gn, min_checked=20, label="wide")  # (neighbours included: eval_gauss_newton's bits)
    pr = fg.projected()
    assert len(pr.lm_step(1e-3, tree=wide[0])) == 9 and not pr.lm_step(1e-3, tree=wide[0]).any()
    print(f"[fit-stats-grad wide] {fmt(worst)}")
    pop.close()


@pytest.mark.parametrize("full_eval", [False, True], ids=["early-exit", "full-eval"])
def test_incomplete_trees_are_nan_and_their_neighbours_unaffected(api, full_eval):
    dtype = np.float32
    x1, x2 = de.Node(feature=1), de.Node(feature=2)
    good = population_trees(22, (1, 2, 3), dtype, per_width=2)
    div0 = de.Node(1, de.Node(4, de.Node(val=1.5), de.Node(2, x1, x1)), de.Node(val=0.5))       # 1.5 / (x1 - x1) + 0.5
    big = de.Node(3, de.Node(val=2.0), de.Node(2, de.Node(2, de.Node(3, de.Node(val=60.0), x2))))  # 2 * exp(exp(60 * x2))
    trees = good[:3] + [div0] + good[3:] + [big]
    bad = [3, len(trees) - 1]
    ctx = api.EvalContext(full_eval=full_eval)
    pop = api.Population(trees, OPS, dtype, n_features=3, eval_context=ctx)
    alone = api.Population(good, OPS, dtype, n_features=3, eval_context=ctx)
    X, y, w = data(700, 3, dtype, 16)
    fg, ref = pop.eval_fit_stats_grad(X, y, weights=w), alone.eval_fit_stats_grad(X, y, weights=w)
    for t in bad:
        assert not fg.ok[t] and not fg.has_jtj[t]
        assert np.isnan(fg.stats.mean_p[t]) and np.isnan(fg.stats.m2_p[t]) and np.isnan(fg.stats.cov[t])
        assert all(np.isnan(v[t]).all() and v[t].size > 0 for v in (fg.d_sum, fg.d_pred, fg.d_targ, fg.jtj))
        assert not fg.projected().lm_step(0.0, tree=t).any()
    keep = [t for t in range(len(trees)) if t not in bad]
    assert np.array_equal(np.asarray(fg.ok)[keep], ref.ok) and ref.ok.sum() >= 4
    for i, t in enumerate(keep):
        for a, b in ((fg.d_sum, ref.d_sum), (fg.d_pred, ref.d_pred), (fg.d_targ, ref.d_targ), (fg.jtj, ref.jtj)):
            assert a[t].tobytes() == b[i].tobytes()
        assert fg.stats.mean_p[t] == ref.stats.mean_p[i] and fg.stats.m2_p[t] == ref.stats.m2_p[i] and fg.stats.cov[t] == ref.stats.cov[i]
    pop.close()
    alone.close()


def test_no_samples_and_no_weight(api):
    dtype = np.float32
    trees = population_trees(23, (0, 2, 3), dtype, per_width=1) + [de.Node(1, de.Node(feature=1), de.Node(val=float("inf")))]
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, _ = data(70, 3, dtype, 2)
    for fg in (pop.eval_fit_stats_grad(np.zeros((3, 0), dtype=dtype, order="F"), np.zeros(0, dtype=dtype)),
               pop.eval_fit_stats_grad(X, y, weights=np.zeros(70, dtype=dtype))):  # N == 0, and W == 0 with samples
        st = fg.stats
        assert fg.ok.tolist() == [True, True, True, False]
        assert st.W == 0.0 and np.isnan(st.mean_y) and st.m2_y == 0.0
        assert np.isnan(st.mean_p).all() and not st.m2_p[:3].any() and not st.cov[:3].any() and np.isnan(st.m2_p[3]) and np.isnan(st.cov[3])
        assert [h.shape for h in fg.jtj] == [(0, 0), (2, 2), (3, 3), (1, 1)]
        for v in (fg.d_sum, fg.d_pred, fg.d_targ, fg.jtj):
            assert not v[1].any() and not v[2].any() and np.isnan(v[3]).all()
        assert fg.has_jtj.tolist() == [True, True, True, False]
    pop.close()


def test_refusals(api):
    lib = api.library()
    cos1 = de.OperatorEnum(binary_operators=("+",), unary_operators=("cos",))
    tree = de.Node(1, de.Node(1, de.Node(feature=1)), de.Node(val=0.5))
    X = np.asfortranarray(np.linspace(-1, 1, 64)[None, :])
    for dtype in (np.float16, np.complex64):
        pop = api.Population([tree], cos1, dtype, n_features=1)
        with pytest.raises(api.DeviceError, match="DE_ERR_UNSUPPORTED"):
            pop.eval_fit_stats_grad(X.astype(dtype), np.zeros(64, dtype=dtype))
        # ... and the library itself, before it touches an output
        sentinel = np.full(16, 7, dtype=np.float64)
        okb = np.full(1, 9, dtype=np.uint8)
        Xc = np.asfortranarray(X.astype(dtype))
        rc = lib.de_eval_fit_stats_grad(pop.ctx._h, pop._h, Xc.ctypes.data, 64, 1, None, 1, Xc.ctypes.data, None, sentinel[0:].ctypes.data,
                                        sentinel[3:].ctypes.data, sentinel[6:].ctypes.data, None, sentinel[9:].ctypes.data, None, okb.ctypes.data)
        assert rc == 7 and (sentinel == 7).all() and okb[0] == 9
        pop.close()
    dtype = np.float32
    trees = [tree, de.Node(1, de.Node(feature=1), de.Node(val=2.0))]
    pop = api.Population(trees, cos1, dtype, n_features=1)
    Xf, y = np.asfortranarray(X.astype(dtype)), np.linspace(0, 1, 64).astype(dtype)
    st, ys, dm = np.full(6, 7.0), np.full(3, 7.0), np.full(6, 7.0)
    jt = np.full(2, 7, dtype=dtype)
    okb = np.full(2, 9, dtype=np.uint8)
    neg = np.array([0, -1], dtype=np.int64)

    def call(mode=1, yp=y.ctypes.data, stp=st.ctypes.data, ysp=ys.ctypes.data, dmp=dm.ctypes.data, moff=None, jtj=jt.ctypes.data, joff=None,
             okp=okb.ctypes.data):
        return lib.de_eval_fit_stats_grad(pop.ctx._h, pop._h, Xf.ctypes.data, 64, 1, None, mode, yp, None, stp, ysp, dmp, moff, jtj, joff, okp)

    for rc in (call(mode=3), call(mode=-1), call(yp=None), call(stp=None), call(ysp=None), call(dmp=None), call(okp=None),
               call(moff=neg.ctypes.data), call(joff=neg.ctypes.data)):
        assert rc == 1  # DE_ERR_INVALID_ARG
        assert (st == 7).all() and (ys == 7).all() and (dm == 7).all() and (jt == 7).all() and (okb == 9).all()
    assert call() == 0 and okb.tolist() == [1, 1] and jt.tolist() == [64.0, 64.0]  # d/dc (f(x) + c) = 1, 64 samples
    assert dm[0] == 64.0 and dm[3] == 64.0 and ys[0] == 64.0  # D = sum w
    assert abs(dm[1]) <= 64 * 64 * 2.0 ** -24 and abs(dm[4]) <= 64 * 64 * 2.0 ** -24  # P = sum (yhat - mean_p) = 0 up to rounding
    jt[:] = 7
    assert call(jtj=None) == 0 and (jt == 7).all()  # no matrix wanted
    with pytest.raises(ValueError):
        pop.eval_fit_stats_grad(Xf, y[:-1])
    pop.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_consistency_with_the_siblings(api, dtype):
    """sse_grad() against eval_loss_grad(loss="L2"), within the sum of the bounds of the two; stats against eval_fit_stats, within twice
    the bounds of DESIGN.md §4.4.2."""
    u = unit(dtype)
    trees = population_trees(24, range(9), dtype, per_width=4)
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = data(777, 3, dtype, 3)
    fg = pop.eval_fit_stats_grad(X, y, weights=w)
    fs, ok_s = pop.eval_fit_stats(X, y, weights=w)
    lo, dl, ok_l = pop.eval_loss_grad(X, y, weights=w, loss="L2")
    out, grads, ok_g = pop.eval_grad(X)
    assert np.array_equal(fg.ok, ok_l)
    sg = fg.sse_grad()
    fmax = float(np.finfo(dtype).max)
    worst_g, worst_s, n = 0.0, 0.0, 0
    for t in np.flatnonzero(np.asarray(fg.ok) & np.asarray(ok_s)):
        r = reference(out[t], grads[t], y, w)
        mags = [r["sq"], r["ysq"]] + [np.max(r[k], initial=0.0) for k in ("AD", "AP", "AQ", "E")]
        if not np.isfinite(np.asarray(grads[t])).all() or not np.isfinite(mags).all() or max(mags) > 0.25 * fmax:
            continue
        t_mean, t_m2, t_c = stat_tolerances(r, dtype)
        # sse_grad = 2 P - 2 Q + 2 (mean_p - mean_y) D: the bounds of its parts (mean_y: ystats' 16 * 2^-53) ...
        mine = 2 * KP * u * r["AP"] + 2 * KP * u * r["AQ"] + 2 * abs(r["mean_p"] - r["mean_y"]) * KD * u * r["AD"] \
            + 2 * (t_mean + 16 * U64 * abs(r["mean_y"])) * np.abs(r["D"])
        theirs = KD * u * r["E"]  # ... and of the fused L2 gradient, sum 2 w e d_k
        worst_g = max(worst_g, ratio(np.abs(sg[t] - np.asarray(dl[t], dtype=np.float64)), mine + theirs))
        worst_s = max(worst_s, ratio(abs(fg.stats.mean_p[t] - fs.mean_p[t]), 2 * t_mean), ratio(abs(fg.stats.m2_p[t] - fs.m2_p[t]), 2 * t_m2),
                      ratio(abs(fg.stats.cov[t] - fs.cov[t]), 2 * t_c))
        n += 1
    assert abs(fg.stats.W - fs.W) <= 32 * U64 * fs.W and abs(fg.stats.mean_y - fs.mean_y) <= 32 * U64 * abs(fs.mean_y) and abs(fg.stats.m2_y - fs.m2_y) <= 32 * U64 * fs.m2_y
    print(f"[fit-stats-grad consistency] {np.dtype(dtype).name}: sse_grad vs eval_loss_grad {worst_g:.3g} of the bound, stats vs eval_fit_stats "
          f"{worst_s:.3g} of twice the bound, {n} trees")
    assert n >= 20 and worst_g <= 1.0 and worst_s <= 1.0
    pop.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_scaled_fit_recovers_the_constants(api, dtype):
    """cos(c1 x1) + c2 x2 has no constant that absorbs scale or offset; y = 2 - 3 tree(x; 1.3, 0.7).  28 copies started at theta* (1 +- 0.3),
    10 iterations of fit_constants_lm(scaled=True): every copy ends at scaled_sse <= max(1e-9 initial, 4 * 1024 u M2_y) — the existing
    loop's figure, and four times the resolution the statistics' bounds give scaled_sse = m2_y - cov^2 / m2_p.
    slope and intercept at the result are -3 and 2 to within sqrt(final / M2_y) relative, final taken no smaller than that resolution
    (1024 u M2_y): below it the computed scaled_sse — which may be exactly 0 — carries no information about the true residual."""
    u = unit(dtype)
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

    def make(c):  # cos(c1 * x1) + c2 * x2: constants in depth-first order c1, c2
        return de.Node(1, de.Node(1, de.Node(3, de.Node(val=c[0]), de.Node(feature=1))), de.Node(3, de.Node(val=c[1]), de.Node(feature=2)))

    trees = [make(c) for c in starts]
    pop = api.Population(trees, OPS, dtype, n_features=2)
    consts0 = np.concatenate([de.get_scalar_constants(t)[0] for t in trees]).astype(dtype)
    assert np.allclose(consts0.reshape(28, 2), starts, rtol=1e-6)
    with pytest.raises(ValueError):
        pop.fit_constants_lm(X, y, consts0, weights=w, scaled=True, loss="huber", loss_param=1.0)
    assert np.array_equal(pop.constants(), consts0)  # refused before the constants were touched
    # the projected system at the start: lm_step_device (de_gn_lm_step, a Cholesky solve in double) gives lm_step's step
    pr = pop.eval_fit_stats_grad(X, y, weights=w).projected()
    host_step, dev_step = np.concatenate(pr.lm_step(1e-3)), np.asarray(pr.lm_step_device(1e-3))
    assert dev_step.shape == host_step.shape == (56,) and np.abs(host_step).min() > 0
    assert np.allclose(dev_step, host_step, rtol=1e-9, atol=0)  # 2 x 2 systems of condition < 10^3, both solved in float64
    hist = []
    consts, loss, ok = pop.fit_constants_lm(X, y, consts0, weights=w, iters=10, history=hist, scaled=True)
    assert ok.all() and len(hist) == 11
    for a, b in zip(hist, hist[1:]):
        assert (b <= a).all()  # the accepted losses never increase
    fs, _ = pop.eval_fit_stats(X, y, weights=w)
    m2y = fs.m2_y
    assert (hist[0] >= 5e-3 * m2y).all()
    bound = np.maximum(1e-9 * hist[0], 4 * 1024 * u * m2y)
    print(f"[fit-stats-grad scaled fit] {np.dtype(dtype).name}: worst final / bound = {(loss / bound).max():.3g}, final / initial = "
          f"{(loss / hist[0]).max():.3g}, slope {fs.slope[0]:.9g}, intercept {fs.intercept[0]:.9g}, constants of tree 0 {consts[:2]}")
    assert (loss <= bound).all(), loss / bound
    tol = np.sqrt(np.maximum(loss, 1024 * u * m2y) / m2y)
    assert (np.abs(fs.slope + 3.0) <= 3.0 * tol).all() and (np.abs(fs.intercept - 2.0) <= 2.0 * tol).all(), (fs.slope, fs.intercept, tol)
    # scaled=False is the loop it was
    pop.set_constants(consts0)
    c_plain, l_plain, _ = pop.fit_constants_lm(X, y, consts0, weights=w, iters=2)
    gn = pop.eval_gauss_newton(X, y, weights=w)
    assert np.array_equal(np.asarray(gn.loss).astype(np.float64), l_plain)
    pop.close()
