"""GPU tests of the fused fit statistics (include/de_hip.h de_eval_fit_stats): per tree the weighted mean of its
values, M2_p = sum w (yhat - mean_p)^2 and C = sum w (yhat - mean_p)(y - mean_y); for the target W, mean_y and M2_y.

The reference is numpy (closed forms, accumulated in long double, rounded to float64) over the DEVICE's own `Population.eval` rows: the fused launch runs the same operator handlers, so those
rows are the values the statistics were formed from.  Bounds for complete trees, u = 2^-24 (Float32) / 2^-53 (Float64):
  |dM2_p|    <= 1024 u M2_p                      or (1024 u)^2 sum w yhat^2                          (a constant tree: M2_p ~ 0)
  |dC|       <= 1024 u sqrt(M2_p M2_y)           or (1024 u)^2 sqrt(sum w yhat^2  sum w y^2)
  |dmean_p|  <= 1024 u sum w |yhat| / W
  ystats     16 * 2^-53 relative (mean_y: relative to sum w |y| / W) against a long-double sum: they are formed in double
1024 = at most 4 roundings per term, a sum of at most 256 terms in the element type, three times over for the cross terms of the
recombination: a worst-case bound, not a fitted one.  The sums of squares are formed in the element type: where sum w yhat^2 is
beyond a quarter of its largest finite value a statistic may also be Inf / NaN."""
import ctypes as C

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de

pytestmark = pytest.mark.gpu
K = 1024.0
U64 = 2.0 ** -53


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _api.library()
    return _api


def unit(dtype):
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def ref_ystats(y, w):
    """(W, mean_y, M2_y, sum w |y| / W) in long double over the values the device received."""
    yl = y.astype(np.longdouble)
    wl = np.ones_like(yl) if w is None else w.astype(np.longdouble)
    W = wl.sum()
    my = (wl * yl).sum() / W
    return float(W), float(my), float((wl * (yl - my) ** 2).sum()), float((wl * np.abs(yl)).sum() / W)


def check_ystats(fs, y, w):
    W, my, m2y, amag = ref_ystats(y, w)
    assert abs(fs.W - W) <= 16 * U64 * W
    assert abs(fs.mean_y - my) <= 16 * U64 * amag
    assert abs(fs.m2_y - m2y) <= 16 * U64 * m2y
    return max(abs(fs.W - W) / (U64 * W), abs(fs.mean_y - my) / (U64 * amag), abs(fs.m2_y - m2y) / (U64 * m2y) if m2y else 0.0)


def ref_stats(out, y, w):
    """The closed forms over rows `out` [n, N] — mean_p, M2_p, C — and the magnitudes of the bounds, as float64.  Accumulated in long
    double: a float64 numpy sum along the rows of a heavy-tailed tree was seen 190 u off, which is the size of what is measured for a
    Float64 program (the device was 0.7 u from the long-double value)."""
    L = np.longdouble
    o = np.asarray(out).astype(L)
    yl = y.astype(L)
    ww = np.ones_like(yl) if w is None else w.astype(L)
    keep = ww != 0
    o, yl, ww = o[:, keep], yl[keep], ww[keep]
    with np.errstate(all="ignore"):
        W = ww.sum()
        my = (ww * yl).sum() / W
        mp = np.array([(row * ww).sum() for row in o]) / W
        d = o - mp[:, None]
        f = lambda a: np.array([row.sum() for row in a]).astype(np.float64)  # (row by row: numpy's pairwise sum of a contiguous vector)
        return dict(mean_p=mp.astype(np.float64), m2_p=f(ww * d * d), cov=f(ww * d * (yl - my)), m2_y=float((ww * (yl - my) ** 2).sum()),
                    W=float(W), mean_y=float(my), abs1=f(ww * np.abs(o)) / float(W), sq=f(ww * o * o), ysq=float((ww * yl * yl).sum()))


def tolerances(r, dtype, constant_rule=True):
    """The three bounds of the module docstring, per tree; constant_rule=False: the centred bounds alone."""
    u = unit(dtype)
    with np.errstate(all="ignore"):
        t_m2, t_c = K * u * r["m2_p"], K * u * np.sqrt(r["m2_p"] * r["m2_y"])
        if constant_rule:
            t_m2 = np.maximum(t_m2, (K * u) ** 2 * r["sq"])
            t_c = np.maximum(t_c, (K * u) ** 2 * np.sqrt(r["sq"] * r["ysq"]))
        t_mean = K * u * r["abs1"]
    return t_mean, t_m2, t_c


def check_stats(fs, ok, out, ok_eval, y, w, dtype, min_ok, constant_rule=True):
    """ok == eval's flags, NaN x 3 for incomplete trees, the bounds for the rest; returns the worst error / (u * magnitude)."""
    ok, ok_eval = np.asarray(ok, dtype=bool), np.asarray(ok_eval, dtype=bool)
    assert np.array_equal(ok, ok_eval), "fit statistics and plain eval disagree on the completion flags"
    bad = ~ok
    assert np.isnan(fs.mean_p[bad]).all() and np.isnan(fs.m2_p[bad]).all() and np.isnan(fs.cov[bad]).all()
    r = ref_stats(out, y, w)
    t_mean, t_m2, t_c = tolerances(r, dtype, constant_rule)
    fmax = float(np.finfo(dtype).max)
    n_ok, worst = 0, 0.0
    for t in np.nonzero(ok)[0]:
        if not np.isfinite(r["sq"][t]) or not np.isfinite(r["m2_p"][t]):  # complete does not promise finite values (untested leaves)
            continue
        if r["sq"][t] > 0.25 * fmax:  # the squares overflow the element type
            for got, want, tol in ((fs.m2_p[t], r["m2_p"][t], t_m2[t]), (fs.cov[t], r["cov"][t], t_c[t])):
                assert not np.isfinite(got) or abs(got - want) <= tol
            continue
        n_ok += 1
        errs = (abs(fs.mean_p[t] - r["mean_p"][t]) / t_mean[t] if t_mean[t] else float(fs.mean_p[t] != r["mean_p"][t]),
                abs(fs.m2_p[t] - r["m2_p"][t]) / t_m2[t] if t_m2[t] else float(fs.m2_p[t] != 0),
                abs(fs.cov[t] - r["cov"][t]) / t_c[t] if t_c[t] else float(fs.cov[t] != 0))
        assert fs.m2_p[t] >= 0
        assert max(errs) <= 1.0, (int(t), errs, fs.mean_p[t], r["mean_p"][t], fs.m2_p[t], r["m2_p"][t], fs.cov[t], r["cov"][t])
        worst = max(worst, max(errs))
    assert n_ok >= min_ok, n_ok
    return worst * K  # in units of u x the magnitude


def weights_for(N, dtype, seed):
    """Non-unit weights with zeros mid-tile and in the ragged tail."""
    g = np.random.Generator(np.random.PCG64(seed))
    w = g.uniform(0.25, 2, N).astype(dtype)
    w[::7] = 0
    w[-(N // 3 + 1):: 2] = 0
    if N == 1:
        w[:] = 1.5
    return w


@pytest.mark.parametrize("dtype,n_trees,sizes", [(np.float32, 150, (1, 255, 256, 257, 1000, 4099)), (np.float64, 80, (1, 127, 128, 129, 2051))],
                         ids=["f32", "f64"])
def test_fit_stats_parity(api, dtype, n_trees, sizes):
    trees = de.synth.random_population(n_trees, seed=0xDE02, dtype=dtype)
    pop = api.Population(trees, de.synth.BENCH_OPERATORS, dtype, n_features=5)
    worst, worst_y = 0.0, 0.0
    for N in sizes:
        X = de.synth.random_X(5, N, seed=1, dtype=dtype)
        out, ok_eval = pop.eval(X)
        g = np.random.Generator(np.random.PCG64(N))
        y = (g.standard_normal(N) + 0.5).astype(dtype)
        for w in (None, weights_for(N, dtype, N + 1)):
            fs, ok = pop.eval_fit_stats(X, y, weights=w)
            if N > 1:
                worst_y = max(worst_y, check_ystats(fs, y, w))
            else:
                assert fs.W == (1.0 if w is None else float(w[0])) and fs.mean_y == float(y[0]) and fs.m2_y == 0.0
            worst = max(worst, check_stats(fs, ok, out, ok_eval, y, w, dtype, min_ok=10 if N > 1 else 5))
    print(f"[fit stats parity {np.dtype(dtype).name}] worst error {worst:.2f} u x magnitude (bound {K:.0f}); ystats {worst_y:.2f} u64 (bound 16)")
    pop.close()


def offset_trees(dtype):
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    N_ = de.Node
    trees = [N_(1, N_(val=dtype(c)), N_(2, N_(val=dtype(s)), N_(1, N_(feature=1)))) for c, s in ((1000.0, 0.1), (-1.0e4, 1.0))]
    return trees, ops


@pytest.mark.parametrize("N", [4099, 131072])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_fit_stats_offset_data(api, dtype, N):
    """c + s cos(x1) with |c| >> s against y = 10^3 + ...: what uncentred sums in the element type miss by 10^5 x the bound.  Held to the
    centred bounds alone: the (1024 u)^2 sum w yhat^2 allowance of a constant tree would be the larger one here and hide exactly that."""
    trees, ops = offset_trees(dtype)
    pop = api.Population(trees, ops, dtype, n_features=2)
    X = de.synth.random_X(2, N, seed=7, dtype=dtype)
    y = (1000.0 + 0.5 * np.cos(X[0].astype(np.float64)) + 0.1 * X[1].astype(np.float64)).astype(dtype)
    out, ok_eval = pop.eval(X)
    assert ok_eval.all()
    worst = 0.0
    for w in (None, weights_for(N, dtype, 3)):
        fs, ok = pop.eval_fit_stats(X, y, weights=w)
        check_ystats(fs, y, w)
        worst = max(worst, check_stats(fs, ok, out, ok_eval, y, w, dtype, min_ok=2, constant_rule=False))
    print(f"[fit stats offsets {np.dtype(dtype).name} N={N}] worst error {worst:.2f} u x magnitude (bound {K:.0f})")
    pop.close()


def stats_bits(fs, ok):
    return (fs.mean_p.tobytes(), fs.m2_p.tobytes(), fs.cov.tobytes(), np.float64([fs.W, fs.mean_y, fs.m2_y]).tobytes(), np.asarray(ok.cpu() if hasattr(ok, "cpu") else ok).tobytes())


def test_fit_stats_exact_properties_on_device_tensors(api):
    import torch
    trees = de.synth.random_population(120, seed=0xDE02)
    pop = api.Population(trees, de.synth.BENCH_OPERATORS, np.float32, n_features=5)
    N = 100_003
    gen = torch.Generator(device="cuda").manual_seed(11)
    Xd = torch.randn((N, 5), generator=gen, device="cuda").t()
    yd = torch.randn(N, generator=gen, device="cuda") + 3.0
    wd = torch.rand(N, generator=gen, device="cuda") + 0.5
    wd[::5] = 0
    a, ok_a = pop.eval_fit_stats(Xd, yd, weights=wd)
    b, ok_b = pop.eval_fit_stats(Xd, yd, weights=wd)
    assert stats_bits(a, ok_a) == stats_bits(b, ok_b), "two runs differ"
    live = ok_a.cpu().numpy()
    assert 20 <= live.sum() < len(trees)
    # doubling every weight doubles W, M2_p, C, M2_y and leaves the means unchanged, bit for bit (a power of two commutes with every
    # rounding on the way; overflowing squares excepted)
    c, ok_c = pop.eval_fit_stats(Xd, yd, weights=wd * 2)
    assert torch.equal(ok_a, ok_c)
    fin = live & np.isfinite(a.m2_p) & np.isfinite(c.m2_p) & np.isfinite(a.cov) & np.isfinite(c.cov)
    assert fin.sum() >= 20
    assert c.W == 2 * a.W and c.m2_y == 2 * a.m2_y and c.mean_y == a.mean_y
    assert (c.mean_p[fin]).tobytes() == (a.mean_p[fin]).tobytes()
    assert (c.m2_p[fin]).tobytes() == (2 * a.m2_p[fin]).tobytes()
    assert (c.cov[fin]).tobytes() == (2 * a.cov[fin]).tobytes()
    # host buffers: the same bits
    Xh = np.asfortranarray(Xd.cpu().numpy())
    h, ok_h = pop.eval_fit_stats(Xh, yd.cpu().numpy(), weights=wd.cpu().numpy())
    assert stats_bits(h, ok_h) == stats_bits(a, ok_a), "host buffers and device tensors differ"
    # ... and without weights
    a0, k0 = pop.eval_fit_stats(Xd, yd)
    h0, kh0 = pop.eval_fit_stats(Xh, yd.cpu().numpy())
    assert stats_bits(a0, k0) == stats_bits(h0, kh0)
    pop.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_fit_stats_sse_matches_the_fused_l2_loss(api, dtype):
    """FitStats.sse = m2_y - 2 cov + m2_p + W (mean_p - mean_y)^2 against eval_loss "L2": within the sum of the components' bounds plus the
    loss's own (64 eps sum w e^2 x 3, tests/test_gpu_loss_kinds.py)."""
    trees = de.synth.random_population(100, seed=0xDE02, dtype=dtype)
    pop = api.Population(trees, de.synth.BENCH_OPERATORS, dtype, n_features=5)
    N = 3001
    X = de.synth.random_X(5, N, seed=2, dtype=dtype)
    g = np.random.Generator(np.random.PCG64(9))
    y = g.standard_normal(N).astype(dtype)
    out, ok_eval = pop.eval(X)
    n = 0
    for w in (None, weights_for(N, dtype, 4)):
        fs, ok = pop.eval_fit_stats(X, y, weights=w)
        loss, ok_l = pop.eval_loss(X, y, weights=w, loss="L2")
        assert np.array_equal(ok, ok_l)
        r = ref_stats(out, y, w)
        t_mean, t_m2, t_c = tolerances(r, dtype)
        sse = fs.sse
        for t in np.nonzero(ok)[0]:
            if not np.isfinite(r["sq"][t]) or r["sq"][t] > 0.25 * float(np.finfo(dtype).max) or not np.isfinite(loss[t]):
                continue
            want = r["m2_y"] - 2 * r["cov"][t] + r["m2_p"][t] + r["W"] * (r["mean_p"][t] - r["mean_y"]) ** 2
            tol = (16 * U64 * r["m2_y"] + 2 * t_c[t] + t_m2[t] + r["W"] * (2 * abs(r["mean_p"][t] - r["mean_y"]) * t_mean[t] + t_mean[t] ** 2)
                   + 64 * float(np.finfo(dtype).eps) * 3 * want)
            assert abs(sse[t] - float(loss[t])) <= tol, (int(t), sse[t], loss[t], want, tol)
            n += 1
    assert n >= 30
    pop.close()


@pytest.mark.parametrize("b,a", [(-3.0, 2.0), (-1.0 / 3.0, 2.0 / 3.0)], ids=["y=2-3p", "y=2/3-p/3"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_fit_stats_recover_a_linear_target(api, dtype, b, a):
    """One tree, y = a + b yhat formed from its own rows (rounded once to the element type: dy_j <= u |y_j|): slope, intercept and r come
    back as b, a and -1, scaled_sse as 0, within the bounds of the moments they are functions of."""
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos", "exp"))
    N_ = de.Node
    tree = N_(1, N_(1, N_(2, N_(val=dtype(0.75)), N_(feature=1))), N_(2, N_(feature=2), N_(val=dtype(0.3))))  # cos(0.75 x1) + 0.3 x2
    pop = api.Population([tree], ops, dtype, n_features=2)
    N = 2500
    X = de.synth.random_X(2, N, seed=5, dtype=dtype)
    out, ok_eval = pop.eval(X)
    assert ok_eval[0]
    y = (a + b * out[0].astype(np.float64)).astype(dtype)
    fs, ok = pop.eval_fit_stats(X, y)
    assert ok[0]
    r = ref_stats(out, y, None)
    t_mean, t_m2, t_c = (float(v[0]) for v in tolerances(r, dtype))
    m2p, m2y, u = float(r["m2_p"][0]), float(r["m2_y"]), unit(dtype)
    ry = u * np.sqrt(float(r["ysq"]))  # the 2-norm of the target's own rounding
    t_m2y = 16 * U64 * m2y
    t_slope = t_c / m2p + abs(b) * t_m2 / m2p + ry / np.sqrt(m2p)
    assert abs(fs.slope[0] - b) <= t_slope, (fs.slope[0], b, t_slope)
    t_icpt = 16 * U64 * abs(r["mean_y"]) + t_slope * abs(float(r["mean_p"][0])) + abs(b) * t_mean + u * abs(r["mean_y"])
    assert abs(fs.intercept[0] - a) <= t_icpt, (fs.intercept[0], a, t_icpt)
    t_r = t_c / np.sqrt(m2p * m2y) + 0.5 * (t_m2 / m2p + t_m2y / m2y) + ry / np.sqrt(m2y)
    assert abs(fs.pearson_r[0] + 1.0) <= t_r, (fs.pearson_r[0], t_r)
    t_sse = t_m2y + 2 * abs(b) * t_c + b * b * t_m2 + ry * ry + 2 * ry * np.sqrt(m2y) * 0  # (first order in the moments' errors; dy enters squared)
    assert abs(fs.scaled_sse[0]) <= t_sse, (fs.scaled_sse[0], t_sse)
    pop.close()


def test_fit_stats_large_launch_compacts_and_matches_the_walking_launch(api, monkeypatch):
    """96 trees x 131072 samples (512 tiles): the probe launch of the priority tiles and the compaction of the live trees — the compacted
    stream names the out-of-line end directly — give the bits of the launch that walks past flagged trees (DE_COMPACT=0)."""
    import torch
    trees = de.synth.random_population(96, seed=0xDE02)
    pop = api.Population(trees, de.synth.BENCH_OPERATORS, np.float32, n_features=5)
    N = 131072
    gen = torch.Generator(device="cuda").manual_seed(4)
    Xd = torch.randn((N, 5), generator=gen, device="cuda").t()
    yd = torch.randn(N, generator=gen, device="cuda")
    out, ok_e = pop.eval(Xd)
    monkeypatch.delenv("DE_COMPACT", raising=False)
    fs, ok = pop.eval_fit_stats(Xd, yd)
    live = pop.last_live_trees()
    assert torch.equal(ok, ok_e)
    n_ok = int(ok.sum())
    assert 0 < n_ok < len(trees), "the population needs complete and incomplete trees"
    assert n_ok <= live < len(trees), (live, n_ok, "the fit-statistics launch did not compact its live trees")
    monkeypatch.setenv("DE_COMPACT", "0")
    fw, ok_w = pop.eval_fit_stats(Xd, yd)
    assert stats_bits(fs, ok) == stats_bits(fw, ok_w)
    worst = check_stats(fs, ok.cpu().numpy(), out.cpu().numpy(), ok_e.cpu().numpy(), yd.cpu().numpy(), None, np.float32, min_ok=10)
    print(f"[fit stats large launch] {live} live trees of {len(trees)}, worst error {worst:.2f} u x magnitude (bound {K:.0f})")
    pop.close()


def test_fit_stats_wave_groups_parametric_and_wide(api):
    """A parametric population (2 parameters, 3 classes, N = 1537: one wave per workgroup, h_param's class row), and the populations that
    run several waves per workgroup: 8 staged parameter rows, and 20 features."""
    ops = de.OperatorEnum(binary_operators=("+", "*", "-"), unary_operators=("cos", "exp"))
    rng = de.synth.Xoshiro256ss(21)
    trees = [de.synth.gen_random_tree_fixed_size(9 + i % 8, ops, 2, rng, np.float32, de.ParametricNode, 2) for i in range(40)]
    N, P, Cn = 1537, 2, 3
    g = np.random.Generator(np.random.PCG64(5))
    X = np.asfortranarray(g.standard_normal((2, N)).astype(np.float32))
    params = np.asfortranarray(g.standard_normal((P, Cn)).astype(np.float32))
    classes = g.integers(1, Cn + 1, N)
    y = g.standard_normal(N).astype(np.float32)
    pop = api.Population(trees, ops, np.float32, n_features=2, n_params=P)
    out, ok_e = pop.eval(X, params=params, classes=classes)
    for w in (None, weights_for(N, np.float32, 8)):
        fs, ok = pop.eval_fit_stats(X, y, weights=w, params=params, classes=classes)
        check_stats(fs, ok, out, ok_e, y, w, np.float32, min_ok=10)
    pop.close()
    # ... and 8 parameters in 11 classes: the staged parameter rows make this one run several waves per workgroup
    P, Cn = 8, 11
    trees = de.synth.random_population(120, seed=0x3A7E, node_type=de.ParametricNode, nparams=P)
    X = np.asfortranarray((g.standard_normal((5, N)) * 1.5).astype(np.float32))
    params = np.asfortranarray((g.standard_normal((P, Cn)) * 2).astype(np.float32))
    classes = g.integers(1, Cn + 1, N).astype(np.int64)
    pop = api.Population(trees, de.synth.BENCH_OPERATORS, np.float32, n_features=5, n_params=P)
    waves_p = pop.meta(0)["waves"]
    assert waves_p > 1, "the 8-parameter population was meant to run in wave groups"
    out, ok_e = pop.eval(X, params=params, classes=classes)
    for w in (None, weights_for(N, np.float32, 8)):
        fs, ok = pop.eval_fit_stats(X, y, weights=w, params=params, classes=classes)
        check_stats(fs, ok, out, ok_e, y, w, np.float32, min_ok=10)
    pop.close()
    F, N = 20, 1537
    trees = de.synth.random_population(120, seed=0x7B0, nfeatures=F)
    X = np.asfortranarray((g.standard_normal((F, N)) * 1.2).astype(np.float32))
    pop = api.Population(trees, de.synth.BENCH_OPERATORS, np.float32, n_features=F)
    waves_w = pop.meta(0)["waves"]
    assert waves_w > 1, "the 20-feature population was meant to run in wave groups"
    out, ok_e = pop.eval(X)
    for w in (None, weights_for(N, np.float32, 9)):
        fs, ok = pop.eval_fit_stats(X, y, weights=w)
        check_stats(fs, ok, out, ok_e, y, w, np.float32, min_ok=10)
    print(f"[fit stats wave groups] parametric: {waves_p} waves, 20 features: {waves_w} waves")
    pop.close()


@pytest.mark.parametrize("kind", ["turbo", "cse"])
def test_fit_stats_turbo_and_cse_populations(api, kind):
    from test_lowering import random_graph
    N = 1500
    g = np.random.Generator(np.random.PCG64(77))
    if kind == "turbo":
        ops, F = de.synth.BENCH_OPERATORS, 5
        trees = de.synth.random_population(100, seed=0xDE02)
        ec = api.EvalContext(turbo=True)
    else:
        ops, F = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp", "safe_log", "square")), 5
        rng = de.synth.Xoshiro256ss(4711)
        trees = [random_graph(rng, ops, 6 + i % 24, F, 1 + i % 4, np.float32) for i in range(100)]
        assert sum(de.flatten_graph(t, ops, np.float32)[2] is not None for t in trees) > 30
        ec = api.EvalContext()
    X = np.asfortranarray(g.standard_normal((F, N)).astype(np.float32))
    y = g.standard_normal(N).astype(np.float32)
    pop = api.Population(trees, ops, np.float32, n_features=F, eval_context=ec)
    out, ok_e = pop.eval(X)
    for w in (None, weights_for(N, np.float32, 10)):
        fs, ok = pop.eval_fit_stats(X, y, weights=w)
        check_stats(fs, ok, out, ok_e, y, w, np.float32, min_ok=10)
    pop.close()


def test_fit_stats_errors(api):
    lib = api.library()
    ops = de.synth.BENCH_OPERATORS
    N = 300
    X = de.synth.random_X(5, N, seed=1)
    y = np.linspace(-1, 1, N).astype(np.float32)

    def call(pop, Xp, n, yp, stats, ystats, okp):
        return lib.de_eval_fit_stats(pop.ctx._h, pop._h, Xp, n, 5, None, yp, None, stats, ystats, okp)

    # Float16 / complex populations: DE_ERR_UNSUPPORTED (7), nothing written
    for dtype in (np.float16, np.complex64, np.complex128):
        small = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
        pop = api.Population([de.Node(1, de.Node(feature=1), de.Node(val=0.5))], small, dtype, n_features=1)
        Xt = np.asfortranarray(X[:1].astype(dtype))
        stats, ystats, ok = np.full(3, -7.0), np.full(3, -7.0), np.full(1, 9, dtype=np.uint8)
        rc = lib.de_eval_fit_stats(pop.ctx._h, pop._h, Xt.ctypes.data, N, 1, None, y.astype(dtype).ctypes.data, None, stats.ctypes.data,
                                   ystats.ctypes.data, ok.ctypes.data)
        assert rc == 7, (dtype, rc)
        assert b"evaluate only" in lib.de_last_error(pop.ctx._h)
        assert (stats == -7.0).all() and (ystats == -7.0).all() and (ok == 9).all()
        with pytest.raises(api.DeviceError):
            pop.eval_fit_stats(Xt, y.astype(dtype))
        pop.close()
    trees = de.synth.random_population(6, seed=1)
    pop = api.Population(trees, ops, np.float32, n_features=5)
    stats, ystats, ok = np.full(18, -7.0), np.full(3, -7.0), np.full(6, 9, dtype=np.uint8)
    # a null pointer: DE_ERR_INVALID_ARG (1), nothing written
    for args in ((X.ctypes.data, N, None, stats.ctypes.data, ystats.ctypes.data, ok.ctypes.data),
                 (X.ctypes.data, N, y.ctypes.data, None, ystats.ctypes.data, ok.ctypes.data),
                 (X.ctypes.data, N, y.ctypes.data, stats.ctypes.data, None, ok.ctypes.data),
                 (X.ctypes.data, N, y.ctypes.data, stats.ctypes.data, ystats.ctypes.data, None),
                 (None, N, y.ctypes.data, stats.ctypes.data, ystats.ctypes.data, ok.ctypes.data)):
        assert call(pop, *args) == 1
        assert (stats == -7.0).all() and (ystats == -7.0).all() and (ok == 9).all()
    # N = 0 follows the W == 0 rule: the means are NaN, M2 and C are 0
    assert call(pop, None, 0, None, stats.ctypes.data, ystats.ctypes.data, ok.ctypes.data) == 0
    assert ystats[0] == 0 and np.isnan(ystats[1]) and ystats[2] == 0
    s = stats.reshape(6, 3)
    assert (ok == 1).all() and np.isnan(s[:, 0]).all() and (s[:, 1:] == 0).all()
    # ... and so do weights that are all zero
    fs, okz = pop.eval_fit_stats(X, y, weights=np.zeros(N, dtype=np.float32))
    assert fs.W == 0 and np.isnan(fs.mean_y) and fs.m2_y == 0
    assert np.isnan(fs.mean_p[okz]).all() and (fs.m2_p[okz] == 0).all() and (fs.cov[okz] == 0).all() and okz.any()
    with pytest.raises(ValueError):
        pop.eval_fit_stats(X, y[:-1])
    with pytest.raises(ValueError):
        pop.eval_fit_stats(X, y, weights=y[:-1])
    # the internal kind stays out of reach of a de_loss_spec_t
    spec = api.LossSpec(25, 0, 0.0)
    loss = np.zeros(6, dtype=np.float32)
    rc = lib.de_eval_loss_ex(pop.ctx._h, pop._h, X.ctypes.data, N, 5, None, y.ctypes.data, None, C.byref(spec), loss.ctypes.data, ok.ctypes.data)
    assert rc == 1 and b"loss_kind" in lib.de_last_error(pop.ctx._h)
    pop.close()
