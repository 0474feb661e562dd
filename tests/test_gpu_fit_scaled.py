"""GPU tests of the matrix-free fits under linear scaling (include/de_hip.h de_fit_consts_bfgs_scaled / de_fit_consts_nm_scaled, DESIGN.md
§4.4.14): de_fit_consts_bfgs's and de_fit_consts_nm's loops with the objective scaled_sse = M2_y - C^2 / M2_p, in double.

The kernels run csrc/de_bfgs.h / csrc/de_nm.h — the code behind the host hooks the Python loops call — and the adapter kernel runs
csrc/de_fit_scaled.h, whose two formulas `FitStats.scaled_sse` and `FitStatsGrad.scaled_sse_grad` write out in the same association
(tests/test_fit_scaled_host.py).  So `fit_constants_*_device(scaled=True)` and `fit_constants_*(scaled=True)` agree BIT FOR BIT: constants,
scaled_sse, flags, every history row and the accept counts.  That equality needs no tolerance and is the core test.  The fits that have a
criterion of their own — a tree with constants that are redundant under scaling, a constant under `round` — take their data and starts
from a run of the same Python loops over a numpy model of the tree (tests/test_fit_scaled_host.py `Model`): 13.4 -> 5e-12 (BFGS, 12 iterations) and
8.8e-4 (Nelder-Mead, 40 rounds) on the redundant tree at N = 1025; 816 -> 331 for Nelder-Mead on the rounded one, BFGS leaving the
constant under `round` at its bits.  The tests only ask for a strict decrease."""
import ctypes as C

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import test_gpu_gauss_newton as GN
from test_gpu_lm import bad_trees, chain, dev_X, offsets

pytestmark = pytest.mark.gpu
OPS = GN.OPS
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
SIZES = pytest.mark.parametrize("N", [1, 255, 257, 1025])  # around the 256-sample tile of the gradient kernels and the eval tile
BFGS_ITERS, NM_ROUNDS = 12, 40
FITS = {"bfgs": dict(iters=BFGS_ITERS), "nm": dict(iters=NM_ROUNDS)}


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


def same(api, a, b):
    return api._host(a).tobytes() == api._host(b).tobytes()


def same_stats(a, b):
    return all(np.asarray(getattr(a, n), dtype=np.float64).tobytes() == np.asarray(getattr(b, n), dtype=np.float64).tobytes()
               for n in ("mean_p", "m2_p", "cov", "W", "mean_y", "m2_y"))


def non_increasing(hist):
    return all(((b <= a) | (np.isnan(a) & np.isnan(b))).all() for a, b in zip(hist, hist[1:]))


def redundant_tree(c=(0.5, 1.0, 1.0)):  # c0 + c1 * cos(c2 * x1): c0 and c1 are redundant under scaling
    x1 = de.Node(feature=1)
    return de.Node(1, de.Node(val=c[0]), de.Node(3, de.Node(val=c[1]), de.Node(1, de.Node(3, de.Node(val=c[2]), x1))))


def n_constants(tree):
    return sum(1 for n in de.postorder(tree) if n.degree == 0 and n.constant)


def mixed_population(dtype):
    """24 random trees over + - * / cos exp of 0 .. 6 constants — 14 small ones, two of every width (most of them affine in one feature:
    every constant is redundant under scaling, the objective is flat and nothing may move but by rounding), and 10 of 20 nodes with 1 .. 6
    constants — one of 20 constants, one of 33 (above the row limit), one that is incomplete at the start and the redundant tree:
    (trees, {index: why it keeps its constants})."""
    trees = GN.population_trees(71, (0, 1, 2, 3, 4, 5, 6), dtype, per_width=2)
    kept = {t: "no constant" for t in range(len(trees)) if t % 7 == 0}
    drawn = de.synth.random_population(80, seed=7, node_count=20, nfeatures=3, operators=OPS, dtype=dtype)
    trees += [t for t in drawn if 1 <= n_constants(t) <= 6][:10]
    n = len(trees)
    assert n == 24
    trees += [chain(20), chain(33), bad_trees()[0], redundant_tree()]
    kept.update({n + 1: "33 constants", n + 2: "incomplete"})
    return trees, kept


def start_constants(pop, kept):
    """The population's constants with a -0 in the tree above the row limit and a -0 and a NaN with a payload in the incomplete tree."""
    c0 = pop.constants().copy()
    at = offsets(pop.n_consts)
    u = np.uint32 if c0.dtype == np.float32 else np.uint64
    payload = np.array([0x7fc00123 if c0.dtype == np.float32 else 0x7ff8000000000123], dtype=u).view(c0.dtype)[0]
    for t, why in kept.items():
        if why == "33 constants":
            c0[at[t] + 5] = -0.0
        if why == "incomplete":
            c0[at[t]], c0[at[t] + 1] = payload, -0.0
    return c0, at


def run(pop, how, where, X, y, c0, w, history, **kw):
    """(consts, scaled_sse, ok, accept counts, scaled_fit_stats) of one scaled fit: how = bfgs / nm, where = host / device."""
    fit = getattr(pop, "fit_constants_" + how + ("_device" if where == "device" else ""))
    consts, sse, ok = fit(X, y, c0, weights=w, history=history, scaled=True, **dict(FITS[how], **kw))
    counts = pop.bfgs_accepts if how == "bfgs" else pop.nm_improves
    return consts, sse, ok, counts, pop.scaled_fit_stats


def evaluation(api, pop, how, X, y, w):
    """(FitStats, ok) of the fit's own evaluation call at the constants the population holds."""
    if how == "bfgs":
        fg = pop.eval_fit_stats_grad(X, y, weights=w, want_jtj=False)
        return fg.stats, api._host(fg.ok).astype(bool)
    st, ok = pop.eval_fit_stats(X, y, weights=w)
    return st, api._host(ok).astype(bool)


# ---- 1 - 3. the trajectory bit for bit, consistency at the result, untouched trees -------------------------------------------------------------
@DTYPES
@SIZES
@pytest.mark.parametrize("how", list(FITS))
def test_device_fit_follows_the_host_loop_bit_for_bit(api, dtype, N, how):
    trees, kept = mixed_population(dtype)
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = GN.data(N, 3, dtype, 90 + N)
    assert N == 1 or (w == 0).any()
    c0, at = start_constants(pop, kept)
    widths = np.diff(at)
    assert len(trees) == 28 and sorted(set(widths[:14].tolist())) == [0, 1, 2, 3, 4, 5, 6] and widths[14:24].min() >= 1
    assert widths[:24].max() == 6 and widths[24:].tolist() == [20, 33, 2, 3]
    assert all((widths[t] == 0) == (why == "no constant") for t, why in kept.items())
    rows = FITS[how]["iters"] + 1
    hh, hd = [], []
    ch, lh, okh, nh, sth = run(pop, how, "host", X, y, c0, w, hh)
    nh = np.asarray(nh).copy()
    cd, ld, okd, nd, std = run(pop, how, "device", X, y, c0, w, hd)
    nd = np.asarray(nd).copy()
    # 1. bit for bit
    assert cd.dtype == ch.dtype == dtype and ld.dtype == lh.dtype == np.float64 and len(hd) == len(hh) == rows
    assert same(api, cd, ch), np.flatnonzero(cd.view(np.uint8) != ch.view(np.uint8))
    assert same(api, ld, lh), (ld, lh)
    assert np.array_equal(okd, okh)
    assert all(a.dtype == np.float64 and a.tobytes() == b.tobytes() for a, b in zip(hd, hh))
    assert nd.dtype == np.int32 and nd.tobytes() == nh.tobytes()
    assert same_stats(std, sth)
    # 2. consistency at the result: the program holds the constants; the fit's own evaluation there gives the statistics and sse
    assert same(api, pop.constants(), cd)
    st, ok = evaluation(api, pop, how, X, y, w)
    assert same_stats(std, st) and np.array_equal(ok, okd)
    assert api._scaled_sse64(st).tobytes() == ld.tobytes() == hd[-1].tobytes()
    assert non_increasing(hd)
    with np.errstate(invalid="ignore"):
        strict = (np.stack(hd)[1:] < np.stack(hd)[:-1]).sum(axis=0)
    assert np.array_equal(nd, strict)  # (an accepted step / an improving round is a strict decrease, by the accept rules)
    # 3. trees that are not fitted keep their constant bits, -0 and NaN payloads included
    incomplete = [t for t, why in kept.items() if why == "incomplete"]
    assert not okd[incomplete].any()
    for t, why in kept.items():
        assert cd[at[t]:at[t + 1]].tobytes() == c0[at[t]:at[t + 1]].tobytes() and nd[t] == 0, (t, why)
        assert all(h[t:t + 1].tobytes() == hd[0][t:t + 1].tobytes() for h in hd), (t, why)
        assert np.isnan(ld[t]) == (why == "incomplete")
    # the fit did something (one sample leaves no variance to fit)
    assert N == 1 or nd.any()
    print(f"[fit scaled] {how} {np.dtype(dtype).name} N={N}: {len(trees)} trees bit-equal to the host loop over {rows - 1} iterations; "
          f"accepted per tree {nd.tolist()}")
    pop.close()


@DTYPES
@pytest.mark.parametrize("how", list(FITS))
def test_no_iterations_and_no_samples(api, dtype, how):
    trees, kept = mixed_population(dtype)
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = GN.data(257, 3, dtype, 12)
    c0, at = start_constants(pop, kept)
    # iters = 0: the first evaluation's values, the constants untouched
    hist = []
    consts, sse, ok, counts, stats = run(pop, how, "device", X, y, c0, w, hist, iters=0)
    st, ok1 = evaluation(api, pop, how, X, y, w)
    assert len(hist) == 1 and same(api, consts, c0) and same(api, pop.constants(), c0) and not np.asarray(counts).any()
    assert same_stats(stats, st) and np.array_equal(ok, ok1) and sse.tobytes() == api._scaled_sse64(st).tobytes() == hist[0].tobytes()
    # N = 0: W = 0, so sse = M2_y = 0 (NaN where a constant already fails the flag); every history row the same; the constants untouched
    hist = []
    X0, y0 = np.zeros((3, 0), dtype=dtype, order="F"), np.zeros(0, dtype=dtype)
    consts, sse, ok, counts, stats = run(pop, how, "device", X0, y0, c0, None, hist, iters=3)
    st, ok1 = evaluation(api, pop, how, X0, y0, None)
    assert len(hist) == 4 and all(h.tobytes() == sse.tobytes() for h in hist) and not np.asarray(counts).any()
    assert same(api, consts, c0) and same(api, pop.constants(), c0) and np.array_equal(ok, ok1) and same_stats(stats, st)
    assert sse.tobytes() == api._scaled_sse64(st).tobytes() and stats.W == 0.0
    bad = [t for t, why in kept.items() if why == "incomplete"]
    assert np.isnan(sse[bad]).all() and not np.delete(sse, bad).any() and not ok[bad].any() and np.delete(ok, bad).all()
    pop.close()
    # a population without constants: the loop has nothing to move
    bare = api.Population([de.Node(1, de.Node(feature=1), de.Node(2, de.Node(feature=2))), de.Node(3, de.Node(feature=1), de.Node(feature=3))],
                          OPS, dtype, n_features=3)
    hist = []
    consts, sse, ok, counts, stats = run(bare, how, "device", X, y, None, w, hist, iters=3)
    st, _ = evaluation(api, bare, how, X, y, w)
    assert consts.size == 0 and ok.all() and len(hist) == 4 and all(h.tobytes() == sse.tobytes() for h in hist)
    assert same_stats(stats, st) and sse.tobytes() == api._scaled_sse64(st).tobytes() and not np.asarray(counts).any()
    bare.close()


# ---- 4. constants that are redundant under scaling ------------------------------------------------------------------------------------------------
def exact_weights(g, N, dtype):
    """Weights of {0, 1/2, 1, 2}: every partial sum of them is exact in either type, so W, the c0 row's D and its diagonal entry of the
    Gauss-Newton matrix are one number and the projected diagonal is W - W W / W - P^2 / M2_p <= 0: the Cholesky step is zero."""
    return g.choice(np.array([0.0, 0.5, 1.0, 2.0]), N).astype(dtype)


@DTYPES
def test_redundant_constants_are_fitted(api, dtype):
    N = 1025
    g = np.random.Generator(np.random.PCG64(404))
    x = g.uniform(-2.0, 2.0, N)
    w = exact_weights(g, N, dtype)
    X = np.asfortranarray(x[None, :].astype(dtype))
    y = (2.5 * np.cos(1.3 * x) - 0.7).astype(dtype)
    ops = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
    pop = api.Population([redundant_tree()], ops, dtype, n_features=1)
    c0 = pop.constants().copy()
    assert c0.tolist() == [0.5, 1.0, 1.0]
    # the scaled Levenberg-Marquardt fit leaves the tree alone: the documented zero step
    hl = []
    cl, ll, okl = pop.fit_constants_lm_device(X, y, c0, weights=w, iters=BFGS_ITERS, history=hl, scaled=True)
    assert okl[0] and cl.tobytes() == c0.tobytes() and not np.asarray(pop.lm_accepts).any() and all(h[0] == ll[0] for h in hl)
    assert float(ll[0]) > 1.0
    for how in FITS:
        hh, hd = [], []
        ch, lh, okh, nh, _ = run(pop, how, "host", X, y, c0, w, hh)  # the reference here
        cd, ld, okd, nd, std = run(pop, how, "device", X, y, c0, w, hd)
        start = float(hh[0][0])
        assert okh[0] and okd[0] and abs(start - float(ll[0])) <= 1e-3 * start
        assert float(lh[0]) < start, (how, lh, start)
        assert cd.tobytes() == ch.tobytes() and ld.tobytes() == lh.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(hd, hh))
        assert float(ld[0]) < start and np.asarray(nd)[0] > 0 and cd.tobytes() != c0.tobytes()
        a, b = float(std.intercept[0]), float(std.slope[0])  # (they come with the fit)
        assert np.isfinite(a) and np.isfinite(b) and b != 0.0
        print(f"[fit scaled] redundant tree, {how} {np.dtype(dtype).name}: scaled_sse {start:.6g} -> {float(ld[0]):.3g} at {cd.tolist()} "
              f"(slope {b:.6g}, intercept {a:.6g}); the scaled LM fit stays at {float(ll[0]):.6g}")
    pop.close()


# ---- 5. a zero gradient row ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_a_constant_under_round(api, dtype):
    """c0 * round(c1 * x1) + c2 * x1 against y = 2 round(3 x1) + x1 / 2 from (1.5, 2.6, 0.2): the gradient row of c1 is zero, so scaled BFGS
    leaves its bits where they are (and fits the ratio of the other two); scaled Nelder-Mead moves it and lowers scaled_sse."""
    N = 1025
    g = np.random.Generator(np.random.PCG64(404))
    x = g.uniform(-2.0, 2.0, N)
    w = exact_weights(g, N, dtype)
    X = np.asfortranarray(x[None, :].astype(dtype))
    y = (2.0 * np.rint(3.0 * x) + 0.5 * x).astype(dtype)
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("round",))
    x1 = de.Node(feature=1)
    tree = de.Node(1, de.Node(2, de.Node(val=1.5), de.Node(1, de.Node(2, de.Node(val=2.6), x1))), de.Node(2, de.Node(val=0.2), x1))
    pop = api.Population([tree], ops, dtype, n_features=1)
    c0 = pop.constants().copy()
    assert c0.tolist() == [dtype(1.5), dtype(2.6), dtype(0.2)]
    hb, hn = [], []
    cb, lb, okb, nb, _ = run(pop, "bfgs", "device", X, y, c0, w, hb)
    cn, ln, okn, nn, _ = run(pop, "nm", "device", X, y, c0, w, hn)
    assert okb[0] and okn[0]  # (the two fits start from different evaluation calls: hb[0] and hn[0] agree to rounding only)
    assert cb[1:2].tobytes() == c0[1:2].tobytes() and float(lb[0]) <= hb[0][0]
    assert float(ln[0]) < hn[0][0] and np.asarray(nn)[0] > 0
    print(f"[fit scaled] c0 round(c1 x1) + c2 x1, {np.dtype(dtype).name}: scaled_sse {hn[0][0]:.6g}; BFGS {float(lb[0]):.6g} at {cb.tolist()}, "
          f"Nelder-Mead {float(ln[0]):.6g} at {cn.tolist()}")
    pop.close()


# ---- 6. a program made by de_program_create_cse -----------------------------------------------------------------------------------------------------
@DTYPES
def test_cse_program(api, dtype):
    lib = api.library()
    Gn = de.GraphNode
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    x1, x2 = Gn(feature=1), Gn(feature=2)
    sh = Gn(1, Gn(2, x1, x2))  # cos(x1 * x2), used three times; no constant is shared
    dag = Gn(1, Gn(2, sh, Gn(val=0.6)), Gn(2, sh, Gn(2, sh, Gn(val=-0.2))))
    plain = Gn(1, Gn(2, Gn(val=1.25), x1), Gn(1, Gn(2, Gn(val=-0.5), x2)))
    pop = api.Population([dag, plain], ops, dtype, n_features=2)
    assert pop._occ is None and pop.n_consts.tolist() == [2, 2]
    X, y, w = GN.data(1025, 2, dtype, 21)
    c0 = pop.constants().copy()
    hh, hd = [], []
    ch, lh, okh, nh, sth = run(pop, "nm", "host", X, y, c0, w, hh)
    nh = np.asarray(nh).copy()
    cd, ld, okd, nd, std = run(pop, "nm", "device", X, y, c0, w, hd)
    assert cd.tobytes() == ch.tobytes() and ld.tobytes() == lh.tobytes() and okd.all() and okh.all() and same_stats(std, sth)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(hd, hh)) and np.asarray(nd).tobytes() == nh.tobytes()
    assert (hd[-1] < hd[0]).any() and non_increasing(hd) and cd.tobytes() != c0.tobytes()
    st, _ = pop.eval_fit_stats(X, y, weights=w)
    assert same_stats(std, st) and api._scaled_sse64(st).tobytes() == ld.tobytes()
    # de_fit_consts_bfgs_scaled refuses the program: outputs and constants untouched
    pop.set_constants(c0)
    bufs = [np.full(256, 7, dtype=np.uint8) for _ in range(6)]
    ptr = [b.ctypes.data for b in bufs]
    args = (pop.ctx._h, pop._h, X.ctypes.data, X.shape[1], X.shape[0], None, y.ctypes.data, w.ctypes.data)
    opts = api.BfgsOpts(3, 0, 1.0, 0.5, 1e-4, 1e-8)
    assert lib.de_fit_consts_bfgs_scaled(*args, C.byref(opts), *ptr) == 7
    assert "de_program_create_cse" in lib.de_last_error(pop.ctx._h).decode()
    assert all((b == 7).all() for b in bufs) and pop.constants().tobytes() == c0.tobytes()
    held = np.empty(c0.size, dtype=dtype)
    assert lib.de_program_get_consts(pop._h, held.ctypes.data) == 0 and held.tobytes() == c0.tobytes()
    with pytest.raises(api.DeviceError, match="de_program_create_cse"):
        pop.fit_constants_bfgs_device(X, y, c0, weights=w, scaled=True)
    assert pop.constants().tobytes() == c0.tobytes()
    pop.close()


# ---- 7. torch device inputs ---------------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("how", list(FITS))
def test_torch_inputs_give_device_tensors_and_the_same_bits(api, torch, dtype, how):
    trees, kept = mixed_population(dtype)
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = GN.data(1025, 3, dtype, 31)
    c0, at = start_constants(pop, kept)
    hd, ht = [], []
    cd, ld, okd, nd, std = run(pop, how, "device", X, y, c0, w, hd)
    nd = np.asarray(nd).copy()
    ct, lt, okt, nt, stt = run(pop, how, "device", dev_X(torch, X), torch.from_numpy(y).cuda(), torch.from_numpy(c0).cuda(),
                               torch.from_numpy(w).cuda(), ht)
    assert all(torch.is_tensor(v) and v.is_cuda for v in (ct, lt, okt, nt, ht[0])) and lt.dtype == torch.float64
    assert same(api, ct, cd) and same(api, lt, ld) and np.array_equal(api._host(okt), okd) and same(api, nt, nd)
    assert len(ht) == len(hd) and all(same(api, a, b) for a, b in zip(ht, hd)) and same_stats(stt, std)
    pop.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_f16_and_complex_programs_are_refused(api):
    lib = api.library()
    cos1 = de.OperatorEnum(binary_operators=("+",), unary_operators=("cos",))
    tree = de.Node(1, de.Node(1, de.Node(feature=1)), de.Node(val=0.5))
    X = np.asfortranarray(np.linspace(-1, 1, 64)[None, :])
    for dtype in (np.float16, np.complex64):
        pop = api.Population([tree], cos1, dtype, n_features=1)
        before = pop.constants().copy()
        Xc = np.asfortranarray(X.astype(dtype))
        for name, fit in (("de_fit_consts_bfgs_scaled", pop.fit_constants_bfgs_device), ("de_fit_consts_nm_scaled", pop.fit_constants_nm_device)):
            bufs = [np.full(256, 7, dtype=np.uint8) for _ in range(6)]
            rc = getattr(lib, name)(pop.ctx._h, pop._h, Xc.ctypes.data, 64, 1, None, Xc.ctypes.data, None, None, *[b.ctypes.data for b in bufs])
            assert rc == 7 and all((b == 7).all() for b in bufs), (name, np.dtype(dtype).name)
            assert pop.constants().tobytes() == before.tobytes()
            with pytest.raises(api.DeviceError, match="DE_ERR_UNSUPPORTED"):
                fit(Xc, np.zeros(64, dtype=dtype), scaled=True)
        pop.close()
    # bad options and null buffers are refused as the unscaled fits refuse them, with everything untouched
    pop = api.Population([tree], cos1, np.float32, n_features=1)
    Xf, y = np.asfortranarray(X.astype(np.float32)), np.cos(X[0]).astype(np.float32)
    before = pop.constants().copy()
    head = (pop.ctx._h, pop._h, Xf.ctypes.data, 64, 1, None)
    for name, bad in (("de_fit_consts_bfgs_scaled", api.BfgsOpts(-1, 0, 1.0, 0.5, 1e-4, 1e-8)),
                      ("de_fit_consts_bfgs_scaled", api.BfgsOpts(3, 0, 1.0, 1.5, 1e-4, 1e-8)),
                      ("de_fit_consts_nm_scaled", api.NmOpts(3, 1, 0.025, 0.5, 0.0)),
                      ("de_fit_consts_nm_scaled", api.NmOpts(3, 0, 0.0, 0.0, 0.0))):
        bufs = [np.full(256, 7, dtype=np.uint8) for _ in range(6)]
        assert getattr(lib, name)(*head, y.ctypes.data, None, C.byref(bad), *[b.ctypes.data for b in bufs]) == 1
        assert all((b == 7).all() for b in bufs) and pop.constants().tobytes() == before.tobytes()
    for name in ("de_fit_consts_bfgs_scaled", "de_fit_consts_nm_scaled"):
        for missing in (0, 3):  # sse, ok
            bufs = [np.full(256, 7, dtype=np.uint8) for _ in range(6)]
            ptr = [b.ctypes.data for b in bufs]
            ptr[missing] = None
            assert getattr(lib, name)(*head, y.ctypes.data, None, None, *ptr) == 1
            assert all((b == 7).all() for b in bufs) and pop.constants().tobytes() == before.tobytes()
        bufs = [np.full(256, 7, dtype=np.uint8) for _ in range(6)]
        assert getattr(lib, name)(*head, None, None, None, *[b.ctypes.data for b in bufs]) == 1  # y
        assert all((b == 7).all() for b in bufs)
    # stats, ystats, history and the counts may be null
    sse, ok = np.full(1, 7.0), np.full(1, 9, dtype=np.uint8)
    for name, opts in (("de_fit_consts_bfgs_scaled", api.BfgsOpts(4, 0, 1.0, 0.5, 1e-4, 1e-8)), ("de_fit_consts_nm_scaled", api.NmOpts(6, 0, 0.025, 0.5, 0.0))):
        pop.set_constants(before)
        assert getattr(lib, name)(*head, y.ctypes.data, None, C.byref(opts), sse.ctypes.data, None, None, ok.ctypes.data, None, None) == 0
        st, _ = pop.eval_fit_stats(Xf, y)
        assert ok[0] == 1 and np.isfinite(sse[0]) and abs(sse[0] - st.scaled_sse[0]) <= 1e-3 * st.m2_y
    pop.close()
