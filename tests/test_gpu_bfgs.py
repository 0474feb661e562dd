"""GPU tests of BFGS on the constants on the device (include/de_hip.h de_fit_consts_bfgs).

The kernels run csrc/de_bfgs.h, the code behind the host hooks de_bfgs_direction_host / de_bfgs_update_host, and the accept rule of
`Population.fit_constants_bfgs` (the host loop: `eval_loss_grad`, the two hooks, `set_constants`, the rule in Python floats).  So the
one-call fit and the host loop agree BIT FOR BIT: constants, loss, flags, the whole history and the accept counts.  That equality is the
test; the hooks themselves are held to numpy in tests/test_bfgs_host.py, whose scenarios (the reference's test/test_optim.jl fit, a hinge
classifier, chain(12) / chain(32)) run here on the device with the bounds established there on the CPU."""
import ctypes as C

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import test_bfgs_host as H
import test_gpu_gauss_newton as GN
from test_gpu_lm import bad_trees, chain, dev_X, offsets

pytestmark = pytest.mark.gpu
OPS = GN.OPS
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
ITERS = 6


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


def none_tree():
    return de.Node(1, de.Node(feature=1), de.Node(2, de.Node(feature=2)))  # x1 + exp(x2): no constant


def same_bytes(api, a, b):
    return api._host(a).tobytes() == api._host(b).tobytes()


# ---- 1. + 2. the trajectory, bit for bit, and its invariants ---------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("N", [64, 257])
@pytest.mark.parametrize("kind", ["L2 weighted", "huber"])
def test_device_fit_follows_the_host_loop_bit_for_bit(api, torch, dtype, N, kind):
    good = GN.population_trees(41, range(9), dtype) + [chain(9), chain(12), chain(32)]
    div0, big = bad_trees()
    trees = good[:5] + [div0] + good[5:20] + [none_tree(), chain(33)] + good[20:] + [big]
    kept = {5: "incomplete", 21: "no constant", 22: "33 constants", len(trees) - 1: "incomplete"}
    keep = [t for t in range(len(trees)) if t not in kept]
    X, y, w = GN.data(N, 3, dtype, 50 + N)
    kw = dict(weights=w) if kind == "L2 weighted" else dict(loss="huber", loss_param=1.3)
    pop, alone = api.Population(trees, OPS, dtype, n_features=3), api.Population(good, OPS, dtype, n_features=3)
    c0 = pop.constants().copy()
    at = offsets(pop.n_consts)
    assert at[23] - at[22] == 33 and at[22] == at[21] and sorted(set(np.diff(at).tolist())) == list(range(10)) + [12, 32, 33]
    # the host loop
    hh = []
    ch, lh, okh = pop.fit_constants_bfgs(X, y, c0, iters=ITERS, history=hh, **kw)
    acc_h = pop.bfgs_accepts.copy()
    # the one call, numpy inputs
    hd = []
    cd, ld, okd = pop.fit_constants_bfgs_device(X, y, c0, iters=ITERS, history=hd, **kw)
    acc_d = np.asarray(pop.bfgs_accepts).copy()
    assert cd.dtype == dtype and ld.dtype == dtype and lh.dtype == dtype and len(hd) == len(hh) == ITERS + 1
    assert same_bytes(api, cd, ch) and same_bytes(api, ld, lh) and np.array_equal(okd, okh)
    assert all(a.dtype == np.float64 and a.tobytes() == b.tobytes() for a, b in zip(hd, hh))
    assert acc_d.dtype == np.int32 and acc_d.tobytes() == acc_h.tobytes()
    # invariants: the population holds the result, eval_loss_grad reproduces the loss, the accepted losses never increase
    assert pop.constants().tobytes() == cd.tobytes()
    lo, _, ok2 = pop.eval_loss_grad(X, y, **kw)
    assert lo.tobytes() == ld.tobytes() and np.array_equal(ok2, okd)
    for a, b in zip(hd, hd[1:]):
        assert ((b <= a) | (np.isnan(a) & np.isnan(b))).all()
    assert np.array_equal(hd[-1], ld.astype(np.float64), equal_nan=True)
    # the one call, device tensors: the same bytes, tensors out
    ht = []
    ta = dict(weights=torch.from_numpy(w).cuda()) if kind == "L2 weighted" else dict(loss="huber", loss_param=1.3)
    ct, lt, okt = pop.fit_constants_bfgs_device(dev_X(torch, X), torch.from_numpy(y).cuda(), torch.from_numpy(c0).cuda(), iters=ITERS, history=ht, **ta)
    assert all(torch.is_tensor(v) and v.is_cuda for v in (ct, lt, okt, pop.bfgs_accepts, ht[0])) and pop.consts_on_device_path
    assert same_bytes(api, ct, cd) and same_bytes(api, lt, ld) and np.array_equal(api._host(okt), okd)
    assert same_bytes(api, pop.bfgs_accepts, acc_d) and all(same_bytes(api, a, b) for a, b in zip(ht, hd))
    # the fit did something, and the shrink branch ran
    fitted = okd & (np.diff(at) >= 1) & (np.diff(at) <= 32)
    assert (acc_d >= 2).sum() >= 30, acc_d
    assert ((acc_d > 0) & (acc_d < ITERS) & fitted).any()
    assert all(acc_d[t] > 0 for t in keep[-3:])  # chain(9), chain(12), chain(32)
    # trees that are not fitted keep consts0 and accept nothing
    for t, why in kept.items():
        assert cd[at[t]:at[t + 1]].tobytes() == c0[at[t]:at[t + 1]].tobytes() and acc_d[t] == 0, (t, why)
        assert bool(okd[t]) == (why != "incomplete") and np.isnan(ld[t]) == (why == "incomplete")
    # neighbours: the population without them gives the same bytes for the rest
    h2 = []
    ca, la, oka = alone.fit_constants_bfgs_device(X, y, iters=ITERS, history=h2, **kw)
    ata = offsets(alone.n_consts)
    for i, t in enumerate(keep):
        assert cd[at[t]:at[t + 1]].tobytes() == ca[ata[i]:ata[i + 1]].tobytes(), t
        assert ld[t:t + 1].tobytes() == la[i:i + 1].tobytes() and okd[t] == oka[i] and acc_d[t] == alone.bfgs_accepts[i]
        assert all(a[t:t + 1].tobytes() == b[i:i + 1].tobytes() for a, b in zip(hd, h2))
    print(f"[bfgs device] {np.dtype(dtype).name} N={N} {kind}: {len(trees)} trees bit-equal to the host loop over {ITERS} iterations; "
          f"accepted steps {np.bincount(acc_d, minlength=ITERS + 1).tolist()} (trees per count)")
    pop.close()
    alone.close()


# ---- 3. the reference's scenario on the device -------------------------------------------------------------------------------------------
@DTYPES
def test_reference_scenario(api, torch, dtype):
    X, y, c0, _ = H.scenario(dtype, 0, 100)
    x1, x2 = de.Node(feature=1), de.Node(feature=2)
    tree = de.Node(1, de.Node(2, de.Node(2, de.Node(3, x1, de.Node(val=0.8)), de.Node(val=0.0))), de.Node(3, de.Node(val=5.2), x2))
    pop = api.Population([tree], OPS, dtype, n_features=2)
    assert pop.constants().tolist() == c0.tolist()
    hist = []
    consts, loss, ok = pop.fit_constants_bfgs_device(X, y, iters=60, history=hist)
    print(f"[bfgs device] the reference's scenario, {np.dtype(dtype).name}: c = {consts.tolist()}, loss {hist[0][0]:.4g} -> {float(loss[0]):.4g}, "
          f"{int(pop.bfgs_accepts[0])} accepted of 60")
    assert ok[0] and abs(float(consts[0]) - 2.1) < 0.01  # the reference's assertion (test/test_optim.jl:27-31)
    ct, lt, okt = pop.fit_constants_bfgs_device(dev_X(torch, X), torch.from_numpy(y).cuda(), torch.from_numpy(c0).cuda(), iters=60)
    assert same_bytes(api, ct, consts) and same_bytes(api, lt, loss)
    pop.close()


# ---- 4. ground the Levenberg-Marquardt fits cannot cover ---------------------------------------------------------------------------------
@DTYPES
def test_hinge_classifier(api, dtype):
    """l1_hinge has no Gauss-Newton matrix (fit_constants_lm_device refuses it); final loss < 0.5 x initial after 20 iterations, seeds
    100 .. 104 (the CPU run of tests/test_bfgs_host.py through the hooks: worst 0.21)."""
    x1, x2 = de.Node(feature=1), de.Node(feature=2)
    for seed in range(100, 105):
        X, y, c0, _ = H.hinge_case(dtype, seed)
        tree = de.Node(1, de.Node(1, de.Node(3, de.Node(val=0.5), x1), de.Node(3, de.Node(val=0.25), x2)), de.Node(val=0.75))
        pop = api.Population([tree], OPS, dtype, n_features=2)
        assert pop.constants().tolist() == c0.tolist()
        hist = []
        consts, loss, ok = pop.fit_constants_bfgs_device(X, y, iters=20, loss="l1_hinge", history=hist)
        ratio = float(loss[0]) / hist[0][0]
        print(f"[bfgs device] hinge {np.dtype(dtype).name} seed {seed}: loss / initial = {ratio:.3g}, {int(pop.bfgs_accepts[0])} accepted of 20")
        assert ok[0] and ratio < 0.5
        if seed == 100:
            pop.set_constants(c0)
            with pytest.raises(ValueError, match="curvature"):
                pop.fit_constants_lm_device(X, y, iters=20, loss="l1_hinge")
            assert pop.constants().tobytes() == c0.tobytes()
        pop.close()


@DTYPES
@pytest.mark.parametrize("k", [12, 32])
@pytest.mark.parametrize("N", [64, 257])
def test_wide_chains_without_a_matrix(api, dtype, k, N):
    """chain(k) against a y made from constants jittered by up to 20 %, L2, 40 iterations: the loss falls below 1e-3 of its start (the CPU
    run through the hooks, tests/test_bfgs_host.py, reaches 1e-11 and less)."""
    X, y, c0, _ = H.chain_case(k, dtype, N)
    pop = api.Population([chain(k)], OPS, dtype, n_features=3)
    assert pop.constants().tolist() == c0.tolist()
    hist = []
    consts, loss, ok = pop.fit_constants_bfgs_device(X, y, iters=40, history=hist)
    print(f"[bfgs device] chain({k}) {np.dtype(dtype).name} N={N}: loss / initial = {float(loss[0]) / hist[0][0]:.3g}, "
          f"{int(pop.bfgs_accepts[0])} accepted of 40")
    assert ok[0] and float(loss[0]) < 1e-3 * hist[0][0]
    pop.close()


# ---- 5. a parametric population ----------------------------------------------------------------------------------------------------------
@DTYPES
def test_parametric_population(api, dtype):
    P, Cn, N = 3, 4, 257
    trees = GN.population_trees(44, (1, 2, 3), dtype, nfeatures=2, per_width=4, node_type=de.ParametricNode, nparams=P)
    pop = api.Population(trees, OPS, dtype, n_features=2, n_params=P)
    X, y, w = GN.data(N, 2, dtype, 13)
    g = np.random.Generator(np.random.PCG64(6))
    params = np.asfortranarray(g.uniform(-1.5, 1.5, (P, Cn)).astype(dtype))
    classes = g.integers(1, Cn + 1, N)
    c0 = pop.constants().copy()
    hh, hd = [], []
    ch, lh, okh = pop.fit_constants_bfgs(X, y, c0, weights=w, iters=4, history=hh, params=params, classes=classes)
    acc_h = pop.bfgs_accepts.copy()
    cd, ld, okd = pop.fit_constants_bfgs_device(X, y, c0, weights=w, iters=4, history=hd, params=params, classes=classes)
    assert cd.tobytes() == ch.tobytes() and ld.tobytes() == lh.tobytes() and np.array_equal(okd, okh)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(hd, hh)) and np.asarray(pop.bfgs_accepts).tobytes() == acc_h.tobytes()
    assert okd.sum() >= 8 and (np.asarray(pop.bfgs_accepts) > 0).sum() >= 4
    lo, _, ok2 = pop.eval_loss_grad(X, y, weights=w, params=params, classes=classes)  # at the returned constants, the parameters fixed
    assert np.array_equal(okd, ok2) and lo.tobytes() == ld.tobytes() and pop.constants().tobytes() == cd.tobytes()
    pop.close()


# ---- 6. edges and refusals ---------------------------------------------------------------------------------------------------------------
def test_edges(api, torch):
    dtype = np.float32
    # (tests/test_gpu_lm.py's population: six complete trees and one whose constant is inf)
    trees = GN.population_trees(35, (0, 2, 3), dtype, per_width=2) + [de.Node(1, de.Node(feature=1), de.Node(val=float("inf")))]
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = GN.data(129, 3, dtype, 5)
    c0 = pop.constants().copy()
    # iters = 0: de_eval_loss_grad_ex's loss and flags, the constants unchanged
    hist = []
    consts, loss, ok = pop.fit_constants_bfgs_device(X, y, weights=w, iters=0, history=hist)
    lo, _, ok1 = pop.eval_loss_grad(X, y, weights=w)
    assert len(hist) == 1 and consts.tobytes() == c0.tobytes() and pop.constants().tobytes() == c0.tobytes()
    assert loss.tobytes() == lo.tobytes() and np.array_equal(ok, ok1) and not ok[-1] and ok[:-1].all()
    assert np.array_equal(hist[0], loss.astype(np.float64), equal_nan=True) and not np.asarray(pop.bfgs_accepts).any()
    # N = 0: losses 0, NaN where a constant already fails the flag; every row of the history the same; the constants unchanged
    hist = []
    consts, loss, ok = pop.fit_constants_bfgs_device(np.zeros((3, 0), dtype=dtype, order="F"), np.zeros(0, dtype=dtype), iters=3, history=hist)
    assert ok.tolist() == [True] * 6 + [False] and not loss[:6].any() and np.isnan(loss[6]) and len(hist) == 4
    assert all(np.array_equal(h, loss.astype(np.float64), equal_nan=True) for h in hist) and not np.asarray(pop.bfgs_accepts).any()
    assert consts.tobytes() == c0.tobytes() and pop.constants().tobytes() == c0.tobytes()
    pop.close()
    # a population without constants
    bare = api.Population([none_tree(), de.Node(3, de.Node(feature=1), de.Node(feature=3))], OPS, dtype, n_features=3)
    hist = []
    consts, loss, ok = bare.fit_constants_bfgs_device(X, y, weights=w, iters=3, history=hist)
    lo, _ = bare.eval_loss(X, y, weights=w)
    assert consts.size == 0 and loss.tobytes() == lo.tobytes() and ok.all() and len(hist) == 4 and not np.asarray(bare.bfgs_accepts).any()
    assert all(h.tobytes() == loss.astype(np.float64).tobytes() for h in hist)
    bare.close()
    # an empty population
    empty = api.Population([], OPS, dtype, n_features=3)
    consts, loss, ok = empty.fit_constants_bfgs_device(X, y, iters=2)
    assert consts.size == 0 and loss.size == 0 and ok.size == 0
    consts, loss, ok = empty.fit_constants_bfgs_device(dev_X(torch, X), torch.from_numpy(y).cuda(), iters=2)
    assert consts.numel() == 0 and loss.numel() == 0 and ok.numel() == 0
    empty.close()


def test_refusals_and_defaults(api):
    lib = api.library()
    cos1 = de.OperatorEnum(binary_operators=("+",), unary_operators=("cos",))
    tree = de.Node(1, de.Node(1, de.Node(feature=1)), de.Node(val=0.5))
    X = np.asfortranarray(np.linspace(-1, 1, 64)[None, :])
    L2 = api.LossSpec(0, 0, 0.0)

    def raw(pop, Xa, ya, opts=None, spec=L2, yp=True, okp=True, n=1, rows=32):
        """de_fit_consts_bfgs itself on sentinel-filled outputs: (status, every output still the sentinel, history)."""
        lo, ok = np.full(2 * n, 7, dtype=np.float64), np.full(n, 9, dtype=np.uint8)
        hist, acc = np.full(rows * n, 7.0), np.full(n, 9, dtype=np.int32)
        rc = lib.de_fit_consts_bfgs(pop.ctx._h, pop._h, Xa.ctypes.data, Xa.shape[1], Xa.shape[0], None, ya.ctypes.data if yp else None, None,
                                    C.byref(spec) if spec is not None else None, C.byref(opts) if opts is not None else None,
                                    lo.ctypes.data, ok.ctypes.data if okp else None, hist.ctypes.data, acc.ctypes.data)
        return rc, bool((lo == 7).all() and (ok == 9).all() and (hist == 7).all() and (acc == 9).all()), hist

    for dtype in (np.float16, np.complex64):  # evaluation-only populations
        pop = api.Population([tree], cos1, dtype, n_features=1)
        before = pop.constants().copy()
        with pytest.raises(api.DeviceError, match="DE_ERR_UNSUPPORTED"):
            pop.fit_constants_bfgs_device(X.astype(dtype), np.zeros(64, dtype=dtype))
        Xc = np.asfortranarray(X.astype(dtype))
        assert raw(pop, Xc, Xc)[:2] == (7, True) and pop.constants().tobytes() == before.tobytes()
        pop.close()
    # a GraphNode population with a shared constant (a program made by de_program_create_cse): the host loop serves it
    Gn = de.GraphNode
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    x1, c, c2 = Gn(feature=1), Gn(val=0.75), Gn(val=-0.4)
    sh = Gn(1, Gn(2, x1, c))
    dag = Gn(1, Gn(1, sh, Gn(2, sh, Gn(2, c, x1))), c2)
    for dtype in (np.float32, np.float64):
        pop = api.Population([dag], ops, dtype, n_features=1)
        before = pop.constants().copy()
        Xf, y = np.asfortranarray(X.astype(dtype)), np.cos(X[0]).astype(dtype)
        with pytest.raises(ValueError, match="fit_constants_bfgs"):
            pop.fit_constants_bfgs_device(Xf, y)
        assert raw(pop, Xf, y)[:2] == (7, True) and pop.constants().tobytes() == before.tobytes()
        hist = []
        consts, loss, ok = pop.fit_constants_bfgs(Xf, y, before, iters=8, history=hist)  # ... the host loop does, on the combined rows
        assert ok[0] and hist[-1][0] < hist[0][0] and pop.constants().tobytes() == consts.tobytes()
        pop.close()
    # bad specs, bad options, a null y, a null ok
    dtype = np.float32
    pop = api.Population([tree, de.Node(1, de.Node(feature=1), de.Node(val=2.0))], cos1, dtype, n_features=1)
    Xf, y = np.asfortranarray(X.astype(dtype)), np.cos(X[0]).astype(dtype)
    before = pop.constants().copy()
    S, O = api.LossSpec, api.BfgsOpts
    for spec in (None, S(2, 0, 0.0), S(0, 1, 0.0), S(99, 0, 0.0), S(16, 0, -1.0), S(16, 0, float("nan")), S(20, 0, 1.5)):
        assert raw(pop, Xf, y, spec=spec, n=2)[:2] == (1, True), spec and (spec.kind, spec.reserved, spec.param)
        assert pop.constants().tobytes() == before.tobytes()
    nan, inf = float("nan"), float("inf")
    for opts in (O(-1, 0, 1.0, 0.5, 1e-4, 1e-8), O(3, 1, 1.0, 0.5, 1e-4, 1e-8), O(3, 0, 0.0, 0.5, 1e-4, 1e-8), O(3, 0, -1.0, 0.5, 1e-4, 1e-8),
                 O(3, 0, inf, 0.5, 1e-4, 1e-8), O(3, 0, nan, 0.5, 1e-4, 1e-8), O(3, 0, 1.0, 0.0, 1e-4, 1e-8), O(3, 0, 1.0, 1.0, 1e-4, 1e-8),
                 O(3, 0, 1.0, -0.5, 1e-4, 1e-8), O(3, 0, 1.0, nan, 1e-4, 1e-8), O(3, 0, 1.0, 1.5, 1e-4, 1e-8), O(3, 0, 1.0, 0.5, 0.0, 1e-8),
                 O(3, 0, 1.0, 0.5, nan, 1e-8), O(3, 0, 1.0, 0.5, inf, 1e-8), O(3, 0, 1.0, 0.5, 1e-4, 0.0), O(3, 0, 1.0, 0.5, 1e-4, -1e-8),
                 O(3, 0, 1.0, 0.5, 1e-4, nan), O(3, 0, 1.0, 0.5, 1e-4, inf)):
        assert raw(pop, Xf, y, opts, n=2)[:2] == (1, True), list(getattr(opts, n) for n, _ in O._fields_)
        assert pop.constants().tobytes() == before.tobytes()
    assert raw(pop, Xf, y, yp=False, n=2)[:2] == (1, True) and raw(pop, Xf, y, okp=False, n=2)[:2] == (1, True)
    assert pop.constants().tobytes() == before.tobytes()
    with pytest.raises(ValueError):
        pop.fit_constants_bfgs_device(Xf, y[:-1])
    with pytest.raises(ValueError):
        pop.fit_constants_bfgs_device(Xf, y, consts0=before[:-1])
    assert pop.constants().tobytes() == before.tobytes()
    # ... and the same call with good arguments runs; null options are {20, 0, 1.0, 0.5, 1e-4, 1e-8}: 21 rows of history, the rest untouched
    rc, untouched, hist = raw(pop, Xf, y, None, n=2)
    assert rc == 0 and not untouched and pop.constants().tobytes() != before.tobytes()
    assert (hist[21 * 2:] == 7).all() and (hist[:21 * 2] != 7).all()
    fitted = pop.constants().copy()
    pop.set_constants(before)
    rc, _, hist2 = raw(pop, Xf, y, O(20, 0, 1.0, 0.5, 1e-4, 1e-8), n=2)
    assert rc == 0 and hist2.tobytes() == hist.tobytes() and pop.constants().tobytes() == fitted.tobytes()
    href = []
    consts, loss, ok = pop.fit_constants_bfgs_device(Xf, y, consts0=before, history=href)  # the Python defaults are the library's
    assert np.concatenate(href).tobytes() == hist[:42].tobytes() and consts.tobytes() == fitted.tobytes()
    pop.close()
