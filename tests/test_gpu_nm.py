"""GPU tests of Nelder-Mead on the constants on the device (include/de_hip.h de_fit_consts_nm).

The kernels run csrc/de_nm.h, the code behind the host hooks de_nm_ask_host / de_nm_tell_host, and `Population.fit_constants_nm` is the
host loop over those hooks (`api.nm_fit`: `set_constants`, `eval_loss`, one ask and one tell per tree).  So the one-call fit and the host
loop agree BIT FOR BIT: constants, loss, flags, the whole history and the improvement counts.  That equality is the test; the hooks
themselves are held to an independent model in tests/test_nm_host.py, whose `Model` also chose — on the CPU, with a numpy objective and
no library call — the starts of the two fits below that have a criterion of their own (the planted fit, and the fit a gradient cannot do)."""
import ctypes as C
import math

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import test_nm_host as H
import test_gpu_gauss_newton as GN
from test_gpu_lm import bad_trees, chain, dev_X, offsets

pytestmark = pytest.mark.gpu
OPS = GN.OPS
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
ROUNDS = 60
KINDS = {"L2": {}, "huber": dict(loss="huber", loss_param=1.3), "hinge": dict(loss="l1_hinge")}


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


def same_bytes(api, a, b):
    return api._host(a).tobytes() == api._host(b).tobytes()


def non_increasing(hist):
    return all(((b <= a) | (np.isnan(a) & np.isnan(b))).all() for a, b in zip(hist, hist[1:]))


def mixed_population(dtype):
    """Trees of 0, 1, 2, 3, 8, 9, 32 and 33 constants and two that are incomplete at the start: (trees, {index: why it is kept})."""
    x1 = de.Node(feature=1)
    good = GN.population_trees(61, (0, 1, 2, 3, 8), dtype, per_width=3)
    div0, _ = bad_trees()  # 1.5 / (x1 - x1) + 0.5: two constants, incomplete
    bare = de.Node(4, x1, de.Node(2, x1, x1))  # x1 / (x1 - x1)
    trees = good[:7] + [div0] + good[7:] + [chain(9), chain(32), chain(33), bare]
    kept = {7: "incomplete", len(trees) - 2: "33 constants", len(trees) - 1: "incomplete"}
    kept.update({t + (t >= 7): "no constant" for t in range(len(good)) if t % 5 == 0})
    return trees, kept


# ---- 1. the trajectory, bit for bit ----------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "unweighted"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_device_fit_follows_the_host_loop_bit_for_bit(api, dtype, kind, weighted):
    N = 2053  # more than one tile, with a ragged tail
    trees, kept = mixed_population(dtype)
    X, y, w = GN.data(N, 3, dtype, 50 + N)
    kw = dict(KINDS[kind], weights=w if weighted else None)
    pop = api.Population(trees, OPS, dtype, n_features=3)
    c0 = pop.constants().copy()
    at = offsets(pop.n_consts)
    widths = np.diff(at)
    assert len(trees) <= 40 and sorted(set(widths.tolist())) == [0, 1, 2, 3, 8, 9, 32, 33]
    assert all(widths[t] == 0 for t, why in kept.items() if why == "no constant") and widths[7] == 2
    lo0, ok0 = pop.eval_loss(X, y, weights=kw["weights"], loss=kw.get("loss", "L2"), loss_param=kw.get("loss_param", 0.0))
    assert [t for t in range(len(trees)) if not ok0[t]] == [7, len(trees) - 1]
    hh, hd = [], []
    ch, lh, okh = pop.fit_constants_nm(X, y, c0, iters=ROUNDS, history=hh, **kw)
    imp_h = pop.nm_improves.copy()
    cd, ld, okd = pop.fit_constants_nm_device(X, y, c0, iters=ROUNDS, history=hd, **kw)
    imp_d = np.asarray(pop.nm_improves).copy()
    assert cd.dtype == dtype and ld.dtype == dtype and lh.dtype == dtype and len(hd) == len(hh) == ROUNDS + 1
    assert same_bytes(api, cd, ch) and same_bytes(api, ld, lh) and np.array_equal(okd, okh) and np.array_equal(okd, ok0)
    assert all(a.dtype == np.float64 and a.tobytes() == b.tobytes() for a, b in zip(hd, hh))
    assert imp_d.dtype == np.int32 and imp_d.tobytes() == imp_h.tobytes()
    # the history: row 0 the loss at the start, never increasing, its last row the returned loss
    assert hd[0].tobytes() == lo0.astype(np.float64).tobytes() and non_increasing(hd)
    assert np.array_equal(hd[-1], ld.astype(np.float64), equal_nan=True)
    # the fit did something: the fitted trees of up to 9 constants have left BUILD, and at least three in four of them improved (a CPU
    # run of the same loop over the oracle: all of them, under every kind)
    narrow = [t for t in range(len(trees)) if t not in kept and widths[t] <= 9]
    assert len(narrow) == 13 and all((imp_d[t] > 0) == (hd[-1][t] < hd[0][t]) for t in narrow)
    assert 4 * sum(imp_d[t] > 0 for t in narrow) >= 3 * len(narrow), imp_d
    # trees that are not fitted keep their constants and report de_eval_loss_ex's loss
    for t, why in kept.items():
        assert cd[at[t]:at[t + 1]].tobytes() == c0[at[t]:at[t + 1]].tobytes() and imp_d[t] == 0, (t, why)
        assert ld[t:t + 1].tobytes() == lo0[t:t + 1].tobytes() and all(h[t:t + 1].tobytes() == hd[0][t:t + 1].tobytes() for h in hd)
        assert bool(okd[t]) == (why != "incomplete") and np.isnan(ld[t]) == (why == "incomplete")
    print(f"[nm device] {np.dtype(dtype).name} {kind} {'weighted' if weighted else 'unweighted'}: {len(trees)} trees bit-equal to the host "
          f"loop over {ROUNDS} rounds; improving rounds per tree {imp_d.tolist()}")
    pop.close()


# ---- 2. the program holds the accepted constants ---------------------------------------------------------------------------------------------
@DTYPES
def test_the_program_holds_the_accepted_constants(api, dtype):
    lib = api.library()
    trees = GN.population_trees(62, (1, 2, 3), dtype, per_width=3) + [chain(9)]
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = GN.data(1000, 3, dtype, 9)
    consts, loss, ok = pop.fit_constants_nm_device(X, y, weights=w, iters=40, loss="huber", loss_param=1.3)
    held = np.empty(consts.size, dtype=dtype)
    assert lib.de_program_get_consts(pop._h, held.ctypes.data) == 0 and held.tobytes() == consts.tobytes()
    lo, ok2 = pop.eval_loss(X, y, weights=w, loss="huber", loss_param=1.3)  # de_eval_loss_ex with the same spec
    assert lo.tobytes() == loss.tobytes() and np.array_equal(ok, ok2) and ok.all()
    pop.close()


# ---- 3. a planted, noiseless fit -------------------------------------------------------------------------------------------------------------
def test_planted_fit(api):
    """y = 2.5 cos(1.3 x1) - 0.7, tree c1 cos(c2 x1) + c3 from (2, 1, 0), 400 rounds, float64: final loss <= 1e-6 x the first.  The
    test's own model (tests/test_nm_host.py `Model`, a numpy objective) reaches 5.4e-24 x from this start on the CPU; the margin covers a
    different rounding of the device loss steering the path."""
    g = np.random.Generator(np.random.PCG64(77))
    x = g.uniform(-2.0, 2.0, 1000)
    y = 2.5 * np.cos(1.3 * x) - 0.7

    def objective(c):
        r = c[0] * np.cos(c[1] * x) + c[2] - y
        return float(np.sum(r * r)), True

    start = [2.0, 1.0, 0.0]
    _, f_model, h_model, _ = H.model_fit(objective, start, np.float64, 400)
    assert f_model <= 1e-12 * h_model[0]
    x1 = de.Node(feature=1)
    tree = de.Node(1, de.Node(3, de.Node(val=start[0]), de.Node(1, de.Node(3, de.Node(val=start[1]), x1))), de.Node(val=start[2]))
    pop = api.Population([tree], OPS, np.float64, n_features=1)
    assert pop.constants().tolist() == start
    hist = []
    consts, loss, ok = pop.fit_constants_nm_device(np.asfortranarray(x[None, :]), y, iters=400, history=hist)
    print(f"[nm device] planted fit: loss {hist[0][0]:.6g} -> {float(loss[0]):.3g} (the model: {f_model:.3g}), c = {consts.tolist()}, "
          f"{int(pop.nm_improves[0])} improving rounds of 400")
    assert ok[0] and float(loss[0]) <= 1e-6 * hist[0][0] and non_increasing(hist)
    pop.close()


# ---- 4. what a gradient cannot do ------------------------------------------------------------------------------------------------------------
def test_a_constant_under_round_moves(api):
    """c1 * round(c2 * x1) against y = 2 round(3 x1) from (1.5, 2.6): the partial of round is zero, so BFGS fits c1 alone and ends at or
    above L_fixed, the closed-form least-squares loss with c2 held; Nelder-Mead moves c2 and must end below half of it (the model on the
    CPU: 8.4e-9 x L_fixed after 60 rounds)."""
    ops = de.OperatorEnum(binary_operators=("*",), unary_operators=("round",))
    x = np.linspace(-2.0, 2.0, 1000)
    y = 2.0 * np.rint(3.0 * x)
    start, rounds = [1.5, 2.6], 60
    r0 = np.rint(start[1] * x)
    L_fixed = float(y @ y - (r0 @ y) ** 2 / (r0 @ r0))

    def objective(c):
        r = c[0] * np.rint(c[1] * x) - y
        return float(np.sum(r * r)), True

    _, f_model, _, _ = H.model_fit(objective, start, np.float64, rounds)
    assert f_model < 0.5 * L_fixed
    x1 = de.Node(feature=1)
    tree = de.Node(1, de.Node(val=start[0]), de.Node(1, de.Node(1, de.Node(val=start[1]), x1)))
    pop = api.Population([tree], ops, np.float64, n_features=1)
    X = np.asfortranarray(x[None, :])
    c0 = pop.constants().copy()
    assert c0.tolist() == start
    cb, lb, okb = pop.fit_constants_bfgs_device(X, y, c0, iters=30)
    cn, ln, okn = pop.fit_constants_nm_device(X, y, c0, iters=rounds)
    print(f"[nm device] c1 round(c2 x1): L_fixed {L_fixed:.6g}; BFGS {float(lb[0]):.6g} at {cb.tolist()}; Nelder-Mead {float(ln[0]):.3g} at "
          f"{cn.tolist()} (the model: {f_model:.3g})")
    assert okb[0] and okn[0]
    assert float(lb[0]) >= L_fixed * (1 - 1e-6)
    assert float(ln[0]) < 0.5 * L_fixed
    pop.close()


# ---- 5. a program made by de_program_create_cse ----------------------------------------------------------------------------------------------
@DTYPES
def test_cse_program(api, dtype):
    """A shared subtree that carries a constant.  The library's constants of the tree are the entries de_program_set_consts takes: one
    per occurrence; the host loop here moves the same entries through the raw calls."""
    lib = api.library()
    Gn = de.GraphNode
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    x1, x2 = Gn(feature=1), Gn(feature=2)
    sh = Gn(1, Gn(2, x1, Gn(val=0.75)))  # cos(x1 * 0.75), used twice
    dag = Gn(1, Gn(1, sh, Gn(2, sh, Gn(2, Gn(val=-0.4), x2))), Gn(val=0.3))
    plain = Gn(1, Gn(2, Gn(val=1.25), x1), Gn(val=-0.5))
    pop = api.Population([dag, plain], ops, dtype, n_features=2)
    slots = pop._slots_per_tree
    assert pop._occ is not None and slots.tolist() == [4, 2] and pop.n_consts.tolist() == [3, 2]
    X, y, w = GN.data(2053, 2, dtype, 21)
    ns = int(slots.sum())
    c0 = np.empty(ns, dtype=dtype)
    assert lib.de_program_get_consts(pop._h, c0.ctypes.data) == 0

    def install(consts):
        consts = np.ascontiguousarray(consts, dtype=dtype)
        pop.ctx.check(lib.de_program_set_consts(pop._h, consts.ctypes.data))

    def evaluate(consts):
        install(consts)
        return pop.eval_loss(X, y, weights=w)

    hh = []
    ch, lh, okh, imp_h = api.nm_fit(evaluate, install, c0, slots, dtype, iters=ROUNDS, history=hh)
    install(c0)
    lo, ok = np.full(2, 7, dtype=dtype), np.full(2, 9, dtype=np.uint8)
    hist, imp = np.full((ROUNDS + 1, 2), 7.0), np.full(2, 9, dtype=np.int32)
    spec, opts = api.LossSpec(0, 0, 0.0), api.NmOpts(ROUNDS, 0, 0.025, 0.5, 0.0)
    args = (pop.ctx._h, pop._h, X.ctypes.data, X.shape[1], X.shape[0], None, y.ctypes.data, w.ctypes.data, C.byref(spec))
    # de_fit_consts_bfgs refuses the program, everything untouched
    assert lib.de_fit_consts_bfgs(*args, None, lo.ctypes.data, ok.ctypes.data, hist.ctypes.data, imp.ctypes.data) == 7
    assert (lo == 7).all() and (ok == 9).all() and (hist == 7).all() and (imp == 9).all()
    assert lib.de_fit_consts_nm(*args, C.byref(opts), lo.ctypes.data, ok.ctypes.data, hist.ctypes.data, imp.ctypes.data) == 0
    cd = np.empty(ns, dtype=dtype)
    assert lib.de_program_get_consts(pop._h, cd.ctypes.data) == 0
    assert cd.tobytes() == ch.tobytes() and lo.tobytes() == lh.tobytes() and ok.astype(bool).tolist() == okh.tolist() == [True, True]
    assert hist.tobytes() == np.array(hh).tobytes() and imp.tobytes() == imp_h.tobytes() and (imp > 0).all()
    assert (hist[-1] < hist[0]).all() and pop.eval_loss(X, y, weights=w)[0].tobytes() == lo.tobytes()
    with pytest.raises(ValueError, match="fit_constants_nm"):  # the Python surface keeps a shared CONSTANT one coordinate: the host loop
        pop.fit_constants_nm_device(X, y)
    hu = []
    cu, lu, oku = pop.fit_constants_nm(X, y, pop.constants(), weights=w, iters=20, history=hu)
    assert cu.size == 5 and oku.all() and non_increasing(hu) and pop.eval_loss(X, y, weights=w)[0].tobytes() == lu.tobytes()
    pop.close()
    # a shared subtree WITHOUT a shared constant is still a program made by de_program_create_cse: the one call serves it from Python
    sh2 = Gn(1, Gn(2, x1, x2))
    dag2 = Gn(1, Gn(2, sh2, Gn(val=0.6)), Gn(2, sh2, Gn(2, sh2, Gn(val=-0.2))))
    pop = api.Population([dag2], ops, dtype, n_features=2)
    assert pop._occ is None
    c0 = pop.constants().copy()
    l_start = float(pop.eval_loss(X, y)[0][0])
    ch, lh, _ = pop.fit_constants_nm(X, y, c0, iters=30)
    cd, ld, _ = pop.fit_constants_nm_device(X, y, c0, iters=30)
    assert cd.tobytes() == ch.tobytes() and ld.tobytes() == lh.tobytes() and float(ld[0]) < l_start and cd.tobytes() != c0.tobytes()
    with pytest.raises(api.DeviceError, match="de_program_create_cse"):
        pop.fit_constants_bfgs_device(X, y, c0)
    pop.close()


# ---- 6. a parametric population --------------------------------------------------------------------------------------------------------------
@DTYPES
def test_parametric_population(api, dtype):
    P, Cn, N = 3, 4, 1000
    trees = GN.population_trees(44, (1, 2, 3), dtype, nfeatures=2, per_width=4, node_type=de.ParametricNode, nparams=P)
    pop = api.Population(trees, OPS, dtype, n_features=2, n_params=P)
    X, y, w = GN.data(N, 2, dtype, 13)
    g = np.random.Generator(np.random.PCG64(6))
    params = np.asfortranarray(g.uniform(-1.5, 1.5, (P, Cn)).astype(dtype))
    before = params.tobytes()
    classes = g.integers(1, Cn + 1, N)
    c0 = pop.constants().copy()
    hh, hd = [], []
    ch, lh, okh = pop.fit_constants_nm(X, y, c0, weights=w, iters=30, history=hh, params=params, classes=classes)
    imp_h = pop.nm_improves.copy()
    cd, ld, okd = pop.fit_constants_nm_device(X, y, c0, weights=w, iters=30, history=hd, params=params, classes=classes)
    assert cd.tobytes() == ch.tobytes() and ld.tobytes() == lh.tobytes() and np.array_equal(okd, okh)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(hd, hh)) and np.asarray(pop.nm_improves).tobytes() == imp_h.tobytes()
    assert okd.sum() >= 8 and (np.asarray(pop.nm_improves) > 0).sum() >= 8 and params.tobytes() == before
    lo, ok2 = pop.eval_loss(X, y, weights=w, params=params, classes=classes)  # at the returned constants, the parameters as they were
    assert np.array_equal(okd, ok2) and lo.tobytes() == ld.tobytes() and pop.constants().tobytes() == cd.tobytes()
    pop.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_defaults(api):
    lib = api.library()
    cos1 = de.OperatorEnum(binary_operators=("+",), unary_operators=("cos",))
    tree = de.Node(1, de.Node(1, de.Node(feature=1)), de.Node(val=0.5))
    X = np.asfortranarray(np.linspace(-1, 1, 64)[None, :])
    L2 = api.LossSpec(0, 0, 0.0)

    def raw(pop, Xa, ya, opts=None, spec=L2, yp=True, okp=True, n=1, rows=201):
        """de_fit_consts_nm itself on sentinel-filled outputs: (status, every output still the sentinel, history)."""
        lo, ok = np.full(2 * n, 7, dtype=np.float64), np.full(n, 9, dtype=np.uint8)
        hist, imp = np.full(rows * n, 7.0), np.full(n, 9, dtype=np.int32)
        rc = lib.de_fit_consts_nm(pop.ctx._h, pop._h, Xa.ctypes.data, Xa.shape[1], Xa.shape[0], None, ya.ctypes.data if yp else None, None,
                                  C.byref(spec) if spec is not None else None, C.byref(opts) if opts is not None else None,
                                  lo.ctypes.data, ok.ctypes.data if okp else None, hist.ctypes.data, imp.ctypes.data)
        return rc, bool((lo == 7).all() and (ok == 9).all() and (hist == 7).all() and (imp == 9).all()), hist

    for dtype in (np.float16, np.complex64):  # evaluation-only populations
        pop = api.Population([tree], cos1, dtype, n_features=1)
        before = pop.constants().copy()
        with pytest.raises(api.DeviceError, match="DE_ERR_UNSUPPORTED"):
            pop.fit_constants_nm_device(X.astype(dtype), np.zeros(64, dtype=dtype))
        Xc = np.asfortranarray(X.astype(dtype))
        assert raw(pop, Xc, Xc)[:2] == (7, True) and pop.constants().tobytes() == before.tobytes()
        pop.close()
    dtype = np.float32
    pop = api.Population([tree, de.Node(1, de.Node(feature=1), de.Node(val=2.0))], cos1, dtype, n_features=1)
    Xf, y = np.asfortranarray(X.astype(dtype)), np.cos(X[0]).astype(dtype)
    before = pop.constants().copy()
    S, O = api.LossSpec, api.NmOpts
    nan, inf = float("nan"), float("inf")
    for spec in (None, S(2, 0, 0.0), S(0, 1, 0.0), S(99, 0, 0.0), S(16, 0, -1.0), S(16, 0, nan), S(20, 0, 1.5)):
        assert raw(pop, Xf, y, spec=spec, n=2)[:2] == (1, True), spec and (spec.kind, spec.reserved, spec.param)
        assert pop.constants().tobytes() == before.tobytes()
    for opts in (O(-1, 0, 0.025, 0.5, 0.0), O(3, 1, 0.025, 0.5, 0.0), O(3, 0, nan, 0.5, 0.0), O(3, 0, inf, 0.5, 0.0), O(3, 0, 0.025, nan, 0.0),
                 O(3, 0, 0.025, -inf, 0.0), O(3, 0, 0.0, 0.0, 0.0), O(3, 0, -0.0, 0.0, 0.0), O(3, 0, 0.025, 0.5, -1e-300), O(3, 0, 0.025, 0.5, nan),
                 O(3, 0, 0.025, 0.5, inf)):
        assert raw(pop, Xf, y, opts, n=2)[:2] == (1, True), list(getattr(opts, n) for n, _ in O._fields_)
        assert pop.constants().tobytes() == before.tobytes()
    assert raw(pop, Xf, y, yp=False, n=2)[:2] == (1, True) and raw(pop, Xf, y, okp=False, n=2)[:2] == (1, True)
    assert pop.constants().tobytes() == before.tobytes()
    with pytest.raises(ValueError):
        pop.fit_constants_nm_device(Xf, y[:-1])
    with pytest.raises(ValueError):
        pop.fit_constants_nm_device(Xf, y, consts0=before[:-1])
    assert pop.constants().tobytes() == before.tobytes()
    # ... and the same call with good arguments runs; null options are {200, 0, 0.025, 0.5, 0.0}: 201 rows of history, the rest untouched
    rc, untouched, hist = raw(pop, Xf, y, None, n=2, rows=203)
    assert rc == 0 and not untouched and pop.constants().tobytes() != before.tobytes()
    assert (hist[201 * 2:] == 7).all() and (hist[:201 * 2] != 7).all()
    fitted = pop.constants().copy()
    pop.set_constants(before)
    rc, _, hist2 = raw(pop, Xf, y, O(200, 0, 0.025, 0.5, 0.0), n=2, rows=203)
    assert rc == 0 and hist2.tobytes() == hist.tobytes() and pop.constants().tobytes() == fitted.tobytes()
    href = []
    consts, loss, ok = pop.fit_constants_nm_device(Xf, y, consts0=before, history=href)  # the Python defaults are the library's
    assert np.concatenate(href).tobytes() == hist[:402].tobytes() and consts.tobytes() == fitted.tobytes()
    # a negative-only simplex (a = 0 with b != 0, b = 0 with a != 0) is served
    for a, b in ((0.0, 0.25), (0.5, 0.0), (-0.1, -0.3)):
        pop.set_constants(before)
        assert raw(pop, Xf, y, O(12, 0, a, b, 0.0), n=2)[0] == 0
    pop.close()


# ---- 8. device pointers ----------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_device_pointers_give_the_bits_of_host_buffers(api, torch, dtype):
    trees = GN.population_trees(63, (0, 1, 2, 3, 8), dtype, per_width=2) + [chain(33), bad_trees()[0]]
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = GN.data(2053, 3, dtype, 31)
    c0 = pop.constants().copy()
    hd, ht = [], []
    cd, ld, okd = pop.fit_constants_nm_device(X, y, c0, weights=w, iters=40, history=hd)
    imp_d = np.asarray(pop.nm_improves).copy()
    ct, lt, okt = pop.fit_constants_nm_device(dev_X(torch, X), torch.from_numpy(y).cuda(), torch.from_numpy(c0).cuda(),
                                              weights=torch.from_numpy(w).cuda(), iters=40, history=ht)
    assert all(torch.is_tensor(v) and v.is_cuda for v in (ct, lt, okt, pop.nm_improves, ht[0])) and pop.consts_on_device_path
    assert same_bytes(api, ct, cd) and same_bytes(api, lt, ld) and np.array_equal(api._host(okt), okd)
    assert same_bytes(api, pop.nm_improves, imp_d) and len(ht) == 41 and all(same_bytes(api, a, b) for a, b in zip(ht, hd))
    assert (imp_d > 0).sum() >= 6
    pop.close()
    # an empty population
    empty = api.Population([], OPS, dtype, n_features=3)
    consts, loss, ok = empty.fit_constants_nm_device(X, y, iters=2)
    assert consts.size == 0 and loss.size == 0 and ok.size == 0
    consts, loss, ok = empty.fit_constants_nm_device(dev_X(torch, X), torch.from_numpy(y).cuda(), iters=2)
    assert consts.numel() == 0 and loss.numel() == 0 and ok.numel() == 0
    empty.close()


# ---- 9. degenerate calls ---------------------------------------------------------------------------------------------------------------------
def test_degenerate_calls(api):
    dtype = np.float32
    trees = GN.population_trees(35, (0, 2, 3), dtype, per_width=2) + [de.Node(1, de.Node(feature=1), de.Node(val=float("inf")))]
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = GN.data(1000, 3, dtype, 5)
    c0 = pop.constants().copy()
    # iters = 0: de_eval_loss_ex's loss and flags, the constants unchanged
    hist = []
    consts, loss, ok = pop.fit_constants_nm_device(X, y, weights=w, iters=0, history=hist)
    lo, ok1 = pop.eval_loss(X, y, weights=w)
    assert len(hist) == 1 and consts.tobytes() == c0.tobytes() and pop.constants().tobytes() == c0.tobytes()
    assert loss.tobytes() == lo.tobytes() and np.array_equal(ok, ok1) and not ok[-1] and ok[:-1].all()
    assert np.array_equal(hist[0], loss.astype(np.float64), equal_nan=True) and not np.asarray(pop.nm_improves).any()
    # N = 0: losses 0, NaN where a constant already fails the flag; every row of the history the same; the constants unchanged
    hist = []
    consts, loss, ok = pop.fit_constants_nm_device(np.zeros((3, 0), dtype=dtype, order="F"), np.zeros(0, dtype=dtype), iters=3, history=hist)
    assert ok.tolist() == [True] * 6 + [False] and not loss[:6].any() and np.isnan(loss[6]) and len(hist) == 4
    assert all(np.array_equal(h, loss.astype(np.float64), equal_nan=True) for h in hist) and not np.asarray(pop.nm_improves).any()
    assert consts.tobytes() == c0.tobytes() and pop.constants().tobytes() == c0.tobytes()
    # N = 1, and f_tol so large that every tree is DONE behind BUILD: a tree of G constants moves in its first G rounds only — row r of
    # the history is the best of the start and the first min(r, G) simplex vertices, the rows from G on are one — as the host loop has it
    X1, y1, _ = GN.data(1, 3, dtype, 8)
    hh, hd = [], []
    ch, lh, okh = pop.fit_constants_nm(X1, y1, c0, iters=6, f_tol=1e30, history=hh)
    cd, ld, okd = pop.fit_constants_nm_device(X1, y1, c0, iters=6, f_tol=1e30, history=hd)
    assert cd.tobytes() == ch.tobytes() and ld.tobytes() == lh.tobytes() and np.array_equal(okd, okh)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(hd, hh)) and non_increasing(hd)
    at = offsets(pop.n_consts)
    for t in range(len(trees) - 1):
        G, a, b = int(at[t + 1] - at[t]), int(at[t]), int(at[t + 1])
        assert all(h[t] == hd[G][t] for h in hd[G:])
        # the accepted constants are the start or ONE vertex of the start simplex: at most one coordinate differs, by (1 + b) c + a
        moved = [j for j in range(a, b) if cd[j] != c0[j]]
        assert len(moved) <= 1 and all(cd[j] == dtype(1.5 * float(c0[j]) + 0.025) for j in moved)
        assert (len(moved) == 1) == (hd[-1][t] < hd[0][t])
    pop.close()
    # a population without constants
    bare = api.Population([de.Node(1, de.Node(feature=1), de.Node(2, de.Node(feature=2))), de.Node(3, de.Node(feature=1), de.Node(feature=3))],
                          OPS, dtype, n_features=3)
    hist = []
    consts, loss, ok = bare.fit_constants_nm_device(X, y, weights=w, iters=3, history=hist)
    lo, _ = bare.eval_loss(X, y, weights=w)
    assert consts.size == 0 and loss.tobytes() == lo.tobytes() and ok.all() and len(hist) == 4 and not np.asarray(bare.nm_improves).any()
    assert all(h.tobytes() == loss.astype(np.float64).tobytes() for h in hist)
    bare.close()
