"""GPU tests of the device fit over constants and parameters (include/de_hip.h de_fit_tree_params_bfgs,
api.ParametricPopulation.fit_bfgs_device).

THE YARDSTICK is the existing host loop ParametricPopulation.fit_bfgs (api.tree_params_fit_bfgs around de_eval_loss_grad_tree_params)
and the existing evaluation entry points, never the new call itself: constants, parameters, loss, flags, the whole history and the
accept counts are compared BYTE for byte.

Shapes: F = 2, 2 parameters, 3 classes of which class 3 has no sample and class 2 exactly one; N in {64, 257} (one tile, and ragged over
several); weights with zeros; 12 iterations; eight trees (TREES below).  The start values are drawn once (START_SEED); that they make
both branches of the accept kernel run (a tree with >= 3 accepted steps, a rejected trial) was settled on the CPU with
api.tree_params_fit_bfgs over tests/test_tree_params_host.py's oracle_evaluator and is asserted here on the device's own counts."""
import ctypes as C

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
from test_tree_params_host import O_, OPS, P_, V_, X_, fixture_case, isapprox

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
P, NCLS, F, ITERS, START_SEED = 2, 3, 2, 12, 21
T_REF, T_LONE, T_TWICE, T_FOLD, T_NOPARAM, T_G32, T_G33, T_DIV = range(8)
SENT = 7


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


def chain(k):
    """c0 + c1 x2 + c2 x1 + ...: k real constants."""
    acc = V_(0.0)
    for i in range(1, k):
        acc = O_("+", acc, O_("*", V_(0.0), X_(1 + i % 2)))
    return acc


def make_trees():
    return [
        O_("+", O_("+", O_("*", X_(1), P_(2)), X_(2)), P_(1)),                           # the reference's tree: no real constant
        P_(1),                                                                           # a lone parameter leaf
        O_("+", O_("*", V_(1.5), P_(1)), O_("*", O_("-", V_(2.5), P_(1)), X_(1))),       # p1 twice between two constants
        O_("+", O_("cos", O_("*", P_(1), V_(2.0))), X_(1)),                              # a parameter inside a constant subtree
        O_("-", O_("*", X_(1), V_(1.5)), O_("/", X_(2), V_(2.5))),                       # no parameter leaf: still G = 2 + 6
        chain(26),                                                                       # G = 32: fitted
        chain(27),                                                                       # G = 33: keeps every bit
        O_("+", O_("/", X_(1), P_(2)), O_("*", O_("exp", O_("*", P_(1), X_(2))), V_(0.5))),  # divides by a parameter that is 0 in class 1
    ]


N_REAL = [0, 0, 2, 1, 2, 26, 27, 1]


def make_data(dtype, N, seed=3):
    g = np.random.Generator(np.random.PCG64(seed))
    X = np.asfortranarray(g.uniform(0.5, 2.0, (F, N)).astype(dtype))
    y = g.standard_normal(N).astype(dtype)
    w = ((g.random(N) > 0.2) * g.uniform(0.5, 1.5, N)).astype(dtype)
    classes = np.ones(N, dtype=np.int64)  # class 3 has no sample ...
    classes[N // 2] = 2                   # ... and class 2 exactly one
    assert (w == 0).sum() > 5
    return X, y, w, classes


def start_values(dtype):
    g = np.random.Generator(np.random.PCG64(START_SEED))
    consts0 = g.uniform(-1.0, 1.0, sum(N_REAL)).astype(dtype)
    params0 = g.uniform(0.5, 1.5, (8, P, NCLS)).astype(dtype)
    params0[T_DIV, 1, 0] = 0.0  # x1 / p2 with p2 = 0 in class 1, which has samples: incomplete at the start
    return consts0, params0


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def loss_kw(kind):
    return dict(loss="huber", loss_param=0.7) if kind == "huber" else dict(loss="L2")


def host_loop(pp, X, y, w, classes, consts0, params0, iters, **kw):
    hist = []
    c, p, lo, ok = pp.fit_bfgs(X, y, params0, classes, consts0=consts0, weights=w, iters=iters, history=hist, **kw)
    return c, p, lo, ok, np.stack(hist), np.asarray(pp.bfgs_accepts).copy()


def device_fit(pp, X, y, w, classes, consts0, params0, iters, **kw):
    c, p, lo, ok = pp.fit_bfgs_device(X, y, params0, classes, consts0=consts0, weights=w, iters=iters, history=True, **kw)
    return c, p, lo, ok, pp.bfgs_history, pp.bfgs_accepts


# ---- 1. bit-for-bit equality with the host loop ----------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("N", [64, 257])
@pytest.mark.parametrize("kind", ["L2", "huber"])
def test_bit_equal_to_the_host_loop(api, dtype, N, kind):
    X, y, w, classes = make_data(dtype, N)
    consts0, params0 = start_values(dtype)
    pp = api.ParametricPopulation(make_trees(), OPS, dtype, n_features=F, n_params=P)
    assert pp.n_consts.tolist() == N_REAL
    at = np.concatenate([[0], np.cumsum(N_REAL)])
    ch, ph, lh, okh, hh, ah = host_loop(pp, X, y, w, classes, consts0, params0, ITERS, **loss_kw(kind))
    cd, pd, ld, okd, hd, ad = device_fit(pp, X, y, w, classes, consts0, params0, ITERS, **loss_kw(kind))
    print(f"[tree_params fit {np.dtype(dtype).name} N={N} {kind}] accepted steps per tree: host {ah.tolist()} device {np.asarray(ad).tolist()}; "
          f"loss {hd[0].tolist()} -> {hd[-1].tolist()}")
    assert cd.dtype == dtype and pd.dtype == dtype and ld.dtype == dtype and pd.shape == (8, P, NCLS) and hd.shape == (ITERS + 1, 8)
    assert bits(cd) == bits(ch) and bits(pd) == bits(ph) and bits(ld) == bits(lh) and np.array_equal(okd, okh)
    assert hd.dtype == np.float64 and bits(hd) == bits(hh)
    assert ad.dtype == np.int32 and bits(ad) == bits(ah)
    # both branches of the accept kernel ran
    fitted = [T_REF, T_LONE, T_TWICE, T_FOLD, T_NOPARAM, T_G32]
    assert (ad >= 3).any() and any(0 < ad[t] < ITERS for t in fitted), ad
    # trees that are not fitted keep every bit
    for t, complete in ((T_G33, True), (T_DIV, False)):
        assert bits(cd[at[t]:at[t + 1]]) == bits(consts0[at[t]:at[t + 1]]) and bits(pd[t]) == bits(params0[t]) and ad[t] == 0
        assert bool(okd[t]) == complete and np.isnan(ld[t]) == (not complete)
    assert okd[fitted].all()
    # the population holds the result and a second evaluation there reproduces the loss
    assert bits(pp.constants()) == bits(cd) and pp.params is pd
    full = pp.pop.constants()
    assert np.all(full[pp._slot_param_all >= 0] == 0)  # parameter slots hold their base values again
    lo2, _, _, ok2 = pp.eval_loss_grad(X, y, pd, classes, weights=w, **loss_kw(kind))
    assert bits(lo2) == bits(ld) and np.array_equal(ok2, okd)
    for a, b in zip(hd, hd[1:]):
        assert ((b <= a) | (np.isnan(a) & np.isnan(b))).all()
    assert np.array_equal(hd[-1], ld.astype(np.float64), equal_nan=True)
    pp.close()


# ---- 2. the reference's scenario -------------------------------------------------------------------------------------------------------
def test_reference_case_through_the_device_fit(api):
    """test/test_parametric_expression.jl:140-199 through fit_bfgs_device (Float64, from zeros, the fixture's 60 iterations): loss <
    minimum_below, initial loss > init_loss_above, parameters isapprox the true ones at rtol = sqrt(eps) — the reference's assertions."""
    tree, ops, X, classes, true_p, init_p, y, case = fixture_case()
    ex = api.ParametricExpression(tree, ops, init_p)
    other = api.ParametricExpression(tree.copy(), ops, true_p)  # a second member that starts at the answer
    pp = api.ParametricPopulation([ex, other], ops, np.float64, n_features=2, n_params=2)
    consts, ps, lo, ok = pp.fit_bfgs_device(X, y, classes=classes, iters=case["iters"], history=True)
    hist = pp.bfgs_history
    print(f"[tree_params fit, one call] loss {hist[0][0]:.3g} -> {lo[0]:.3g}, {int(pp.bfgs_accepts[0])} accepted steps of {case['iters']}, "
          f"parameter error {np.linalg.norm(ps[0] - true_p):.3g}")
    assert ok.all() and consts.size == 0 and hist.shape == (case["iters"] + 1, 2)
    assert lo[0] < case["expect"]["minimum_below"] and hist[0][0] > case["expect"]["init_loss_above"]
    assert isapprox(ps[0], true_p) and pp.params is ps
    assert lo[1] == 0 and bits(ps[1]) == bits(true_p) and pp.bfgs_accepts[1] == 0
    lo2, _, _, ok2 = pp.eval_loss_grad(X, y, classes=classes)
    assert bits(lo2) == bits(lo) and ok2.all()
    pp.close()


# ---- 3. torch device tensors -----------------------------------------------------------------------------------------------------------
def raw_fit(api, pp, X, y, w, classes, params, iters, out_ptr, spec=None, opts=None, y_null=False, pop=None):
    """de_fit_tree_params_bfgs itself on buffers of the test's own: (status, loss, ok, history, n_accept, tp, keepalives)."""
    dtype = pp.dtype
    ptr, N, ldX, yp, wp, tp, _, is_t, keep = pp._prepare(X, params, classes, 1, False, y, w)
    nt = pp.n_trees
    lo, ok = np.full(nt, SENT, dtype=dtype), np.full(nt, SENT, dtype=np.uint8)
    hist, acc = np.full((max(iters, 0) + 1, nt), float(SENT)), np.full(nt, SENT, dtype=np.int32)
    spec = api.loss_spec("L2") if spec is None else spec
    opts = api.BfgsOpts(iters, 0, 1.0, 0.5, 1e-4, 1e-8) if opts is None else opts
    handle = (pop or pp.pop)._h
    rc = api.library().de_fit_tree_params_bfgs(pp.ctx._h, handle, ptr, N, ldX, C.byref(tp), None if y_null else yp, wp, C.byref(spec),
                                               C.byref(opts), out_ptr, lo.ctypes.data, ok.ctypes.data, hist.ctypes.data, acc.ctypes.data)
    return rc, lo, ok, hist, acc, tp, keep


@DTYPES
def test_torch_device_tensors_give_the_bits_of_the_numpy_call(api, torch, dtype):
    N = 257
    X, y, w, classes = make_data(dtype, N)
    consts0, params0 = start_values(dtype)
    pp = api.ParametricPopulation(make_trees(), OPS, dtype, n_features=F, n_params=P)
    a = device_fit(pp, X, y, w, classes, consts0, params0, ITERS, loss="huber", loss_param=0.7)
    a = [np.array(v) for v in a]
    Xd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()
    yd, wd, cd = torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(classes).cuda()
    b = device_fit(pp, Xd, yd, wd, cd, torch.from_numpy(consts0).cuda(), torch.from_numpy(params0).cuda(), ITERS, loss="huber", loss_param=0.7)
    assert all(torch.is_tensor(v) and v.is_cuda for v in b) and pp.params is b[1]
    for u, v in zip(b, a):
        assert bits(u.cpu().numpy()) == bits(v)
    assert bits(pp.constants()) == bits(a[0])
    # params_out aliasing tp->params (a device block): the block holds the accepted parameters afterwards
    pp.set_constants(consts0)
    block = torch.from_numpy(np.ascontiguousarray(params0.transpose(0, 2, 1))).cuda()  # [n_trees, n_classes, n_params]: used in place
    rc, lo, ok, hist, acc, tp, keep = raw_fit(api, pp, Xd, yd, wd, cd, block.transpose(1, 2), ITERS, block.data_ptr(),
                                              spec=api.loss_spec("huber", 0.7))
    assert rc == 0 and tp.params == block.data_ptr()
    torch.cuda.synchronize()
    assert bits(block.cpu().numpy().transpose(0, 2, 1)) == bits(a[1]) and bits(lo) == bits(a[2]) and bits(hist) == bits(a[4]) and bits(acc) == bits(a[5])
    assert bits(pp.constants()) == bits(a[0])
    pp.close()


# ---- 4. edges --------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_edges(api, dtype):
    N = 64
    X, y, w, classes = make_data(dtype, N)
    consts0, params0 = start_values(dtype)
    it = np.uint32 if dtype == np.float32 else np.uint64
    pp = api.ParametricPopulation(make_trees(), OPS, dtype, n_features=F, n_params=P)
    pp.set_constants(consts0)
    lo0, _, _, ok0 = pp.eval_loss_grad(X, y, params0, classes, weights=w)
    # iters = 0: one history row, nothing changes
    c, p, lo, ok, hist, acc = device_fit(pp, X, y, w, classes, consts0, params0, 0)
    assert hist.shape == (1, 8) and bits(c) == bits(consts0) and bits(p) == bits(params0) and bits(lo) == bits(lo0) and np.array_equal(ok, ok0)
    assert np.array_equal(hist[0], lo0.astype(np.float64), equal_nan=True) and not acc.any()
    # N = 0: every history row is the first (the empty sum), nothing changes
    blk = np.ascontiguousarray(params0.transpose(0, 2, 1))
    out = np.full_like(blk, SENT)
    starts, sp = np.zeros(NCLS + 1, dtype=np.int64), pp._slot_param_all
    tp = api.TreeParams(blk.ctypes.data, P, NCLS, P, 0, starts.ctypes.data, sp.ctypes.data)
    lo, ok = np.full(8, SENT, dtype=dtype), np.full(8, SENT, dtype=np.uint8)
    hist, acc = np.full((4, 8), float(SENT)), np.full(8, SENT, dtype=np.int32)
    spec, opts = api.loss_spec("L2"), api.BfgsOpts(3, 0, 1.0, 0.5, 1e-4, 1e-8)
    rc = api.library().de_fit_tree_params_bfgs(pp.ctx._h, pp.pop._h, None, 0, F, C.byref(tp), y.ctypes.data, None, C.byref(spec), C.byref(opts),
                                               out.ctypes.data, lo.ctypes.data, ok.ctypes.data, hist.ctypes.data, acc.ctypes.data)
    assert rc == 0 and ok.all() and np.all(lo == 0) and np.all(hist == 0) and not acc.any()
    assert bits(out) == bits(blk) and bits(pp.constants()) == bits(consts0)
    # ld_params = 3 with NaN padding: the padding of params_out is not written, that of params not read
    pad = np.full((8, NCLS, 3), np.nan, dtype=dtype)
    pad[:, :, :P] = blk
    out = np.full((8, NCLS, 3), SENT, dtype=dtype)
    want = device_fit(pp, X, y, w, classes, consts0, params0, ITERS)
    want = [np.array(v) for v in want]
    pp.set_constants(consts0)
    rc, lo, ok, hist, acc, tp, keep = raw_fit(api, pp, X, y, w, classes, pad[:, :, :P].transpose(0, 2, 1), ITERS, out.ctypes.data)
    assert rc == 0 and tp.ld_params == 3 and tp.params == pad.ctypes.data
    assert np.all(out[:, :, P] == SENT) and bits(out[:, :, :P].transpose(0, 2, 1)) == bits(want[1])
    assert bits(lo) == bits(want[2]) and bits(hist) == bits(want[4]) and bits(acc) == bits(want[5]) and bits(pp.constants()) == bits(want[0])
    assert np.isnan(pad[:, :, P]).all() and bits(pad[:, :, :P]) == bits(blk)
    # an Inf in the empty class's column is never read by an evaluation: the flags and the first losses are those of the clean run, the
    # column keeps its bits, and the call is still the host loop bit for bit.  (The later trajectory is NOT the clean run's, in either
    # implementation: the step of such an entry is Inf - Inf = NaN, so the curvature test of de_bfgs.h refuses every update of B.)
    poisoned = params0.copy()
    poisoned[:, :, 2] = np.inf
    h = host_loop(pp, X, y, w, classes, consts0, poisoned, ITERS)
    d = device_fit(pp, X, y, w, classes, consts0, poisoned, ITERS)
    for u, v in zip(d, h):
        assert bits(u) == bits(v)
    assert np.array_equal(d[3], want[3]) and bits(d[4][0]) == bits(want[4][0])
    assert np.all(d[1][:, :, 2].view(it) == np.array([np.inf], dtype=dtype).view(it)) and d[5][:6].all()
    lo2, _, _, ok2 = pp.eval_loss_grad(X, y, d[1], classes, weights=w)
    assert bits(lo2) == bits(d[2]) and np.array_equal(ok2, d[3])
    pp.close()


def test_a_population_without_any_unknown(api):
    X, y, w, classes = make_data(np.float64, 64)
    pp = api.ParametricPopulation([O_("+", X_(1), X_(2)), O_("cos", X_(1))], OPS, np.float64, n_features=F, n_params=0)
    params = np.zeros((2, 0, NCLS))
    lo0, _, _, ok0 = pp.eval_loss_grad(X, y, params, classes, weights=w)
    c, p, lo, ok, hist, acc = device_fit(pp, X, y, w, classes, None, params, 5)
    assert c.size == 0 and p.shape == (2, 0, NCLS) and bits(lo) == bits(lo0) and ok.all() and not acc.any()
    assert hist.shape == (6, 2) and all(bits(r) == bits(lo0) for r in hist)
    pp.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(api):
    lib = api.library()
    plain = O_("+", O_("*", X_(1), V_(1.5)), P_(1))

    def attempt(ctx, handle, dtype, n_slots, spec=None, opts=None, y_null=False):
        """One call on sentinel-filled outputs: (status, outputs and params untouched)."""
        es = np.dtype(dtype)
        X, y = np.asfortranarray(np.ones((F, 8), dtype=es)), np.ones(8, dtype=es)
        starts, sp = np.array([0, 8], dtype=np.int64), np.full(max(n_slots, 1), -1, dtype=np.int32)
        prm, out = np.ones((1, 1, P), dtype=es), np.full((1, 1, P), SENT, dtype=es)
        tp = api.TreeParams(prm.ctypes.data, P, 1, P, 0, starts.ctypes.data, sp.ctypes.data)
        lo, ok = np.full(1, SENT, dtype=es), np.full(1, SENT, dtype=np.uint8)
        hist, acc = np.full((21, 1), float(SENT)), np.full(1, SENT, dtype=np.int32)
        spec = api.loss_spec("L2") if spec is None else spec
        rc = lib.de_fit_tree_params_bfgs(ctx._h, handle, X.ctypes.data, 8, F, C.byref(tp), None if y_null else y.ctypes.data, None, C.byref(spec),
                                         C.byref(opts) if opts is not None else None, out.ctypes.data, lo.ctypes.data, ok.ctypes.data,
                                         hist.ctypes.data, acc.ctypes.data)
        clean = bool((out == SENT).all() and (lo == SENT).all() and (ok == SENT).all() and (hist == SENT).all() and (acc == SENT).all()
                     and (prm == 1).all())
        return rc, clean, out, lo, ok

    # a program with n_params != 0
    pop = api.Population([O_("+", P_(1), V_(0.5))], OPS, np.float64, n_features=F, n_params=P)
    before = pop.constants().copy()
    assert attempt(pop.ctx, pop._h, np.float64, 1)[:2] == (7, True) and bits(pop.constants()) == bits(before)
    pop.close()
    # an F16 population
    pp = api.ParametricPopulation([O_("+", O_("*", X_(1), V_(1.5)), V_(0.25))], OPS, np.float16, n_features=F, n_params=P)
    before = pp.pop.constants().copy()
    assert attempt(pp.ctx, pp.pop._h, np.float16, 2)[:2] == (7, True) and bits(pp.pop.constants()) == bits(before)
    with pytest.raises(api.DeviceError, match="Float16"):
        pp.fit_bfgs_device(np.ones((F, 4), dtype=np.float16), np.ones(4, dtype=np.float16), np.ones((1, P, 1), dtype=np.float16), np.ones(4, dtype=np.int64))
    pp.close()
    # a program made by de_program_create_cse
    Gn = de.GraphNode
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    sh = Gn(1, Gn(2, Gn(feature=1), Gn(val=0.75)))
    pop = api.Population([Gn(1, Gn(1, sh, Gn(2, sh, Gn(feature=2))), Gn(val=-0.4))], ops, np.float64, n_features=F)
    before = pop.constants().copy()
    assert attempt(pop.ctx, pop._h, np.float64, int(pop._slots_per_tree.sum()))[:2] == (7, True) and bits(pop.constants()) == bits(before)
    pop.close()
    # a good population: the spec, the options and a null y
    pp = api.ParametricPopulation([plain], OPS, np.float64, n_features=F, n_params=P)
    assert pp.slot_param[0].tolist() == [-1, 0]
    before = pp.pop.constants().copy()

    def good(**kw):
        rc, clean, out, lo, ok = attempt(pp.ctx, pp.pop._h, np.float64, 2, **kw)
        return rc, clean and bits(pp.pop.constants()) == bits(before)

    # (attempt's slot_param marks both slots as real constants: the program is served either way)
    assert good(spec=api.loss_spec("pullback")) == (1, True)
    assert good(opts=api.BfgsOpts(-1, 0, 1.0, 0.5, 1e-4, 1e-8)) == (1, True)
    assert good(opts=api.BfgsOpts(20, 0, 1.0, 1.0, 1e-4, 1e-8)) == (1, True)
    assert good(opts=api.BfgsOpts(20, 1, 1.0, 0.5, 1e-4, 1e-8)) == (1, True)
    assert good(opts=api.BfgsOpts(20, 0, np.inf, 0.5, 1e-4, 1e-8)) == (1, True)
    assert good(y_null=True) == (1, True)
    # then a valid call on the same context still works
    rc, clean, out, lo, ok = attempt(pp.ctx, pp.pop._h, np.float64, 2, opts=api.BfgsOpts(20, 0, 1.0, 0.5, 1e-4, 1e-8))
    assert rc == 0 and ok[0] == 1 and np.isfinite(lo[0]) and lo[0] < 8 * (1.5 + 0.0 - 1.0) ** 2 and np.isfinite(out).all()
    pp.close()
