"""GPU tests of the device L-BFGS fits (include/de_hip.h de_fit_consts_lbfgs / de_fit_tree_params_lbfgs, api.Population
.fit_constants_lbfgs_device, api.ParametricPopulation.fit_lbfgs_device).

THE YARDSTICK is the host loop — api.lbfgs_fit over the hooks de_lbfgs_direction_host / de_lbfgs_update_host (held to an independent
reference in tests/test_lbfgs_host.py) and the existing evaluation entry points — never the new call itself: constants, parameters,
loss, flags, the whole history and the accept counts are compared BYTE for byte.

Plain populations: chain(k) sums of G in {0, 1, 3, 8, 33, 40, 65} constants, a tree that is incomplete at its first evaluation, one whose
first trial overflows (2 exp(exp(c x2)) from c = 1 with step0 = 8: the trial is c = -7) and the reference's test/test_optim.jl tree;
N in {64, 2053}; weights with zeros; 12 iterations with memory 1 and 4, so the ring wraps.  Parametric populations: 3 parameters, 16
classes of which class 16 has no sample, G = 48 + n_real.  That both branches of the accept kernel run was settled on the CPU with
api.lbfgs_fit over numpy models of the chain trees and is asserted here on the device's own counts."""
import ctypes as C

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import test_gpu_gauss_newton as GN
from test_gpu_lm import bad_trees, chain, offsets
from test_tree_params_host import O_, P_, V_, X_

pytestmark = pytest.mark.gpu
OPS = GN.OPS
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
ITERS, STEP0, SENT = 12, 8.0, 7
WIDTHS = (1, 3, 8, 33, 40, 65)
T_NONE, T_DIV0, T_OVER, T_REF = 0, 7, 8, 9


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


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def plain_trees():
    x1, x2 = de.Node(feature=1), de.Node(feature=2)
    none = de.Node(1, x1, de.Node(2, x2))                                                              # x1 + exp(x2): no constant
    div0 = bad_trees()[0]                                                                               # 1.5 / (x1 - x1) + 0.5
    over = de.Node(3, de.Node(val=2.0), de.Node(2, de.Node(2, de.Node(3, de.Node(val=1.0), x2))))       # 2 exp(exp(1 x2))
    ref = de.Node(1, de.Node(2, de.Node(2, de.Node(3, x1, de.Node(val=0.8)), de.Node(val=0.0))), de.Node(3, de.Node(val=5.2), x2))
    return [none] + [chain(k) for k in WIDTHS] + [div0, over, ref]


class Recorder:
    """Population.eval_loss_grad with the flags of every call kept: what the host loop saw of its trials."""

    def __init__(self, pop):
        self.pop, self.inner, self.flags = pop, pop.eval_loss_grad, []
        pop.eval_loss_grad = self

    def __call__(self, *a, **kw):
        out = self.inner(*a, **kw)
        self.flags.append(np.array(out[2], dtype=bool))
        return out

    def stop(self):
        del self.pop.eval_loss_grad


# ---- 1. plain populations: the trajectory, bit for bit ---------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("N", [64, 2053])
@pytest.mark.parametrize("memory", [1, 4])
def test_plain_population_follows_the_host_loop_bit_for_bit(api, dtype, N, memory):
    trees = plain_trees()
    X, y, w = GN.data(N, 3, dtype, 60 + N)
    assert (w == 0).sum() > 5
    pop = api.Population(trees, OPS, dtype, n_features=3)
    c0 = pop.constants().copy()
    at = offsets(pop.n_consts)
    assert np.diff(at).tolist() == [0] + list(WIDTHS) + [2, 2, 3]
    kw = dict(weights=w, iters=ITERS, memory=memory, step0=STEP0)
    rec, hh = Recorder(pop), []
    ch, lh, okh = pop.fit_constants_lbfgs(X, y, c0, history=hh, **kw)
    rec.stop()
    acc_h = pop.lbfgs_accepts.copy()
    hd = []
    cd, ld, okd = pop.fit_constants_lbfgs_device(X, y, c0, history=hd, **kw)
    acc_d = np.asarray(pop.lbfgs_accepts).copy()
    print(f"[lbfgs device] {np.dtype(dtype).name} N={N} memory={memory}: accepted steps per tree host {acc_h.tolist()} device {acc_d.tolist()}; "
          f"loss {hd[0].tolist()} -> {hd[-1].tolist()}")
    assert cd.dtype == dtype and ld.dtype == dtype and len(hd) == len(hh) == ITERS + 1 and len(rec.flags) == ITERS + 1
    assert bits(cd) == bits(ch) and bits(ld) == bits(lh) and np.array_equal(okd, okh)
    assert all(a.dtype == np.float64 and bits(a) == bits(b) for a, b in zip(hd, hh))
    assert acc_d.dtype == np.int32 and bits(acc_d) == bits(acc_h)
    # the population holds the result; eval_loss there reproduces the loss, eval_loss_grad the last row of the history (the accept
    # rule's losses), and the two kernels' sums of N non-negative terms agree to 2 (N + 2) u
    assert bits(pop.constants()) == bits(cd)
    lo, ok2 = pop.eval_loss(X, y, weights=w)
    assert bits(lo) == bits(ld) and np.array_equal(ok2, okd)
    lg, _, ok3 = pop.eval_loss_grad(X, y, weights=w)
    assert np.array_equal(lg.astype(np.float64), hd[-1], equal_nan=True) and np.array_equal(ok3, okd)
    for a, b in zip(hd, hd[1:]):
        assert ((b <= a) | (np.isnan(a) & np.isnan(b))).all()
    assert np.allclose(hd[-1], ld.astype(np.float64), rtol=2 * (N + 2) * GN.unit(dtype), atol=0, equal_nan=True)
    # every chain tree is fitted — 33, 40 and 65 constants too — and the ring wrapped: more accepted pairs than it holds
    chains = list(range(1, 1 + len(WIDTHS)))
    assert all(acc_d[t] >= 1 and hd[-1][t] < hd[0][t] for t in chains), acc_d
    assert (acc_d >= 3).any() and (acc_d[chains] > memory).any()
    assert any(0 < acc_d[t] < ITERS for t in chains + [T_OVER, T_REF])  # a rejected trial
    # a tree that is incomplete at the start, and one without constants, keep every bit
    assert bits(cd[at[T_DIV0]:at[T_DIV0 + 1]]) == bits(c0[at[T_DIV0]:at[T_DIV0 + 1]]) and acc_d[T_DIV0] == 0
    assert not okd[T_DIV0] and np.isnan(ld[T_DIV0]) and acc_d[T_NONE] == 0 and okd[T_NONE]
    # a trial that turns incomplete is rejected: the first trial of T_OVER is c = -7
    assert rec.flags[0][T_OVER] and not rec.flags[1][T_OVER] and hd[1][T_OVER] == hd[0][T_OVER]
    assert okd[T_OVER] and np.isfinite(cd[at[T_OVER]:at[T_OVER + 1]]).all() and acc_d[T_OVER] < ITERS
    pop.close()


@DTYPES
def test_eval_loss_at_the_result_reproduces_the_loss(api, dtype):
    """Population.eval_loss (the fused loss alone, de_eval_loss_ex) at the result against the fit's loss, bit for bit: the fit ends
    with that evaluation, because the losses of its accept rule are the loss-and-gradient kernel's, which sums a tree's samples in
    another order (measured on an MI355X at this shape: 1 ulp apart in Float32 on one tree of ten, 1 to 4 ulps in Float64 on six)."""
    trees = plain_trees()
    X, y, w = GN.data(2053, 3, dtype, 71)
    pop = api.Population(trees, OPS, dtype, n_features=3)
    cd, ld, okd = pop.fit_constants_lbfgs_device(X, y, weights=w, iters=ITERS, memory=4, step0=STEP0)
    lo, ok = pop.eval_loss(X, y, weights=w)
    print(f"[lbfgs device] {np.dtype(dtype).name}: loss of the fit {ld.tolist()}, eval_loss at the result {lo.tolist()}")
    assert bits(lo) == bits(ld) and np.array_equal(ok, okd)
    pop.close()


def test_torch_device_tensors_give_the_bits_of_the_numpy_call(api, torch):
    dtype = np.float32
    trees = plain_trees()
    X, y, w = GN.data(257, 3, dtype, 72)
    pop = api.Population(trees, OPS, dtype, n_features=3)
    c0 = pop.constants().copy()
    ha, hb = [], []
    a = pop.fit_constants_lbfgs_device(X, y, c0, weights=w, iters=ITERS, memory=2, step0=STEP0, history=ha)
    acc_a = np.asarray(pop.lbfgs_accepts).copy()
    Xd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()
    b = pop.fit_constants_lbfgs_device(Xd, torch.from_numpy(y).cuda(), torch.from_numpy(c0).cuda(), weights=torch.from_numpy(w).cuda(),
                                       iters=ITERS, memory=2, step0=STEP0, history=hb)
    assert all(torch.is_tensor(v) and v.is_cuda for v in b + (pop.lbfgs_accepts, hb[0]))
    assert all(bits(api._host(u)) == bits(api._host(v)) for u, v in zip(b, a)) and bits(api._host(pop.lbfgs_accepts)) == bits(acc_a)
    assert all(bits(api._host(u)) == bits(v) for u, v in zip(hb, ha))
    pop.close()


# ---- 2. parametric populations ---------------------------------------------------------------------------------------------------------
P, NCLS, F = 3, 16, 2
N_REAL = [1, 2, 0, 1]
M_LIN, M_COS, M_NOREAL, M_DIV = range(4)


def members():
    x1, x2 = X_(1), X_(2)
    return [
        O_("+", O_("*", V_(0.0), O_("*", x1, x2)), O_("+", O_("+", P_(1), O_("*", P_(2), x1)), O_("*", P_(3), x2))),  # linear in its 49 unknowns
        O_("+", O_("*", V_(0.0), O_("cos", O_("*", P_(1), x1))), O_("+", O_("*", P_(2), x2), O_("*", V_(0.0), P_(3)))),  # G = 50
        O_("+", P_(1), O_("*", P_(2), O_("exp", O_("*", P_(3), x1)))),                                                   # no real constant: G = 48
        O_("+", O_("/", x1, P_(2)), O_("*", P_(1), V_(0.0))),                                                            # p2 = 0 in class 1: incomplete
    ]


def param_data(dtype, N, seed=5):
    g = np.random.Generator(np.random.PCG64(seed))
    X = np.asfortranarray(g.uniform(0.5, 2.0, (F, N)).astype(dtype))
    y = g.standard_normal(N).astype(dtype)
    w = ((g.random(N) > 0.2) * g.uniform(0.5, 1.5, N)).astype(dtype)
    classes = (1 + np.arange(N) % (NCLS - 1)).astype(np.int64)  # class 16 has no sample
    g.shuffle(classes)
    consts0 = g.uniform(-1.0, 1.0, sum(N_REAL)).astype(dtype)
    params0 = g.uniform(0.5, 1.5, (4, P, NCLS)).astype(dtype)
    params0[M_DIV, 1, 0] = 0.0
    return X, y, w, classes, consts0, params0


def raw_param_fit(api, pp, X, y, w, classes, params, out_ptr, opts=None, spec=None, entry="de_fit_tree_params_lbfgs", iters=ITERS):
    """The entry point itself on sentinel-filled buffers of the test's own: (status, loss, ok, history, n_accept, tp, keepalives)."""
    ptr, N, ldX, yp, wp, tp, _, is_t, keep = pp._prepare(X, params, classes, 1, False, y, w)
    nt = pp.n_trees
    lo, ok = np.full(nt, SENT, dtype=pp.dtype), np.full(nt, SENT, dtype=np.uint8)
    hist, acc = np.full((max(iters, 0) + 1, nt), float(SENT)), np.full(nt, SENT, dtype=np.int32)
    spec = api.loss_spec("L2") if spec is None else spec
    opts = api.LbfgsOpts(iters, 0, 4, 0, STEP0, 0.5, 1e-4, 1e-8) if opts is None else opts
    rc = getattr(api.library(), entry)(pp.ctx._h, pp.pop._h, ptr, N, ldX, C.byref(tp), yp, wp, C.byref(spec), C.byref(opts), out_ptr,
                                       lo.ctypes.data, ok.ctypes.data, hist.ctypes.data, acc.ctypes.data)
    return rc, lo, ok, hist, acc, tp, keep


@DTYPES
def test_parametric_population_follows_the_host_loop_bit_for_bit(api, torch, dtype):
    N = 257
    X, y, w, classes, consts0, params0 = param_data(dtype, N)
    pp = api.ParametricPopulation(members(), OPS, dtype, n_features=F, n_params=P)
    assert pp.n_consts.tolist() == N_REAL
    at = offsets(N_REAL)
    fitted = [M_LIN, M_COS, M_NOREAL]
    hh = []
    ch, ph, lh, okh = pp.fit_lbfgs(X, y, params0, classes, consts0=consts0, weights=w, iters=ITERS, memory=4, step0=STEP0, history=hh)
    ah = np.asarray(pp.lbfgs_accepts).copy()
    cd, pd, ld, okd = pp.fit_lbfgs_device(X, y, params0, classes, consts0=consts0, weights=w, iters=ITERS, memory=4, step0=STEP0, history=True)
    hd, ad = pp.lbfgs_history, np.asarray(pp.lbfgs_accepts)
    print(f"[lbfgs tree_params {np.dtype(dtype).name}] accepted steps per member: host {ah.tolist()} device {ad.tolist()}; "
          f"loss {hd[0].tolist()} -> {hd[-1].tolist()}")
    assert cd.dtype == dtype and pd.dtype == dtype and pd.shape == (4, P, NCLS) and hd.shape == (ITERS + 1, 4)
    assert bits(cd) == bits(ch) and bits(pd) == bits(ph) and bits(ld) == bits(lh) and np.array_equal(okd, okh)
    assert bits(hd) == bits(np.stack(hh)) and ad.dtype == np.int32 and bits(ad) == bits(ah)
    assert (ad[fitted] >= 3).all() and any(ad[t] < ITERS for t in fitted) and okd[fitted].all()
    assert all(hd[-1][t] < hd[0][t] for t in fitted)
    # the member that is incomplete at the start keeps every bit; the empty class's columns never move
    assert bits(cd[at[M_DIV]:at[M_DIV + 1]]) == bits(consts0[at[M_DIV]:at[M_DIV + 1]]) and bits(pd[M_DIV]) == bits(params0[M_DIV])
    assert ad[M_DIV] == 0 and not okd[M_DIV] and bits(pd[:, :, NCLS - 1]) == bits(params0[:, :, NCLS - 1])
    # de_eval_loss_grad_tree_params with the result reproduces the loss
    assert bits(pp.constants()) == bits(cd) and pp.params is pd
    lo2, _, _, ok2 = pp.eval_loss_grad(X, y, pd, classes, weights=w)
    assert bits(lo2) == bits(ld) and np.array_equal(ok2, okd)

    # ld_params = 4 > P with NaN padding, params_out a host pointer: the padding of params_out is not written, that of params not read
    blk = np.ascontiguousarray(params0.transpose(0, 2, 1))
    pad = np.full((4, NCLS, 4), np.nan, dtype=dtype)
    pad[:, :, :P] = blk
    out = np.full((4, NCLS, 4), SENT, dtype=dtype)
    pp.set_constants(consts0)
    rc, lo, ok, hist, acc, tp, keep = raw_param_fit(api, pp, X, y, w, classes, pad[:, :, :P].transpose(0, 2, 1), out.ctypes.data)
    assert rc == 0 and tp.ld_params == 4 and tp.params == pad.ctypes.data
    assert np.all(out[:, :, P] == SENT) and bits(out[:, :, :P].transpose(0, 2, 1)) == bits(pd)
    assert bits(lo) == bits(ld) and bits(hist) == bits(hd) and bits(acc) == bits(ad) and bits(pp.constants()) == bits(cd)
    assert np.isnan(pad[:, :, P]).all() and bits(pad[:, :, :P]) == bits(blk)
    # ... and a device pointer
    outd = torch.full((4, NCLS, 4), float(SENT), dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
    pp.set_constants(consts0)
    rc, lo, ok, hist, acc, tp, keep = raw_param_fit(api, pp, X, y, w, classes, pad[:, :, :P].transpose(0, 2, 1), outd.data_ptr())
    torch.cuda.synchronize()
    outh = outd.cpu().numpy()
    assert rc == 0 and np.all(outh[:, :, P] == SENT) and bits(outh[:, :, :P].transpose(0, 2, 1)) == bits(pd)
    assert bits(lo) == bits(ld) and bits(hist) == bits(hd) and bits(acc) == bits(ad)

    # THE FEATURE: de_fit_tree_params_bfgs leaves these members alone (48 + n_real unknowns > 32), the new call lowers their loss
    cb, pb, lb, okb = pp.fit_bfgs_device(X, y, params0, classes, consts0=consts0, weights=w, iters=ITERS, step0=STEP0, history=True)
    assert not np.asarray(pp.bfgs_accepts).any() and bits(cb) == bits(consts0) and bits(pb) == bits(params0)
    assert bits(pp.bfgs_history[-1]) == bits(pp.bfgs_history[0]) == bits(hd[0])
    assert all(float(ld[t]) < float(lb[t]) for t in fitted)
    pp.close()


# ---- 3. the edge of the limit ----------------------------------------------------------------------------------------------------------
def test_a_member_at_the_row_limit_is_fitted_and_one_past_it_keeps_every_bit(api):
    """P = 8, 511 classes of 2 rows each (N = 1022), Float32, 3 iterations: 8 real constants make G = 8 + 8 * 511 = 4096 =
    de_lbfgs_max_rows(), 9 make 4097."""
    dtype, Pw, ncls = np.float32, 8, 511
    N = 2 * ncls
    assert api.LBFGS_MAX_ROWS == 4096 == 8 + Pw * ncls

    def member(n_real):
        acc = P_(1)
        for i in range(1, Pw):
            acc = O_("+", acc, O_("*", P_(i + 1), X_(1 + i % 2)))
        for k in range(n_real):
            acc = O_("+", acc, O_("*", V_(0.0), O_("cos", X_(1 + k % 2))))
        return acc

    g = np.random.Generator(np.random.PCG64(9))
    X = np.asfortranarray(g.uniform(0.5, 2.0, (F, N)).astype(dtype))
    y = g.standard_normal(N).astype(dtype)
    classes = np.repeat(np.arange(1, ncls + 1), 2).astype(np.int64)
    pp = api.ParametricPopulation([member(8), member(9)], OPS, dtype, n_features=F, n_params=Pw)
    assert pp.n_consts.tolist() == [8, 9]
    consts0 = g.uniform(0.2, 1.0, 17).astype(dtype)
    params0 = g.uniform(-0.5, 0.5, (2, Pw, ncls)).astype(dtype)
    hh = []
    ch, ph, lh, okh = pp.fit_lbfgs(X, y, params0, classes, consts0=consts0, iters=3, memory=2, history=hh)
    ah = np.asarray(pp.lbfgs_accepts).copy()
    cd, pd, ld, okd = pp.fit_lbfgs_device(X, y, params0, classes, consts0=consts0, iters=3, memory=2, history=True)
    hd, ad = pp.lbfgs_history, np.asarray(pp.lbfgs_accepts)
    print(f"[lbfgs tree_params, G = 4096 / 4097] accepted {ad.tolist()}, loss {hd[0].tolist()} -> {hd[-1].tolist()}")
    assert bits(cd) == bits(ch) and bits(pd) == bits(ph) and bits(ld) == bits(lh) and np.array_equal(okd, okh)
    assert bits(hd) == bits(np.stack(hh)) and bits(ad) == bits(ah)
    assert okd.all() and ad[0] >= 1 and hd[-1][0] < hd[0][0]                                           # G = 4096: fitted
    assert ad[1] == 0 and bits(cd[8:]) == bits(consts0[8:]) and bits(pd[1]) == bits(params0[1])         # G = 4097: every bit
    assert hd[-1][1] == hd[0][1]
    pp.close()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------
def bad_opts(api):
    L = api.LbfgsOpts
    return [L(20, 0, 0, 0, 1.0, 0.5, 1e-4, 1e-8), L(20, 0, 17, 0, 1.0, 0.5, 1e-4, 1e-8), L(20, 1, 8, 0, 1.0, 0.5, 1e-4, 1e-8),
            L(20, 0, 8, 1, 1.0, 0.5, 1e-4, 1e-8), L(-1, 0, 8, 0, 1.0, 0.5, 1e-4, 1e-8), L(20, 0, 8, 0, 1.0, 1.0, 1e-4, 1e-8),
            L(20, 0, 8, 0, np.inf, 0.5, 1e-4, 1e-8), L(20, 0, 8, 0, 1.0, 0.5, 0.0, 1e-8), L(20, 0, 8, 0, 1.0, 0.5, 1e-4, np.nan)]


def test_refusals_of_de_fit_consts_lbfgs(api):
    lib, name = api.library(), "de_fit_consts_lbfgs"

    def attempt(pop, dtype, spec=None, opts=None):
        """One call on sentinel-filled outputs: (status, the error text, outputs and constants untouched)."""
        es = np.dtype(dtype)
        X, y = np.asfortranarray(np.ones((3, 8), dtype=es)), np.ones(8, dtype=es)
        before = bits(pop.constants())
        lo, ok = np.full(pop.n_trees, SENT, dtype=es), np.full(pop.n_trees, SENT, dtype=np.uint8)
        hist, acc = np.full((21, pop.n_trees), float(SENT)), np.full(pop.n_trees, SENT, dtype=np.int32)
        spec = api.loss_spec("L2") if spec is None else spec
        rc = lib.de_fit_consts_lbfgs(pop.ctx._h, pop._h, X.ctypes.data, 8, 3, None, y.ctypes.data, None, C.byref(spec),
                                     C.byref(opts) if opts is not None else None, lo.ctypes.data, ok.ctypes.data, hist.ctypes.data, acc.ctypes.data)
        clean = bool((lo == SENT).all() and (ok == SENT).all() and (hist == SENT).all() and (acc == SENT).all() and bits(pop.constants()) == before)
        return rc, lib.de_last_error(pop.ctx._h).decode(), clean

    # DE_F16 and complex programs
    for dt in (np.float16, np.complex64):
        pop = api.Population([chain(3)], OPS, dt, n_features=3)
        rc, msg, clean = attempt(pop, dt)
        assert rc == 7 and name in msg and clean, (dt, rc, msg)
        pop.close()
    # a program made by de_program_create_cse
    Gn = de.GraphNode
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    sh = Gn(1, Gn(2, Gn(feature=1), Gn(val=0.75)))
    pop = api.Population([Gn(1, Gn(1, sh, Gn(2, sh, Gn(feature=2))), Gn(val=-0.4))], ops, np.float64, n_features=3)
    rc, msg, clean = attempt(pop, np.float64)
    assert rc == 7 and name in msg and "de_program_create_cse" in msg and clean, (rc, msg)
    pop.close()
    # a good population: the spec and the options
    pop = api.Population([chain(3), chain(40)], OPS, np.float64, n_features=3)
    rc, msg, clean = attempt(pop, np.float64, spec=api.loss_spec("pullback"))
    assert rc == 1 and name in msg and "PULLBACK" in msg and clean, (rc, msg)
    for o in bad_opts(api):
        rc, msg, clean = attempt(pop, np.float64, opts=o)
        assert rc == 1 and name in msg and "de_lbfgs_opts_t" in msg and clean, (rc, msg)
    # then a valid call on the same context works, the defaults included
    rc, msg, clean = attempt(pop, np.float64, opts=None)
    assert rc == 0 and not clean
    with pytest.raises(ValueError, match="memory"):
        pop.fit_constants_lbfgs_device(np.ones((3, 8)), np.ones(8), memory=0)
    pop.close()


def test_refusals_of_de_fit_tree_params_lbfgs(api):
    lib, name = api.library(), "de_fit_tree_params_lbfgs"

    def attempt(ctx, handle, constants, dtype, n_slots, spec=None, opts=None):
        es = np.dtype(dtype)
        X, y = np.asfortranarray(np.ones((F, 8), dtype=es)), np.ones(8, dtype=es)
        before = bits(constants())
        starts, sp = np.array([0, 8], dtype=np.int64), np.full(max(n_slots, 1), -1, dtype=np.int32)
        prm, out = np.ones((1, 1, 2), dtype=es), np.full((1, 1, 2), SENT, dtype=es)
        tp = api.TreeParams(prm.ctypes.data, 2, 1, 2, 0, starts.ctypes.data, sp.ctypes.data)
        lo, ok = np.full(1, SENT, dtype=es), np.full(1, SENT, dtype=np.uint8)
        hist, acc = np.full((21, 1), float(SENT)), np.full(1, SENT, dtype=np.int32)
        spec = api.loss_spec("L2") if spec is None else spec
        rc = lib.de_fit_tree_params_lbfgs(ctx._h, handle, X.ctypes.data, 8, F, C.byref(tp), y.ctypes.data, None, C.byref(spec),
                                          C.byref(opts) if opts is not None else None, out.ctypes.data, lo.ctypes.data, ok.ctypes.data,
                                          hist.ctypes.data, acc.ctypes.data)
        clean = bool((out == SENT).all() and (lo == SENT).all() and (ok == SENT).all() and (hist == SENT).all() and (acc == SENT).all()
                     and (prm == 1).all() and bits(constants()) == before)
        return rc, lib.de_last_error(ctx._h).decode(), clean

    pp = api.ParametricPopulation([O_("+", O_("*", X_(1), V_(1.5)), V_(0.25))], OPS, np.float16, n_features=F, n_params=2)
    rc, msg, clean = attempt(pp.ctx, pp.pop._h, pp.pop.constants, np.float16, 2)
    assert rc == 7 and name in msg and clean, (rc, msg)
    pp.close()
    Gn = de.GraphNode
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    sh = Gn(1, Gn(2, Gn(feature=1), Gn(val=0.75)))
    pop = api.Population([Gn(1, Gn(1, sh, Gn(2, sh, Gn(feature=2))), Gn(val=-0.4))], ops, np.float64, n_features=F)
    rc, msg, clean = attempt(pop.ctx, pop._h, pop.constants, np.float64, int(pop._slots_per_tree.sum()))
    assert rc == 7 and name in msg and "de_program_create_cse" in msg and clean, (rc, msg)
    pop.close()
    pp = api.ParametricPopulation([O_("+", O_("*", X_(1), V_(1.5)), P_(1))], OPS, np.float64, n_features=F, n_params=2)
    rc, msg, clean = attempt(pp.ctx, pp.pop._h, pp.pop.constants, np.float64, 2, spec=api.loss_spec("pullback"))
    assert rc == 1 and name in msg and "PULLBACK" in msg and clean, (rc, msg)
    for o in bad_opts(api):
        rc, msg, clean = attempt(pp.ctx, pp.pop._h, pp.pop.constants, np.float64, 2, opts=o)
        assert rc == 1 and name in msg and "de_lbfgs_opts_t" in msg and clean, (rc, msg)
    rc, msg, clean = attempt(pp.ctx, pp.pop._h, pp.pop.constants, np.float64, 2)
    assert rc == 0 and not clean
    pp.close()
