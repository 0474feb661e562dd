"""GPU tests of the generalised Gauss-Newton fit (include/de_hip.h de_eval_loss_gn_ex / de_fit_consts_lm_ex): per tree
the loss of a kind, its gradient and M = sum_j w_j c_j d(j) d(j)^T with the kind's curvature weight c, and the Levenberg-Marquardt loop
over them.

The matrix reference is numpy over the DEVICE's own `Population.eval_grad` values and Jacobian (same handlers, same dual rows), in long
double: e = yhat - y (a = y * yhat for the margin kind) is formed in the element type, so it holds the kernel's bits; the kind's
parameter and the residual floor are rounded to the element type; c comes from the float64 table of tests/gn_kinds_reference.py.
    M_ref[i, k] = sum w c d_i d_k,   A[i, k] = sum w c |d_i d_k|,   |M - M_ref| <= 288 u A   entrywise
u = 2^-24 (Float32) / 2^-53 (Float64).  288 = the 256 of tests/test_gpu_gauss_newton.py (two roundings per product and a wave sum of at
most 128 terms, doubled for the FMA / no-FMA choice) + 2 (1 + 15): one more rounding (w c) and at most 15 u of error in c itself —
OCML's tanh / exp / pow are 1-2 ulp (csrc/de_loss_kinds.h) and the longest chain of further roundings is the margin's two sigmoids and
three products —, doubled likewise.  Trees whose Jacobian has a non-finite entry, or whose A is beyond a quarter of the type's largest
finite value, are compared on finiteness only; at most 5 % of a case's complete trees may be.

Every case prints the worst |M - M_ref| / (u A) it saw and the exempt share ("[gn kinds ...]" lines of the parity report)."""
import ctypes as C

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import gn_kinds_reference as gk
import loss_reference as lr
from test_gpu_gauss_newton import OPS, data, population_trees, unit

pytestmark = pytest.mark.gpu
K = 288.0
FLOOR = 1e-4
# (label, kind, parameter): every admitted kind, lp below, at the kink's edge and above two
CASES = [("L2", "L2", 0.0), ("L1", "L1", 0.0)] + [(k, k, lr.PARAMS[k]) for k in ("huber", "logcosh", "l1_eps", "l2_eps", "quantile", "lp",
                                                                                "logit_dist", "logit_margin")] + [("lp1", "lp", 1.0), ("lp3", "lp", 3.0)]
SIZES = {np.dtype(np.float32): (1, 65, 257, 513), np.dtype(np.float64): (1, 129, 513)}


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _api.library()
    return _api


def targets(y, kind):
    """standard normal targets for the distance kinds, +-1 for the margin kind"""
    return np.where(y < 0, -1, 1).astype(y.dtype) if kind == "logit_margin" else y


def weights_c(kind, p, out_t, y, w, dtype):
    """w c of every sample of one tree in long double: e (or a) in the element type, p and f rounded to it, c from the float64 table"""
    dt = np.dtype(dtype).type
    e = out_t - y  # element type: the kernel's bits
    c = gk.curvature(kind, e, y, out_t, float(dt(p)), float(dt(FLOOR)), gk.TAU[np.dtype(dtype)])
    ww = np.ones(len(y)) if w is None else np.asarray(w, dtype=np.float64)
    return ww.astype(np.longdouble) * c.astype(np.longdouble), ww != 0


def check_bound(gn, out, grads, y, w, kind, p, dtype, min_checked=1, label=""):
    """The bound of the module docstring for every complete tree with has_jtj; returns (worst ratio in u, exempt share)."""
    u, fmax = unit(dtype), float(np.finfo(dtype).max)
    ok, has = np.asarray(gn.ok, dtype=bool), np.asarray(gn.has_jtj, dtype=bool)
    worst, checked, exempt, complete = 0.0, 0, 0, 0
    for t in range(len(gn)):
        H = np.asarray(gn.jtj[t]).astype(np.float64)
        J = np.asarray(grads[t])
        G = J.shape[0]
        assert H.shape == (G, G)
        if not ok[t]:
            assert np.isnan(H).all() and np.isnan(np.asarray(gn.grad[t])).all() and np.isnan(np.asarray(gn.loss)[t])
            continue
        if not has[t]:
            assert G > 8 and np.isnan(H).all()
            continue
        complete += 1
        if G == 0:
            checked += 1
            continue
        with np.errstate(all="ignore"):
            wc, keep = weights_c(kind, p, out[t], y, w, dtype)
            Jl = J.astype(np.longdouble)[:, keep] * 1
            wk = wc[keep]
            Href = ((Jl * wk) @ Jl.T).astype(np.float64)
            A = ((np.abs(Jl) * wk) @ np.abs(Jl).T).astype(np.float64)
        if not np.isfinite(J).all() or not np.isfinite(out[t]).all() or not np.isfinite(A).all() or A.max() > 0.25 * fmax:
            exempt += 1
            continue
        assert np.array_equal(H, H.T), f"{label} tree {t}: not symmetric"
        with np.errstate(all="ignore"):
            err = np.abs(H - Href)
        assert (err <= K * u * A).all(), (label, t, H, Href, (err / (u * np.maximum(A, np.finfo(np.float64).tiny))).max())
        worst = max(worst, float((err[A > 0] / (u * A[A > 0])).max()) if (A > 0).any() else 0.0)
        checked += 1
    share = exempt / max(complete, 1)
    assert share <= 0.05, (label, exempt, complete)
    assert checked >= min_checked, (label, checked)
    return worst, share


_SHARED = {}


def shared(api, dtype, mode):
    """One population per (element type, mode) with, per sample count, its data and the device's own values and Jacobian: computed once,
    read by every kind's case."""
    key = (np.dtype(dtype), mode)
    if key not in _SHARED:
        trees = population_trees(11, range(9), dtype)  # 63 trees of <= 15 nodes, 0 ... 8 constants, 3 features
        pop = api.Population(trees, OPS, dtype, n_features=3)
        per_n = {}
        for N in SIZES[np.dtype(dtype)]:
            X, y, w = data(N, 3, dtype, 100 + N, True)
            out, grads, ok = pop.eval_grad(X, variable=mode)
            per_n[N] = (X, y, w, np.array(out), [np.array(g) for g in grads], np.array(ok))
        _SHARED[key] = (pop, per_n)
    return _SHARED[key]


def run_parity(api, dtype, mode, label, kind, p):
    pop, per_n = shared(api, dtype, mode)
    worst, share_max, n_has = 0.0, 0.0, 0
    for N, (X, y0, w, out, grads, ok_g) in per_n.items():
        y = targets(y0, kind)
        gn = pop.eval_gauss_newton(X, y, weights=w, variable=mode, loss=kind, loss_param=p, e_floor=FLOOR)
        assert np.array_equal(gn.ok, ok_g)
        lo, dl, ok_l = pop.eval_loss_grad(X, y, weights=w, loss=kind, loss_param=p, variable=mode)
        assert lo.tobytes() == np.asarray(gn.loss).tobytes() and np.array_equal(ok_l, gn.ok)
        assert all(a.tobytes() == np.asarray(b).tobytes() for a, b in zip(dl, gn.grad))
        wst, share = check_bound(gn, out, grads, y, w, kind, p, dtype, min_checked=20, label=f"{label} {mode} N={N}")
        worst, share_max, n_has = max(worst, wst), max(share_max, share), n_has + int(np.sum(gn.has_jtj))
    print(f"[gn kinds parity] {np.dtype(dtype).name} {label} {mode}: worst |M - M_ref| = {worst:.2f} u A (bound {K:.0f}), exempt share <= "
          f"{100 * share_max:.1f} %, {n_has} matrices, kernel {pop.ctx.last_kernel_name()}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("label,kind,p", CASES, ids=[c[0] for c in CASES])
def test_matrix_parity(api, dtype, label, kind, p):
    run_parity(api, dtype, False, label, kind, p)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_matrix_parity_huber_both(api, dtype):
    run_parity(api, dtype, "both", "huber", "huber", lr.PARAMS["huber"])


def gn_ex(api, pop, X, y, w, spec, floor, mode=1, n_out=None):
    """de_eval_loss_gn_ex over host buffers, packed offsets: (rc, loss, dloss, jtj, ok) — outputs start as sentinels"""
    lib = api.library()
    ng = pop._n_grad_all(mode)
    dt = pop.dtype
    lo = np.full(pop.n_trees, 7, dtype=dt)
    dl = np.full(max(int(ng.sum()), 1), 7, dtype=dt)
    jt = np.full(max(int((ng * ng).sum()), 1), 7, dtype=dt)
    ok = np.full(pop.n_trees, 9, dtype=np.uint8)
    rc = lib.de_eval_loss_gn_ex(pop.ctx._h, pop._h, X.ctypes.data, X.shape[1], X.shape[0], None, mode, y.ctypes.data,
                                None if w is None else w.ctypes.data, None if spec is None else C.byref(spec), float(floor), lo.ctypes.data,
                                dl.ctypes.data, None, jt.ctypes.data, None, ok.ctypes.data)
    return rc, lo, dl, jt, ok


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_l2_through_ex_returns_the_bytes_of_the_l2_call(api, dtype):
    lib = api.library()
    pop, per_n = shared(api, dtype, False)
    ng = pop._n_grad_all(1)
    for N, (X, y, w, *_rest) in per_n.items():
        for floor in (0.0, 1e-4):
            rc, lo, dl, jt, ok = gn_ex(api, pop, X, y, w, api.LossSpec(0, 0, 0.0), floor)
            assert rc == 0
            lo2, dl2, jt2, ok2 = np.full_like(lo, 7), np.full_like(dl, 7), np.full_like(jt, 7), np.full_like(ok, 9)
            rc2 = lib.de_eval_loss_gn(pop.ctx._h, pop._h, X.ctypes.data, N, 3, None, 1, y.ctypes.data, w.ctypes.data, lo2.ctypes.data,
                                      dl2.ctypes.data, None, jt2.ctypes.data, None, ok2.ctypes.data)
            assert rc2 == 0
            assert (lo.tobytes(), dl.tobytes(), jt.tobytes(), ok.tobytes()) == (lo2.tobytes(), dl2.tobytes(), jt2.tobytes(), ok2.tobytes())
    assert int(ng.max()) == 8 and ok.sum() > 30


def test_huber_on_a_parametric_population(api):
    dtype, P, Cn, N = np.float32, 3, 4, 700
    trees = population_trees(21, (0, 1, 2, 3), dtype, nfeatures=2, per_width=6, node_type=de.ParametricNode, nparams=P)
    pop = api.Population(trees, OPS, dtype, n_features=2, n_params=P)
    X, y, w = data(N, 2, dtype, 12)
    g = np.random.Generator(np.random.PCG64(5))
    params = np.asfortranarray(g.uniform(-1.5, 1.5, (P, Cn)).astype(dtype))
    classes = g.integers(1, Cn + 1, N)
    kw = dict(variable="both", params=params, classes=classes)
    gn = pop.eval_gauss_newton(X, y, weights=w, loss="huber", loss_param=1.3, **kw)
    out, grads, ok = pop.eval_grad(X, **kw)
    assert np.array_equal(ok, gn.ok) and all(h.shape[0] >= P + 2 for h in gn.jtj)
    worst, _ = check_bound(gn, out, grads, y, w, "huber", 1.3, dtype, min_checked=12, label="parametric")
    lo, dl, _ = pop.eval_loss_grad(X, y, weights=w, loss="huber", loss_param=1.3, **kw)
    assert lo.tobytes() == np.asarray(gn.loss).tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(dl, gn.grad))
    print(f"[gn kinds parametric] huber: worst {worst:.2f} u A over {int(np.sum(gn.has_jtj))} trees")
    pop.close()


def test_huber_on_shared_leaf_rows(api):
    dtype, F = np.float32, 60  # from 16 leaf rows on, the four waves of a workgroup share one staged copy of X
    trees = population_trees(20, range(9), dtype, nfeatures=F, per_width=4)
    pop = api.Population(trees, OPS, dtype, n_features=F)
    worst = 0.0
    for N in (321, 64):
        X, y, w = data(N, F, dtype, 30 + N)
        gn = pop.eval_gauss_newton(X, y, weights=w, loss="huber", loss_param=1.3)
        assert pop.ctx.last_kernel_name() == "de_grad_threaded_kernel<GN>"
        out, grads, _ = pop.eval_grad(X)
        wst, _ = check_bound(gn, out, grads, y, w, "huber", 1.3, dtype, min_checked=15, label=f"shared rows N={N}")
        worst = max(worst, wst)
        lo, dl, _ = pop.eval_loss_grad(X, y, weights=w, loss="huber", loss_param=1.3)
        assert lo.tobytes() == np.asarray(gn.loss).tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(dl, gn.grad))
    print(f"[gn kinds shared rows] huber: worst {worst:.2f} u A")
    pop.close()


def test_huber_on_the_flat_kernel(api, monkeypatch):
    worst = {}
    for dtype, widths, env in ((np.float64, (6, 7, 8, 2), None), (np.float32, range(9), "0")):
        if env is not None:
            monkeypatch.setenv("DE_GRAD_THREADED", env)
        trees = population_trees(18, widths, dtype, per_width=3)
        pop = api.Population(trees, OPS, dtype, n_features=3)
        X, y, w = data(515 if dtype == np.float64 else 300, 3, dtype, 6)
        gn = pop.eval_gauss_newton(X, y, weights=w, loss="huber", loss_param=1.3)
        assert pop.ctx.last_kernel_name() == "de_grad_tape_kernel<GN>"
        out, grads, _ = pop.eval_grad(X)
        worst[np.dtype(dtype).name], _ = check_bound(gn, out, grads, y, w, "huber", 1.3, dtype, min_checked=8, label="flat")
        lo, dl, _ = pop.eval_loss_grad(X, y, weights=w, loss="huber", loss_param=1.3)
        assert lo.tobytes() == np.asarray(gn.loss).tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(dl, gn.grad))
        pop.close()
    print(f"[gn kinds flat kernel] huber: worst |M - M_ref| / (u A) {worst}")


def test_float64_threaded_modules(api):
    """The shared Float64 population holds trees of 8 constants and runs the flat kernel; trees of at most 5 run the threaded modules."""
    dtype = np.float64
    trees = population_trees(18, (0, 1, 2, 3, 4, 5), dtype, per_width=4)
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y0, w = data(515, 3, dtype, 6)
    out, grads, _ = pop.eval_grad(X)
    worst = {}
    for kind, p in (("huber", 1.3), ("lp", 1.5), ("logcosh", 0.0), ("logit_margin", 0.0)):
        y = targets(y0, kind)
        gn = pop.eval_gauss_newton(X, y, weights=w, loss=kind, loss_param=p)
        assert pop.ctx.last_kernel_name() == "de_grad_threaded_kernel<GN>"
        worst[kind], _ = check_bound(gn, out, grads, y, w, kind, p, dtype, min_checked=15, label=f"f64 threaded {kind}")
        lo, dl, _ = pop.eval_loss_grad(X, y, weights=w, loss=kind, loss_param=p)
        assert lo.tobytes() == np.asarray(gn.loss).tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(dl, gn.grad))
    print(f"[gn kinds f64 threaded] worst |M - M_ref| / (u A): " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    pop.close()


def test_two_samples_per_lane(api, monkeypatch):
    monkeypatch.setenv("DE_GRAD_VS2_MIN_N", "0")  # before the population's first gradient call
    dtype = np.float32
    trees = population_trees(12, range(6), dtype, per_width=6)  # windows <= 6: the widths that have two-sample modules
    pop = api.Population(trees, OPS, dtype, n_features=3)
    vs = []
    for t in trees:  # the plan: the encoder's own answer for every tree under the same switch (form 1 = wide)
        tape, consts = de.flatten(t, OPS, dtype)
        _, meta = api.lower_tape_grad(tape, consts, 3, 1, 1, dtype=dtype)
        vs.append(int(meta[1]))
    assert vs.count(2) >= len(trees) // 2, vs
    worst = {}
    for N in (513, 1000):
        X, y0, w = data(N, 3, dtype, 7 + N)
        out, grads, _ = pop.eval_grad(X)
        for kind, p in (("huber", 1.3), ("lp", 1.5), ("L1", 0.0)):
            y = targets(y0, kind)
            gn = pop.eval_gauss_newton(X, y, weights=w, loss=kind, loss_param=p)
            assert pop.ctx.last_kernel_name() == "de_grad_threaded_kernel<GN>"
            wst, _ = check_bound(gn, out, grads, y, w, kind, p, dtype, min_checked=20, label=f"vs2 {kind} N={N}")
            worst[kind] = max(worst.get(kind, 0.0), wst)
            lo, dl, _ = pop.eval_loss_grad(X, y, weights=w, loss=kind, loss_param=p)
            assert lo.tobytes() == np.asarray(gn.loss).tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(dl, gn.grad))
    print(f"[gn kinds two samples per lane] {vs.count(2)} of {len(trees)} trees in two-sample buckets, worst " +
          ", ".join(f"{k} {v:.2f}" for k, v in worst.items()) + " u A")
    pop.close()


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------
ROBUST = (("huber", 1.3), ("logcosh", 0.0), ("logit_dist", 0.0), ("L1", 0.0), ("quantile", 0.5))


def line_population(api, dtype):
    def make():  # c0 * x1 + c1
        return de.Node(1, de.Node(3, de.Node(val=0.5), de.Node(feature=1)), de.Node(val=-0.5))

    pop = api.Population([make() for _ in range(30)], OPS, dtype, n_features=1)
    x, y = gk.outlier_line(dtype)
    return pop, np.asfortranarray(x[None, :]), y, np.tile(np.array([0.5, -0.5], dtype=dtype), 30)


def check_fit(api, pop, X, y, kind, p, consts, loss, ok, hist):
    consts, loss, ok = api._host(consts), api._host(loss), api._host(ok)
    hist = [np.asarray(api._host(h), dtype=np.float64) for h in hist]
    assert ok.all() and len(hist) == 21
    c = np.asarray(consts, dtype=np.float64).reshape(30, 2)
    if kind == "L2":
        assert (c[:, 1] > 2.5).all(), c[0]
    else:
        assert (np.abs(c[:, 0] - 2) < 0.05).all() and (np.abs(c[:, 1] - 1) < 0.3).all(), (kind, c[0])
    for a, b in zip(hist, hist[1:]):
        assert (b <= a).all(), kind  # every history column is non-increasing
    assert np.array_equal(hist[-1], np.asarray(loss, dtype=np.float64))
    lo, _, _ = pop.eval_loss_grad(X, y, loss=kind, loss_param=p)  # the population holds the accepted constants
    assert lo.astype(np.float64).tobytes() == np.asarray(loss, dtype=np.float64).tobytes()
    return c[0]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_device_fit_under_the_robust_kinds(api, dtype, where):
    import torch
    pop, X, y, c0 = line_population(api, dtype)
    Xa, ya, ca = X, y, c0
    if where == "device":
        Xa, ya, ca = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t(), torch.from_numpy(y).cuda(), torch.from_numpy(c0).cuda()
    got = {}
    for kind, p in ROBUST + (("L2", 0.0),):
        hist = []
        consts, loss, ok = pop.fit_constants_lm_device(Xa, ya, ca, iters=20, history=hist, loss=kind, loss_param=p)
        assert np.asarray(api._host(loss)).dtype == np.dtype(dtype)
        lo, _, _ = pop.eval_loss_grad(X, y, loss=kind, loss_param=p)
        assert lo.tobytes() == np.asarray(api._host(loss)).tobytes()  # ... bit for bit in the element type
        got[kind] = check_fit(api, pop, X, y, kind, p, consts, loss, ok, hist)
    print(f"[gn kinds fit] {np.dtype(dtype).name} {where} pointers, (c0, c1) after 20 iterations: " +
          ", ".join(f"{k} {v[0]:.4f} / {v[1]:.4f}" for k, v in got.items()))
    pop.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_host_loop_fit_under_the_robust_kinds(api, dtype):
    pop, X, y, c0 = line_population(api, dtype)
    got = {}
    for kind, p in ROBUST + (("L2", 0.0),):
        hist = []
        consts, loss, ok = pop.fit_constants_lm(X, y, c0, iters=20, history=hist, loss=kind, loss_param=p)
        got[kind] = check_fit(api, pop, X, y, kind, p, consts, loss, ok, hist)
    print(f"[gn kinds host loop] {np.dtype(dtype).name}, (c0, c1) after 20 iterations: " + ", ".join(f"{k} {v[0]:.4f} / {v[1]:.4f}" for k, v in got.items()))
    pop.close()


# ---- edges and refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_touch_neither_outputs_nor_constants(api):
    lib = api.library()
    for dtype in (np.float32, np.float64):
        pop, X, y, c0 = line_population(api, dtype)
        pop.set_constants(c0 * dtype(1.5))
        before = pop.constants().copy()
        K_ = api.LOSS_KINDS
        bad = [(api.LossSpec(K_["l1_hinge"], 0, 0.0), 1e-4, 7), (api.LossSpec(K_["pullback"], 0, 0.0), 1e-4, 1), (None, 1e-4, 1),
               (api.LossSpec(99, 0, 0.0), 1e-4, 1), (api.LossSpec(K_["huber"], 0, -1.0), 1e-4, 1), (api.LossSpec(K_["huber"], 1, 1.0), 1e-4, 1)]
        for f in (0.0, -1.0, float("nan"), float("inf")):
            bad += [(api.LossSpec(K_[k], 0, 0.5), f, 1) for k in ("L1", "l1_eps", "quantile")] + [(api.LossSpec(K_["lp"], 0, 1.5), f, 1)]
        if dtype == np.float32:  # a floor that rounds to 0 in the element type
            bad.append((api.LossSpec(K_["L1"], 0, 0.0), 1e-60, 1))
        for spec, floor, want in bad:
            rc, lo, dl, jt, ok = gn_ex(api, pop, X, y, None, spec, floor)
            assert rc == want, (spec and spec.kind, floor, rc)
            assert (lo == 7).all() and (dl == 7).all() and (jt == 7).all() and (ok == 9).all()
            lo[:] = 7
            hist, acc = np.full((3, 30), 7.0), np.full(30, 7, dtype=np.int32)
            opts = api.LmOpts(2, 0, 1e-3, 10.0, 0.1, 1e-12)
            rc = lib.de_fit_consts_lm_ex(pop.ctx._h, pop._h, X.ctypes.data, X.shape[1], 1, None, y.ctypes.data, None,
                                         None if spec is None else C.byref(spec), float(floor), C.byref(opts), lo.ctypes.data, ok.ctypes.data,
                                         hist.ctypes.data, acc.ctypes.data)
            assert rc == want
            assert (lo == 7).all() and (ok == 9).all() and (hist == 7).all() and (acc == 7).all()
            assert pop.constants().tobytes() == before.tobytes()
        # the floor is ignored by the kinds that do not read it, and 1e-60 is a floor in Float64
        for spec, floor in [(api.LossSpec(0, 0, 0.0), 0.0), (api.LossSpec(K_["huber"], 0, 1.3), float("nan")), (api.LossSpec(K_["lp"], 0, 2.0), 0.0),
                            (api.LossSpec(K_["logit_margin"], 0, 0.0), -1.0)] + ([(api.LossSpec(K_["L1"], 0, 0.0), 1e-60)] if dtype == np.float64 else []):
            rc, lo, dl, jt, ok = gn_ex(api, pop, X, y, None, spec, floor)
            assert rc == 0 and ok.all() and np.isfinite(jt).all()
        with pytest.raises(ValueError):
            pop.eval_gauss_newton(X, y, loss="l1_hinge")
        with pytest.raises(KeyError):
            pop.fit_constants_lm_device(X, y, loss="nope")
        assert pop.constants().tobytes() == before.tobytes()
        pop.close()


def test_incomplete_and_wide_trees_under_a_kind(api):
    dtype = np.float32
    x1 = de.Node(feature=1)

    def chain(k):  # x1 * c1 + x2 * c2 + ...: k constants
        t = de.Node(3, de.Node(feature=1), de.Node(val=0.5))
        for i in range(1, k):
            t = de.Node(1, t, de.Node(3, de.Node(feature=1 + i % 3), de.Node(val=0.25 * (i + 1))))
        return t

    div0 = de.Node(1, de.Node(4, de.Node(val=1.5), de.Node(2, x1, x1)), de.Node(val=0.5))  # 1.5 / (x1 - x1) + 0.5
    trees = population_trees(22, (1, 2, 3), dtype, per_width=2) + [div0, chain(9)]
    bad, wide = len(trees) - 2, len(trees) - 1
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = data(600, 3, dtype, 16)
    gn = pop.eval_gauss_newton(X, y, weights=w, loss="huber", loss_param=1.3)
    lo, dl, ok = pop.eval_loss_grad(X, y, weights=w, loss="huber", loss_param=1.3)
    assert not gn.ok[bad] and not gn.has_jtj[bad]
    assert np.isnan(gn.loss[bad]) and np.isnan(gn.grad[bad]).all() and np.isnan(gn.jtj[bad]).all() and gn.jtj[bad].size > 0
    assert gn.ok[wide] and not gn.has_jtj[wide] and gn.jtj[wide].shape == (9, 9) and np.isnan(gn.jtj[wide]).all()
    assert gn.grad[wide].tobytes() == dl[wide].tobytes() and np.isfinite(dl[wide]).all() and np.isfinite(gn.loss[wide])
    assert lo.tobytes() == np.asarray(gn.loss).tobytes() and np.array_equal(ok, gn.ok)
    out, grads, _ = pop.eval_grad(X)
    check_bound(gn, out, grads, y, w, "huber", 1.3, dtype, min_checked=5, label="neighbours")
    pop.close()


def test_no_samples_and_no_iterations_behave_as_under_l2(api):
    dtype = np.float32
    trees = population_trees(23, (0, 2, 3), dtype, per_width=1) + [de.Node(1, de.Node(feature=1), de.Node(val=float("inf")))]
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X0, y0 = np.zeros((3, 0), dtype=dtype, order="F"), np.zeros(0, dtype=dtype)
    a, b = pop.eval_gauss_newton(X0, y0), pop.eval_gauss_newton(X0, y0, loss="logcosh")
    assert np.array_equal(a.ok, b.ok) and b.ok.tolist() == [True, True, True, False]
    assert np.asarray(a.loss).tobytes() == np.asarray(b.loss).tobytes()
    assert all(h.tobytes() == k.tobytes() for h, k in zip(a.jtj, b.jtj)) and all(h.tobytes() == k.tobytes() for h, k in zip(a.grad, b.grad))
    before = pop.constants().copy()
    h2, hk = [], []
    _, l2, ok2 = pop.fit_constants_lm_device(X0, y0, iters=3, history=h2)
    _, lk, okk = pop.fit_constants_lm_device(X0, y0, iters=3, history=hk, loss="logcosh")
    assert l2.tobytes() == lk.tobytes() and np.array_equal(ok2, okk) and len(hk) == 4
    assert all(np.array_equal(r, s, equal_nan=True) for r, s in zip(h2, hk))
    X, y, w = data(300, 3, dtype, 9)
    hist = []
    consts, loss, ok = pop.fit_constants_lm_device(X, y, weights=w, iters=0, history=hist, loss="huber", loss_param=1.3)
    gn = pop.eval_gauss_newton(X, y, weights=w, loss="huber", loss_param=1.3)
    assert len(hist) == 1 and loss.tobytes() == np.asarray(gn.loss).tobytes() and np.array_equal(ok, gn.ok)
    assert np.array_equal(hist[0], np.asarray(loss, dtype=np.float64), equal_nan=True)
    assert pop.constants().tobytes() == before.tobytes() and consts.tobytes() == before.tobytes()
    pop.close()
