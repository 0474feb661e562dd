"""GPU tests of the fused Gauss-Newton normal equations (include/de_hip.h de_eval_loss_gn): per tree the L2 loss, its
gradient and jtj = sum_j w_j d(j) d(j)^T over the gradient rows of the mode, without the [n_grad, N] Jacobian.

The reference is numpy over the DEVICE's own `Population.eval_grad` Jacobian (same handlers, same dual rows), accumulated in long
double and rounded to float64:  H_ref[i, k] = sum w d_i d_k,  A[i, k] = sum w |d_i d_k|.  Bound for complete trees with has_jtj,
u = 2^-24 (Float32) / 2^-53 (Float64):
    |H - H_ref| <= 256 u A   entrywise
256 = two roundings per product and a wave sum of at most 128 terms in the element type, doubled for the FMA / no-FMA choice; the sums
across waves and tiles are in double.  A worst case, not a fit.  Trees whose Jacobian has a non-finite entry, or whose A is beyond a
quarter of the type's largest finite value, are compared on finiteness only; at most 5 % of a case's complete trees may be.

Every case prints the worst |H - H_ref| / (u A) it saw and the exempt share ("[gauss-newton ...]" lines of the parity report)."""
import numpy as np
import pytest

import dynamicexpressions_jl_amd as de

pytestmark = pytest.mark.gpu
K = 256.0
OPS = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))


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


def reference(J, w):
    """(H_ref, A) of one tree from its Jacobian rows J [G, N], in long double -> float64; zero weights are excluded by a select."""
    L = np.longdouble
    Jl = np.asarray(J).astype(L)
    ww = np.ones(Jl.shape[1], dtype=L) if w is None else np.asarray(w).astype(L)
    keep = ww != 0
    Jl, ww = Jl[:, keep], ww[keep]
    G = Jl.shape[0]
    H, A = np.zeros((G, G)), np.zeros((G, G))
    with np.errstate(all="ignore"):
        for i in range(G):
            for k in range(G):
                p = (ww * Jl[i]) * Jl[k]
                H[i, k], A[i, k] = float(p.sum()), float(np.abs(p).sum())
    return H, A


def check_bound(gn, grads, w, dtype, min_checked=1, label=""):
    """The bound of the module docstring for every complete tree with has_jtj; returns (worst ratio in u, exempt share)."""
    u, fmax = unit(dtype), float(np.finfo(dtype).max)
    ok, has = np.asarray(gn.ok, dtype=bool), np.asarray(gn.has_jtj, dtype=bool)
    worst, checked, exempt, complete = 0.0, 0, 0, 0
    for t in range(len(gn)):
        H = np.asarray(gn.jtj[t]).astype(np.float64)
        G = np.asarray(grads[t]).shape[0]
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
        Href, A = reference(grads[t], w)
        if not np.isfinite(np.asarray(grads[t])).all() or not np.isfinite(A).all() or A.max() > 0.25 * fmax:
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


MODES = {"constant": False, "variable": True, "both": "both"}


@pytest.mark.parametrize("dtype,sizes", [(np.float32, (1, 63, 64, 65, 255, 256, 257, 513, 1000)), (np.float64, (1, 127, 128, 129, 513))],
                         ids=["f32", "f64"])
@pytest.mark.parametrize("mode", list(MODES))
def test_gauss_newton_parity(api, dtype, sizes, mode):
    # 63 trees of <= 15 nodes, every number of constants 0 ... 8; 3 features: G = 3 (variable), 0 ... 8 (constant), 3 ... 11 (both: some wide)
    trees = population_trees(11, range(9), dtype)
    pop = api.Population(trees, OPS, dtype, n_features=3)
    ng = pop._n_grad_all(api._grad_mode(MODES[mode]))
    if mode == "constant":
        assert sorted(set(ng.tolist())) == list(range(9))
    worst, share_max, n_has = 0.0, 0.0, 0
    for N in sizes:
        for weighted in (False, True):
            X, y, w = data(N, 3, dtype, 100 + N, weighted)
            gn = pop.eval_gauss_newton(X, y, weights=w, variable=MODES[mode])
            _, grads, ok_g = pop.eval_grad(X, variable=MODES[mode])
            assert np.array_equal(gn.ok, ok_g)
            assert np.array_equal(np.asarray(gn.has_jtj), np.asarray(gn.ok) & (ng <= 8))
            lo, dl, ok_l = pop.eval_loss_grad(X, y, weights=w, loss="L2", variable=MODES[mode])
            assert np.array_equal(lo, gn.loss, equal_nan=True) and np.array_equal(ok_l, gn.ok)  # G = 0: an empty block, the loss still right
            wst, share = check_bound(gn, grads, w, dtype, min_checked=20, label=f"{mode} N={N} w={weighted}")
            worst, share_max, n_has = max(worst, wst), max(share_max, share), n_has + int(np.sum(gn.has_jtj))
    print(f"[gauss-newton parity] {np.dtype(dtype).name} {mode}: worst |H - H_ref| = {worst:.2f} u A (bound {K:.0f}), exempt share <= "
          f"{100 * share_max:.1f} %, {n_has} matrices, kernel {pop.ctx.last_kernel_name()}")
    pop.close()


def test_two_samples_per_lane(api, monkeypatch):
    monkeypatch.setenv("DE_GRAD_VS2_MIN_N", "0")  # before the population's first gradient call
    dtype = np.float32
    trees = population_trees(12, range(6), dtype, per_width=6)  # windows <= 6: the widths that have two-sample modules
    pop = api.Population(trees, OPS, dtype, n_features=3)
    # the plan: the encoder's own answer for every tree under the same switch (form 1 = wide)
    vs = []
    for t in trees:
        tape, consts = de.flatten(t, OPS, dtype)
        _, meta = api.lower_tape_grad(tape, consts, 3, 1, 1, dtype=dtype)
        vs.append(int(meta[1]))
    assert vs.count(2) >= len(trees) // 2, vs
    for N in (513, 1000):
        X, y, w = data(N, 3, dtype, 7 + N)
        gn = pop.eval_gauss_newton(X, y, weights=w)
        assert pop.ctx.last_kernel_name() == "de_grad_threaded_kernel<GN>"
        _, grads, _ = pop.eval_grad(X)
        worst, _ = check_bound(gn, grads, w, dtype, min_checked=20, label=f"vs2 N={N}")
        lo, dl, ok = pop.eval_loss_grad(X, y, weights=w)
        assert np.array_equal(lo, gn.loss, equal_nan=True) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(dl, gn.grad))
    print(f"[gauss-newton two samples per lane] {vs.count(2)} of {len(trees)} trees in two-sample buckets, worst {worst:.2f} u A")
    pop.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_same_bits_as_the_gradient_call(api, dtype):
    trees = population_trees(13, range(9), dtype, per_width=4) + de.synth.random_population(30, seed=5, node_count=20, nfeatures=3, operators=OPS, dtype=dtype)
    X, y, w = data(777, 3, dtype, 3)
    pop = api.Population(trees, OPS, dtype, n_features=3)
    rev = api.Population(trees, OPS, dtype, n_features=3, eval_context=api.EvalContext(reverse_grad=True))
    for mode in MODES.values():
        for ww in (None, w):
            lo, dl, ok = pop.eval_loss_grad(X, y, weights=ww, loss="L2", variable=mode)
            for p in (pop, rev):  # DE_OPT_REVERSE_GRAD is ignored by this call: forward duals, the default population's bits
                gn = p.eval_gauss_newton(X, y, weights=ww, variable=mode)
                assert np.array_equal(ok, gn.ok)
                assert lo.tobytes() == np.asarray(gn.loss).tobytes()
                assert all(a.tobytes() == np.asarray(b).tobytes() for a, b in zip(dl, gn.grad))
                assert "rev" not in p.ctx.last_kernel_name()
    assert ok.sum() >= 30
    pop.close()
    rev.close()


def test_exact_properties_on_device_tensors(api):
    import torch
    dtype = np.float32
    trees = population_trees(14, range(9), dtype, per_width=5)
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = data(300, 3, dtype, 9)
    w[256:] = 0
    Xd, yd, wd = torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t(), torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda()

    def bits(g):
        torch.cuda.synchronize()
        return [np.asarray(api._host(h)).tobytes() for h in g.jtj]

    a = pop.eval_gauss_newton(Xd, yd, weights=wd)
    assert all(torch.is_tensor(h) and h.is_cuda for h in a.jtj) and torch.is_tensor(a.loss) and a.has_jtj.dtype == torch.bool
    ba = bits(a)
    assert a.has_jtj.sum().item() >= 30
    for h in a.jtj:
        assert torch.equal(h, h.t()) or torch.isnan(h).all()  # exactly symmetric
    assert bits(pop.eval_gauss_newton(Xd, yd, weights=wd)) == ba  # run to run
    hst = pop.eval_gauss_newton(X, y, weights=w)  # host buffers
    assert [np.asarray(h).tobytes() for h in hst.jtj] == ba
    assert np.asarray(hst.loss).tobytes() == api._host(a.loss).tobytes()
    dbl = pop.eval_gauss_newton(Xd, yd, weights=wd * 2)  # a power of two scales every sum exactly
    for h2, h1, has in zip(dbl.jtj, a.jtj, api._host(a.has_jtj)):
        if has and h1.numel() and torch.isfinite(h1 * 2).all():
            assert torch.equal(h2, h1 * 2)
    # zero weights behind sample 256 == the 256 leading samples alone
    lead = pop.eval_gauss_newton(Xd[:, :256], yd[:256], weights=wd[:256])
    assert bits(lead) == ba
    assert api._host(lead.loss).tobytes() == api._host(a.loss).tobytes()
    pop.close()


def test_wide_trees_get_nan_and_leave_their_neighbours_alone(api):
    dtype = np.float32
    rng = de.synth.Xoshiro256ss(15)

    def chain(k):  # x1 * c1 + x2 * c2 + ... : k constants, every one with a non-trivial row
        t = de.Node(3, de.Node(feature=1), de.Node(val=0.5))
        for i in range(1, k):
            t = de.Node(1, t, de.Node(3, de.Node(feature=1 + i % 3), de.Node(val=0.25 * (i + 1))))
        return t

    trees = population_trees(16, range(9), dtype, per_width=2) + [chain(9), chain(12)] + population_trees(17, (1, 4, 8), dtype, per_width=2)
    wide = [18, 19]
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = data(600, 3, dtype, 4)
    gn = pop.eval_gauss_newton(X, y, weights=w)
    lo, dl, ok = pop.eval_loss_grad(X, y, weights=w)
    for t in wide:
        G = pop.n_grad(t, 1)
        assert G in (9, 12) and gn.ok[t] and not gn.has_jtj[t]
        assert gn.jtj[t].shape == (G, G) and np.isnan(gn.jtj[t]).all()
        assert gn.grad[t].tobytes() == dl[t].tobytes() and np.isfinite(dl[t]).all()
    assert lo.tobytes() == np.asarray(gn.loss).tobytes() and np.array_equal(ok, gn.ok)
    _, grads, _ = pop.eval_grad(X)
    worst, _ = check_bound(gn, grads, w, dtype, min_checked=15, label="wide")
    assert len(gn.lm_step(1e-3, tree=wide[0])) == 9 and not gn.lm_step(1e-3, tree=wide[0]).any()
    pop.close()


def test_float64_on_the_flat_and_on_the_threaded_kernels(api):
    dtype = np.float64
    X, y, w = data(515, 3, dtype, 6)
    worst = {}
    for name, widths, kernel in (("flat", (6, 7, 8, 2), "de_grad_tape_kernel<GN>"), ("threaded", (0, 1, 2, 3, 4, 5), "de_grad_threaded_kernel<GN>")):
        trees = population_trees(18, widths, dtype, per_width=4)
        pop = api.Population(trees, OPS, dtype, n_features=3)
        gn = pop.eval_gauss_newton(X, y, weights=w)
        assert pop.ctx.last_kernel_name() == kernel
        _, grads, _ = pop.eval_grad(X)
        worst[name], _ = check_bound(gn, grads, w, dtype, min_checked=10, label=name)
        lo, dl, ok = pop.eval_loss_grad(X, y, weights=w)
        assert lo.tobytes() == np.asarray(gn.loss).tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(dl, gn.grad))
        pop.close()
    print(f"[gauss-newton f64] worst |H - H_ref| / (u A): flat kernel {worst['flat']:.2f}, threaded modules {worst['threaded']:.2f}")


def test_flat_kernel_float32(api, monkeypatch):
    monkeypatch.setenv("DE_GRAD_THREADED", "0")
    dtype = np.float32
    trees = population_trees(19, range(9), dtype, per_width=3) + [de.Node(1, de.Node(feature=1), de.Node(val=1.0))]
    pop = api.Population(trees, OPS, dtype, n_features=3)
    X, y, w = data(300, 3, dtype, 8)
    gn = pop.eval_gauss_newton(X, y, weights=w)
    assert pop.ctx.last_kernel_name() == "de_grad_tape_kernel<GN>"
    _, grads, _ = pop.eval_grad(X)
    check_bound(gn, grads, w, dtype, min_checked=15, label="flat f32")
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
            gn = pop.eval_gauss_newton(X, y, weights=w)
            got[share, N] = [h.tobytes() for h in gn.jtj] + [np.asarray(gn.loss).tobytes()] + [g.tobytes() for g in gn.grad]
            if share == "1" and N == 321:
                _, grads, _ = pop.eval_grad(X)
                check_bound(gn, grads, w, dtype, min_checked=15, label="shared rows")
        pop.close()
    for N in (321, 64, 1000):
        assert got["0", N] == got["1", N], N


def test_parametric_population(api):
    dtype, P, Cn, N = np.float32, 3, 4, 700
    trees = population_trees(21, (0, 1, 2, 3), dtype, nfeatures=2, per_width=6, node_type=de.ParametricNode, nparams=P)
    pop = api.Population(trees, OPS, dtype, n_features=2, n_params=P)
    X, y, w = data(N, 2, dtype, 12)
    g = np.random.Generator(np.random.PCG64(5))
    params = np.asfortranarray(g.uniform(-1.5, 1.5, (P, Cn)).astype(dtype))
    classes = g.integers(1, Cn + 1, N)
    gn = pop.eval_gauss_newton(X, y, weights=w, variable="both", params=params, classes=classes)
    _, grads, ok = pop.eval_grad(X, variable="both", params=params, classes=classes)
    assert np.array_equal(ok, gn.ok) and all(h.shape[0] >= P + 2 for h in gn.jtj)
    worst, _ = check_bound(gn, grads, w, dtype, min_checked=12, label="parametric")
    lo, dl, _ = pop.eval_loss_grad(X, y, weights=w, variable="both", params=params, classes=classes)
    assert lo.tobytes() == np.asarray(gn.loss).tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(dl, gn.grad))
    print(f"[gauss-newton parametric] worst {worst:.2f} u A over {int(np.sum(gn.has_jtj))} trees")
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
        gn = pop.eval_gauss_newton(X, y, weights=w)
        _, grads, _ = pop.eval_grad(X)  # combined rows: [2, N]
        assert gn.jtj[0].shape == (2, 2) and grads[0].shape[0] == 2 and gn.has_jtj.all()
        # S H S^T against the reference formed from the COMBINED Jacobian rows, within the bound applied to the combined A
        u = unit(dtype)
        for t in range(2):
            Href, A = reference(grads[t], w)
            err = np.abs(np.asarray(gn.jtj[t]).astype(np.float64) - Href)
            assert (err <= K * u * A).all(), (t, err / (u * A))
        lo, dl, _ = pop.eval_loss_grad(X, y, weights=w)
        assert all(np.array_equal(a, b) for a, b in zip(dl, gn.grad))
        both = pop.eval_gauss_newton(X, y, weights=w, variable="both")
        assert both.jtj[0].shape == (3, 3) and np.allclose(both.jtj[0][1:, 1:], gn.jtj[0], rtol=64 * u)
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
    gn, ref = pop.eval_gauss_newton(X, y, weights=w), alone.eval_gauss_newton(X, y, weights=w)
    for t in bad:
        assert not gn.ok[t] and not gn.has_jtj[t]
        assert np.isnan(gn.loss[t]) and np.isnan(gn.grad[t]).all() and np.isnan(gn.jtj[t]).all() and gn.jtj[t].size > 0
        assert not gn.lm_step(0.0, tree=t).any()
    keep = [t for t in range(len(trees)) if t not in bad]
    assert np.array_equal(np.asarray(gn.ok)[keep], ref.ok) and ref.ok.sum() >= 4
    for i, t in enumerate(keep):
        assert gn.jtj[t].tobytes() == ref.jtj[i].tobytes() and gn.grad[t].tobytes() == ref.grad[i].tobytes()
        assert gn.loss[t:t + 1].tobytes() == ref.loss[i:i + 1].tobytes()
    pop.close()
    alone.close()


def test_no_samples(api):
    dtype = np.float32
    trees = population_trees(23, (0, 2, 3), dtype, per_width=1) + [de.Node(1, de.Node(feature=1), de.Node(val=float("inf")))]
    pop = api.Population(trees, OPS, dtype, n_features=3)
    gn = pop.eval_gauss_newton(np.zeros((3, 0), dtype=dtype, order="F"), np.zeros(0, dtype=dtype))
    assert gn.ok.tolist() == [True, True, True, False]
    assert np.array_equal(gn.loss[:3], np.zeros(3, dtype=dtype)) and np.isnan(gn.loss[3])
    assert [h.shape for h in gn.jtj] == [(0, 0), (2, 2), (3, 3), (1, 1)]
    assert not gn.jtj[1].any() and not gn.jtj[2].any() and not gn.grad[2].any() and np.isnan(gn.jtj[3]).all() and np.isnan(gn.grad[3]).all()
    pop.close()


def test_refusals(api):
    lib = api.library()
    assert lib.de_gn_max_rows() == 8
    cos1 = de.OperatorEnum(binary_operators=("+",), unary_operators=("cos",))
    tree = de.Node(1, de.Node(1, de.Node(feature=1)), de.Node(val=0.5))
    X = np.asfortranarray(np.linspace(-1, 1, 64)[None, :])
    for dtype in (np.float16, np.complex64):
        pop = api.Population([tree], cos1, dtype, n_features=1)
        with pytest.raises(api.DeviceError, match="DE_ERR_UNSUPPORTED"):
            pop.eval_gauss_newton(X.astype(dtype), np.zeros(64, dtype=dtype))
        # ... and the library itself, before it touches an output
        sentinel = np.full(4, 7, dtype=np.float64)
        okb = np.full(1, 9, dtype=np.uint8)
        Xc = np.asfortranarray(X.astype(dtype))
        rc = lib.de_eval_loss_gn(pop.ctx._h, pop._h, Xc.ctypes.data, 64, 1, None, 1, Xc.ctypes.data, None, sentinel[0:].ctypes.data,
                                 sentinel[1:].ctypes.data, None, sentinel[2:].ctypes.data, None, okb.ctypes.data)
        assert rc == 7 and (sentinel == 7).all() and okb[0] == 9
        pop.close()
    dtype = np.float32
    trees = [tree, de.Node(1, de.Node(feature=1), de.Node(val=2.0))]
    pop = api.Population(trees, cos1, dtype, n_features=1)
    Xf, y = np.asfortranarray(X.astype(dtype)), np.zeros(64, dtype=dtype)
    lo, dl, jt = np.full(2, 7, dtype=dtype), np.full(2, 7, dtype=dtype), np.full(2, 7, dtype=dtype)
    okb = np.full(2, 9, dtype=np.uint8)
    neg = np.array([0, -1], dtype=np.int64)

    def call(mode=1, jtj=jt.ctypes.data, joff=None, yp=y.ctypes.data, dlp=dl.ctypes.data, okp=okb.ctypes.data):
        return lib.de_eval_loss_gn(pop.ctx._h, pop._h, Xf.ctypes.data, 64, 1, None, mode, yp, None, lo.ctypes.data, dlp, None, jtj, joff, okp)

    for rc in (call(jtj=None), call(mode=3), call(mode=-1), call(joff=neg.ctypes.data), call(yp=None), call(dlp=None), call(okp=None)):
        assert rc == 1  # DE_ERR_INVALID_ARG
        assert (lo == 7).all() and (dl == 7).all() and (jt == 7).all() and (okb == 9).all()
    assert call() == 0 and okb.tolist() == [1, 1] and jt.tolist() == [64.0, 64.0]  # d/dc (f(x) + c) = 1, 64 samples
    with pytest.raises(ValueError):
        pop.eval_gauss_newton(Xf, y[:-1])
    pop.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_lm_step_solves_a_linear_model(api, dtype):
    g = np.random.default_rng(1)
    N = 1000
    X = np.asfortranarray(g.standard_normal((2, N)).astype(dtype))
    truth = np.array([1.5, -0.7, 0.3])
    y = (truth[0] * X[0] + truth[1] * X[1] + truth[2]).astype(dtype) + (0.1 * g.standard_normal(N)).astype(dtype)
    x1, x2 = de.Node(feature=1), de.Node(feature=2)
    c0 = np.array([0.3, 2.0, -1.0], dtype=dtype)  # arbitrary constants
    tree = de.Node(1, de.Node(1, de.Node(3, de.Node(val=c0[0]), x1), de.Node(3, de.Node(val=c0[1]), x2)), de.Node(val=c0[2]))
    pop = api.Population([tree], OPS, dtype, n_features=2)
    assert list(de.get_scalar_constants(tree)[0]) == pytest.approx(list(c0))
    Jd = np.stack([X[0], X[1], np.ones(N, dtype=dtype)]).astype(np.float64)
    cond = np.linalg.cond(Jd @ Jd.T)
    assert 1.0 < cond < 1.3  # ~1.17
    want = np.linalg.lstsq(Jd.T, y.astype(np.float64), rcond=None)[0]
    gn = pop.eval_gauss_newton(X, y)
    got = c0.astype(np.float64) + gn.lm_step(0.0, tree=0)
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"[gauss-newton lm_step] {np.dtype(dtype).name}: |c + step - lstsq| / |lstsq| = {rel / unit(dtype):.2f} u (bound {4 * K * cond:.0f} u)")
    assert rel <= 4 * K * unit(dtype) * cond
    pop.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_lm_loop_recovers_the_constants(api, dtype):
    g = np.random.default_rng(0)
    N = 1000
    x = g.uniform(-2, 2, N)
    X = np.asfortranarray(x[None, :].astype(dtype))
    y = (2.0 * np.cos(1.5 * X[0].astype(np.float64)) - 0.5).astype(dtype)
    start = np.array([1.7, 1.4, 0.0])
    starts = start[None, :] * np.concatenate([[np.ones(3)], 1 + g.uniform(-0.05, 0.05, (29, 3))])  # 30 copies, starts jittered by +-5 %

    def make(c):  # c0 * cos(c1 * x1) + c2: constants in depth-first order c0, c1, c2
        return de.Node(1, de.Node(3, de.Node(val=c[0]), de.Node(1, de.Node(3, de.Node(val=c[1]), de.Node(feature=1)))), de.Node(val=c[2]))

    trees = [make(c) for c in starts]
    pop = api.Population(trees, OPS, dtype, n_features=1)
    consts0 = np.concatenate([de.get_scalar_constants(t)[0] for t in trees]).astype(dtype)
    assert np.allclose(consts0.reshape(30, 3), starts, rtol=1e-6, atol=1e-7)
    hist = []
    consts, loss, ok = pop.fit_constants_lm(X, y, consts0, iters=10, history=hist)
    assert ok.all() and len(hist) == 11
    for a, b in zip(hist, hist[1:]):
        assert (b <= a).all()  # the accepted losses never increase
    ratio = loss / hist[0]
    print(f"[gauss-newton lm loop] {np.dtype(dtype).name}: worst loss_final / loss_initial = {ratio.max():.3g} (bound 1e-9), "
          f"constants of tree 0 {consts[:3]}")
    assert (ratio <= 1e-9).all(), ratio
    assert np.allclose(consts.reshape(30, 3), [2.0, 1.5, -0.5], atol=1e-3)
    # the population holds the accepted constants
    lo, _, _ = pop.eval_loss_grad(X, y)
    assert np.array_equal(lo.astype(np.float64), loss)
    pop.close()
