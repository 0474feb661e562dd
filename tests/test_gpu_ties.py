"""GPU tests of the tied device fits (include/de_hip.h de_fit_consts_{bfgs,lbfgs,nm,lm}_tied): a shared GraphNode
constant is ONE unknown of the optimiser kernels; pack / unpack / fold kernels (csrc/de_ties.hip) sit around every evaluation.

The kernels run csrc/de_ties.h, the code behind the host hooks (tests/test_ties_host.py holds those to `_sum_occurrence_rows` /
`gn_combine`, what the host loops compute), and the optimiser kernels are the untied fits', which equal their host loops bit for bit.  So
`fit_constants_*_device(tied=True)` and the host loop `fit_constants_*` agree BIT FOR BIT on a GraphNode population: constants, loss,
flags, every history row and the accept counts.  For Levenberg-Marquardt the host loop is built here from `eval_gauss_newton` (which
returns the combined gradient and S H S^T) and `api.lm_solve_host`, the step kernel's own arithmetic, with `fit_constants_lm`'s rule."""
import ctypes as C

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import test_gpu_gauss_newton as GN
from test_gpu_lm import chain, dev_X, offsets

pytestmark = pytest.mark.gpu
OPS = GN.OPS  # binary + - * / (1 .. 4), unary cos exp (1, 2)
Gn = de.GraphNode
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
FITS = ("bfgs", "lbfgs", "nm", "lm")
N_RAGGED = 2053  # more than one tile, with a ragged tail


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


def bits(api, a):
    return np.ascontiguousarray(api._host(a)).tobytes()


# ---- the populations ---------------------------------------------------------------------------------------------------------------------------
def shared_population():
    """(trees, slots per tree, unknowns per tree): two DAGs with a shared constant, a plain tree, a tree without constants and a tree that
    is incomplete from the start (it shares its constant too)."""
    x1, x2 = Gn(feature=1), Gn(feature=2)
    c, c2 = Gn(val=0.75), Gn(val=0.3)
    sh = Gn(1, Gn(3, x1, c))  # cos(x1 * c)
    leaf = Gn(1, Gn(1, sh, Gn(3, sh, Gn(3, c, x1))), c2)  # sh + sh (c x1) + c2: c fills three slots
    sh2 = Gn(1, Gn(3, x1, Gn(val=0.75)))  # the DAG of test_gpu_nm.py::test_cse_program: a shared subtree that carries a constant
    sub = Gn(1, Gn(1, sh2, Gn(3, sh2, Gn(3, Gn(val=-0.4), x2))), Gn(val=0.3))
    plain = Gn(1, Gn(3, Gn(val=1.25), x1), Gn(val=-0.5))
    bare = Gn(1, x1, Gn(1, x2))
    k = Gn(val=1.5)
    div0 = Gn(1, Gn(4, k, Gn(2, x1, x1)), k)  # k / (x1 - x1) + k
    return [leaf, sub, plain, bare, div0], [4, 4, 2, 0, 2], [2, 3, 2, 0, 1]


def sum_tree(S, U):
    """sum_i c_i x_j over S terms whose first U constants are distinct nodes and whose last S - U reuse the first ones."""
    cs = [Gn(val=0.25 + 0.05 * i * (-1) ** i) for i in range(U)]
    feats = [Gn(feature=1), Gn(feature=2)]
    t = None
    for i in range(S):
        term = Gn(3, cs[i if i < U else i - U], feats[(i + i // U) % 2])
        t = term if t is None else Gn(1, t, term)
    return t


EDGES = [(36, 32), (36, 33), (48, 40), (8, 5), (9, 5)]


def make(api, trees, dtype, slots=None, unknowns=None):
    pop = api.Population(trees, OPS, dtype, n_features=2)
    if slots is not None:
        assert pop._occ is not None and pop._slots_per_tree.tolist() == slots and pop.n_consts.tolist() == unknowns
    return pop


def raw_slots(api, pop):
    out = np.empty(int(pop._slots_per_tree.sum()), dtype=pop.dtype)
    assert api.library().de_program_get_consts(pop._h, out.ctypes.data if out.size else None) == 0
    return out


def ties_hold(api, pop, consts):
    """The program's slots are unique[tie[s]] bit for bit, tree by tree; de_program_verify is clean."""
    slots, tie = raw_slots(api, pop), pop._tie_map()
    s_at, u_at = offsets(pop._slots_per_tree), offsets(pop.n_consts)
    consts = api._host(consts)
    for t in range(pop.n_trees):
        want = consts[u_at[t]:u_at[t + 1]][tie[s_at[t]:s_at[t + 1]]]
        assert slots[s_at[t]:s_at[t + 1]].tobytes() == np.ascontiguousarray(want).tobytes(), t
    pop.verify()


# ---- the host loops ----------------------------------------------------------------------------------------------------------------------------
def host_lm(api, pop, X, y, w, c0, iters, lam0=1e-3, up=10.0, down=0.1, lam_min=1e-12, **kind):
    """`fit_constants_lm`'s loop with the step of the device: `lm_solve_host` (Cholesky) of eval_gauss_newton's combined system, the trial
    T(double(c) + step) where a step was produced, else the bits of c."""
    dtype, nt, f64 = pop.dtype, pop.n_trees, np.float64
    at = offsets(pop.n_consts)
    consts = np.array(c0, dtype=dtype).copy()

    def evaluate(cs):
        pop.set_constants(cs)
        gn = pop.eval_gauss_newton(X, y, weights=w, **kind)
        return (gn.loss.copy(), gn.ok.copy(), np.asarray(gn.has_jtj).copy(), [np.array(g) for g in gn.grad], [np.array(h) for h in gn.jtj])

    loss, ok, has, grad, jtj = evaluate(consts)
    lam, acc, hist = np.full(nt, float(lam0)), np.zeros(nt, dtype=np.int32), [loss.astype(f64)]
    for _ in range(iters):
        trial = consts.copy()
        for t in range(nt):
            a, b = at[t], at[t + 1]
            if has[t] and 1 <= b - a <= api.GN_MAX_ROWS:
                step, produced = api.lm_solve_host(jtj[t], grad[t], lam[t])
                if produced:
                    trial[a:b] = (consts[a:b].astype(f64) + step).astype(dtype)
        loss_t, ok_t, has_t, grad_t, jtj_t = evaluate(trial)
        for t in range(nt):
            if has[t] and has_t[t] and float(loss_t[t]) < float(loss[t]):
                consts[at[t]:at[t + 1]] = trial[at[t]:at[t + 1]]
                loss[t], ok[t], grad[t], jtj[t] = loss_t[t], ok_t[t], grad_t[t], jtj_t[t]
                lam[t] = max(lam[t] * down, lam_min)
                acc[t] += 1
            else:
                lam[t] = lam[t] * up
        hist.append(loss.astype(f64))
    pop.set_constants(consts)
    return consts, loss, ok, hist, acc


def host_fit(api, pop, which, X, y, w, c0, iters, opts, kind):
    """(consts, loss, ok, history, counts) of the host loop."""
    hist = []
    if which == "lm":
        cs, lo, ok, hist, acc = host_lm(api, pop, X, y, w, c0, iters, **opts, **kind)
        return cs, lo, ok.astype(bool), hist, acc
    fit = getattr(pop, f"fit_constants_{which}")
    cs, lo, ok = fit(X, y, c0, weights=w, iters=iters, history=hist, **opts, **kind)
    acc = {"bfgs": "bfgs_accepts", "lbfgs": "lbfgs_accepts", "nm": "nm_improves"}[which]
    return cs, lo, ok, hist, np.asarray(getattr(pop, acc)).copy()


def device_fit(api, pop, which, X, y, w, c0, iters, opts, kind, **more):
    hist = []
    fit = getattr(pop, f"fit_constants_{which}_device")
    opts = {k: v for k, v in opts.items() if k != "lam_min"}
    cs, lo, ok = fit(X, y, c0, weights=w, iters=iters, history=hist, tied=True, **opts, **kind, **more)
    acc = {"bfgs": "bfgs_accepts", "lbfgs": "lbfgs_accepts", "nm": "nm_improves", "lm": "lm_accepts"}[which]
    return cs, lo, ok, hist, getattr(pop, acc)


def same_fit(api, dev, host, label):
    cd, ld, okd, hd, ad = dev
    ch, lh, okh, hh, ah = host
    assert bits(api, cd) == bits(api, ch), label
    assert bits(api, ld) == bits(api, lh) and np.array_equal(api._host(okd).astype(bool), np.asarray(okh).astype(bool)), label
    assert len(hd) == len(hh) and all(bits(api, a) == bits(api, b) for a, b in zip(hd, hh)), label
    assert api._host(ad).dtype == np.int32 and bits(api, ad) == bits(api, np.asarray(ah, dtype=np.int32)), label


def reproduces_the_loss(api, pop, which, X, y, w, kind, loss):
    if which == "bfgs":
        lo = pop.eval_loss_grad(X, y, weights=w, **kind)[0]
    elif which == "lm":
        lo = pop.eval_gauss_newton(X, y, weights=w, **kind).loss
    else:
        lo = pop.eval_loss(X, y, weights=w, **kind)[0]
    assert bits(api, lo) == bits(api, loss), which


SETTINGS = {  # (iterations, non-default options, the other loss kind)
    "bfgs": (12, dict(step0=0.5, shrink=0.3, c1=1e-3, curv=1e-6), dict(loss="huber", loss_param=1.3)),
    "lbfgs": (12, dict(memory=3, step0=0.5, shrink=0.3, c1=1e-3, curv=1e-6), dict(loss="huber", loss_param=1.3)),
    "nm": (40, dict(a=0.05, b=0.4, f_tol=1e-9), dict(loss="huber", loss_param=1.3)),
    "lm": (8, dict(lam0=1e-2, up=4.0, down=0.25), dict(loss="huber", loss_param=1.3)),
}


# ---- 1. and 2. the trajectory, bit for bit; the ties hold ---------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("which", FITS)
@pytest.mark.parametrize("variant", ["defaults-L2", "options-other-kind"])
def test_tied_device_fit_follows_the_host_loop_bit_for_bit(api, dtype, which, variant):
    trees, slots, unknowns = shared_population()
    pop = make(api, trees, dtype, slots, unknowns)
    assert pop._tie_map().tolist() == [0, 0, 0, 1, 0, 0, 1, 2, 0, 1, 0, 0]
    X, y, w = GN.data(N_RAGGED, 2, dtype, 21)
    iters, opts, kind = SETTINGS[which]
    if variant == "defaults-L2":
        opts, kind = {}, {}
    c0 = pop.constants().copy()
    host = host_fit(api, pop, which, X, y, w, c0, iters, opts, kind)
    dev = device_fit(api, pop, which, X, y, w, c0, iters, opts, kind)
    same_fit(api, dev, host, (which, variant))
    cd, ld, okd, hd, ad = dev
    assert cd.dtype == dtype and cd.size == sum(unknowns) and len(hd) == iters + 1 and okd.tolist() == [True, True, True, True, False]
    assert bits(api, pop.constants()) == bits(api, cd)
    ties_hold(api, pop, cd)
    reproduces_the_loss(api, pop, which, X, y, w, kind, ld)
    # the trees with a shared constant were fitted: strictly below their starting loss; the others as the untied fits leave them
    assert hd[-1][0] < hd[0][0] and hd[-1][1] < hd[0][1] and ad[0] > 0 and ad[1] > 0, (hd[0], hd[-1], ad)
    at = offsets(pop.n_consts)
    assert cd[at[4]:at[5]].tobytes() == c0[at[4]:at[5]].tobytes() and np.isnan(ld[4]) and ad[3] == 0 and ad[4] == 0
    print(f"[ties] {which} {np.dtype(dtype).name} {variant}: bit-equal to the host loop over {iters} iterations; loss {hd[0][:3]} -> {hd[-1][:3]}, "
          f"counts {np.asarray(ad).tolist()}")
    pop.close()


@DTYPES
def test_one_sample(api, dtype):
    trees, slots, unknowns = shared_population()
    pop = make(api, trees, dtype, slots, unknowns)
    X, y, w = GN.data(1, 2, dtype, 8)
    c0 = pop.constants().copy()
    for which in ("bfgs", "lm"):
        host = host_fit(api, pop, which, X, y, w, c0, 5, {}, {})
        dev = device_fit(api, pop, which, X, y, w, c0, 5, {}, {})
        same_fit(api, dev, host, which)
        ties_hold(api, pop, dev[0])
    pop.close()


# ---- 3. the identity: the untied twin's bits -----------------------------------------------------------------------------------------------------
def raw_fit(api, pop, which, X, y, w, tie="untied", opts=None, spec=None, N=None, y_null=False, ok_null=False, rows=None, iters=6):
    """The raw call on sentinel-filled outputs: (status, every output still the sentinel, (loss, ok, history, counts))."""
    lib, nt = api.library(), pop.n_trees
    Opts = {"bfgs": api.BfgsOpts, "lbfgs": api.LbfgsOpts, "nm": api.NmOpts, "lm": api.LmOpts}[which]
    default = {"bfgs": (iters, 0, 1.0, 0.5, 1e-4, 1e-8), "lbfgs": (iters, 0, 4, 0, 1.0, 0.5, 1e-4, 1e-8), "nm": (iters, 0, 0.025, 0.5, 0.0),
               "lm": (iters, 0, 1e-3, 10.0, 0.1, 1e-12)}[which]
    opts = Opts(*default) if opts is None else opts
    rows = (opts.iters if opts.iters >= 0 else 0) + 1 if rows is None else rows
    spec = api.LossSpec(0, 0, 0.0) if spec is None else spec
    lo, ok = np.full(2 * max(nt, 1), 7, dtype=np.float64), np.full(max(nt, 1), 9, dtype=np.uint8)
    hist, acc = np.full(rows * max(nt, 1), 7.0), np.full(max(nt, 1), 9, dtype=np.int32)
    N = X.shape[1] if N is None else N
    head = [pop.ctx._h, pop._h, X.ctypes.data, N, X.shape[0], None, None if y_null else y.ctypes.data, w.ctypes.data if w is not None else None,
            C.byref(spec)]
    if which == "lm":
        head.append(1e-4)
    head.append(C.byref(opts))
    untied = isinstance(tie, str)
    if not untied:
        head.append(tie.ctypes.data if tie is not None else None)
    name = f"de_fit_consts_{'lm_ex' if which == 'lm' and untied else which}{'' if untied else '_tied'}"
    rc = getattr(lib, name)(*head, lo.ctypes.data, None if ok_null else ok.ctypes.data, hist.ctypes.data, acc.ctypes.data)
    untouched = bool((lo == 7).all() and (ok == 9).all() and (hist == 7).all() and (acc == 9).all())
    return rc, untouched, (lo.tobytes(), ok.tobytes(), hist.tobytes(), acc.tobytes())


@DTYPES
def test_identity_map_gives_the_untied_twins_bits(api, dtype):
    trees = GN.population_trees(63, (0, 1, 2, 3, 8), dtype, nfeatures=2, per_width=2) + [chain(9), chain(33)]
    pop = api.Population(trees, OPS, dtype, n_features=3)
    assert pop._occ is None
    X, y, w = GN.data(N_RAGGED, 3, dtype, 31)
    c0 = pop.constants().copy()
    identity = np.concatenate([np.arange(n, dtype=np.int32) for n in pop.n_consts])
    for which in FITS:
        got = {}
        for label, tie in (("untied", "untied"), ("NULL", None), ("identity", identity)):
            pop.set_constants(c0)
            rc, untouched, outs = raw_fit(api, pop, which, X, y, w, tie)
            assert rc == 0 and not untouched, (which, label)
            got[label] = outs + (pop.constants().tobytes(),)
        assert got["NULL"] == got["untied"] and got["identity"] == got["untied"], which
        assert got["untied"][4] != c0.tobytes()
    pop.close()


# ---- 4. the edges of the limits ------------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("which", FITS)
def test_edges_of_the_limits(api, dtype, which):
    pop = make(api, [sum_tree(S, U) for S, U in EDGES], dtype, [S for S, _ in EDGES], [U for _, U in EDGES])
    X, y, w = GN.data(N_RAGGED, 2, dtype, 33)
    c0 = pop.constants().copy()
    iters = {"bfgs": 6, "lbfgs": 6, "nm": 45, "lm": 4}[which]
    host = host_fit(api, pop, which, X, y, w, c0, iters, {}, {})
    dev = device_fit(api, pop, which, X, y, w, c0, iters, {}, {})
    same_fit(api, dev, host, which)
    cd, ld, okd, hd, ad = dev
    ties_hold(api, pop, cd)
    reproduces_the_loss(api, pop, which, X, y, w, {}, ld)
    assert okd.all()
    fitted = {"bfgs": [0, 3, 4], "nm": [0, 3, 4], "lbfgs": [0, 1, 2, 3, 4], "lm": [3]}[which]  # U <= 32; U <= 4096; S <= 8
    at = offsets(pop.n_consts)
    lo0 = hd[0]
    for t in range(len(EDGES)):
        moved = cd[at[t]:at[t + 1]].tobytes() != c0[at[t]:at[t + 1]].tobytes()
        if t in fitted:
            assert moved and ad[t] > 0 and hd[-1][t] < lo0[t], (which, t, EDGES[t])
        else:  # the bits of the constants, the loss of the evaluation
            assert not moved and ad[t] == 0 and all(h[t] == lo0[t] for h in hd), (which, t, EDGES[t])
    print(f"[ties edges] {which} {np.dtype(dtype).name}: (S, U) = {EDGES}, fitted {fitted}, counts {np.asarray(ad).tolist()}")
    pop.close()


# ---- 5. refusals through the raw calls -----------------------------------------------------------------------------------------------------------
def test_refusals(api):
    lib = api.library()
    dtype = np.float32
    trees, slots, unknowns = shared_population()
    pop = make(api, trees, dtype, slots, unknowns)
    X, y, w = GN.data(64, 2, dtype, 3)
    good = pop._tie_map().copy()
    before = raw_slots(api, pop)
    nan = float("nan")

    def kept():
        return raw_slots(api, pop).tobytes() == before.tobytes()

    bad_maps = {0: [0, 0, 2, 1], 1: [0, -1, 1, 2], 2: [1, 0], 4: [0, 2]}  # a gap, a negative id, a later id first, a jump
    bad_opts = {"bfgs": api.BfgsOpts(3, 0, 1.0, 1.5, 1e-4, 1e-8), "lbfgs": api.LbfgsOpts(3, 0, 99, 0, 1.0, 0.5, 1e-4, 1e-8),
                "nm": api.NmOpts(3, 0, 0.0, 0.0, 0.0), "lm": api.LmOpts(3, 0, nan, 10.0, 0.1, 1e-12)}
    s_at = offsets(pop._slots_per_tree)
    for which in FITS:
        for t, ids in bad_maps.items():
            tie = good.copy()
            tie[s_at[t]:s_at[t + 1]] = ids
            assert raw_fit(api, pop, which, X, y, w, tie)[:2] == (1, True) and kept(), (which, t)
            msg = lib.de_last_error(pop.ctx._h).decode()
            assert f"tree {t}" in msg and f"de_fit_consts_{which}_tied" in msg, msg
        assert raw_fit(api, pop, which, X, y, w, good, opts=bad_opts[which])[:2] == (1, True) and kept(), which
        assert raw_fit(api, pop, which, X, y, w, good, spec=api.LossSpec(99, 0, 0.0))[:2] == (1, True) and kept(), which
        assert raw_fit(api, pop, which, X, y, w, good, y_null=True)[:2] == (1, True) and kept(), which
        assert raw_fit(api, pop, which, X, y, w, good, ok_null=True)[:2] == (1, True) and kept(), which
        # iters = 0 and N = 0: nothing is written to the program, every history row is the first
        zero = {"bfgs": (0, 0, 1.0, 0.5, 1e-4, 1e-8), "lbfgs": (0, 0, 4, 0, 1.0, 0.5, 1e-4, 1e-8), "nm": (0, 0, 0.025, 0.5, 0.0),
                "lm": (0, 0, 1e-3, 10.0, 0.1, 1e-12)}[which]
        Opts = type(bad_opts[which])
        assert raw_fit(api, pop, which, X, y, w, good, opts=Opts(-1, *zero[1:]))[:2] == (1, True) and kept(), which
        rc, untouched, outs = raw_fit(api, pop, which, X, y, w, good, opts=Opts(*zero))
        assert rc == 0 and not untouched and kept(), which
        rc, untouched, outs = raw_fit(api, pop, which, X, y, w, good, N=0, iters=3)
        hist = np.frombuffer(outs[2]).reshape(4, pop.n_trees)
        assert rc == 0 and kept() and all(h.tobytes() == hist[0].tobytes() for h in hist), which
        assert not np.frombuffer(outs[3], dtype=np.int32).any()
        # ... and the same call with good arguments runs and moves the constants
        rc, untouched, outs = raw_fit(api, pop, which, X, y, w, good)
        assert rc == 0 and not untouched and not kept(), which
        pop.ctx.check(lib.de_program_set_consts(pop._h, before.ctypes.data))
        assert kept()
    # the Python surface: tied with scaled / wide is refused before the constants are touched; tied=False keeps its refusal
    for call, kw in ((pop.fit_constants_bfgs_device, dict(scaled=True)), (pop.fit_constants_nm_device, dict(scaled=True)),
                     (pop.fit_constants_lm_device, dict(scaled=True)), (pop.fit_constants_lm_device, dict(wide=True))):
        with pytest.raises(ValueError, match="tied"):
            call(X, y, np.zeros(int(pop.n_consts.sum()), dtype=dtype), tied=True, **kw)
        assert kept()
    for which in FITS:
        with pytest.raises(ValueError, match=f"fit_constants_{which}"):
            getattr(pop, f"fit_constants_{which}_device")(X, y)
    pop.close()
    # evaluation-only populations: DE_ERR_UNSUPPORTED, everything untouched
    cos1 = de.OperatorEnum(binary_operators=("+",), unary_operators=("cos",))
    tree = de.Node(1, de.Node(1, de.Node(feature=1)), de.Node(val=0.5))
    X1 = np.asfortranarray(np.linspace(-1, 1, 64)[None, :])
    for other in (np.float16, np.complex64):
        pop = api.Population([tree], cos1, other, n_features=1)
        held = pop.constants().copy()
        Xc = np.asfortranarray(X1.astype(other))
        for which in FITS:
            for tie in (None, np.zeros(1, dtype=np.int32)):
                assert raw_fit(api, pop, which, Xc, Xc, None, tie)[:2] == (7, True), (other, which)
            assert pop.constants().tobytes() == held.tobytes()
        pop.close()


# ---- 6. device pointers --------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_device_pointers_give_the_bits_of_host_buffers(api, torch, dtype):
    trees, slots, unknowns = shared_population()
    pop = make(api, trees + [sum_tree(9, 5)], dtype, slots + [9], unknowns + [5])
    X, y, w = GN.data(N_RAGGED, 2, dtype, 41)
    c0 = pop.constants().copy()
    Xd, yd, wd = dev_X(torch, X), torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda()
    for which in FITS:
        iters = 30 if which == "nm" else 6
        host = device_fit(api, pop, which, X, y, w, c0, iters, {}, {})
        host = tuple(np.asarray(v).copy() if not isinstance(v, list) else v for v in host)
        dev = device_fit(api, pop, which, Xd, yd, wd, torch.from_numpy(c0).cuda(), iters, {}, {})
        assert all(torch.is_tensor(v) and v.is_cuda for v in (dev[0], dev[1], dev[2], dev[4], dev[3][0])), which
        same_fit(api, dev, host, which)
        ties_hold(api, pop, dev[0])
    pop.close()
