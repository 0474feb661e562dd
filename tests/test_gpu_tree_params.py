"""GPU tests of the per-tree parameter entry points (include/de_hip.h de_eval_tree_params / de_eval_loss_tree_params /
de_eval_loss_grad_tree_params, api.ParametricPopulation).

THE YARDSTICK is the existing shared-matrix path run one tree at a time with that tree's own matrix: Population([tree], n_params = 2)
.eval / .eval_loss / .eval_loss_grad_by_class.  It runs other kernels (parameter rows staged in LDS against constants patched into the
streams), so the comparison is a real one.  The flags are also checked against the CPU oracle.

    values                bit-equal for the trees made of + - * / only; tests/helpers.py parity_tolerance (the north-star bound + 8 x the
                          measured conditioning of the sample) for the others
    loss, dloss, dparams  |got - yardstick| <= 64 eps sum |terms| with the terms' conditioning under any association
                          (tests/test_gpu_loss.py's bound for the by-class gradient: path_abs_jacobian), under L2 and Huber

Shapes: 7 trees of 1 .. 15 nodes over + - * / cos exp, 2 parameters, 4 classes of which class 3 (0-based) has no sample and class 1
exactly one, N = 300 (ragged against every tile width), F = 2, ld_params = 3 > n_params, weights with zeros."""
import ctypes as C

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
from helpers import parity_tolerance, path_abs_jacobian
from oracle import oracle
from test_tree_params_host import O_, OPS, P_, V_, X_, fixture_case, isapprox

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
P, NCLS, N, F = 2, 4, 300, 2
T_PLAIN, T_NOCONST, T_LONE, T_TWICE, T_FOLD, T_DIV, T_RANDOM = range(7)
EXACT = (T_PLAIN, T_NOCONST, T_LONE, T_TWICE)  # + - * / only: IEEE-exact operators, the same bits on every path


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


def make_trees(dtype):
    rng = de.synth.Xoshiro256ss(5)
    return [
        O_("-", O_("*", X_(1), V_(1.5)), O_("/", X_(2), V_(2.5))),                       # no parameter
        O_("+", O_("+", O_("*", X_(1), P_(2)), X_(2)), P_(1)),                           # no real constant (the reference's tree)
        P_(1),                                                                           # a lone parameter leaf
        O_("+", O_("*", V_(1.5), P_(1)), O_("*", O_("-", V_(2.5), P_(1)), X_(1))),       # p1 twice, two constants
        O_("+", O_("cos", O_("*", P_(1), V_(2.0))), X_(1)),                              # a parameter inside a constant subtree
        O_("+", O_("/", X_(1), P_(2)), O_("*", O_("exp", O_("*", P_(1), X_(2))), V_(0.5))),  # a division by a parameter
        de.synth.gen_random_tree_fixed_size(15, OPS, F, rng, dtype, de.ParametricNode, P),
    ]


def make_data(dtype, seed=3):
    g = np.random.Generator(np.random.PCG64(seed))
    X = np.asfortranarray(g.uniform(0.5, 2.0, (F, N)).astype(dtype))
    y = g.standard_normal(N).astype(dtype)
    w = ((g.random(N) > 0.2) * g.uniform(0.5, 1.5, N)).astype(dtype)
    classes = g.choice([1, 3], N).astype(np.int64)  # class 4 has no sample ...
    classes[137] = 2  # ... and class 2 exactly one
    assert (classes == 2).sum() == 1 and (classes == 4).sum() == 0 and (w == 0).sum() > 20
    block = np.zeros((7, NCLS, 3), dtype=dtype)  # ld_params = 3 > n_params: the third entry of every column is poison
    block[:, :, :P] = g.uniform(0.5, 1.5, (7, NCLS, P))
    block[:, :, P] = np.nan
    params = block[:, :, :P].transpose(0, 2, 1)  # [n_trees, n_params, n_classes], a view: used in place
    return X, y, w, classes, params


class Case:
    """One dtype's population, data and yardstick results (computed once, shared by the tests, never modified)."""

    def __init__(self, api, dtype):
        self.dtype = dtype
        self.trees = make_trees(dtype)
        self.X, self.y, self.w, self.classes, self.params = make_data(dtype)
        self.pp = api.ParametricPopulation(self.trees, OPS, dtype, n_features=F, n_params=P)
        self.pp.pop.verify()
        self.single = [api.Population([t], OPS, dtype, n_features=F, n_params=P) for t in self.trees]
        self.yard_eval = [s.eval(self.X, np.asfortranarray(self.params[t]), self.classes) for t, s in enumerate(self.single)]
        self.yard_grad = {}

    def yard(self, kind):
        if kind not in self.yard_grad:
            kw = dict(loss="huber", loss_param=0.7) if kind == "huber" else dict(loss="L2")
            self.yard_grad[kind] = [s.eval_loss_grad_by_class(self.X, self.y, np.asfortranarray(self.params[t]), self.classes, weights=self.w,
                                                              variable="both", **kw) for t, s in enumerate(self.single)]
        return self.yard_grad[kind]


_cases = {}


@pytest.fixture
def case(api, dtype):
    key = np.dtype(dtype).name
    if key not in _cases:
        _cases[key] = Case(api, dtype)
    return _cases[key]


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def loss_kw(kind):
    return dict(loss="huber", loss_param=0.7) if kind == "huber" else dict(loss="L2")


# ---- values and flags ------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_values_and_flags_against_the_one_tree_populations(api, case, dtype):
    pp = case.pp
    assert pp.slot_param[T_PLAIN].tolist() == [-1, -1] and pp.slot_param[T_NOCONST].tolist() == [1, 0] and pp.slot_param[T_LONE].tolist() == [0]
    assert pp.slot_param[T_TWICE].tolist() == [-1, 0, -1, 0] and pp.slot_param[T_FOLD].tolist() == [0, -1]
    assert pp.n_consts.tolist()[:6] == [2, 0, 0, 2, 1, 1]
    before = pp.pop.constants().copy()
    out, ok = pp.eval(case.X, case.params, case.classes)
    assert out.shape == (7, N) and out.dtype == dtype and bits(pp.pop.constants()) == bits(before)
    n_bounded = 0
    for t, tree in enumerate(case.trees):
        yo, yok = case.yard_eval[t]
        tape, consts = de.flatten(tree, OPS, dtype)
        ref, rok = oracle.eval_tree_array_parametric(tape, consts, case.X, np.asfortranarray(case.params[t]), case.classes.astype(np.int32),
                                                     elementwise=True)
        assert bool(ok[t]) == bool(yok[0]) == rok, (t, ok[t], yok[0], rok)
        if not ok[t]:
            continue
        if t in EXACT:
            assert bits(out[t]) == bits(yo[0]), t
        else:
            tol = parity_tolerance(tree, OPS, case.X, dtype, params=np.asfortranarray(case.params[t]), classes0=case.classes - 1)
            err = np.abs(out[t].astype(np.float64) - yo[0].astype(np.float64))
            fin = np.isfinite(tol)
            print(f"[tree_params values {np.dtype(dtype).name} tree {t}] max err / tol {np.max(err[fin] / tol[fin]):.3g}, {int((~fin).sum())} ill-conditioned")
            assert np.all(err[fin] <= tol[fin]) and fin.mean() > 0.9, t
            n_bounded += int(fin.sum())
    assert ok[:6].all() and n_bounded > 2 * N * 0.9
    # a second call returns the same bits; grouped=True on pre-sorted input gives the bits of the unsorted call
    out2, ok2 = pp.eval(case.X, case.params, case.classes)
    assert bits(out2) == bits(out) and np.array_equal(ok, ok2)
    order = np.argsort(case.classes, kind="stable")
    out3, ok3 = pp.eval(np.asfortranarray(case.X[:, order]), case.params, case.classes[order], grouped=True)
    assert bits(out3) == bits(out[:, order]) and np.array_equal(ok, ok3)


# ---- loss, dloss, dparams --------------------------------------------------------------------------------------------------------------
def loss_terms(kind, e):
    if kind == "huber":
        d = 0.7
        return np.where(np.abs(e) <= d, e * e / 2, d * (np.abs(e) - d / 2)), np.clip(e, -d, d)
    return e * e, 2 * e


@DTYPES
@pytest.mark.parametrize("kind", ["L2", "huber"])
def test_loss_and_gradients_against_the_one_tree_populations(api, case, dtype, kind):
    pp, eps, tiny = case.pp, np.finfo(dtype).eps, 1e-300
    before = pp.pop.constants().copy()
    lo, dc, dp, ok, dl = pp.eval_loss_grad(case.X, case.y, case.params, case.classes, weights=case.w, return_slots=True, **loss_kw(kind))
    lo1, ok1 = pp.eval_loss(case.X, case.y, case.params, case.classes, weights=case.w, **loss_kw(kind))
    assert bits(pp.pop.constants()) == bits(before) and bits(pp.constants()) == bits(before[pp._slot_param_all < 0])
    assert dp.shape == (7, P, NCLS) and lo.dtype == dtype and dp.dtype == dtype and len(dc) == 7
    w64, y64 = case.w.astype(np.float64), case.y.astype(np.float64)
    worst = 0.0
    for t, tree in enumerate(case.trees):
        ylo, ydl, ydp, yok = case.yard(kind)[t]
        assert bool(ok[t]) == bool(yok[0]) == bool(ok1[t]), t
        sp = pp.slot_param[t]
        slots = dl[pp._slot_off[t]:pp._slot_off[t + 1]]
        assert len(dc[t]) == int((sp < 0).sum()) and bits(dc[t]) == bits(slots[sp < 0])
        if not ok[t]:
            assert np.isnan(lo[t]) and np.isnan(slots).all() and np.isnan(dp[t]).all()
            continue
        assert np.all(dp[t][:, 3] == 0) and not np.isnan(dp[t]).any()  # the empty class
        # the conditioning of every sum, from the yardstick population's own Jacobian (rows: parameters, features, constants)
        o, grads, okg = case.single[t].eval_grad(case.X, "both", params=np.asfortranarray(case.params[t]), classes=case.classes)
        o64, g64 = o[0].astype(np.float64), np.asarray(grads[0], dtype=np.float64)
        l, lp = loss_terms(kind, o64 - y64)
        terms = (w64 * lp)[None, :] * g64
        gabs = path_abs_jacobian(tree, OPS, case.X, "both", np.asfortranarray(case.params[t]), case.classes)
        aterms = np.abs(terms) if gabs is None else np.maximum(np.abs(terms), np.nan_to_num(np.abs(w64 * lp)[None, :] * gabs, nan=np.inf))
        lmag = np.abs(w64 * l).sum()
        for got in (lo[t], lo1[t]):
            assert abs(float(got) - float(ylo[0])) <= 64 * eps * lmag + tiny, (t, got, ylo[0])
            worst = max(worst, abs(float(got) - float(ylo[0])) / (64 * eps * lmag + tiny))
        # the real constants against the constant rows of the yardstick
        mag = aterms.sum(axis=1)
        err = np.abs(dc[t].astype(np.float64) - ydl[0][P + F:].astype(np.float64))
        assert np.all(err <= 64 * eps * mag[P + F:] + tiny), (t, dc[t], ydl[0][P + F:])
        worst = max([worst] + list(err / (64 * eps * mag[P + F:] + tiny)))
        for c in range(NCLS):
            sel = case.classes == c + 1
            cmag = aterms[:P, sel].sum(axis=1)
            err = np.abs(dp[t][:, c].astype(np.float64) - ydp[0][:, c].astype(np.float64))
            assert np.all(err <= 64 * eps * cmag + tiny), (t, c, dp[t][:, c], ydp[0][:, c])
            worst = max([worst] + list(err[cmag > 0] / (64 * eps * cmag[cmag > 0] + tiny)))
        # the parameter-slot rows of dloss equal the per-class cells summed
        for p in range(P):
            occ = np.nonzero(sp == p)[0]
            cells = dp[t][p].astype(np.float64)
            if len(occ) == 1:  # one occurrence: a cell IS the class's entry, so the row is the cells added in class order, rounded once
                acc = 0.0
                for c in range(NCLS):
                    acc = acc + cells[c]
                assert slots[occ[0]] == dtype(acc), (t, p)
            elif len(occ):
                assert abs(slots[occ].astype(np.float64).sum() - cells.sum()) <= 8 * eps * (np.abs(slots[occ]).sum() + np.abs(cells).sum()) + tiny
            err = np.abs(slots[occ].astype(np.float64).sum() - float(ydl[0][p])) if len(occ) else 0.0
            assert err <= 64 * eps * mag[p] + 8 * eps * np.abs(slots[occ]).sum() + tiny, (t, p)
    print(f"[tree_params {kind} {np.dtype(dtype).name}] worst error / bound {worst:.3g}")
    assert ok[:6].all()
    # a second call returns the same bits; grouped=True on pre-sorted input gives the bits of the unsorted call
    again = pp.eval_loss_grad(case.X, case.y, case.params, case.classes, weights=case.w, return_slots=True, **loss_kw(kind))
    order = np.argsort(case.classes, kind="stable")
    sortd = pp.eval_loss_grad(np.asfortranarray(case.X[:, order]), case.y[order], case.params, case.classes[order], weights=case.w[order],
                              grouped=True, return_slots=True, **loss_kw(kind))
    for other in (again, sortd):
        assert bits(other[0]) == bits(lo) and bits(other[2]) == bits(dp) and bits(other[4]) == bits(dl) and np.array_equal(other[3], ok)


# ---- flags -----------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_flags_empty_class_poison_and_a_cleared_flag(api, case, dtype):
    pp = case.pp
    base = pp.eval_loss_grad(case.X, case.y, case.params, case.classes, weights=case.w, return_slots=True)
    base_out = pp.eval(case.X, case.params, case.classes)
    # an Inf in the empty class's column: never read — the flags and every number are untouched
    poisoned = np.array(case.params)
    poisoned[:, :, 3] = np.inf
    got = pp.eval_loss_grad(case.X, case.y, poisoned, case.classes, weights=case.w, return_slots=True)
    assert np.array_equal(got[3], base[3]) and bits(got[0]) == bits(base[0]) and bits(got[2]) == bits(base[2]) and bits(got[4]) == bits(base[4])
    got_out = pp.eval(case.X, poisoned, case.classes)
    assert bits(got_out[0]) == bits(base_out[0]) and np.array_equal(got_out[1], base_out[1])

    def others_unchanged(got, bad):
        keep = [t for t in range(7) if t != bad]
        assert not got[3][bad] and np.array_equal(got[3][keep], base[3][keep])
        assert np.isnan(got[0][bad]) and np.isnan(got[2][bad]).all() and np.isnan(got[4][pp._slot_off[bad]:pp._slot_off[bad + 1]]).all()
        assert bits(got[0][keep]) == bits(base[0][keep]) and bits(got[2][keep]) == bits(base[2][keep])
        for t in keep:
            a, b = pp._slot_off[t], pp._slot_off[t + 1]
            assert bits(got[4][a:b]) == bits(base[4][a:b])

    # an Inf in a used class (the one-sample class) clears that tree's flag alone
    bad = np.array(case.params)
    bad[T_NOCONST, 0, 1] = np.inf
    others_unchanged(pp.eval_loss_grad(case.X, case.y, bad, case.classes, weights=case.w, return_slots=True), T_NOCONST)
    lo, ok = pp.eval_loss(case.X, case.y, bad, case.classes, weights=case.w)
    assert not ok[T_NOCONST] and np.isnan(lo[T_NOCONST]) and ok[[0, 2, 3, 4, 5]].all()
    out, ok = pp.eval(case.X, bad, case.classes)
    assert not ok[T_NOCONST] and np.isnan(out[T_NOCONST]).all() and bits(out[[0, 2, 3, 4, 5]]) == bits(base_out[0][[0, 2, 3, 4, 5]])
    # a division by a parameter that is 0 in one class only
    zero = np.array(case.params)
    zero[T_DIV, 1, 2] = 0.0
    others_unchanged(pp.eval_loss_grad(case.X, case.y, zero, case.classes, weights=case.w, return_slots=True), T_DIV)
    out, ok = pp.eval(case.X, zero, case.classes)
    assert not ok[T_DIV] and ok[:5].all()


# ---- the real constants and update -----------------------------------------------------------------------------------------------------
@DTYPES
def test_real_constants_and_update(api, dtype):
    """set_constants / constants cover the real constants only (get_scalar_constants order); update() leaves what a fresh population of
    the resulting members is."""
    from dynamicexpressions_jl_amd.node import get_scalar_constants, set_scalar_constants
    trees = make_trees(dtype)
    X, y, w, classes, params = make_data(dtype)
    pp = api.ParametricPopulation(trees, OPS, dtype, n_features=F, n_params=P)
    want = np.concatenate([get_scalar_constants(t)[0] for t in trees]).astype(dtype)
    assert bits(pp.constants()) == bits(want) and pp.n_consts.sum() == want.size
    scaled = [t.copy() for t in trees]
    for t in scaled:
        cs, refs = get_scalar_constants(t)
        set_scalar_constants(t, (cs.astype(dtype) * dtype(1.25)).astype(np.float64), refs)
    pp.set_constants(want * dtype(1.25))
    fresh = api.ParametricPopulation(scaled, OPS, dtype, n_features=F, n_params=P)
    a, b = pp.eval_loss_grad(X, y, params, classes, weights=w, return_slots=True), fresh.eval_loss_grad(X, y, params, classes, weights=w, return_slots=True)
    assert bits(a[0]) == bits(b[0]) and bits(a[2]) == bits(b[2]) and bits(a[4]) == bits(b[4]) and np.array_equal(a[3], b[3])
    assert bits(pp.constants()) == bits(fresh.constants())
    with pytest.raises(ValueError, match="wrong number"):
        pp.set_constants(want[:-1])
    # replace members 1 and 4 (their slot counts change: 2 -> 4 and 2 -> 1)
    new = [scaled[T_TWICE].copy(), scaled[T_LONE].copy()]
    pp.update([T_NOCONST, T_FOLD], new)
    members = list(scaled)
    members[T_NOCONST], members[T_FOLD] = new
    fresh2 = api.ParametricPopulation(members, OPS, dtype, n_features=F, n_params=P)
    assert [s.tolist() for s in pp.slot_param] == [s.tolist() for s in fresh2.slot_param] and bits(pp.constants()) == bits(fresh2.constants())
    a, b = pp.eval_loss_grad(X, y, params, classes, weights=w, return_slots=True), fresh2.eval_loss_grad(X, y, params, classes, weights=w, return_slots=True)
    assert bits(a[0]) == bits(b[0]) and bits(a[2]) == bits(b[2]) and bits(a[4]) == bits(b[4]) and np.array_equal(a[3], b[3])
    oa, ob = pp.eval(X, params, classes), fresh2.eval(X, params, classes)
    good = np.nonzero(oa[1])[0]
    assert np.array_equal(oa[1], ob[1]) and bits(oa[0][good]) == bits(ob[0][good])
    for q in (pp, fresh, fresh2):
        q.close()


# ---- torch device tensors --------------------------------------------------------------------------------------------------------------
@DTYPES
def test_torch_device_tensors_give_the_bits_of_the_numpy_call(api, torch, case, dtype):
    pp = case.pp
    Xd = torch.from_numpy(np.ascontiguousarray(case.X.T)).cuda().t()
    yd, wd, cd = torch.from_numpy(case.y).cuda(), torch.from_numpy(case.w).cuda(), torch.from_numpy(case.classes).cuda()
    pd = torch.from_numpy(np.ascontiguousarray(case.params)).cuda()
    a = pp.eval_loss_grad(case.X, case.y, case.params, case.classes, weights=case.w, loss="huber", loss_param=0.7, return_slots=True)
    b = pp.eval_loss_grad(Xd, yd, pd, cd, weights=wd, loss="huber", loss_param=0.7, return_slots=True)
    assert all(x.is_cuda for x in (b[0], b[2], b[3], b[4])) and all(x.is_cuda for x in b[1])
    assert bits(b[0].cpu().numpy()) == bits(a[0]) and bits(b[2].cpu().numpy()) == bits(a[2]) and bits(b[4].cpu().numpy()) == bits(a[4])
    assert np.array_equal(b[3].cpu().numpy(), a[3]) and all(bits(u.cpu().numpy()) == bits(v) for u, v in zip(b[1], a[1]))
    lo_a, ok_a = pp.eval_loss(case.X, case.y, case.params, case.classes, weights=case.w)
    lo_b, ok_b = pp.eval_loss(Xd, yd, pd, cd, weights=wd)
    assert lo_b.is_cuda and bits(lo_b.cpu().numpy()) == bits(lo_a) and np.array_equal(ok_b.cpu().numpy(), ok_a)
    out_a, oka = pp.eval(case.X, case.params, case.classes)
    out_b, okb = pp.eval(Xd, pd, cd)
    assert out_b.is_cuda and okb.is_cuda and np.array_equal(okb.cpu().numpy(), oka)
    good = np.nonzero(oka)[0]
    assert bits(out_b.cpu().numpy()[good]) == bits(out_a[good])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def raw_calls(api, pop, n_slots, dtype):
    """The three entry points on sentinel-filled outputs: [(status, every output still the sentinel)]."""
    lib, nt = api.library(), pop.n_trees
    es = np.dtype(dtype)
    X = np.asfortranarray(np.ones((F, 8), dtype=es))
    y = np.ones(8, dtype=es)
    starts = np.array([0, 8], dtype=np.int64)
    sp = np.full(max(n_slots, 1), -1, dtype=np.int32)
    prm = np.ones((nt, 1, P), dtype=es)
    tp = api.TreeParams(prm.ctypes.data, P, 1, P, 0, starts.ctypes.data, sp.ctypes.data)
    spec = api.loss_spec("L2")
    res = []

    def fresh():
        return (np.full((nt, 8), 7, dtype=es), np.full(nt, 7, dtype=es), np.full(max(n_slots, 1), 7, dtype=es), np.full((nt, 1, P), 7, dtype=es),
                np.full(nt, 7, dtype=np.uint8))

    out, lo, dl, dp, ok = fresh()
    rc = lib.de_eval_tree_params(pop.ctx._h, pop._h, X.ctypes.data, 8, F, C.byref(tp), out.ctypes.data, 8, ok.ctypes.data)
    res.append((rc, bool((out == 7).all() and (ok == 7).all())))
    out, lo, dl, dp, ok = fresh()
    rc = lib.de_eval_loss_tree_params(pop.ctx._h, pop._h, X.ctypes.data, 8, F, C.byref(tp), y.ctypes.data, None, C.byref(spec), lo.ctypes.data,
                                      ok.ctypes.data)
    res.append((rc, bool((lo == 7).all() and (ok == 7).all())))
    out, lo, dl, dp, ok = fresh()
    rc = lib.de_eval_loss_grad_tree_params(pop.ctx._h, pop._h, X.ctypes.data, 8, F, C.byref(tp), y.ctypes.data, None, C.byref(spec),
                                           lo.ctypes.data, dl.ctypes.data, None, dp.ctypes.data, ok.ctypes.data)
    res.append((rc, bool((lo == 7).all() and (dl == 7).all() and (dp == 7).all() and (ok == 7).all())))
    return res


def test_refusals_leave_outputs_and_constants_untouched(api):
    plain = O_("+", O_("*", X_(1), V_(1.5)), V_(0.25))
    # an F16 population
    pp = api.ParametricPopulation([plain], OPS, np.float16, n_features=F, n_params=P)
    before = pp.pop.constants().copy()
    assert raw_calls(api, pp.pop, 2, np.float16) == [(7, True)] * 3 and bits(pp.pop.constants()) == bits(before)
    with pytest.raises(api.DeviceError, match="unsupported request.*DE_F16"):
        pp.eval(np.ones((F, 4), dtype=np.float16), np.ones((1, P, 1), dtype=np.float16), np.ones(4, dtype=np.int64))
    pp.close()
    # a program with n_params != 0
    pop = api.Population([O_("+", P_(1), V_(0.5))], OPS, np.float64, n_features=F, n_params=P)
    before = pop.constants().copy()
    assert raw_calls(api, pop, 1, np.float64) == [(7, True)] * 3 and bits(pop.constants()) == bits(before)
    pop.close()
    # a program made by de_program_create_cse
    Gn = de.GraphNode
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    sh = Gn(1, Gn(2, Gn(feature=1), Gn(val=0.75)))
    pop = api.Population([Gn(1, Gn(1, sh, Gn(2, sh, Gn(feature=2))), Gn(val=-0.4))], ops, np.float64, n_features=F)
    before = pop.constants().copy()
    n_slots = int(pop._slots_per_tree.sum())
    assert raw_calls(api, pop, n_slots, np.float64) == [(7, True)] * 3 and bits(pop.constants()) == bits(before)
    pop.close()
    # invalid arguments on a good program: reserved != 0, a slot_param entry out of range, class_starts that do not end at N
    pp = api.ParametricPopulation([plain], OPS, np.float64, n_features=F, n_params=P)
    lib = api.library()
    X, starts, sp = np.asfortranarray(np.ones((F, 8))), np.array([0, 8], dtype=np.int64), np.array([-1, -1], dtype=np.int32)
    prm, out, ok = np.ones((1, 1, P)), np.full((1, 8), 7.0), np.full(1, 7, dtype=np.uint8)

    def call(tp):
        return lib.de_eval_tree_params(pp.ctx._h, pp.pop._h, X.ctypes.data, 8, F, C.byref(tp) if tp else None, out.ctypes.data, 8, ok.ctypes.data)

    good = (prm.ctypes.data, P, 1, P, 0, starts.ctypes.data, sp.ctypes.data)
    assert call(api.TreeParams(*good)) == 0 and ok[0] == 1 and np.all(out == 1.75)
    out[...], ok[...] = 7.0, 7
    bad_sp, bad_starts = np.array([-1, 2], dtype=np.int32), np.array([0, 7], dtype=np.int64)
    for tp in (None, api.TreeParams(*good[:4], 1, *good[5:]), api.TreeParams(*good[:6], bad_sp.ctypes.data), api.TreeParams(*good[:6], None),
               api.TreeParams(*good[:5], bad_starts.ctypes.data, good[6]), api.TreeParams(*good[:5], None, good[6]),
               api.TreeParams(good[0], P - 1, *good[2:])):
        assert call(tp) == 1 and np.all(out == 7.0) and ok[0] == 7
    pp.close()


# ---- the reference's fit on the device -------------------------------------------------------------------------------------------------
def test_fit_bfgs_reference_case_on_the_device(api):
    """test/test_parametric_expression.jl:140-199 through ParametricPopulation.fit_bfgs with the device evaluator (Float64, as the
    reference): loss < 1e-5, initial loss > 0.1, parameters isapprox the true ones — at the fixture's 60 iterations."""
    tree, ops, X, classes, true_p, init_p, y, case = fixture_case()
    ex = api.ParametricExpression(tree, ops, init_p)
    other = api.ParametricExpression(tree.copy(), ops, true_p)  # a second member that starts at the answer
    pp = api.ParametricPopulation([ex, other], ops, np.float64, n_features=2, n_params=2)
    hist = []
    consts, ps, lo, ok = pp.fit_bfgs(X, y, classes=classes, iters=case["iters"], history=hist)
    print(f"[tree_params fit, device] loss {hist[0][0]:.3g} -> {lo[0]:.3g}, {int(pp.bfgs_accepts[0])} accepted steps of {case['iters']}, "
          f"parameter error {np.linalg.norm(ps[0] - true_p):.3g}")
    assert ok.all() and consts.size == 0
    assert lo[0] < case["expect"]["minimum_below"] and hist[0][0] > case["expect"]["init_loss_above"]
    assert isapprox(ps[0], true_p) and pp.params is ps
    assert lo[1] == 0 and bits(ps[1]) == bits(true_p) and pp.bfgs_accepts[1] == 0
    lo2, _, _, ok2 = pp.eval_loss_grad(X, y, classes=classes)
    assert bits(lo2) == bits(lo) and ok2.all()
    pp.close()
