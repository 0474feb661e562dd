"""GPU tests of de_program_set_consts_device / Population.set_constants(device tensor).

The yardstick everywhere: the SAME population given the SAME values through de_program_set_consts.  Equality is bit for bit and NaN
positions must be equal (sign and payload of a NaN are not compared); no tolerance: the same kernels read the same
immediates.  Rows and Jacobians of incomplete trees are only partly written on the device (early exit at tree granularity), so those are
compared where the flag is set; flags, losses, loss gradients, statistics and Gauss-Newton blocks everywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_, G_ = de.Node, de.GraphNode
# binary 1 + 2 - 3 * 4 / 5 ^; unary 1 cos 2 exp (hot handlers) 3 sqrt 4 tanh (cold operators)
OPS = de.OperatorEnum(binary_operators=("+", "-", "*", "/", "^"), unary_operators=("cos", "exp", "sqrt", "tanh"))
ADD, SUB, MUL, DIV, POW = 1, 2, 3, 4, 5
COS, EXP, SQRT, TANH = 1, 2, 3, 4


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    _api.library()
    return _api


@pytest.fixture(scope="module")
def torch():
    import torch as _torch
    return _torch


def c(v=0.5, T=N_):
    return T(val=v)


def x(i, T=N_):
    return T(feature=i)


def fold_trees():
    """Every route a constant subtree takes, one tree each; trees without constants between them."""
    return [
        N_(ADD, x(1), x(2)),                                                                            # no constant
        N_(MUL, x(1), N_(SUB, N_(MUL, N_(ADD, c(1.5), c(-2.0)), c(0.75)), N_(DIV, c(3.0), c(7.0)))),   # + - * /: the host route
        N_(ADD, x(2), N_(COS, N_(MUL, c(1.25), c(-0.4)))),                                             # cos of an operator: de_fold_kernel
        N_(SUB, x(1), N_(TANH, N_(SQRT, N_(ADD, c(2.0), c(0.3))))),                                    # cold operators
        N_(MUL, x(1), N_(COS, c(-0.456))),                                                              # a hot unary on a constant LEAF (the cosf quirk)
        N_(MUL, N_(EXP, c(0.3)), x(2)),
        N_(COS, x(1)),                                                                                  # no constant
        N_(ADD, x(1), N_(POW, c(1.5), c(2.0))),                                                         # inner branch: flagged under early exit only
        N_(ADD, x(1), N_(DIV, c(1.0), c(3.0))),                                                         # division (by zero below)
        N_(MUL, N_(ADD, x(1), c(0.1)), N_(SUB, x(2), c(-0.7))),                                         # plain constant operands, no subtree
        N_(EXP, N_(MUL, c(0.2), N_(ADD, x(1), c(1.0)))),
    ]


def special_values(dtype, consts, g):
    """Copies of `consts` whose subtrees overflow, underflow to subnormals, divide by zero and give NaN; and with Inf / NaN constants."""
    big, tiny = (1e38, 1e-30) if dtype == np.float32 else (1e308, 1e-300)
    sets = []
    for fill in ((big, big), (tiny, 1e-10), (1.0, 0.0), (0.0, 0.0), (np.inf, 1.0), (np.nan, 2.0), (-big, big)):
        v = consts.copy()
        at = g.choice(len(v), size=max(len(v) // 3, 1), replace=False)
        v[at[::2]] = fill[0]
        v[at[1::2]] = fill[1]
        sets.append(v.astype(dtype))
    return sets


def host(v):
    return v.detach().cpu().numpy() if type(v).__module__.startswith("torch") else np.asarray(v)


def same(a, b, what, rows=None):
    a, b = host(a), host(b)
    assert a.shape == b.shape, f"{what}: shapes {a.shape} {b.shape}"
    if rows is not None:
        a, b = a[rows], b[rows]
    if a.dtype.kind != "f":
        assert np.array_equal(a, b), what
        return
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), f"{what}: NaN positions"
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    assert np.array_equal(np.ascontiguousarray(a[~na]).view(u), np.ascontiguousarray(b[~nb]).view(u)), f"{what}: bits"


def dev_X(torch, X):
    return torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t()


def run_all(pop, X, y, kw=None, grads=True, by_class=False):
    """Outputs and flags of every entry point: (name, array, flags the rows are compared under | None) triples."""
    kw = kw or {}
    res = []
    out, ok = pop.eval(X, **kw)
    res += [("eval ok", ok, None), ("eval rows", out, host(ok))]
    for name, lkw in (("L2", {}), ("huber", dict(loss="huber", loss_param=0.7))):
        loss, okl = pop.eval_loss(X, y, **lkw, **kw)
        res += [(f"eval_loss {name} ok", okl, None), (f"eval_loss {name}", loss, None)]
    fs, okf = pop.eval_fit_stats(X, y, **kw)
    res += [("fit_stats ok", okf, None), ("fit_stats", np.stack([fs.mean_p, fs.m2_p, fs.cov]), None)]
    if not grads:
        return res
    loss, dls, okg = pop.eval_loss_grad(X, y, **kw)
    res += [("loss_grad ok", okg, None), ("loss_grad loss", loss, None), ("loss_grad dloss", np.concatenate([host(d) for d in dls] + [np.zeros(0, host(loss).dtype)]), None)]
    assert np.all(np.isnan(host(loss)[~host(okg)])), "loss is NaN where ok is 0"
    for d, k in zip(dls, host(okg)):
        assert k or np.all(np.isnan(host(d))), "gradient is NaN where ok is 0"
    gn = pop.eval_gauss_newton(X, y, **kw)
    res += [("gn ok", gn.ok, None), ("gn loss", gn.loss, None), ("gn grads", np.concatenate([host(d) for d in gn.grad] + [np.zeros(0, host(loss).dtype)]), None)]
    res += [("gn jtj", np.concatenate([host(m).reshape(-1) for m in gn.jtj] + [np.zeros(0, host(loss).dtype)]), None)]
    for variable in (False, True, "both"):
        o, gs, okj = pop.eval_grad(X, variable, **kw)
        okh = host(okj)
        res += [(f"eval_grad {variable} ok", okj, None), (f"eval_grad {variable} rows", o, okh)]
        live = [host(gq).reshape(-1) for gq, k in zip(gs, okh) if k]
        res += [(f"eval_grad {variable} jac", np.concatenate(live + [np.zeros(0, host(o).dtype)]), None)]
    if not kw:
        o, do, okd = pop.eval_diff(X, 1)
        res += [("eval_diff ok", okd, None), ("eval_diff rows", o, host(okd)), ("eval_diff drows", do, host(okd))]
    if by_class:
        lo, dl, dp, okc = pop.eval_loss_grad_by_class(X, y, kw["params"], kw["classes"], variable="both", grouped=True)
        res += [("by_class ok", okc, None), ("by_class loss", lo, None), ("by_class dparams", dp, None),
                ("by_class dloss", np.concatenate([host(d) for d in dl] + [np.zeros(0, host(lo).dtype)]), None)]
    return res


def compare(ra, rb, tag):
    assert [r[0] for r in ra] == [r[0] for r in rb]
    for (name, a, rows_a), (_, b, rows_b) in zip(ra, rb):
        if rows_a is not None:
            assert np.array_equal(rows_a, rows_b), f"{tag}: {name}: flags"
        same(a, b, f"{tag}: {name}", rows=rows_a)


def tree_consts(trees, ops, dtype):
    parts = [de.flatten(t, ops, dtype)[1] for t in trees]
    return np.concatenate(parts + [np.zeros(0, dtype)]).astype(dtype)


def twin(api, torch, trees, ops, dtype, X, y, value_sets, ec=None, F=None, P=0, kw=None, grads=True, by_class=False, device_path=True, tag=""):
    """The same population twice: one set through the host, one from a device tensor; every value set, every entry point, twice — the
    first round builds the lazily made streams behind a device set, the later ones find them on the device."""
    F = F or X.shape[0]
    mk = lambda: api.Population(trees, ops, dtype, n_features=F, n_params=P, eval_context=ec or api.EvalContext())
    ph, pd = mk(), mk()
    Xd, yd = dev_X(torch, X), torch.from_numpy(y).cuda()
    dkw = {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in (kw or {}).items()}
    if "params" in dkw:
        dkw["params"] = torch.from_numpy(np.ascontiguousarray((kw["params"]).T)).cuda().t()
    try:
        for i, vals in enumerate(value_sets):
            ph.set_constants(vals)
            pd.set_constants(torch.from_numpy(vals).cuda())
            if len(vals):
                assert pd.consts_on_device_path == device_path, f"{tag}: device path"
            assert not ph.consts_on_device_path
            compare(run_all(ph, Xd, yd, dkw, grads, by_class), run_all(pd, Xd, yd, dkw, grads, by_class), f"{tag} set {i}")
        same(ph.constants(), pd.constants(), f"{tag}: constants()")
        same(ph.constants(), pd.constants(device=True), f"{tag}: constants(device=True)")
        pd.set_constants(torch.from_numpy(value_sets[0]).cuda())
        ph.set_constants(value_sets[0])
        pd.verify()
        assert ph.stream_hash() == pd.stream_hash(), f"{tag}: stream_hash"
        for t in range(0, len(trees), max(len(trees) // 7, 1)):
            assert np.array_equal(ph.dump(t), pd.dump(t)) and ph.meta(t) == pd.meta(t), f"{tag}: dump of tree {t}"
    finally:
        ph.close()
        pd.close()


def base_case(dtype, N, seed=0xC0DE, n_random=90, F=5):
    g = np.random.Generator(np.random.PCG64(seed))
    trees = fold_trees() + de.synth.random_population(n_random, seed=seed, node_count=15, nfeatures=F, operators=OPS, dtype=dtype)
    X = np.asfortranarray((g.standard_normal((F, N)) * 1.3).astype(dtype))
    y = g.standard_normal(N).astype(dtype)
    consts = tree_consts(trees, OPS, dtype)
    return trees, X, y, consts, g


@pytest.mark.parametrize("N", [1, 257, 1000])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_every_entry_point_has_the_bits_of_the_host_path(api, torch, dtype, N):
    """One-wave programs, every fold route in one population, trees without constants between the others; plain and special values
    (overflow, subnormal results, division by zero, NaN, Inf / NaN constants in checked and unchecked positions)."""
    trees, X, y, consts, g = base_case(dtype, N)
    sets = [(consts * dtype(1.25) - dtype(0.5)).astype(dtype)] + (special_values(dtype, consts, g) if N == 257 else []) + [consts]
    twin(api, torch, trees, OPS, dtype, X, y, sets, tag=f"base N={N}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_without_early_exit_and_with_reverse_accumulation(api, torch, dtype):
    """early_exit=False: the inner-branch fold x + (c1 ^ c2) and the EE-only constant checks do not clear the flag; reverse_grad=True: the
    reverse stream has sites of its own (trees of >= 8 gradient rows take it by the rule; DE_LOSS_GRAD_REVERSE is not set)."""
    trees, X, y, consts, g = base_case(dtype, 257, seed=0xE1)
    wide = [N_(ADD, N_(MUL, c(0.1 * k), x(1 + k % 5)), N_(COS, N_(MUL, c(1.0 + k), x(1)))) for k in range(1, 3)]
    for _ in range(3):  # sums of them: 8 and 16 constants per tree
        wide = [N_(ADD, a.copy(), b.copy()) for a, b in zip(wide, wide[::-1])]
    trees = trees + wide
    consts = tree_consts(trees, OPS, dtype)
    sets = [consts] + special_values(dtype, consts, g)[:5]
    twin(api, torch, trees, OPS, dtype, X, y, sets, ec=api.EvalContext(early_exit=False), tag="no early exit")
    twin(api, torch, [t for t in trees[-2:]] * 40, OPS, dtype, X, y, [tree_consts(trees[-2:] * 40, OPS, dtype) * dtype(0.5), tree_consts(trees[-2:] * 40, OPS, dtype)],
         ec=api.EvalContext(reverse_grad=True), tag="reverse")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_wave_groups_and_shared_leaf_rows(api, torch, dtype):
    """20 features: the eval program runs in wave groups (a stream variant per wave, var_stride records apart) and the threaded gradient
    program shares its leaf rows (four variants gt_stride records apart): every variant carries the device's constants."""
    F, N = 20, 257
    trees, X, y, consts, g = base_case(dtype, N, seed=0x77, n_random=70, F=F)
    pop = api.Population(trees, OPS, dtype, n_features=F)
    assert pop.meta(0)["waves"] > 1, pop.meta(0)
    pop.close()
    twin(api, torch, trees, OPS, dtype, X, y, [(consts * dtype(0.9)).astype(dtype), consts], tag="wide X")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_parametric_population_by_class_and_in_wave_groups(api, torch, dtype):
    g = np.random.Generator(np.random.PCG64(5))
    P, C, N = 8, 5, 257
    trees = de.synth.random_population(63, seed=0x3A7E, node_count=15, dtype=dtype, node_type=de.ParametricNode, nparams=P)
    X = np.asfortranarray((g.standard_normal((5, N)) * 1.2).astype(dtype))
    y = g.standard_normal(N).astype(dtype)
    params = np.asfortranarray(g.standard_normal((P, C)).astype(dtype))
    classes = np.sort(g.integers(1, C + 1, N)).astype(np.int64)
    consts = tree_consts(trees, de.synth.BENCH_OPERATORS, dtype)
    pop = api.Population(trees, de.synth.BENCH_OPERATORS, dtype, n_features=5, n_params=P)
    assert pop.meta(0)["waves"] > 1, pop.meta(0)  # (staged parameter rows)
    pop.close()
    for ec in (api.EvalContext(), api.EvalContext(reverse_grad=True)):
        twin(api, torch, trees, de.synth.BENCH_OPERATORS, dtype, X, y, [(consts + dtype(0.25)).astype(dtype), consts], ec=ec, P=P,
             kw=dict(params=params, classes=classes), by_class=True, tag=f"parametric reverse={ec.reverse_grad}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_graph_population_with_shared_constants(api, torch, dtype):
    """A shared constant is ONE constant to the caller: the fan-out to occurrence slots is a device gather; the eval program is the CSE
    lowering (one instruction for several occurrence slots)."""
    from test_lowering import random_graph
    rng = de.synth.Xoshiro256ss(77)
    trees = []
    for k in range(30):
        s = G_(val=0.5 + 0.01 * k)
        sub = G_(MUL, s, G_(feature=1 + k % 3))
        trees.append(G_(ADD, G_(COS, sub), G_(MUL, sub, G_(ADD, s, G_(val=-1.0 - k)))))
    trees += [random_graph(rng, OPS, 6 + i % 10, 3, 1 + i % 3, dtype) for i in range(40)]
    g = np.random.Generator(np.random.PCG64(8))
    X = np.asfortranarray(g.standard_normal((3, 257)).astype(dtype))
    y = g.standard_normal(257).astype(dtype)
    pop = api.Population(trees, OPS, dtype, n_features=3)
    assert pop._occ is not None and int(pop.n_consts.sum()) < int(pop._slots_per_tree.sum())
    n = int(pop.n_consts.sum())
    pop.close()
    sets = [g.standard_normal(n).astype(dtype), (g.standard_normal(n) * 3).astype(dtype)]
    twin(api, torch, trees, OPS, dtype, X, y, sets, tag="graph")


def test_float64_tree_wider_than_the_threaded_windows(api, torch):
    """More gradient rows than the Float64 threaded modules have windows for: the flat gradient kernel reads d_gcode, which has sites of
    its own."""
    terms = [N_(MUL, c(0.3 * k - 1.0), N_(COS, N_(ADD, x(1 + k % 2), c(0.1 * k)))) for k in range(1, 25)]
    t = terms[0]
    for u in terms[1:]:
        t = N_(ADD, t, u)
    trees = [t.copy() for _ in range(63)] + fold_trees()
    g = np.random.Generator(np.random.PCG64(4))
    X = np.asfortranarray(g.standard_normal((2, 257)))
    y = g.standard_normal(257)
    consts = tree_consts(trees, OPS, np.float64)
    twin(api, torch, trees, OPS, np.float64, X, y, [consts * 0.5, consts], tag="wide f64 tree")


@pytest.mark.parametrize("n_consts", [0, 1, 63, 65, 300])
def test_total_constant_counts(api, torch, n_consts):
    def term(k):
        return N_(MUL, x(1 + k % 2), c(0.25 + k))

    trees, left = [], n_consts
    for k in range(100):  # up to four constants in every other tree (15 nodes), trees without constants between them
        m = min(4, left) if k % 4 != 3 else 0
        left -= m
        ts = [term(4 * k + i) for i in range(m)]
        while len(ts) > 1:
            ts = [N_(ADD, ts[i], ts[i + 1]) if i + 1 < len(ts) else ts[i] for i in range(0, len(ts), 2)]
        trees.append(ts[0] if ts else N_(ADD, x(1), x(2)))
    assert left == 0
    g = np.random.Generator(np.random.PCG64(n_consts))
    X = np.asfortranarray(g.standard_normal((2, 257)).astype(np.float32))
    y = g.standard_normal(257).astype(np.float32)
    vals = g.standard_normal(n_consts).astype(np.float32)
    twin(api, torch, trees, OPS, np.float32, X, y, [vals, vals * np.float32(2)], tag=f"{n_consts} constants")


def test_empty_population(api, torch):
    pop = api.Population([], OPS, np.float32, n_features=2)
    pop.set_constants(torch.zeros(0, dtype=torch.float32, device="cuda"))
    assert pop.constants().size == 0 and pop.constants(device=True).numel() == 0
    pop.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_order_of_operations(api, torch, dtype):
    trees, X, y, consts, g = base_case(dtype, 1000, seed=0xAB)
    Xd, yd = dev_X(torch, X), torch.from_numpy(y).cuda()
    c1, c2, c3 = (consts * dtype(0.5)).astype(dtype), (consts + dtype(1)).astype(dtype), special_values(dtype, consts, g)[2]
    mk = lambda: api.Population(trees, OPS, dtype, n_features=5)
    ph, pd = mk(), mk()
    dev = lambda v: torch.from_numpy(v).cuda()
    # a device set on a fresh program, then the first gradient call: the lazily built streams carry the device's constants
    pd.set_constants(dev(c1))
    ph.set_constants(c1)
    assert pd.consts_on_device_path
    compare(run_all(ph, Xd, yd), run_all(pd, Xd, yd), "fresh")
    # device -> host -> device
    pd.set_constants(c2)
    assert not pd.consts_on_device_path
    ph.set_constants(c2)
    compare(run_all(ph, Xd, yd, grads=False), run_all(pd, Xd, yd, grads=False), "host set behind a device set")
    pd.set_constants(dev(c3))
    ph.set_constants(c3)
    assert pd.consts_on_device_path
    compare(run_all(ph, Xd, yd), run_all(pd, Xd, yd), "device set behind a host set")
    # two device sets back to back, an evaluation queued between them, no synchronisation; the caller's buffer is reused at once
    buf = dev(c1)
    pd.set_constants(buf)
    out1, ok1 = pd.eval(Xd)
    l1, d1, k1 = pd.eval_loss_grad(Xd, yd)
    buf.copy_(dev(c2))
    pd.set_constants(buf)
    buf.fill_(7)
    out2, ok2 = pd.eval(Xd)
    l2, d2, k2 = pd.eval_loss_grad(Xd, yd)
    for vals, out, ok, lo, dl, kk in ((c1, out1, ok1, l1, d1, k1), (c2, out2, ok2, l2, d2, k2)):
        ph.set_constants(vals)
        ro, rk = ph.eval(Xd)
        rl, rd, rkk = ph.eval_loss_grad(Xd, yd)
        same(ok, rk, "queued eval: flags")
        same(out, ro, "queued eval: rows", rows=host(rk))
        same(kk, rkk, "queued loss_grad: flags")
        same(lo, rl, "queued loss_grad: loss")
        same(torch.cat(list(dl)), torch.cat(list(rd)), "queued loss_grad: dloss")
    same(pd.constants(), c2, "constants() behind two sets")
    # device set -> update of some trees -> a fresh creation of the resulting population with those constants
    pd.set_constants(dev(c1))
    ids = [1, 4, 17, len(trees) - 1]
    new = [N_(ADD, x(1), N_(MUL, c(2.5), c(-1.5))), N_(COS, x(2)), N_(MUL, c(0.3), N_(EXP, c(0.2))), N_(SUB, x(1), c(9.0))]
    pd.update(ids, new)
    now = list(trees)
    off = np.concatenate([[0], np.cumsum([len(de.flatten(t, OPS, dtype)[1]) for t in trees])])
    parts = [c1[off[t]:off[t + 1]] for t in range(len(trees))]
    for i, t in zip(ids, new):
        now[i] = t
        parts[i] = de.flatten(t, OPS, dtype)[1].astype(dtype)
    fresh = api.Population(now, OPS, dtype, n_features=5)
    fresh.set_constants(np.concatenate(parts).astype(dtype))
    assert fresh.stream_hash() == pd.stream_hash(), "update behind a device set"
    compare(run_all(fresh, Xd, yd), run_all(pd, Xd, yd), "update behind a device set")
    for p in (ph, pd, fresh):
        p.close()


def deep_constant_tree(with_cos):
    t = N_(COS, c(0.01)) if with_cos else c(0.01)
    for k in range(20):  # right-leaning: every leaf is on the stack before the first addition
        t = N_(ADD, c(0.02 * k), t)
    return N_(MUL, x(1), t)


@pytest.mark.parametrize("kind", ["turbo", "deep host-route fold", "deep kernel-route fold", "f16", "complex"])
def test_staged_programs_give_the_host_path_results(api, torch, kind):
    g = np.random.Generator(np.random.PCG64(12))
    ec, dtype, ops = api.EvalContext(), np.float32, OPS
    trees = fold_trees() + de.synth.random_population(60, seed=0x51, node_count=15, operators=OPS)
    if kind == "turbo":
        ec = api.EvalContext(turbo=True)
    elif kind.startswith("deep"):
        trees = trees + [deep_constant_tree(kind == "deep kernel-route fold")]
    elif kind == "f16":
        dtype = np.float16
    else:
        dtype, ops = np.complex64, de.synth.BENCH_OPERATORS
        trees = de.synth.random_population(63, seed=0x52, node_count=15)
    N = 257
    X = (g.standard_normal((5, N)) * 0.8).astype(np.float32)
    X = np.asfortranarray(X.astype(dtype) if dtype != np.complex64 else (X + 1j * X[::-1]).astype(dtype))
    consts = tree_consts(trees, ops, dtype)
    vals = [(consts * dtype(0.5)).astype(dtype), consts]
    mk = lambda: api.Population(trees, ops, dtype, n_features=5, eval_context=ec)
    ph, pd = mk(), mk()
    Xd = dev_X(torch, X)
    for v in vals:
        ph.set_constants(v)
        pd.set_constants(torch.from_numpy(v).cuda())
        assert not pd.consts_on_device_path, kind
        (o1, k1), (o2, k2) = ph.eval(Xd), pd.eval(Xd)
        same(k1, k2, f"{kind}: flags")
        a, b = host(o1)[host(k1)], host(o2)[host(k1)]
        if dtype == np.complex64:
            a, b = a.view(np.float32), b.view(np.float32)
        elif dtype == np.float16:
            a, b = a.astype(np.float32), b.astype(np.float32)  # (exact: the comparison below is still bit for bit)
        same(a, b, f"{kind}: rows")
        if kind in ("turbo", "deep host-route fold", "deep kernel-route fold"):
            y = torch.from_numpy(g.standard_normal(N).astype(np.float32)).cuda()
            (l1, d1, q1), (l2, d2, q2) = ph.eval_loss_grad(Xd, y), pd.eval_loss_grad(Xd, y)
            same(q1, q2, f"{kind}: loss_grad flags")
            same(l1, l2, f"{kind}: loss")
            same(torch.cat(list(d1)), torch.cat(list(d2)), f"{kind}: dloss")
    same(host(ph.constants()).view(np.uint8), host(pd.constants(device=True)).view(np.uint8), f"{kind}: constants")
    assert ph.stream_hash() == pd.stream_hash()
    ph.close()
    pd.close()


def test_refusals_come_before_any_work(api, torch):
    import ctypes as C
    trees, X, y, consts, g = base_case(np.float32, 257)
    pop = api.Population(trees, OPS, np.float32, n_features=5)
    Xd = dev_X(torch, X)
    before = [host(v) for v in pop.eval(Xd)]
    lib = api.library()
    hostbuf = np.ascontiguousarray(consts + 1)
    rc = lib.de_program_set_consts_device(pop._h, hostbuf.ctypes.data)
    assert rc == 1 and "de_program_set_consts" in lib.de_last_error(pop.ctx._h).decode()
    assert lib.de_program_set_consts_device(pop._h, None) == 1
    with pytest.raises(ValueError):
        pop.set_constants(torch.zeros(len(consts) + 1, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        pop.set_constants(torch.zeros(len(consts), dtype=torch.float64, device="cuda"))
    after = [host(v) for v in pop.eval(Xd)]
    same(before[1], after[1], "flags unchanged")
    same(before[0], after[0], "rows unchanged", rows=before[1])
    same(pop.constants(), consts, "constants unchanged")
    assert not pop.consts_on_device_path
    pop.close()


def test_plain_library_in_a_child_process(api):
    """The same comparison against csrc/libde_hip_plain.so (DE_HIP_LIB), a process of its own."""
    plain = os.path.join(ROOT, "dynamicexpressions.jl_amd", "csrc", "libde_hip_plain.so")
    assert os.path.exists(plain), "csrc/libde_hip_plain.so is missing: run __graft_entry__.build()"
    code = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_consts_device as T
from dynamicexpressions_jl_amd import api
assert api.LIB_PATH.endswith("libde_hip_plain.so")
trees, X, y, consts, g = T.base_case(np.float32, 257)
T.twin(api, torch, trees, T.OPS, np.float32, X, y, [consts * np.float32(0.5)] + T.special_values(np.float32, consts, g)[:3] + [consts], tag="plain")
print("PLAIN OK")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DE_HIP_LIB=plain), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "PLAIN OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["one wave", "wide X", "reverse", "wide trees", "parametric"])
def test_calls_whose_streams_exist_run_from_the_device_side_alone(api, torch, dtype, kind, monkeypatch, capfd):
    """Once an entry point's streams exist, a device set followed by that entry point never touches the host side: the streams (chained
    records and wave variants, d_gcode, every d_gtcode variant, d_rtcode) and the initial flags are the ones the kernels of the device
    path wrote.  The host function reports its phases on stderr under DE_DEBUG_TIMING: no such line may appear — and one does as soon as
    the host side is asked for (constants())."""
    monkeypatch.setenv("DE_DEBUG_TIMING", "1")
    ec, P, kw, ops = api.EvalContext(), 0, {}, OPS
    g = np.random.Generator(np.random.PCG64(21))
    N, F = 257, 5
    if kind == "wide X":
        F = 20
    trees = fold_trees() + de.synth.random_population(60, seed=0x99, node_count=15, nfeatures=F, operators=OPS, dtype=dtype)
    if kind in ("reverse", "wide trees"):
        terms = [N_(MUL, c(0.3 * k - 1.0), N_(COS, N_(ADD, x(1 + k % 2), c(0.1 * k)))) for k in range(1, 9)]
        t = terms[0]
        for u in terms[1:]:
            t = N_(ADD, t, u)
        trees = [t.copy() for _ in range(63)] + fold_trees()[1:4]  # 16 constants a tree: reverse accumulation by the rule; no Float64 window
        if kind == "reverse":
            ec = api.EvalContext(reverse_grad=True)
    if kind == "parametric":
        P, ops = 8, de.synth.BENCH_OPERATORS
        trees = de.synth.random_population(63, seed=0x3A7E, node_count=15, dtype=dtype, node_type=de.ParametricNode, nparams=P)
        ec = api.EvalContext(reverse_grad=True)
        params = torch.from_numpy(np.ascontiguousarray(g.standard_normal((5, P)).astype(dtype))).cuda().t()
        kw = dict(params=params, classes=torch.from_numpy(np.sort(g.integers(1, 6, N)).astype(np.int64)).cuda())
    X = dev_X(torch, np.asfortranarray((g.standard_normal((F, N)) * 1.3).astype(dtype)))
    y = torch.from_numpy(g.standard_normal(N).astype(dtype)).cuda()
    consts = tree_consts(trees, ops, dtype)
    sets = [(consts * dtype(0.75)).astype(dtype)] + special_values(dtype, consts, g)[2:6]

    def flat(parts, like):
        return np.concatenate([host(q).reshape(-1) for q in parts] + [np.zeros(0, host(like).dtype)])

    def ev(p):
        o, k = p.eval(X, **kw)
        l, kl = p.eval_loss(X, y, **kw)
        fs, kf = p.eval_fit_stats(X, y, **kw)
        return [("ok", k, None), ("rows", o, host(k)), ("loss", l, None), ("okl", kl, None), ("stats", np.stack([fs.mean_p, fs.m2_p, fs.cov]), None), ("okf", kf, None)]

    def lg(p):
        l, d, k = p.eval_loss_grad(X, y, **kw)
        return [("ok", k, None), ("loss", l, None), ("dloss", flat(d, l), None)]

    def gn(p):
        r = p.eval_gauss_newton(X, y, **kw)
        return [("ok", r.ok, None), ("loss", r.loss, None), ("grad", flat(r.grad, r.loss), None), ("jtj", flat(r.jtj, r.loss), None)]

    def jac(variable):
        def f(p):
            o, gs, k = p.eval_grad(X, variable, **kw)
            return [("ok", k, None), ("rows", o, host(k)), ("jac", flat([q for q, kk in zip(gs, host(k)) if kk], o), None)]
        return f

    def bc(p):
        lo, dl, dp, k = p.eval_loss_grad_by_class(X, y, kw["params"], kw["classes"], variable="both", grouped=True)
        return [("ok", k, None), ("loss", lo, None), ("dparams", dp, None), ("dloss", flat(dl, lo), None)]

    calls = [("eval", ev), ("loss_grad", lg), ("gauss_newton", gn), ("grad constant", jac(False)), ("grad variable", jac(True)), ("grad both", jac("both"))]
    if kind == "parametric":
        calls = [("eval", ev), ("by_class", bc), ("loss_grad", lg)]
    mk = lambda: api.Population(trees, ops, dtype, n_features=F, n_params=P, eval_context=ec)
    ph, pd = mk(), mk()
    try:
        for name, fn in calls:
            pd.set_constants(torch.from_numpy(consts).cuda())
            ph.set_constants(consts)
            fn(pd), fn(ph)  # (the entry point's streams, made behind a device set)
            for i, vals in enumerate(sets):
                ph.set_constants(vals)
                want = fn(ph)
                torch.cuda.synchronize()
                capfd.readouterr()
                pd.set_constants(torch.from_numpy(vals).cuda())
                got = fn(pd)
                torch.cuda.synchronize()
                err = capfd.readouterr().err
                assert pd.consts_on_device_path
                assert "set_consts us" not in err, f"{kind}: {name}: the host function ran:\n{err}"
                compare(want, got, f"{kind}: {name}: set {i}")
        same(pd.constants(), sets[-1], "constants()")
        assert "set_consts us" in capfd.readouterr().err  # (the host side, asked for: the mirror is materialised now)
        assert ph.stream_hash() == pd.stream_hash()
    finally:
        ph.close()
        pd.close()
