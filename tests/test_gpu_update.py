"""de_program_update / Population.update: after every update the program is a fresh creation of the resulting population —
equal de_program_stream_hash, de_program_verify clean, and the same bits from every entry point the dtype serves — and an invalid request
changes nothing."""

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
from helpers import sexpr_to_node

pytestmark = pytest.mark.gpu

OPS = de.synth.BENCH_OPERATORS
KERNEL_OPS = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp", "sin", "square"))


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    return _api


def _eq(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), f"{what}: not bit-equal"


def _rows(out, ok, what_a, out2, ok2):
    _eq(ok, ok2, what_a + " flags")
    live = np.asarray(ok).astype(bool)
    _eq(np.asarray(out)[live], np.asarray(out2)[live], what_a + " rows")


def _grads(g, g2, ok, what):
    live = np.asarray(ok).astype(bool)
    assert len(g) == len(g2)
    for t in range(len(g)):
        if live[t]:
            _eq(g[t], g2[t], f"{what} tree {t}")


def _battery(api, a, b, case):
    """Every entry point the population's dtype serves, on `a` (updated) and `b` (fresh): the same bits."""
    X, params, classes, y = case["X"], case.get("params"), case.get("classes"), case["y"]
    kw = dict(params=params, classes=classes) if params is not None else {}
    o1, k1 = a.eval(X, **kw)
    o2, k2 = b.eval(X, **kw)
    _rows(o1, k1, "eval", o2, k2)
    if case.get("certificate", True):
        for x, z, w in zip(a.sum_certificate(X, **kw), b.sum_certificate(X, **kw), ("ok", "cert", "max")):
            _eq(x, z, "sum_certificate " + w)
    if not case.get("grad", True):
        return
    for variable in (False, True, "both"):
        o1, g1, k1 = a.eval_grad(X, variable=variable, **kw)
        o2, g2, k2 = b.eval_grad(X, variable=variable, **kw)
        _rows(o1, k1, f"eval_grad({variable})", o2, k2)
        _grads(g1, g2, k1, f"eval_grad({variable}) gradient")
    if params is None:
        o1, d1, k1 = a.eval_diff(X, 1)
        o2, d2, k2 = b.eval_diff(X, 1)
        _rows(o1, k1, "eval_diff", o2, k2)
        _rows(d1, k1, "eval_diff derivative", d2, k2)
    l1, k1 = a.eval_loss(X, y, **kw)
    l2, k2 = b.eval_loss(X, y, **kw)
    _rows(l1, k1, "eval_loss", l2, k2)
    for variable in (False, True):
        l1, g1, k1 = a.eval_loss_grad(X, y, variable=variable, **kw)
        l2, g2, k2 = b.eval_loss_grad(X, y, variable=variable, **kw)
        _rows(l1, k1, f"eval_loss_grad({variable})", l2, k2)
        _grads(g1, g2, k1, f"eval_loss_grad({variable}) gradient")
    if params is not None:
        r1 = a.eval_loss_grad_by_class(X, y, params, classes)
        r2 = b.eval_loss_grad_by_class(X, y, params, classes)
        _rows(r1[0], r1[3], "eval_loss_grad_by_class", r2[0], r2[3])
        _grads(r1[1], r2[1], r1[3], "eval_loss_grad_by_class dloss")
        live = np.asarray(r1[3]).astype(bool)
        _eq(np.asarray(r1[2])[live], np.asarray(r2[2])[live], "eval_loss_grad_by_class dparams")


def _check(api, pop, trees, case, battery=True, set_consts=False):
    """`pop` against a fresh Population of `trees`.  set_consts: also set new constants on both and compare (the population's constants are
    then no longer the trees' own: only on a test's last check)."""
    fresh = api.Population(trees, case["ops"], case["dtype"], n_features=case["F"], n_params=case.get("P", 0), eval_context=case["ec"])
    try:
        assert pop.stream_hash() == fresh.stream_hash(), "updated program differs from a fresh creation"
        pop.verify()
        assert pop.n_nodes == fresh.n_nodes and np.array_equal(pop.n_consts, fresh.n_consts)
        assert [pop.meta(t) for t in range(len(trees))] == [fresh.meta(t) for t in range(len(trees))]
        for t in (0, len(trees) - 1):
            assert np.array_equal(pop.dump(t), fresh.dump(t))
            assert pop.n_grad(t, 2) == fresh.n_grad(t, 2)
        if battery:
            _battery(api, pop, fresh, case)
        if set_consts:
            # set_constants (the new total) followed by eval
            g = np.random.Generator(np.random.PCG64(int(pop.n_consts.sum())))
            c = (g.standard_normal(int(pop.n_consts.sum())) * 1.5).astype(case["dtype"])
            if np.dtype(case["dtype"]).kind == "c":
                c = c + 1j * (g.standard_normal(c.size) * 0.5).astype(c.dtype)
            pop.set_constants(c)
            fresh.set_constants(c)
            assert pop.stream_hash() == fresh.stream_hash()
            kw = dict(params=case["params"], classes=case["classes"]) if case.get("params") is not None else {}
            o1, k1 = pop.eval(case["X"], **kw)
            o2, k2 = fresh.eval(case["X"], **kw)
            _rows(o1, k1, "eval after set_constants", o2, k2)
    finally:
        fresh.close()


def _case(api, kind, dtype=np.float32):
    g = np.random.Generator(np.random.PCG64(99))
    ec = api.EvalContext()
    F, P, N = 5, 0, 2003
    ops = OPS
    if kind == "plain":
        make = lambda n, s: de.synth.random_population(n, seed=s, dtype=dtype)
    elif kind == "parametric":
        P = 3
        make = lambda n, s: de.synth.random_population(n, seed=s, dtype=dtype, node_type=de.ParametricNode, nparams=P)
    elif kind == "graph":
        from test_lowering import random_graph
        ops = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp", "safe_log", "square"))

        def make(n, s):
            rng = de.synth.Xoshiro256ss(s)
            return [random_graph(rng, ops, 6 + i % 20, F, 1 + i % 3, dtype) for i in range(n)]
    elif kind == "wide":
        F = 48
        make = lambda n, s: de.synth.random_population(n, seed=s, dtype=dtype, nfeatures=F)
    elif kind == "f16":
        dtype = np.float16
        ops = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
        make = lambda n, s: de.synth.random_population(n, seed=s, node_count=12, operators=ops, dtype=np.float32)
    elif kind == "cf32":
        dtype = np.complex64
        ops = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
        make = lambda n, s: de.synth.random_population(n, seed=s, node_count=12, operators=ops, dtype=np.float32)
    X = (g.standard_normal((F, N)) * 1.3)
    if np.dtype(dtype).kind == "c":
        X = X + 1j * g.standard_normal((F, N)) * 0.5
    X = np.asfortranarray(X.astype(dtype))
    case = dict(ops=ops, dtype=dtype, F=F, P=P, ec=ec, X=X, certificate=kind != "wide", y=np.ascontiguousarray(X[0].real.astype(dtype) if np.dtype(dtype).kind != "c" else X[0]),
                make=make, grad=kind not in ("f16", "cf32"))
    if P:
        C_ = 4
        case["params"] = np.asfortranarray((g.standard_normal((P, C_)) * 2).astype(dtype))
        case["classes"] = g.integers(1, C_ + 1, N).astype(np.int64)
    return case


@pytest.mark.parametrize("kind,dtype", [("plain", np.float32), ("plain", np.float64), ("parametric", np.float32), ("graph", np.float64),
                                        ("wide", np.float32), ("f16", None), ("cf32", None)],
                         ids=["f32", "f64", "parametric", "graph", "wide", "f16", "cf32"])
def test_random_update_sequences_equal_a_fresh_creation(api, kind, dtype):
    case = _case(api, kind, dtype or np.float32)
    n = 96
    trees = case["make"](n, 0x5EED)
    pool = case["make"](400, 0x900D)
    pop = api.Population(trees, case["ops"], case["dtype"], n_features=case["F"], n_params=case["P"], eval_context=case["ec"])
    rng = np.random.default_rng(5)
    rounds = [[], [0], [n - 1], [40, 41], list(rng.choice(n, 7, replace=False)), [n - 2, 3, n - 1], list(range(n)),
              list(rng.choice(n, 30, replace=False))]
    at = 0
    try:
        _check(api, pop, trees, case, battery=False)
        for r, ids in enumerate(rounds):
            new = pool[at:at + len(ids)]
            at += len(ids)
            pop.update(ids, new)
            for i, t in enumerate(ids):
                trees[int(t)] = new[i]
            _check(api, pop, trees, case, battery=r in (1, 3, 4, 6, 7), set_consts=r == len(rounds) - 1)
    finally:
        pop.close()


def _tree(s, ops=KERNEL_OPS, dtype=np.float32, node_type=None):
    return sexpr_to_node(s, ops, node_type or de.Node)


def test_targeted_updates(api):
    """Spill slots grow and shrink; host-, kernel- and auxiliary-program folds come and go; a non-finite constant; constant counts change."""
    dtype = np.float32
    case = _case(api, "plain", dtype)
    case["ops"] = KERNEL_OPS
    trees = de.synth.random_population(40, seed=3, operators=KERNEL_OPS, node_count=9)
    deep = de.synth.random_population(4, seed=4, operators=KERNEL_OPS, node_count=61, max_depth=40)
    special = {
        "host fold": ["+", ["*", 1.5, 2.25], ["x", 1]],
        "kernel fold": ["*", ["cos", 0.75], ["x", 2]],
        "aux fold": ["+", ["exp", ["*", 0.5, ["sin", 0.25]]], ["x", 3]],  # (a turbo program folds it through the auxiliary program)
        "inf": ["+", float("inf"), ["x", 1]],
        "no constant": ["cos", ["x", 4]],
        "many constants": ["+", ["+", ["*", 1.0, ["x", 1]], ["*", 2.0, ["x", 2]]], ["+", ["*", 3.0, ["x", 3]], 4.0]],
    }
    base = list(trees)
    pop = api.Population(trees, KERNEL_OPS, dtype, n_features=5)
    try:
        s0 = pop.meta(0)["n_slots"]
        for ids, new in [([5], [deep[0]]), ([5], [trees[6]]), ([0, 1, 2], [_tree(special[k]) for k in ("host fold", "kernel fold", "aux fold")]),
                         ([7], [_tree(special["inf"])]), ([8, 9], [_tree(special["no constant"]), _tree(special["many constants"])]),
                         ([0, 1, 2, 7], [trees[10], trees[11], trees[12], trees[13]]), ([39], [deep[1]]), ([39, 5], [trees[14], trees[15]])]:
            before = pop.meta(0)["n_slots"]
            pop.update(ids, new)
            for i, t in enumerate(ids):
                trees[t] = new[i]
            _check(api, pop, trees, case)
            if new[0] is deep[0]:
                assert pop.meta(0)["n_slots"] > s0, "the deep tree was meant to need more spill slots"
            if ids == [7] and len(new) == 1:
                assert not pop.meta(7)["host_ok_eval"] and not pop.meta(7)["host_ok_grad"]
        assert pop.meta(0)["n_slots"] == s0 and before > s0, "spill slots were meant to shrink back"
        _check(api, pop, trees, case, battery=False, set_consts=True)
    finally:
        pop.close()
    # turbo: every constant subtree goes through the auxiliary program, which is updated with its trees
    case["ec"] = api.EvalContext(turbo=True)
    trees = base
    pop = api.Population(trees, KERNEL_OPS, dtype, n_features=5, eval_context=case["ec"])
    try:
        for ids, new in [([2, 3], [_tree(special["kernel fold"]), _tree(special["aux fold"])]), ([20], [_tree(special["host fold"])]),
                         ([3], [trees[30]]), ([2, 20, 21], [trees[31], _tree(special["aux fold"]), _tree(special["kernel fold"])])]:
            pop.update(ids, new)
            for i, t in enumerate(ids):
                trees[t] = new[i]
            _check(api, pop, trees, case)
    finally:
        pop.close()


def test_update_changes_the_wave_choice(api):
    """Parameter rows make the program run wave groups; replacing every parametric tree removes them (a whole-program geometry change)."""
    case = _case(api, "parametric", np.float32)
    P = 8
    case["P"] = P
    g = np.random.Generator(np.random.PCG64(8))
    case["params"] = np.asfortranarray((g.standard_normal((P, 4)) * 2).astype(np.float32))
    trees = de.synth.random_population(60, seed=0x3A7E, node_type=de.ParametricNode, nparams=P)
    plain = de.synth.random_population(60, seed=0x3A80)
    pop = api.Population(trees, OPS, np.float32, n_features=5, n_params=P)
    try:
        w0 = pop.meta(0)["waves"]
        pop.update(range(60), plain)
        _check(api, pop, plain, case)
        w1 = pop.meta(0)["waves"]
        assert w0 != w1, (w0, w1)
        pop.update([0, 30], trees[:2])
        plain[0], plain[30] = trees[0], trees[1]
        _check(api, pop, plain, case, set_consts=True)
        assert pop.meta(0)["waves"] == w0
    finally:
        pop.close()


def test_gradient_caches_do_not_survive_an_update(api):
    case = _case(api, "plain", np.float32)
    trees = de.synth.random_population(50, seed=11)
    pool = de.synth.random_population(50, seed=12)
    for ec in (api.EvalContext(), api.EvalContext(reverse_grad=True), api.EvalContext(early_exit=False), api.EvalContext(full_eval=True)):
        case["ec"] = ec
        pop = api.Population(trees, OPS, np.float32, n_features=5, eval_context=ec)
        try:
            X, y = case["X"], case["y"]
            for variable in (False, True, "both"):
                pop.eval_grad(X, variable=variable)
            pop.eval_loss_grad(X, y, variable=False)
            pop.eval_loss_grad(X, y, variable=True)
            pop.sum_certificate(X)
            new = list(trees)
            new[3], new[17], new[49] = pool[0], pool[1], pool[2]
            pop.update([3, 17, 49], [pool[0], pool[1], pool[2]])
            _check(api, pop, new, case, set_consts=True)
        finally:
            pop.close()


def test_invalid_requests_change_nothing(api):
    lib = api.library()
    trees = de.synth.random_population(20, seed=21)
    X = np.asfortranarray(de.synth.random_X(5, 500, 3))
    pop = api.Population(trees, OPS, np.float32, n_features=5)
    cpop = api.Population(de.synth.random_population(6, seed=22, node_count=8,
                                                     operators=de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))),
                          de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",)), np.complex64, n_features=5)
    try:
        h0, (o0, k0) = pop.stream_hash(), pop.eval(X)
        tape, noff, consts, coff = de.flatten_population(trees[:2], OPS, np.float32)

        def call(p, ids, tape=tape, noff=noff, consts=consts, coff=coff):
            ids = np.asarray(ids, dtype=np.int64)
            return lib.de_program_update(p._h, ids.ctypes.data, len(ids), tape.ctypes.data, noff.ctypes.data, None, None,
                                         consts.ctypes.data if len(consts) else None, coff.ctypes.data)

        assert call(pop, [4, 4]) == 1                          # duplicate id: DE_ERR_INVALID_ARG
        assert call(pop, [3, 20]) == 6                         # id outside [0, n_trees): DE_ERR_OUT_OF_RANGE
        assert call(pop, [3, -1]) == 6
        assert lib.de_program_update(pop._h, None, 2, tape.ctypes.data, noff.ctypes.data, None, None, consts.ctypes.data, coff.ctypes.data) == 1
        wide = de.flatten_population([sexpr_to_node(["+", ["x", 6], 1.0], OPS), trees[0]], OPS, np.float32)
        assert call(pop, [1, 2], *wide) == 6                   # feature >= n_features: DE_ERR_OUT_OF_RANGE
        bad = tape.copy()
        bad[noff[1] - 1] = (0, 1, 0)                           # the root becomes a feature leaf: two values left on the stack
        assert call(pop, [1, 2], bad) == 2                     # DE_ERR_BAD_TAPE
        assert call(pop, []) == 0
        assert pop.stream_hash() == h0
        pop.verify()
        o1, k1 = pop.eval(X)
        _rows(o1, k1, "eval after refused updates", o0, k0)
        with pytest.raises(ValueError):
            pop.update([1, 1], trees[:2])
        with pytest.raises(ValueError):
            pop.update([20], trees[:1])
        # complex: a refused opcode fails as at creation, named in de_last_error
        ch = cpop.stream_hash()
        mx = de.OperatorEnum(binary_operators=("+", "*", "max"), unary_operators=("cos",))
        sq = de.flatten_population([sexpr_to_node(["max", ["x", 1], 2.0], mx)], mx, np.complex64)
        assert call(cpop, [0], *sq) == 3                       # DE_ERR_UNSUPPORTED_OP
        assert "max" in lib.de_last_error(cpop.ctx._h).decode()
        assert cpop.stream_hash() == ch
    finally:
        pop.close()
        cpop.close()


@pytest.mark.parametrize("kind", ["plain", "wave groups", "turbo aux"])
def test_update_after_set_constants_keeps_the_optimised_constants(api, kind):
    """The search loop: optimise the constants (de_program_set_consts patches them in place), then replace a few trees.  The kept trees keep
    the optimised constants in every stream — the program equals a fresh creation from the resulting trees carrying those constants."""
    import copy
    case = _case(api, "plain", np.float32)
    P = 0
    if kind == "plain":
        make = lambda n, s: de.synth.random_population(n, seed=s)
    elif kind == "wave groups":  # staged parameter rows: four waves per workgroup, stream variants per wave
        P = 8
        case["P"] = P
        g = np.random.Generator(np.random.PCG64(8))
        case["params"] = np.asfortranarray((g.standard_normal((P, 4)) * 2).astype(np.float32))
        case["classes"] = g.integers(1, 5, case["X"].shape[1]).astype(np.int64)
        make = lambda n, s: de.synth.random_population(n, seed=s, node_type=de.ParametricNode, nparams=P)
    else:  # every constant subtree through the auxiliary program, whose constants set_consts patches too
        case["ops"] = KERNEL_OPS
        case["ec"] = api.EvalContext(turbo=True)
        make = lambda n, s: de.synth.random_population(n, seed=s, operators=KERNEL_OPS, node_count=12)
    ops = case["ops"]
    trees = make(80, 0xC0)
    pool = make(40, 0xC1)
    pop = api.Population(trees, ops, np.float32, n_features=5, n_params=P, eval_context=case["ec"])
    try:
        if kind == "wave groups":
            assert pop.meta(0)["waves"] > 1
        if kind == "turbo aux":
            assert sum(len(de.get_scalar_constants(t)[0]) for t in trees) > 0
        g = np.random.Generator(np.random.PCG64(17))
        at = 0
        for r, ids in enumerate([[5], [0, 1, 40, 79], list(g.choice(80, 9, replace=False))]):
            c1 = (g.standard_normal(int(pop.n_consts.sum())) * 1.7).astype(np.float32)
            pop.set_constants(c1)
            new = pool[at:at + len(ids)]
            at += len(ids)
            # the trees the program now stands for: the optimised constants on the kept trees, the new trees as given
            cuts = np.concatenate([[0], np.cumsum(pop.n_consts)])
            cur = []
            for t, tr in enumerate(trees):
                tr = copy.deepcopy(tr)
                _, refs = de.get_scalar_constants(tr)
                de.set_scalar_constants(tr, c1[cuts[t]:cuts[t + 1]], refs)
                cur.append(tr)
            pop.update(ids, new)
            for i, t in enumerate(ids):
                cur[int(t)] = new[i]
            trees = cur
            _check(api, pop, trees, case, battery=r == 2)
            fresh = api.Population(trees, ops, np.float32, n_features=5, n_params=P, eval_context=case["ec"])
            try:  # the eval bits directly, whatever the hash says
                kw = dict(params=case["params"], classes=case["classes"]) if P else {}
                o1, k1 = pop.eval(case["X"], **kw)
                o2, k2 = fresh.eval(case["X"], **kw)
                _rows(o1, k1, "eval after set_constants + update", o2, k2)
            finally:
                fresh.close()
    finally:
        pop.close()
