"""CPU tests of the per-tree parameter entry points (include/de_hip.h de_tape_params_to_consts / de_tree_params_accumulate_host, DESIGN.md
§4.4.11) and of the Python layer's host half (api.ParametricPopulation argument checks, api.tree_params_fit_bfgs).

    the rewrite      every constant and parameter leaf becomes a constant leaf numbered in tape order; slot_param names the parameter rows
    the accumulation de_tree_params_accumulate_host runs csrc/de_tree_params.h, the code the kernels run: against a float64 numpy
                     restatement that adds in the same order (classes ascending, occurrences in slot order), so the result is BIT-equal
    the fit          api.tree_params_fit_bfgs driven by the CPU oracle as evaluator on the reference's own case
                     (test/test_parametric_expression.jl:140-199, tests/golden/tree_params_fit.json): the reference's three assertions

`fixture_case`, `oracle_evaluator` and `isapprox` are shared with tests/test_gpu_tree_params.py."""
import json
import os
import re

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
from dynamicexpressions_jl_amd import api
from helpers import sexpr_to_node
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF_CONST, LEAF_FEATURE, LEAF_PARAM, LEAF_SHARED, OP_SHARE = 0, 1, 2, 3, 0xFE
OPS = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))


def P_(i):
    return de.ParametricNode(parameter=i)


def X_(i):
    return de.ParametricNode(feature=i)


def V_(v):
    return de.ParametricNode(val=v)


def O_(name, *kids):
    return de.ParametricNode(OPS.index(name, len(kids)), *kids)


def leaves(tape):
    return [(int(n["op"]), int(n["arg"])) for n in tape if n["degree"] == 0]


# ---- the rewrite -----------------------------------------------------------------------------------------------------------------------
def test_rewrite_reference_tree():
    """(x * p2) + y + p1: two parameter slots in tape order, rows 1 and 0; operators and features untouched."""
    tree = O_("+", O_("+", O_("*", X_(1), P_(2)), X_(2)), P_(1))
    tape, consts = de.flatten(tree, OPS, np.float64)
    out, sp = api.tape_params_to_consts(tape, 2)
    assert sp.tolist() == [1, 0] and len(consts) == 0
    assert leaves(out) == [(LEAF_FEATURE, 0), (LEAF_CONST, 0), (LEAF_FEATURE, 1), (LEAF_CONST, 1)]
    ops_in, ops_out = tape[tape["degree"] > 0], out[out["degree"] > 0]
    assert np.array_equal(ops_in, ops_out) and np.array_equal(tape["degree"], out["degree"])


def test_rewrite_repeated_parameter_and_constants():
    """p1 twice and two constants: slots in depth-first order, slot_param == [-1, 0, -1, 0]."""
    tree = O_("+", O_("*", V_(1.5), P_(1)), O_("-", V_(2.5), P_(1)))
    tape, consts = de.flatten(tree, OPS, np.float64)
    out, sp = api.tape_params_to_consts(tape, 1)
    assert sp.tolist() == [-1, 0, -1, 0] and consts.tolist() == [1.5, 2.5]
    assert leaves(out) == [(LEAF_CONST, 0), (LEAF_CONST, 1), (LEAF_CONST, 2), (LEAF_CONST, 3)]


def test_rewrite_lone_parameter_and_identity():
    tape, _ = de.flatten(P_(2), OPS, np.float64)
    out, sp = api.tape_params_to_consts(tape, 2)
    assert sp.tolist() == [1] and leaves(out) == [(LEAF_CONST, 0)] and len(out) == 1
    # a tape without parameters comes back unchanged
    plain = O_("cos", O_("*", X_(1), O_("+", V_(2.0), O_("exp", V_(0.5)))))
    tape, _ = de.flatten(plain, OPS, np.float64)
    out, sp = api.tape_params_to_consts(tape, 0)
    assert np.array_equal(out, tape) and sp.tolist() == [-1, -1]
    out, sp = api.tape_params_to_consts(tape[:0], 3)  # the empty tape
    assert len(out) == 0 and len(sp) == 0


def test_rewrite_refusals():
    lib = api.library()
    tape, _ = de.flatten(O_("+", P_(3), X_(1)), OPS, np.float64)
    with pytest.raises(ValueError, match="OUT_OF_RANGE"):
        api.tape_params_to_consts(tape, 2)
    out, sp = np.empty_like(tape), np.full(4, 77, dtype=np.int32)
    assert lib.de_tape_params_to_consts(tape.ctypes.data, len(tape), 2, out.ctypes.data, sp.ctypes.data, 4) == -6  # DE_ERR_OUT_OF_RANGE
    assert (sp == 77).all()  # nothing written
    for node in ((0, LEAF_SHARED, 0), (1, OP_SHARE, 0)):
        cse = np.array([(0, LEAF_FEATURE, 0), node], dtype=de.node.TAPE_DTYPE)
        assert lib.de_tape_params_to_consts(cse.ctypes.data, len(cse), 2, out.ctypes.data, sp.ctypes.data, 4) == -7  # DE_ERR_UNSUPPORTED
        with pytest.raises(api.DeviceError, match="UNSUPPORTED"):
            api.tape_params_to_consts(cse, 2)
    tape, _ = de.flatten(O_("+", P_(1), V_(1.0)), OPS, np.float64)
    assert lib.de_tape_params_to_consts(tape.ctypes.data, len(tape), 2, out.ctypes.data, sp.ctypes.data, 1) == -1  # more slots than cap
    assert lib.de_tape_params_to_consts(None, 3, 2, out.ctypes.data, sp.ctypes.data, 4) == -1


def test_rewritten_tape_lowers_like_a_plain_tape():
    """The rewritten tape is an ordinary non-parametric tape: it lowers with n_params = 0, and with the parameter values as constants it is
    the tree the oracle evaluates with the parameters of one class."""
    tree = O_("+", O_("cos", O_("*", P_(1), V_(2.0))), O_("/", X_(1), P_(2)))
    tape, consts = de.flatten(tree, OPS, np.float64)
    out, sp = api.tape_params_to_consts(tape, 2)
    params = np.array([[0.3], [1.7]])
    full = np.array([params[r, 0] if r >= 0 else 0.0 for r in sp])
    full[sp < 0] = consts
    words, meta = api.lower_tape(out, full, 1, 0, 7, np.float64)
    assert len(words) > 0 and not meta["uses_params"]
    X = np.asfortranarray(np.linspace(0.5, 2.0, 7).reshape(1, 7))
    a, oka = oracle.eval_tree_array(out, full, X, elementwise=True)
    b, okb = oracle.eval_tree_array_parametric(tape, consts, X, params, np.ones(7, dtype=np.int32), elementwise=True)
    assert oka and okb and np.array_equal(a, b)


# ---- the accumulation ------------------------------------------------------------------------------------------------------------------
def np_accumulate(sp, P, used, loss_c, dloss_c, ok_c, dtype):
    """The documented order in float64: classes ascending, a cell's occurrences in slot order; rounded once; NaN where the flag is 0."""
    C, S = len(used), len(sp)
    lo, dl, dp, ok = np.float64(0), np.zeros(S), np.zeros((C, P)), True
    for c in range(C):
        if not used[c]:
            continue
        lo = lo + np.float64(loss_c[c])
        ok = ok and bool(ok_c[c])
        for s in range(S):
            dl[s] = dl[s] + np.float64(dloss_c[c, s])
            if sp[s] >= 0:
                dp[c, sp[s]] = dp[c, sp[s]] + np.float64(dloss_c[c, s])
    if not ok:
        lo, dl, dp = np.nan, np.full(S, np.nan), np.full((C, P), np.nan)
    return np.asarray(lo, dtype=dtype), dl.astype(dtype), dp.astype(dtype), ok


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_accumulate_host_is_bit_equal_to_the_numpy_restatement(dtype):
    """3 classes of which the middle one is empty (its entries are poison: never read), a tree with p1 twice; then a cleared flag."""
    g = np.random.Generator(np.random.PCG64(11))
    sp = np.array([-1, 0, 1, -1, 0], dtype=np.int32)
    used = np.array([1, 0, 1], dtype=np.uint8)
    it = np.uint32 if dtype == np.float32 else np.uint64
    for trial in range(8):
        loss_c = (g.standard_normal(3) * 10.0 ** g.integers(-6, 7)).astype(dtype)
        dloss_c = (g.standard_normal((3, 5)) * 10.0 ** g.integers(-6, 7, (3, 5))).astype(dtype)
        loss_c[1], dloss_c[1] = np.inf, np.nan
        ok_c = np.array([1, 0, 1], dtype=np.uint8)  # (the empty class's flag is never read either)
        lo, dl, dp, ok = api.tree_params_accumulate_host(sp, 2, used, loss_c, dloss_c, ok_c, dtype)
        wl, wd, wp, wok = np_accumulate(sp, 2, used, loss_c, dloss_c, ok_c, dtype)
        assert ok and wok
        assert np.asarray(lo, dtype=dtype).view(it) == wl.view(it)
        assert np.array_equal(dl.view(it), wd.view(it)) and np.array_equal(dp.view(it), wp.view(it))
        assert np.all(dp[1] == 0)  # the empty class
        # the parameter-slot rows of dloss are the per-class cells summed (here: exactly, one occurrence of row 1)
        assert dl[2] == dtype(np.float64(dloss_c[0, 2]) + np.float64(dloss_c[2, 2]))
        # a cleared flag in one used class: everything of the tree is NaN
        ok_c2 = np.array([1, 1, 0], dtype=np.uint8)
        lo, dl, dp, ok = api.tree_params_accumulate_host(sp, 2, used, loss_c, dloss_c, ok_c2, dtype)
        assert not ok and np.isnan(lo) and np.isnan(dl).all() and np.isnan(dp).all()
    # ... and nothing of its neighbour: one call per tree, the neighbour's inputs and so its bits are unchanged
    a = api.tree_params_accumulate_host(sp, 2, used, loss_c, dloss_c, ok_c, dtype)
    b = api.tree_params_accumulate_host(sp, 2, used, loss_c, dloss_c, ok_c, dtype)
    assert np.array_equal(a[1].view(it), b[1].view(it)) and np.array_equal(a[2].view(it), b[2].view(it))
    # no slot, no parameter, no used class
    lo, dl, dp, ok = api.tree_params_accumulate_host(np.zeros(0, dtype=np.int32), 0, np.zeros(2, dtype=np.uint8), np.zeros(2), np.zeros((2, 0)),
                                                     np.zeros(2, dtype=np.uint8), dtype)
    assert ok and lo == 0 and dl.size == 0 and dp.shape == (2, 0)


def test_abi_additions():
    """Additions only: ABI 3, opcode table 1, every new symbol declared, exported and listed under (o)."""
    raw = open(os.path.join(ROOT, "include", "de_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    lib = api.library()
    for name, n_args in (("de_tape_params_to_consts", 6), ("de_eval_tree_params", 9), ("de_eval_loss_tree_params", 11),
                         ("de_eval_loss_grad_tree_params", 14), ("de_tree_params_accumulate_host", 13)):
        m = re.search(r"^(?:int|int64_t) " + name + r"\(([^;]*)\);", src, re.M | re.S)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == n_args and name in api.EXPORTS
    assert re.search(r"typedef struct de_tree_params \{\s*const void \*params;\s*int64_t ld_params;\s*int64_t n_classes;\s*int32_t n_params, reserved;"
                     r"\s*const int64_t \*class_starts;\s*const int32_t \*slot_param;\s*\} de_tree_params_t;", src)
    import ctypes as C
    assert C.sizeof(api.TreeParams) == 48
    assert lib.de_abi_version() == 3 == api.ABI_VERSION and lib.de_opcode_table_version() == 1
    assert re.search(r"\(o\) de_tape_params_to_consts", raw)
    assert lib.de_eval_tree_params(None, None, None, 0, 0, None, None, 0, None) == 1  # no context: DE_ERR_INVALID_ARG


# ---- ParametricPopulation: the checks that need no device ------------------------------------------------------------------------------
def test_parametric_population_argument_checks():
    chk = api.ParametricPopulation.check_args
    cls = np.array([1, 2, 3, 3, 1])
    assert chk(np.zeros((4, 2, 3)), cls, 4, 2, 5) == 3
    with pytest.raises(ValueError, match="dimension"):
        chk(np.zeros((2, 3)), cls, 4, 2, 5)  # one shared matrix: the wrong rank
    with pytest.raises(ValueError, match="n_trees = 4"):
        chk(np.zeros((5, 2, 3)), cls, 4, 2, 5)
    with pytest.raises(ValueError, match="n_params = 2"):
        chk(np.zeros((4, 3, 3)), cls, 4, 2, 5)
    with pytest.raises(ValueError, match=r"class ids must lie in \[1, 4\)"):
        chk(np.zeros((4, 2, 3)), np.array([1, 2, 4, 3, 1]), 4, 2, 5)
    with pytest.raises(ValueError, match=r"class ids must lie in \[1, 4\)"):
        chk(np.zeros((4, 2, 3)), np.array([0, 2, 3, 3, 1]), 4, 2, 5)
    assert chk(np.zeros((4, 2, 3)), np.array([0, 2, 1, 0, 1]), 4, 2, 5, class_base=0) == 3
    with pytest.raises(ValueError, match="length"):
        chk(np.zeros((4, 2, 3)), cls, 4, 2, 6)
    # n_params mismatch: refused by the constructor before any device object is made
    with pytest.raises(ValueError, match="OUT_OF_RANGE"):
        api.ParametricPopulation([O_("+", P_(3), X_(1))], OPS, np.float64, n_features=1, n_params=2)
    ex = api.ParametricExpression(O_("+", P_(1), X_(1)), OPS, np.zeros((3, 2)))
    with pytest.raises(ValueError, match="n_params = 2"):
        api.ParametricPopulation([ex], OPS, np.float64, n_features=1, n_params=2)


# ---- the reference's fit ---------------------------------------------------------------------------------------------------------------
def fixture_case():
    """(tree, ops, X[2, 9], classes, true parameters [2, 3], init parameters, target y, the fixture)."""
    with open(os.path.join(ROOT, "tests", "golden", "tree_params_fit.json")) as fh:
        case = json.load(fh)
    ops = de.OperatorEnum(binary_operators=case["binary"], unary_operators=case["unary"])
    tree = sexpr_to_node(case["tree"], ops, de.ParametricNode)
    X = np.asfortranarray(np.asarray(case["X"], dtype=np.float64))
    classes = np.asarray(case["classes"], dtype=np.int64)
    true_p, init_p = np.asarray(case["true_parameters"], dtype=np.float64), np.asarray(case["init_parameters"], dtype=np.float64)
    y = X[0] * true_p[1, classes - 1] + X[1] + true_p[0, classes - 1]  # (:172-177)
    return tree, ops, X, classes, true_p, init_p, y, case


def isapprox(a, b, dtype=np.float64):
    """Julia's isapprox(a, b) for arrays: norm(a - b) <= sqrt(eps) * max(norm(a), norm(b))."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) <= np.sqrt(np.finfo(dtype).eps) * max(np.linalg.norm(a), np.linalg.norm(b))


def oracle_evaluator(trees, ops, X, y, classes, dtype=np.float64):
    """``evaluate`` of api.tree_params_fit_bfgs from the CPU oracle: L2 loss, its gradient w.r.t. the real constants and w.r.t. each
    tree's own parameter matrix (the scatter-add of the Jacobian rows through parameters[i, classes[j]])."""
    tapes = [de.flatten(t, ops, dtype)[0] for t in trees]

    def evaluate(consts_list, params):
        nt, P, Cn = params.shape
        lo, dcs, dps, oks = np.zeros(nt, dtype=dtype), [], np.zeros((nt, P, Cn), dtype=dtype), np.zeros(nt, dtype=bool)
        for t in range(nt):
            t2, PX = oracle.parametric_to_plain(tapes[t], X, params[t], classes)
            out, grad, ok = oracle.eval_grad_tree_array(t2, consts_list[t], PX, 2, elementwise=True)  # rows: parameters, features, constants
            e = out - y
            lo[t], oks[t] = np.sum(e * e), ok
            g = 2.0 * e[None, :] * grad
            dcs.append(g[P + X.shape[0]:].sum(axis=1))
            for c in range(Cn):
                dps[t, :, c] = g[:P, classes == c + 1].sum(axis=1)
        return lo, dcs, dps, oks

    return evaluate


def test_fit_bfgs_reference_case_with_the_oracle_as_evaluator():
    """test/test_parametric_expression.jl:140-199 in Float64: 9 samples, 3 classes, 2 parameters, from zeros.  With iters = 60 the loss is
    < 1e-5, the initial loss > 0.1 and the parameters are isapprox the true ones (rtol = sqrt(eps)): the reference's own assertions.
    20 iterations (the default) are not enough for the parameters."""
    tree, ops, X, classes, true_p, init_p, y, case = fixture_case()
    ev = oracle_evaluator([tree], ops, X, y, classes)
    hist = []
    cs, ps, lo, ok, acc = api.tree_params_fit_bfgs(ev, [np.zeros(0)], init_p[None], iters=case["iters"], history=hist)
    print(f"[tree_params fit, oracle] loss {hist[0][0]:.3g} -> {lo[0]:.3g}, {int(acc[0])} accepted steps of {case['iters']}, "
          f"parameter error {np.linalg.norm(ps[0] - true_p):.3g}")
    assert ok[0] and len(hist) == case["iters"] + 1 and len(cs[0]) == 0
    assert lo[0] < case["expect"]["minimum_below"] and hist[0][0] > case["expect"]["init_loss_above"]
    assert isapprox(ps[0], true_p)
    assert all(b[0] <= a[0] for a, b in zip(hist, hist[1:]))  # only steps that lower the loss are taken
    _, ps20, lo20, _, _ = api.tree_params_fit_bfgs(ev, [np.zeros(0)], init_p[None], iters=20)
    assert not isapprox(ps20[0], true_p)


def test_fit_bfgs_combined_vector_order_and_wide_trees():
    """The combined vector is vcat(constants, parameters[:]) (column-major over [n_params, n_classes]); a tree with more than
    BFGS_MAX_ROWS unknowns keeps its values."""
    seen = []

    def ev(consts_list, params):  # loss = |v - target|^2 over the combined vector, so the gradient names every entry's position
        nt, P, Cn = params.shape
        lo, dcs, dps = np.zeros(nt), [], np.zeros((nt, P, Cn))
        for t in range(nt):
            v = np.concatenate([consts_list[t], params[t].T.reshape(-1)])
            target = np.arange(1, len(v) + 1, dtype=np.float64)
            lo[t] = np.sum((v - target) ** 2)
            g = 2 * (v - target)
            dcs.append(g[:len(consts_list[t])])
            dps[t] = g[len(consts_list[t]):].reshape(Cn, P).T
        seen.append(params.copy())
        return lo, dcs, dps, np.ones(nt, dtype=bool)

    cs, ps, lo, ok, acc = api.tree_params_fit_bfgs(ev, [np.zeros(2), np.zeros(30)], np.zeros((2, 2, 3)), iters=12)
    assert lo[0] < 1e-20 and np.allclose(cs[0], [1, 2]) and np.allclose(ps[0], np.array([[3, 5, 7], [4, 6, 8]]))
    assert acc[1] == 0 and np.all(cs[1] == 0) and np.all(ps[1] == 0)  # 30 + 6 unknowns > 32
