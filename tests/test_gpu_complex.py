"""DE_CF32 / DE_CF64 (ComplexF32 / ComplexF64) evaluation on the MI355X (csrc/de_complex.hip): the reference's complex known answers,
seeded random populations against the complex CPU oracle (tests/oracle_complex/), bit-equality across the program's paths, the real
anchor, the edges of the operator table, the wide-X gather variant, the entry points that refuse complex programs and the sum
certificate.  Run with `pytest -m gpu`.  DESIGN.md §14."""
import json
import os

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
from dynamicexpressions_jl_amd import api
import complex_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_known_answers_complex.json")))["cases"]
CDTYPES = (np.complex64, np.complex128)
REAL_OF = {np.dtype(np.complex64): np.float32, np.dtype(np.complex128): np.float64}

ARITH = de.OperatorEnum(binary_operators=("+", "-", "*", "/"))
BENCH = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
ALL19 = de.OperatorEnum(binary_operators=("+", "-", "*", "/"),
                        unary_operators=("neg", "square", "cube", "inv", "sqrt", "exp", "log", "sin", "cos", "tan", "sinh", "cosh", "tanh",
                                         "custom_cos"),
                        ternary_operators=("+",))
OPSETS = {"arith": ARITH, "bench": BENCH, "all19": ALL19}
RING = de.OperatorEnum(binary_operators=("+", "-", "*"))
EE, NOEE, FULL = 7, 6, 7 | 32  # early exit (+ the fused-kernel bits), early_exit = false, early exit with DE_OPT_FULL_EVAL
MODES = {"ee": EE, "noee": NOEE, "full": FULL}


@pytest.fixture(scope="module")
def co(tmp_path_factory):
    return complex_oracle.build(str(tmp_path_factory.mktemp("complex_oracle")))


def _complexify(trees, seed):
    rng = np.random.default_rng(seed)
    for t in trees:
        for n in t:
            if n.degree == 0 and n.constant:
                n.val = complex(n.val, float(rng.standard_normal()))
    return trees


def _population(opset, n=48, seed=0):
    ops = OPSETS[opset]
    base = ARITH if opset == "all19" else ops
    trees = de.synth.random_population(n, seed=seed, node_count=12, nfeatures=5, operators=base)
    if opset == "all19":  # every tree becomes +(a unary of the tree, a smaller tree, a leaf): all 19 opcodes over the population
        rng = np.random.default_rng(seed + 7)
        small = de.synth.random_population(n, seed=seed + 1, node_count=4, nfeatures=5, operators=base)
        un = [rng.integers(1, 15) for _ in range(n)]
        trees = [de.Node(1, de.Node(int(un[t]), trees[t]), small[t], de.Node(feature=1 + t % 5) if t % 3 else de.Node(val=0.5))
                 for t in range(n)]
    return _complexify(trees, seed + 11), ops


def _X(F, N, dtype, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return np.asfortranarray((scale * (rng.standard_normal((F, N)) + 1j * rng.standard_normal((F, N)))).astype(dtype))


# ---- the tolerance model: helpers.parity_tolerance's perturbation idea restated for complex values -----------------------------------
_NP = {"neg": np.negative, "square": lambda z: z * z, "cube": lambda z: (z * z) * z, "inv": lambda z: 1 / z, "sqrt": np.sqrt, "exp": np.exp,
       "log": np.log, "sin": np.sin, "cos": np.cos, "tan": np.tan, "sinh": np.sinh, "cosh": np.cosh, "tanh": np.tanh,
       "custom_cos": lambda z: np.cos(z) ** 2}
_NPB = {"+": np.add, "-": np.subtract, "*": np.multiply, "/": np.divide}


def _np_eval(tree, ops, X, rng=None, eps=0.0):
    """complex128 numpy evaluation; with rng, every operator result is multiplied componentwise by (1 +- u eps), u in [1/4, 1]."""
    def pert(v):
        if rng is None:
            return v
        n = v.shape[0]
        fr = 1 + eps * rng.choice([-1.0, 1.0], n) * rng.uniform(0.25, 1.0, n)
        fi = 1 + eps * rng.choice([-1.0, 1.0], n) * rng.uniform(0.25, 1.0, n)
        return v.real * fr + 1j * (v.imag * fi)

    def rec(n):
        if n.degree == 0:
            return np.full(X.shape[1], complex(n.val)) if n.constant else X[n.feature - 1].astype(np.complex128)
        kids = [rec(c) for c in n.children]
        name = ops.ops[n.degree - 1][n.op - 1]
        if n.degree == 1:
            v = _NP[name](kids[0])
        elif n.degree == 2:
            v = _NPB[name](kids[0], kids[1])
        else:
            v = (kids[0] + kids[1]) + kids[2]
        return pert(v)

    with np.errstate(all="ignore"):
        return rec(tree)


def complex_tolerance(tree, ops, X, dtype, draws=8, seed=0):
    """Per sample: tolerance = 8 ulp of the component type x |y| + 8 x the spread of `draws` evaluations with every operator result
    perturbed by <= 1 ulp per component; ILL-CONDITIONED (tolerance +inf, flags only) where the spread exceeds 1e-3 |y| or a draw is not
    finite.  Returns (tolerance, ill mask)."""
    eps = float(np.finfo(REAL_OF[np.dtype(dtype)]).eps)
    clean = _np_eval(tree, ops, X)
    rng = np.random.default_rng(seed)
    spread = np.zeros(X.shape[1])
    bad = ~np.isfinite(clean)
    for _ in range(draws):
        v = _np_eval(tree, ops, X, rng, eps)
        with np.errstate(all="ignore"):
            spread = np.maximum(spread, np.abs(v - clean))
        bad |= ~np.isfinite(v)
    with np.errstate(all="ignore"):
        ill = bad | (spread > 1e-3 * np.abs(clean))
    tol = 8 * eps * np.abs(clean) + 8 * spread
    tol[ill] = np.inf
    return tol, ill


def _is_ring(tree, ops):
    return all(n.degree == 0 or ops.ops[n.degree - 1][n.op - 1] in ("+", "-", "*") and n.degree == 2 for n in tree)


def _oracle_rows(co, trees, ops, X, dtype, options):
    rows, oks = [], []
    for t in trees:
        tape, consts = de.flatten(t, ops, dtype)
        y, ok = co.eval_tree_array(tape, consts, X, dtype, options, elementwise=True)
        rows.append(y)
        oks.append(ok)
    return np.array(rows), np.array(oks)


def _compare(trees, ops, X, dtype, out, ok, co, options, label):
    ref, ref_ok = _oracle_rows(co, trees, ops, X, dtype, options)
    np.testing.assert_array_equal(np.asarray(ok, dtype=bool), ref_ok, err_msg=f"{label}: flags")
    n_ill = n_all = 0
    for t, tree in enumerate(trees):
        if not ref_ok[t] and options & 1:
            continue  # rows of incomplete trees are unspecified under early exit
        if _is_ring(tree, ops):
            np.testing.assert_array_equal(out[t].view(REAL_OF[np.dtype(dtype)]), ref[t].view(REAL_OF[np.dtype(dtype)]),
                                          err_msg=f"{label}: + - * tree {t} not bit-equal")
            continue
        tol, ill = complex_tolerance(tree, ops, X, dtype, seed=t)
        fin = np.isfinite(ref[t])
        assert np.array_equal(np.isfinite(out[t]) | ill, fin | ill), f"{label}: tree {t} finiteness"
        with np.errstate(all="ignore"):
            err = np.abs(out[t].astype(np.complex128) - ref[t].astype(np.complex128))
        okm = fin & ~ill
        assert (err[okm] <= tol[okm] + 1e-300).all(), f"{label}: tree {t} max excess {np.max(err[okm] - tol[okm])}"
        n_ill += int(ill.sum())
        n_all += ill.size
    return n_ill, n_all


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_golden_cases_on_the_device(case):
    dt = np.dtype(case["dtype"])
    tape = np.zeros(len(case["tape"]), dtype=de.node.TAPE_DTYPE)
    for i, r in enumerate(case["tape"]):
        tape[i] = tuple(r)
    consts = np.array([complex(*v) for v in case["consts"]], dtype=dt)
    X = np.asfortranarray(np.array([[complex(*v) for v in row] for row in case["X"]], dtype=dt))
    F, N = X.shape
    out = np.zeros(N, dtype=dt)
    ok = np.zeros(1, dtype=np.uint8)
    lib, ctx = api.library(), api.default_context()
    ctx.check(lib.de_eval_tree_array(ctx._h, api._dtype_code(dt), tape.ctypes.data, len(tape), consts.ctypes.data if len(consts) else None,
                                     len(consts), X.ctypes.data, F, N, 7, out.ctypes.data, ok.ctypes.data))
    assert bool(ok[0]) == case["ok"]
    if case["ok"]:
        want = np.array([complex(*v) for v in case["out"]])
        np.testing.assert_allclose(out.astype(np.complex128), want, rtol=max(case["rtol"], 1e-15) * 4, atol=0)


_ILL = {}


@pytest.mark.parametrize("dtype", CDTYPES, ids=["cf32", "cf64"])
@pytest.mark.parametrize("N", [1, 63, 1000, 4097])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("opset", sorted(OPSETS))
def test_random_populations_against_the_oracle(co, opset, mode, N, dtype):
    trees, ops = _population(opset, seed=1000 + 7 * N)
    X = _X(5, N, dtype, seed=N)
    pop = _raw_population(trees, ops, dtype, MODES[mode])
    out, ok = pop.eval(X)
    n_ill, n_all = _compare(trees, ops, X, dtype, out, ok, co, MODES[mode], f"{opset}/{mode}/N={N}")
    if n_all:
        print(f"{opset} {mode} N={N} {np.dtype(dtype).name}: ill-conditioned share {n_ill / n_all:.4f}")
        assert n_ill <= 0.25 * n_all
    # torch device tensors with ldX > F: same bits as the host buffers
    import torch
    Xt = torch.zeros((N, 8), dtype=api._torch_dtype(dtype), device="cuda")
    Xt[:, :5] = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    outd, okd = pop.eval(Xt[:, :5].t())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(okd.cpu().numpy(), np.asarray(ok, dtype=bool))
    keep = np.asarray(ok, dtype=bool) | (MODES[mode] & 1 == 0) | (MODES[mode] == FULL)
    od = outd.cpu().numpy()
    np.testing.assert_array_equal(od[keep].view(REAL_OF[np.dtype(dtype)]), out[keep].view(REAL_OF[np.dtype(dtype)]))
    pop.close()


def _raw_population(trees, ops, dtype, options):
    """A Population whose program carries exactly `options` (DE_OPT_FULL_EVAL has no EvalContext field)."""
    pop = api.Population.__new__(api.Population)
    import ctypes as C
    from dynamicexpressions_jl_amd.node import flatten_population
    pop.ctx, pop.dtype, pop.operators, pop.eval_context = api.default_context(), np.dtype(dtype), ops, api.EvalContext()
    pop.n_trees, pop._occ, pop._classes_checked = len(trees), None, set()
    nodes, noff, consts, coff = flatten_population(trees, ops, pop.dtype)
    pop.n_features, pop.n_params = 5, 0
    pop.n_consts = np.diff(coff)
    pop._slots_per_tree = np.diff(coff)
    pop._h = C.c_void_p()
    pop._keep = (nodes, noff, consts, coff)
    pop.ctx.check(api.library().de_program_create(pop.ctx._h, api._dtype_code(dtype), nodes.ctypes.data, noff.ctypes.data, len(trees),
                                                   consts.ctypes.data if len(consts) else None, coff.ctypes.data, 5, 0, options,
                                                   C.byref(pop._h)))
    pop.uncertified = np.zeros(0, dtype=np.int64)
    return pop


@pytest.mark.parametrize("dtype", CDTYPES, ids=["cf32", "cf64"])
def test_same_bits_across_paths(dtype, monkeypatch):
    trees, ops = _population("all19", seed=77)
    X = _X(5, 1000, dtype, seed=5)
    pop = api.Population(trees, ops, dtype, n_features=5, eval_context=api.EvalContext(early_exit=False))
    out, ok = pop.eval(X)
    # set_consts = a fresh creation with those constants
    new = [c * (0.5 - 0.25j) for c in np.concatenate([de.flatten(t, ops, dtype)[1] for t in trees])]
    pop.set_constants(np.array(new, dtype=dtype))
    out2, ok2 = pop.eval(X)
    at = 0
    for t in trees:
        _, refs = de.get_scalar_constants(t)
        de.set_scalar_constants(t, new[at:at + len(refs)], refs)
        at += len(refs)
    fresh = api.Population(trees, ops, dtype, n_features=5, eval_context=api.EvalContext(early_exit=False))
    out3, ok3 = fresh.eval(X)
    R = REAL_OF[np.dtype(dtype)]
    np.testing.assert_array_equal(ok2, ok3)
    np.testing.assert_array_equal(out2.view(R), out3.view(R))
    # DE_NO_FOLD=1 (every constant subtree evaluated in place) = folding (constant subtrees through the auxiliary program)
    monkeypatch.setenv("DE_NO_FOLD", "1")
    nofold = api.Population(trees, ops, dtype, n_features=5, eval_context=api.EvalContext(early_exit=False))
    out4, ok4 = nofold.eval(X)
    np.testing.assert_array_equal(ok3, ok4)
    np.testing.assert_array_equal(out3.view(R), out4.view(R))
    for p in (pop, fresh, nofold):
        p.close()


@pytest.mark.parametrize("dtype", CDTYPES, ids=["cf32", "cf64"])
def test_cse_tape_equals_expanded(dtype):
    x1, x2 = de.Node(feature=1), de.Node(feature=2)
    ops = BENCH
    graphs, expanded = [], []
    for k in range(16):
        s = de.GraphNode(3, de.GraphNode(1, de.GraphNode(feature=1), de.GraphNode(val=complex(0.5 + k, -0.25))), de.GraphNode(feature=2))
        graphs.append(de.GraphNode(1, de.GraphNode(1, s), s))
        e = de.Node(3, de.Node(1, x1, de.Node(val=complex(0.5 + k, -0.25))), x2)
        expanded.append(de.Node(1, de.Node(1, e), de.Node(3, de.Node(1, x1, de.Node(val=complex(0.5 + k, -0.25))), x2)))
    X = _X(2, 700, dtype, seed=9)
    pg = api.Population(graphs, ops, dtype, n_features=2)
    pe = api.Population(expanded, ops, dtype, n_features=2)
    og, okg = pg.eval(X)
    oe, oke = pe.eval(X)
    R = REAL_OF[np.dtype(dtype)]
    np.testing.assert_array_equal(okg, oke)
    np.testing.assert_array_equal(og.view(R), oe.view(R))
    pg.close()
    pe.close()


@pytest.mark.parametrize("dtype", CDTYPES, ids=["cf32", "cf64"])
def test_ring_trees_on_real_inputs_anchor_to_the_real_kernels(dtype):
    # + - * trees over inputs and constants with zero imaginary parts: the real parts are the DE_F32 / DE_F64 rows bit for bit
    R = REAL_OF[np.dtype(dtype)]
    trees = de.synth.random_population(48, seed=4242, node_count=12, nfeatures=5, operators=RING)
    Xr = np.asfortranarray(np.random.default_rng(3).standard_normal((5, 1000)).astype(R))
    preal = api.Population(trees, RING, R, n_features=5, eval_context=api.EvalContext(early_exit=False))
    outr, okr = preal.eval(Xr)
    ctrees = [_with_complex_consts(t) for t in trees]
    pc = api.Population(ctrees, RING, dtype, n_features=5, eval_context=api.EvalContext(early_exit=False))
    outc, okc = pc.eval(np.asfortranarray(Xr.astype(dtype)))
    np.testing.assert_array_equal(okr, okc)
    np.testing.assert_array_equal(outc.real, outr)
    preal.close()
    pc.close()


def _with_complex_consts(tree):
    import copy
    t = copy.deepcopy(tree)
    for n in t:
        if n.degree == 0 and n.constant:
            n.val = complex(n.val, 0.0)
    return t


EDGES = [
    ("sqrt", [complex(-4.0, 0.0), complex(-4.0, -0.0), complex(-0.0, 0.0), complex(-1e-30, 0.0)]),
    ("log", [complex(-1.0, 0.0), complex(-1.0, -0.0), complex(0.0, 0.0), complex(-2.5, -0.0)]),
    ("exp", [complex(89.0, 0.0), complex(710.0, 0.0), complex(-200.0, 3.0), complex(88.0, 0.0)]),
    ("cosh", [complex(0.5, 100.0), complex(0.0, 800.0), complex(1.0, -95.0), complex(0.0, 1e4)]),
    ("cos", [complex(0.5, 100.0), complex(1.0, 800.0), complex(3.0, -95.0), complex(0.0, 1e4)]),
]


@pytest.mark.parametrize("dtype", CDTYPES, ids=["cf32", "cf64"])
@pytest.mark.parametrize("name,zs", EDGES, ids=[e[0] for e in EDGES])
def test_edges_flags_equal_the_oracle(co, dtype, name, zs):
    ops = de.OperatorEnum(binary_operators=("+",), unary_operators=(name,))
    tree = de.Node(1, de.Node(feature=1))
    X = np.asfortranarray(np.array([zs], dtype=dtype))
    for options in (EE, NOEE):
        out = np.zeros(len(zs), dtype=dtype)
        ok = np.zeros(1, dtype=np.uint8)
        tape, consts = de.flatten(tree, ops, dtype)
        lib, ctx = api.library(), api.default_context()
        ctx.check(lib.de_eval_tree_array(ctx._h, api._dtype_code(dtype), tape.ctypes.data, len(tape), None, 0, X.ctypes.data, 1, len(zs),
                                         options | 32, out.ctypes.data, ok.ctypes.data))
        ref, rok = co.eval_tree_array(tape, consts, X, dtype, options, elementwise=True)
        assert bool(ok[0]) == rok
        # per element: same finiteness, same signs of zero parts, values close
        for z, a, b in zip(zs, out, ref):
            assert np.isfinite(a) == np.isfinite(b), (name, z, a, b)
            for pa, pb in ((a.real, b.real), (a.imag, b.imag)):
                assert np.isnan(pa) == np.isnan(pb), (name, z, a, b)
                if pa == 0 and pb == 0:
                    assert np.signbit(pa) == np.signbit(pb), (name, z, a, b)
                elif np.isfinite(pb):
                    assert abs(pa - pb) <= 1e-5 * max(abs(b), 1e-300) if dtype == np.complex64 else abs(pa - pb) <= 1e-13 * abs(b), (name, z, a, b)


@pytest.mark.parametrize("dtype", CDTYPES, ids=["cf32", "cf64"])
def test_division_by_tiny_and_huge_denominators(co, dtype):
    R = REAL_OF[np.dtype(dtype)]
    fi = np.finfo(R)
    ws = [complex(fi.tiny, fi.tiny), complex(fi.max / 4, fi.max / 4), complex(fi.tiny * 4, 0.0), complex(1.0, fi.max / 2),
          complex(fi.max, 0.0), complex(0.0, 0.0)]
    X = np.asfortranarray(np.array([[1.5 - 0.5j] * len(ws), ws], dtype=dtype))
    tree = de.Node(4, de.Node(feature=1), de.Node(feature=2))
    tape, consts = de.flatten(tree, ARITH, dtype)
    for options in (EE, NOEE):
        out = np.zeros(len(ws), dtype=dtype)
        ok = np.zeros(1, dtype=np.uint8)
        lib, ctx = api.library(), api.default_context()
        ctx.check(lib.de_eval_tree_array(ctx._h, api._dtype_code(dtype), tape.ctypes.data, len(tape), None, 0, X.ctypes.data, 2, len(ws),
                                         options | 32, out.ctypes.data, ok.ctypes.data))
        ref, rok = co.eval_tree_array(tape, consts, X, dtype, options, elementwise=True)
        assert bool(ok[0]) == rok
        assert (np.isfinite(out) == np.isfinite(ref)).all()
        with np.errstate(all="ignore"):
            fin = np.isfinite(ref)
            err = np.abs(out[fin].astype(np.complex128) - ref[fin].astype(np.complex128))
            assert (err <= 4 * fi.eps * np.abs(ref[fin].astype(np.complex128)) + fi.tiny).all(), (out, ref)


@pytest.mark.parametrize("dtype", CDTYPES, ids=["cf32", "cf64"])
def test_wide_X_takes_the_gather_variant(co, dtype):
    F = 17  # 17 feature rows of 4096 B are past the 64 KB tile: the DIRECT kernel
    trees, ops = _population("bench", n=24, seed=31)
    rng = np.random.default_rng(5)
    for t in trees:
        for n in t:
            if n.degree == 0 and not n.constant:
                n.feature = int(rng.integers(1, F + 1))
    X = _X(F, 1500, dtype, seed=17)
    pop = api.Population(trees, ops, dtype, n_features=F, eval_context=api.EvalContext(early_exit=False))
    out, ok = pop.eval(X)
    assert "direct" in api.library().de_ctx_last_kernel_name(pop.ctx._h).decode()
    _compare(trees, ops, X, dtype, out, ok, co, NOEE, "wide")
    pop.close()


@pytest.mark.parametrize("dtype", CDTYPES, ids=["cf32", "cf64"])
def test_refused_entry_points_touch_no_output(dtype):
    lib = api.library()
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    tree = de.Node(1, de.Node(feature=1), de.Node(val=0.5 + 0.5j))
    pop = api.Population([tree], ops, dtype, n_features=1)
    N = 16
    X = np.asfortranarray(np.ones((1, N), dtype=dtype))
    y = np.ones(N, dtype=dtype)
    ctx, p = pop.ctx._h, pop._h
    bufs = [np.full(512, 7, dtype=np.uint8) for _ in range(5)]
    ptr = [b.ctypes.data for b in bufs]
    off = np.zeros(1, dtype=np.int64)
    starts = np.array([0, N], dtype=np.int64)
    calls = {
        "de_eval_grad": lambda: lib.de_eval_grad(ctx, p, X.ctypes.data, N, 1, None, 0, ptr[0], N, ptr[1], None, ptr[2]),
        "de_eval_diff": lambda: lib.de_eval_diff(ctx, p, X.ctypes.data, N, 1, 0, ptr[0], ptr[1], N, ptr[2]),
        "de_eval_pullback_dX": lambda: lib.de_eval_pullback_dX(ctx, p, X.ctypes.data, N, 1, None, y.ctypes.data, ptr[0], None, ptr[2]),
        "de_eval_loss": lambda: lib.de_eval_loss(ctx, p, X.ctypes.data, N, 1, None, y.ctypes.data, None, 0, ptr[0], ptr[2]),
        "de_eval_loss_grad": lambda: lib.de_eval_loss_grad(ctx, p, X.ctypes.data, N, 1, None, 1, y.ctypes.data, None, 0, ptr[0],
                                                            ptr[1], None, ptr[2]),
        "de_eval_loss_grad_by_class": lambda: lib.de_eval_loss_grad_by_class(ctx, p, X.ctypes.data, N, 1, None, 0, y.ctypes.data, None,
                                                                              0, starts.ctypes.data, ptr[0], ptr[1], off.ctypes.data,
                                                                              ptr[3], ptr[2]),
        "de_ctx_declare_dataset": lambda: lib.de_ctx_declare_dataset(ctx, api._dtype_code(dtype), ptr[4], N, 1, 1),
    }
    for name, call in calls.items():
        rc = call()
        assert rc == 7, (name, rc)
        assert "complex" in lib.de_last_error(ctx).decode(), name
        assert all((b == 7).all() for b in bufs), f"{name} wrote an output"
    for meth, args in (("eval_grad", (X,)), ("eval_diff", (X, 1)), ("eval_loss", (X, y)), ("eval_loss_grad", (X, y)),
                       ("eval_pullback_dX", (X, y))):
        with pytest.raises(api.DeviceError, match="DE_ERR_UNSUPPORTED"):
            getattr(pop, meth)(*args)
    # parametric complex programs are refused at creation; a refused opcode names itself
    import ctypes as C
    h = C.c_void_p()
    tape, consts = de.flatten(tree, ops, dtype)
    noff, coff = np.array([0, len(tape)], dtype=np.int64), np.array([0, len(consts)], dtype=np.int64)
    assert lib.de_program_create(ctx, api._dtype_code(dtype), tape.ctypes.data, noff.ctypes.data, 1, consts.ctypes.data, coff.ctypes.data,
                                 1, 2, 7, C.byref(h)) == 7
    opsa = de.OperatorEnum(binary_operators=("+",), unary_operators=("abs",))
    ta, ca = de.flatten(de.Node(1, de.Node(feature=1)), opsa, dtype)
    assert lib.de_program_create(ctx, api._dtype_code(dtype), ta.ctypes.data, noff.ctypes.data, 1, None, np.zeros(2, np.int64).ctypes.data,
                                 1, 0, 7, C.byref(h)) == 3
    assert "abs" in lib.de_last_error(ctx).decode()
    out, ok = pop.eval(X)
    assert ok[0] and (out[0] == np.array(1.5 + 0.5j, dtype=dtype)).all()
    pop.close()


@pytest.mark.parametrize("dtype", CDTYPES, ids=["cf32", "cf64"])
def test_certificate(co, dtype):
    trees, ops = _population("bench", n=48, seed=99)
    X = _X(5, 2000, dtype, seed=4)
    pop = api.Population(trees, ops, dtype, n_features=5, eval_context=api.EvalContext(strict_flags=True))
    out, ok = pop.eval(X)
    okc, cert, mx = pop.sum_certificate(X)
    np.testing.assert_array_equal(okc, np.asarray(ok, dtype=bool))
    assert cert.sum() > 0
    R = REAL_OF[np.dtype(dtype)]
    top = float(np.finfo(R).max)
    for t in np.nonzero(cert)[0]:
        # a certified tree's `sum` flag equals its element flag (the reference's is_valid_array, summed componentwise)
        tape, consts = de.flatten(trees[t], ops, dtype)
        _, ok_sum = co.eval_tree_array(tape, consts, X, dtype, EE, elementwise=False)
        _, ok_el = co.eval_tree_array(tape, consts, X, dtype, EE, elementwise=True)
        assert ok_sum == ok_el == bool(okc[t]), t
        if okc[t]:
            assert mx[t] * X.shape[1] * 1.001 < top
    pop.close()
