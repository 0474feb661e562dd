"""DE_CF32 / DE_CF64 (ComplexF32 / ComplexF64) on the host, no GPU: dtype codes, complex constants through flatten, the lowering's
opcode admission, and the complex CPU oracle (tests/oracle_complex/de_oracle_complex.c) pinned against Python's cmath on ordinary
arguments and against the reference's complex known answers (tests/golden/reference_known_answers_complex.json).  DESIGN.md §14."""
import cmath
import json
import os

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
from dynamicexpressions_jl_amd import api
from dynamicexpressions_jl_amd.operators import UnsupportedOperatorError
import complex_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_known_answers_complex.json")))["cases"]
CDTYPES = (np.complex64, np.complex128)
SUPPORTED_UNARY = ("neg", "square", "cube", "inv", "sqrt", "exp", "log", "sin", "cos", "tan", "sinh", "cosh", "tanh", "custom_cos")
SUPPORTED_BINARY = ("+", "-", "*", "/")
REFUSED = [("abs", 1), ("relu", 1), ("sign", 1), ("round", 1), ("floor", 1), ("ceil", 1), ("cbrt", 1), ("gamma", 1), ("safe_log", 1),
           ("safe_log2", 1), ("safe_log10", 1), ("safe_log1p", 1), ("safe_sqrt", 1), ("safe_acosh", 1), ("exp2", 1), ("log2", 1),
           ("log10", 1), ("log1p", 1), ("asin", 1), ("acos", 1), ("atan", 1), ("asinh", 1), ("acosh", 1), ("atanh", 1),
           ("max", 2), ("min", 2), ("mod", 2), ("rem", 2), ("greater", 2), ("pow_abs2", 2), ("^", 2), ("fma", 3), ("clamp", 3), ("max", 3)]


@pytest.fixture(scope="module")
def co(tmp_path_factory):
    return complex_oracle.build(str(tmp_path_factory.mktemp("complex_oracle")))


def test_dtype_codes():
    assert (api.DE_CF32, api.DE_CF64) == (3, 4)
    assert api._dtype_code(np.complex64) == 3
    assert api._dtype_code(np.complex128) == 4
    assert api._x_dtype(np.zeros((2, 3), dtype=np.complex64)) == np.complex64
    assert api._x_dtype(np.zeros((2, 3), dtype=np.complex128)) == np.complex128
    with pytest.raises(TypeError):
        api._dtype_code(np.complex256) if hasattr(np, "complex256") else api._dtype_code(np.int8)


@pytest.mark.parametrize("dtype", [0, 1, 2, 5, 6, -1])
def test_complex_lowering_hooks_take_complex_dtypes_only(dtype):
    tape, consts = de.flatten(de.Node(1, de.Node(feature=1), de.Node(val=0.5)), de.OperatorEnum(binary_operators=("+",)), np.complex128)
    lib = api.library()
    assert lib.de_lower_tape_complex(dtype, tape.ctypes.data, len(tape), consts.ctypes.data, 1, 1, 0, 7, None, 0, None) == -1
    assert lib.de_lower_tape_stage_complex(dtype, tape.ctypes.data, len(tape), consts.ctypes.data, 1, 1, 0, 7, 2, None, 0) == -1


@pytest.mark.parametrize("dtype", CDTYPES)
def test_real_lowering_hooks_keep_refusing_complex_codes(dtype):
    tape, consts = de.flatten(de.Node(1, de.Node(feature=1), de.Node(val=0.5 + 1j)), de.OperatorEnum(binary_operators=("+",)), dtype)
    lib, code = api.library(), api._dtype_code(dtype)
    assert lib.de_lower_tape(code, tape.ctypes.data, len(tape), consts.ctypes.data, 1, 1, 0, 7, None, 0, None) == -1
    assert lib.de_lower_tape_stage(code, tape.ctypes.data, len(tape), consts.ctypes.data, 1, 1, 0, 7, 2, None, 0) == -1
    assert lib.de_lower_tape_complex(code, tape.ctypes.data, len(tape), consts.ctypes.data, 1, 1, 0, 7, None, 0, None) > 0
    b = api.lower_tape_stage(tape, consts, 1, 2, dtype=dtype)
    assert b.shape[0] > 0 and api.lower_tape_stage(tape, consts, 1, 3, dtype=dtype).shape[0] == 0  # no threaded form


def test_complex_constants_survive_flatten():
    ops = de.OperatorEnum(binary_operators=("+", "*"), unary_operators=("cos",))
    tree = de.Node(1, de.Node(2, de.Node(val=0.1j), de.Node(feature=1)), de.Node(1, de.Node(val=2 - 3j)))
    for dt in CDTYPES:
        _, consts = de.flatten(tree, ops, dt)
        assert consts.dtype == dt
        np.testing.assert_array_equal(consts, np.array([0.1j, 2 - 3j], dtype=dt))
    vals, refs = de.get_scalar_constants(tree)
    assert vals.dtype == np.complex128 and vals[0] == 0.1j
    de.set_scalar_constants(tree, [1 + 1j, 0.0 + 0j], refs)
    assert tree.children[0].children[0].val == 1 + 1j and isinstance(tree.children[1].children[0].val, complex)
    # a real tree flattens as before
    real = de.Node(1, de.Node(feature=1), de.Node(val=0.5))
    assert de.get_scalar_constants(real)[0].dtype == np.float64
    assert de.flatten(real, ops, np.float32)[1].dtype == np.float32


@pytest.mark.parametrize("dtype", CDTYPES)
def test_supported_opcodes_lower_and_constants_are_table_indices(dtype):
    ops = de.OperatorEnum(binary_operators=SUPPORTED_BINARY, unary_operators=SUPPORTED_UNARY)
    x = de.Node(feature=1)
    for k in range(1, len(SUPPORTED_UNARY) + 1):
        tape, consts = de.flatten(de.Node(k, x), ops, dtype)
        api.lower_tape(tape, consts, 1, dtype=dtype)
    for k in range(1, len(SUPPORTED_BINARY) + 1):
        tape, consts = de.flatten(de.Node(k, x, de.Node(val=2.5 - 1j)), ops, dtype)
        w, meta = api.lower_tape(tape, consts, 1, dtype=dtype)
        assert meta["host_ok_eval"]
        assert 0 in w[:, 2].tolist()  # the constant operand's immediate: index 0 of the constant table
    # +(x, y, z)
    ops3 = de.OperatorEnum(binary_operators=("+",), unary_operators=(), ternary_operators=("+",)) if _has_ternary() else None
    if ops3 is not None:
        tape, consts = de.flatten(de.Node(1, x, de.Node(feature=2), de.Node(val=1j)), ops3, dtype)
        api.lower_tape(tape, consts, 2, dtype=dtype)


def _has_ternary():
    import inspect
    return "ternary_operators" in inspect.signature(de.OperatorEnum).parameters


@pytest.mark.parametrize("dtype", CDTYPES)
def test_non_finite_complex_constant_clears_the_host_flag(dtype):
    ops = de.OperatorEnum(binary_operators=("+",))
    for v in (complex(0.0, float("inf")), complex(float("nan"), 0.0)):
        tape, consts = de.flatten(de.Node(1, de.Node(feature=1), de.Node(val=v)), ops, dtype)
        _, meta = api.lower_tape(tape, consts, 1, dtype=dtype)
        assert not meta["host_ok_eval"]


@pytest.mark.parametrize("name,degree", REFUSED)
def test_refused_opcodes_fail_the_lowering(name, degree):
    code = de.OPCODES[(name, degree)]
    lib = api.library()
    deg = [0] * degree + [degree]
    tape = np.zeros(degree + 1, dtype=de.TAPE_DTYPE) if hasattr(de, "TAPE_DTYPE") else None
    if tape is None:
        from dynamicexpressions_jl_amd.node import TAPE_DTYPE
        tape = np.zeros(degree + 1, dtype=TAPE_DTYPE)
    tape["degree"] = deg
    tape["op"] = [1] * degree + [code]
    tape["arg"] = list(range(degree)) + [0]
    for dt in (3, 4):
        assert lib.de_lower_tape_complex(dt, tape.ctypes.data, len(tape), None, 0, 3, 0, 7, None, 0, None) == -3  # DE_ERR_UNSUPPORTED_OP
    # ... and the same tape is a valid real tape
    assert lib.de_lower_tape(1, tape.ctypes.data, len(tape), None, 0, 3, 0, 7, None, 0, None) > 0


def test_lower_tape_raises_unsupported_operator():
    ops = de.OperatorEnum(binary_operators=("+",), unary_operators=("abs",))
    tape, consts = de.flatten(de.Node(1, de.Node(feature=1)), ops, np.complex128)
    with pytest.raises(UnsupportedOperatorError):
        api.lower_tape(tape, consts, 1, dtype=np.complex128)


ORDINARY = [0.3 + 0.7j, -1.2 + 0.4j, 2.5 - 1.5j, -0.7 - 0.2j, 1.5 + 0j, 0.25j]
CMATH = {"sqrt": cmath.sqrt, "exp": cmath.exp, "log": cmath.log, "sin": cmath.sin, "cos": cmath.cos, "tan": cmath.tan, "sinh": cmath.sinh,
         "cosh": cmath.cosh, "tanh": cmath.tanh, "neg": lambda z: -z, "square": lambda z: z * z, "cube": lambda z: z * z * z,
         "inv": lambda z: 1 / z, "custom_cos": lambda z: cmath.cos(z) ** 2}


@pytest.mark.parametrize("name", sorted(CMATH))
def test_oracle_unary_against_cmath(co, name):
    code = de.OPCODES[(name, 1)]
    for z in ORDINARY:
        want = CMATH[name](z)
        got = co.op(np.complex128, 1, code, z)
        assert abs(got - want) <= 1e-14 * max(abs(want), 1e-300), (name, z, got, want)
        z32 = complex(np.complex64(z))
        got32 = co.op(np.complex64, 1, code, z32)
        assert abs(got32 - CMATH[name](z32)) <= 3e-6 * max(abs(CMATH[name](z32)), 1e-30), (name, z, got32)


@pytest.mark.parametrize("name", SUPPORTED_BINARY)
def test_oracle_binary_against_cmath(co, name):
    code = de.OPCODES[(name, 2)]
    f = {"+": lambda a, b: a + b, "-": lambda a, b: a - b, "*": lambda a, b: a * b, "/": lambda a, b: a / b}[name]
    for a in ORDINARY:
        for b in ORDINARY:
            want = f(a, b)
            got = co.op(np.complex128, 2, code, a, b)
            assert abs(got - want) <= 1e-15 * max(abs(want), 1e-300) * 4, (name, a, b, got, want)
            if name != "/":
                assert got == want  # + - * : one rounding per component operation, as Python's complex arithmetic


def test_oracle_edge_cases(co):
    # branch cuts: the sign of a zero imaginary part picks the side
    sq = de.OPCODES[("sqrt", 1)]
    lg = de.OPCODES[("log", 1)]
    assert co.op(np.complex128, 1, sq, complex(-4.0, 0.0)) == 2j
    r = co.op(np.complex128, 1, sq, complex(-4.0, -0.0))
    assert r.imag == -2.0
    assert co.op(np.complex128, 1, lg, complex(-1.0, 0.0)).imag == np.pi
    assert co.op(np.complex128, 1, lg, complex(-1.0, -0.0)).imag == -np.pi
    # exp with a zero imaginary part keeps it: exp(89 + 0im) in ComplexF32 overflows the real part only
    e = co.op(np.complex64, 1, de.OPCODES[("exp", 1)], complex(89.0, 0.0))
    assert np.isinf(e.real) and e.imag == 0.0
    # tanh's overflow branch
    t = co.op(np.complex128, 1, de.OPCODES[("tanh", 1)], complex(400.0, 1.0))
    assert t == complex(1.0, 0.0)


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_golden_cases_in_the_oracle(co, case):
    dt = np.dtype(case["dtype"])
    tape = np.zeros(len(case["tape"]), dtype=de.node.TAPE_DTYPE)
    for i, (d, o, a) in enumerate(case["tape"]):
        tape[i] = (d, o, a)
    consts = np.array([complex(*v) for v in case["consts"]], dtype=dt)
    X = np.array([[complex(*v) for v in row] for row in case["X"]], dtype=dt)
    out, ok = co.eval_tree_array(tape, consts, X, dt)
    assert ok == case["ok"]
    if case["ok"]:
        want = np.array([complex(*v) for v in case["out"]])
        np.testing.assert_allclose(out.astype(np.complex128), want, rtol=max(case["rtol"], 1e-15), atol=0)
