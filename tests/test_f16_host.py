"""DE_F16 (Float16) on the host, no GPU: the lowering of binary16 tapes, the dtype checks of the C ABI and the Python layer, and the
Float16 CPU oracle (tests/oracle_f16/de_oracle_f16.c) pinned against a numpy binary16 interpreter and the reference's Float16 known
answers (tests/golden/reference_known_answers_f16.json).  DESIGN.md §13."""
import json
import os
import warnings

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
from dynamicexpressions_jl_amd import api
from helpers import case_options, case_tree
import f16_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_known_answers_f16.json")))["cases"]
OPS4 = de.OperatorEnum(binary_operators=("+", "-", "*", "/"), unary_operators=("cos",))


@pytest.fixture(scope="module")
def f16o(tmp_path_factory):
    return f16_oracle.build(str(tmp_path_factory.mktemp("f16_oracle")))


def _lower(tree, dtype=np.float16, options=7):
    tape, consts = de.flatten(tree, OPS4, dtype)
    return api.lower_tape(tape, consts, 1, options=options, dtype=dtype)


def test_dtype_codes():
    assert api.DE_F16 == 2
    assert api._dtype_code(np.float16) == 2
    assert api._dtype_code(np.float32) == 0 and api._dtype_code(np.float64) == 1
    with pytest.raises(TypeError):
        api._dtype_code(np.int32)
    assert api._x_dtype(np.zeros((2, 3), dtype=np.float16)) == np.float16


def test_lower_tape_rounds_constants_to_binary16():
    # x1 + 0.1: the constant operand carries Float16(0.1) = 0.0999755859375, exactly, in its Float32 immediate
    w, meta = _lower(de.Node(1, de.Node(feature=1), de.Node(val=0.1)))
    imm = w[:, 2].copy().view(np.float32)
    assert 0.0999755859375 in imm.tolist()
    assert float(np.float16(0.1)) == 0.0999755859375
    assert meta["host_ok_eval"] and meta["host_ok_grad"]
    # ... while the Float32 lowering keeps Float32(0.1)
    w32, _ = _lower(de.Node(1, de.Node(feature=1), de.Node(val=0.1)), np.float32)
    assert float(np.float32(0.1)) in w32[:, 2].copy().view(np.float32).tolist()


def test_constant_beyond_floatmax16_is_inf_and_clears_the_host_flag():
    tree = de.Node(1, de.Node(feature=1), de.Node(val=1e5))
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # Float16(1e5) == Inf16 is data, not a warning
        tape, consts = de.flatten(tree, OPS4, np.float16)
    assert np.isinf(consts[0])
    _, meta = api.lower_tape(tape, consts, 1, dtype=np.float16)
    assert not meta["host_ok_eval"] and not meta["host_ok_grad"]
    # 65504 = floatmax(Float16) is finite; 65520 rounds to Inf
    assert _lower(de.Node(1, de.Node(feature=1), de.Node(val=65504.0)))[1]["host_ok_eval"]
    assert not _lower(de.Node(1, de.Node(feature=1), de.Node(val=65520.0)))[1]["host_ok_eval"]


@pytest.mark.parametrize("dtype", [3, 5, -1])
def test_other_dtypes_stay_invalid(dtype):
    tape, consts = de.flatten(de.Node(1, de.Node(feature=1), de.Node(val=0.5)), OPS4, np.float32)
    lib = api.library()
    assert lib.de_lower_tape(dtype, tape.ctypes.data, len(tape), consts.ctypes.data, 1, 1, 0, 7, None, 0, None) == -1
    assert lib.de_lower_tape_stage(dtype, tape.ctypes.data, len(tape), consts.ctypes.data, 1, 1, 0, 7, 2, None, 0) == -1


def test_lower_tape_stages_f16():
    tape, consts = de.flatten(de.Node(1, de.Node(feature=1), de.Node(val=0.1)), OPS4, np.float16)
    b16 = api.lower_tape_stage(tape, consts, 1, 2, dtype=np.float16)
    b32 = api.lower_tape_stage(tape, consts.astype(np.float32), 1, 2, dtype=np.float32)
    np.testing.assert_array_equal(b16, b32)  # a binary16 tape binds like the Float32 tape of the same (binary16) constants
    assert api.lower_tape_stage(tape, consts, 1, 3, dtype=np.float16).shape[0] == 0  # no threaded form: F16 never runs that kernel


def test_f16_oracle_is_binary16_per_operation(f16o):
    assert f16o.lib.de_oracle_f16_abi() == api.ABI_VERSION
    cube = de.OPCODES[("cube", 1)]
    assert np.isinf(f16o.unary(cube, 300.0))  # 300 * 300 = 90000 is Inf in binary16 before the second product
    sq = de.OPCODES[("square", 1)]
    assert f16o.unary(sq, 255.0) == np.float16(255.0) * np.float16(255.0)
    c = np.float16(np.cos(np.float32(np.float16(0.7))))  # custom_cos = cos(x)^2: cos rounded, then the product
    assert f16o.unary(de.OPCODES[("custom_cos", 1)], 0.7) == c * c
    pa2 = de.OPCODES[("pow_abs2", 2)]
    x, y = np.float16(1.7), np.float16(2.3)
    lx = np.float16(np.log(np.float32(x)))
    assert f16o.binary(pa2, x, y) == np.float16(np.exp(np.float32(np.float16(y * lx))))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_f16_oracle_bit_equal_to_numpy_binary16_on_ieee_exact_trees(f16o, seed):
    ops = de.OperatorEnum(binary_operators=("+", "-", "*", "/"))
    trees = de.synth.random_population(40, seed=seed, node_count=11, nfeatures=3, operators=ops)
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((3, 257)) * 4).astype(np.float16)
    X[0, :8] = np.float16([6e-8, -6e-8, 1e-5, 65504, -65504, 0.0, -0.0, 3e-7])  # subnormals and the edges
    n_cmp = 0
    for tree in trees:
        tape, consts = de.flatten(tree, ops, np.float16)
        y, ok = f16o.eval_tree_array(tape, consts, X, options=7 & ~1)  # no early exit: every sample is computed
        y_np, _ = f16_oracle.np_eval_f16(tree, ops, X)
        np.testing.assert_array_equal(y.view(np.uint16)[np.isfinite(y_np)], y_np.view(np.uint16)[np.isfinite(y_np)])
        assert np.array_equal(np.isnan(y), np.isnan(y_np)) and np.array_equal(np.isinf(y), np.isinf(y_np))
        n_cmp += int(np.isfinite(y_np).sum())
    assert n_cmp > 1000


def test_f16_oracle_keeps_subnormals(f16o):
    sub = np.float16(2.0 ** -24)  # the smallest binary16 subnormal
    X = np.array([[sub, np.float16(2.0 ** -20), np.float16(-3 * 2.0 ** -24)]], dtype=np.float16)
    x1 = de.Node(feature=1)
    for tree, want in [(x1, X[0]), (de.Node(1, x1, x1), X[0] + X[0]), (de.Node(4, x1, de.Node(val=2.0)), X[0] / np.float16(2.0))]:
        tape, consts = de.flatten(tree, OPS4, np.float16)
        y, ok = f16o.eval_tree_array(tape, consts, X)
        assert ok
        np.testing.assert_array_equal(y.view(np.uint16), want.astype(np.float16).view(np.uint16))
    assert (X[0] / np.float16(2.0))[0] == 0.0  # (2^-25 ties to even: 0)


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_f16_oracle_reproduces_golden(f16o, case):
    tree, ops = case_tree(case)
    tape, consts = de.flatten(tree, ops, np.float16)
    X = np.asfortranarray(np.asarray(case["X"], dtype=np.float64).astype(np.float16))
    exp = case["expect"]
    y, ok = f16o.eval_tree_array(tape, consts, X, case_options(case))
    assert ok == exp["ok"], f"{case['name']} ({case['cite']})"
    y2, ok2 = f16o.eval_tree_array(tape, consts, X, case_options(case), elementwise=True)
    assert ok2 == exp["ok"]
    if ok and "y" in exp:
        want = np.asarray(exp["y"], dtype=np.float64)
        got = y.astype(np.float64)
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), fin), case["name"]
        assert np.all(np.abs(got[fin] - want[fin]) <= exp.get("atol", 0) + exp.get("rtol", 0) * np.abs(want[fin])), case["name"]


def test_golden_f16_file_is_what_the_generator_writes(tmp_path):
    """The JSON is generated (tests/golden/make_reference_known_answers_f16.py): re-running the generator reproduces its cases — names,
    citations, trees, inputs, flags and tolerances exactly; the expected values within each case's own tolerance (numpy's float16 sin / cos
    run numpy's CPU-dispatched float32 kernels: another build may round a binary16 result the other way)."""
    import runpy
    import shutil
    src = os.path.join(ROOT, "tests", "golden", "make_reference_known_answers_f16.py")
    dst = tmp_path / "gen.py"
    shutil.copy(src, dst)
    runpy.run_path(str(dst), run_name="__main__")
    with open(tmp_path / "reference_known_answers_f16.json") as fh:
        regenerated = json.load(fh)["cases"]
    assert len(regenerated) == len(GOLDEN)
    for new, old in zip(regenerated, GOLDEN):
        ne, oe = dict(new["expect"]), dict(old["expect"])
        yn, yo = ne.pop("y", None), oe.pop("y", None)
        assert json.dumps({**new, "expect": ne}, sort_keys=True) == json.dumps({**old, "expect": oe}, sort_keys=True), old["name"]
        assert (yn is None) == (yo is None), old["name"]
        if yo is not None:
            a, b = np.asarray(yn, dtype=np.float64), np.asarray(yo, dtype=np.float64)
            fin = np.isfinite(b)
            assert np.array_equal(np.isfinite(a), fin), old["name"]
            assert np.all(np.abs(a[fin] - b[fin]) <= oe.get("atol", 0) + oe.get("rtol", 0) * np.abs(b[fin])), old["name"]
