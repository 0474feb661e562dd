"""Float16 forward-mode gradients, host side: the Float16 CPU oracle's eval_grad_tree_array / eval_diff_tree_array
(tests/oracle_f16/, de_oracle_grad_f16 / de_oracle_diff_f16) against an independent numpy binary16 dual interpreter, the reference's own
Float16 acceptance (test/test_derivatives.jl:40-144) on the oracle, and the option bit of the Python interface.  No GPU."""
import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import f16_grad_oracle as fg
import f16_oracle

H = np.float16
IEEE_OPS = de.OperatorEnum(binary_operators=("+", "-", "*", "/"))


@pytest.fixture(scope="module")
def gorc(tmp_path_factory):
    return fg.GradOracle(f16_oracle.build(str(tmp_path_factory.mktemp("f16_oracle"))))


def same_bits(a, b):
    a, b = np.asarray(a, dtype=H), np.asarray(b, dtype=H)
    return (a.view(np.uint16) == b.view(np.uint16)) | (np.isnan(a) & np.isnan(b))


def test_oracle_equals_numpy_dual_interpreter(gorc):
    """200 random 12-node + - * / trees over 3 features, X = 2 randn, 65 columns: values, every gradient row of the three modes, the
    derivative of every direction and the flags, bit for bit on the trees complete in both."""
    trees = de.synth.random_population(200, seed=7, node_count=12, nfeatures=3, operators=IEEE_OPS)
    X = np.asfortranarray((2.0 * np.random.Generator(np.random.PCG64(7)).standard_normal((3, 65))).astype(H))
    complete = {m: 0 for m in (fg.VARIABLE, fg.CONSTANT, fg.BOTH)}
    elements = differences = 0
    for tree in trees:
        tape, consts = de.flatten(tree, IEEE_OPS, H)
        for mode in complete:
            v, g, ok = gorc.grad(tape, consts, X, mode)
            nv, ng, nok = fg.np_dual(tape, consts, X, mode)
            assert ok == nok
            if not ok:
                continue
            complete[mode] += 1
            elements += g.size
            differences += int((~same_bits(g, ng)).sum()) + int((~same_bits(v, nv)).sum())
        for d in range(3):   # eval_diff tests nothing: every tree compares
            v, dv, ok = gorc.diff(tape, consts, X, d)
            nv, ng, _ = fg.np_dual(tape, consts, X, fg.VARIABLE, direction=d)
            assert ok
            differences += int((~same_bits(dv, ng[0])).sum()) + int((~same_bits(v, nv)).sum())
    print(f"[f16 grad] complete trees per mode {complete}, {elements} gradient elements, {differences} differences")
    assert min(complete.values()) >= 100, complete
    assert differences == 0


@pytest.mark.parametrize("seed", range(5))
def test_reference_acceptance_on_the_oracle(gorc, seed):
    """test_derivatives.jl equations 1, 2 (variables) and 4, 5 (constants) on Float16, against the float64 closed forms by the
    reference's rule isapprox(rtol = 0.1) on the norm; eval_diff per feature gives the same rows."""
    X = fg.acceptance_X(seed)
    X64 = X.astype(np.float64)
    for name, tree, ops, mode, closed in fg.acceptance_cases():
        tape, consts = de.flatten(tree, ops, H)
        _, g, ok = gorc.grad(tape, consts, X, mode)
        assert ok, (name, seed)
        want = closed(X64)
        good, err = fg.isapprox_norm(g, want)
        print(f"[f16 grad] {name} seed {seed}: relative norm error {err:.4f}")
        assert good, (name, seed, err)
        assert not fg.isapprox_norm(np.zeros_like(want), want)[0]
        if mode == fg.VARIABLE:
            rows = np.stack([gorc.diff(tape, consts, X, d)[1] for d in range(3)])
            assert same_bits(rows, g).all(), name


def test_option_bit_of_the_python_interface():
    from dynamicexpressions_jl_amd import api
    assert api.OPT_F16_GRAD == 256
    assert api.EvalContext(half_grad=True).option_bits(IEEE_OPS) & 256
    assert not api.EvalContext().option_bits(IEEE_OPS) & 256
