"""CPU tests of the fused loss of Float16 and complex programs (DE_OPT_TYPED_LOSS): the option bit through
EvalContext, the constant in the header, the Python module and the Julia source, and the reference helper of the GPU tests
(tests/typed_loss_reference.py) against hand values."""
import os
import re

import numpy as np

from dynamicexpressions_jl_amd import api
import dynamicexpressions_jl_amd as de
import typed_loss_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eval_context_sets_the_option_bit():
    ops = de.synth.BENCH_OPERATORS
    assert api.EvalContext(typed_loss=True).option_bits(ops) & (1 << 9)
    assert not api.EvalContext().option_bits(ops) & (1 << 9)
    # the bit changes no other one
    assert api.EvalContext(typed_loss=True).option_bits(ops) ^ api.EvalContext().option_bits(ops) == 1 << 9
    assert api.EvalContext(typed_loss=True, half_grad=True).option_bits(ops) & (1 << 8)


def test_header_python_and_julia_agree_on_the_constant():
    header = open(os.path.join(ROOT, "include", "de_hip.h")).read()
    m = re.search(r"DE_OPT_TYPED_LOSS\s*=\s*1u\s*<<\s*(\d+)", header)
    assert m and 1 << int(m.group(1)) == api.OPT_TYPED_LOSS == 512
    julia = open(os.path.join(ROOT, "dynamicexpressions.jl_amd", "julia", "DynamicExpressionsHIPExt.jl")).read()
    mj = re.search(r"const DE_OPT_TYPED_LOSS\s*=\s*UInt32\((\d+)\)", julia)
    assert mj and int(mj.group(1)) == api.OPT_TYPED_LOSS
    assert re.search(r"typed_loss\s*&&\s*\(bits \|= DE_OPT_TYPED_LOSS\)", julia)
    # no other option of the header owns the bit
    bits = [int(b) for b in re.findall(r"DE_OPT_\w+\s*=\s*1u\s*<<\s*(\d+),", header)]
    assert len(bits) == len(set(bits)) and max(bits) == 9


def test_binary16_terms_round_like_float16():
    H = np.float16
    # e = 255: 65025 rounds to 65024 (the spacing there is 32); e = 256: 65536 is past floatmax(Float16) = 65504
    assert ref.f16_terms("L2", H([255]), H([0]))[0] == H(65024) and ref.f16_loss("L2", H([255]), H([0])) == 65024.0
    assert np.isposinf(ref.f16_terms("L2", H([256]), H([0]))[0]) and np.isposinf(ref.f16_loss("L2", H([256]), H([0])))
    assert ref.f16_loss("L1", H([256]), H([0])) == 256.0
    # the residual itself is rounded first: 2049 is no binary16 number (the spacing at 2048 is 2), ties to even
    assert ref.f16_terms("L1", H([2048]), H([-1]))[0] == H(2048)
    # the weighted term is rounded once more: 0.1 (binary16) * 3 = 0.2999..., one binary16
    t = ref.f16_terms("L1", H([3]), H([0]), H([0.1]))
    assert t.dtype == H and t[0] == H(H(0.1) * H(3))
    # the sum of many terms does not saturate at 65504: it is the library's, in a wider type
    assert ref.f16_loss("L2", np.full(100, 255, H), np.zeros(100, H)) == 100 * 65024.0


def test_complex_terms():
    for kind, want in (("L1", 5.0), ("L2", 25.0)):
        s, m = ref.complex_loss(kind, np.array([3 + 4j]), np.array([0j]))
        assert s == want and m == (2.0 if kind == "L1" else 3.0) * want
    s, _ = ref.complex_loss("L2", np.array([1 + 1j, 2 - 1j]), np.array([1j, 2 + 0j]), np.array([2.0, 0.5]))
    assert s == 2.0 * 1.0 + 0.5 * 1.0


def test_weight_zero_excludes_a_nan_sample():
    nan = float("nan")
    assert ref.f16_loss("L2", np.float16([1, nan, 3]), np.float16([0, 0, 0]), np.float16([1, 0, 2])) == 1.0 + 2 * 9.0
    assert np.isnan(ref.f16_loss("L2", np.float16([1, nan, 3]), np.float16([0, 0, 0])))
    s, m = ref.complex_loss("L1", np.array([3 + 4j, complex(nan, 0)]), np.zeros(2, complex), np.array([1.0, 0.0]))
    assert s == 5.0 and m == 10.0
    s, m, big = ref.real_loss("L2", [1.0, nan], [0.0, 0.0], np.array([1.0, 0.0]))
    assert (s, m, big) == (1.0, 3.0, 1.0)
    s, _, _ = ref.real_loss("huber", [3.0, nan], [0.0, 0.0], np.array([2.0, 0.0]), p=1.0)
    assert s == 2.0 * 1.0 * (3.0 - 0.5)


def test_real_terms_match_the_kind_table():
    e = np.array([-2.0, 0.0, 0.5])
    l, m = ref.real_terms("L2", e, np.zeros(3))
    assert np.array_equal(l, e * e) and np.array_equal(m, 3 * e * e)
    l, m = ref.real_terms("L1", e, np.zeros(3))
    assert np.array_equal(l, np.abs(e)) and np.array_equal(m, 2 * np.abs(e))
    l, _ = ref.real_terms("l1_hinge", np.array([0.5, 2.0]), np.array([1.0, 1.0]))
    assert np.array_equal(l, [0.5, 0.0])
