"""The complex CPU oracle (tests/oracle_complex/de_oracle_complex.c) against mpmath, per operator, input region and dtype: no GPU.

The oracle restates Julia's Complex methods on the host libm; tests/test_gpu_complex_accuracy.py bounds the device by the oracle's
error on the same inputs, so the oracle's own error is pinned here: its maximum normwise error |got - true| / spacing(|true|) for every
operator, and its maximum componentwise error where the formula delivers one (tests/complex_accuracy.py has the regions, the reference
and both measures).  A cap is the maximum measured on this file's populations (`PYTHONPATH=. python tests/complex_accuracy.py` prints them), rounded
up to the next half ulp, plus 0.5; the comment above each cap names the region and the input of the maximum.  neg is a sign flip: 0."""
import numpy as np
import pytest

import complex_accuracy as ca
import complex_oracle

# (operator, dtype) -> (normwise cap, componentwise cap or None), in ulps of the component type
CAPS = {
    # normwise 1.55 in circle at (-0.16587257385253906+0.9858723878860474j); componentwise 2.04 in circle at (-1.0851147174835205-0.5182570815086365j)
    ("sqrt", "complex64"): (2.5, 3.0),
    # normwise 1.41 in ring at (0.25467675967935066+0.8090722357675186j); componentwise 1.81 in circle at (-1.0665113589842534-0.1222962535529388j)
    ("sqrt", "complex128"): (2.0, 2.5),
    # normwise 1.90 in ring at (0.8158071637153625-0.10185881704092026j)
    ("log", "complex64"): (2.5, None),
    # normwise 1.48 in ordinary at (0.8863609139451211-0.004757748419028933j)
    ("log", "complex128"): (2.0, None),
    # normwise 0.69 in wide_eq at (-0.0004833797283936292-0.00044170126784592867j); componentwise 0.50 in circle at (0.003806991269811988+1.3738499879837036j)
    ("inv", "complex64"): (1.5, 1.0),
    # normwise 1.75 in circle at (0.6976626029408282+0.7164265323514801j); componentwise 2.20 in ring at (0.4224838699581657-0.8257840703835263j)
    ("inv", "complex128"): (2.5, 3.0),
    # normwise 1.38 in expz at (16.394596099853516+13.431607246398926j); componentwise 1.74 in expz at (12.463960647583008+12.036782264709473j)
    ("exp", "complex64"): (2.0, 2.5),
    # normwise 1.49 in ordinary at (-0.005463113151493137-0.7864474926900934j); componentwise 1.75 in ordinary at (0.0021773868455151903+0.1840049909851772j)
    ("exp", "complex128"): (2.0, 2.5),
    # normwise 1.74 in trigbig at (-5897.1435546875+0.30658644437789917j); componentwise 2.18 in ordinary at (3.335049867630005-0.015630990266799927j)
    ("sin", "complex64"): (2.5, 3.0),
    # normwise 1.79 in trigbig at (6167.902492494004-0.4461819423676179j); componentwise 2.23 in trigbig at (-388.30282977151-1.8301665571701955j)
    ("sin", "complex128"): (2.5, 3.0),
    # normwise 1.70 in ordinary at (-9.665090560913086-0.10585086792707443j); componentwise 2.41 in ordinary at (0.4663936495780945-0.5239940881729126j)
    ("cos", "complex64"): (2.5, 3.0),
    # normwise 1.67 in trigbig at (-1838.6064726155137+0.14044445617691537j); componentwise 2.48 in trigbig at (-2589.2182896452496+0.7407533290176249j)
    ("cos", "complex128"): (2.5, 3.0),
    # normwise 1.74 in ordinary at (-0.0028234533965587616+1.2426559925079346j); componentwise 2.22 in ordinary at (-7.944713115692139+0.002793086925521493j)
    ("sinh", "complex64"): (2.5, 3.0),
    # normwise 1.62 in ordinary at (-0.01272509296461046+0.006726721290109966j); componentwise 2.19 in ordinary at (9.141192712826873+1.7576632902947338j)
    ("sinh", "complex128"): (2.5, 3.0),
    # normwise 1.77 in ordinary at (0.026454798877239227+0.03443583473563194j); componentwise 2.17 in expz at (-5.54984188079834-4.242259502410889j)
    ("cosh", "complex64"): (2.5, 3.0),
    # normwise 1.94 in ordinary at (-0.42261801130794896-8.933978719155592j); componentwise 2.26 in ordinary at (-0.0011180278888353694-0.011969156760935197j)
    ("cosh", "complex128"): (2.5, 3.0),
    # normwise 3.20 in poles at (0.11811202764511108-6.281193733215332j); componentwise 4.56 in poles at (-0.08836859464645386+4.712385177612305j)
    ("tanh", "complex64"): (4.0, 5.5),
    # normwise 3.46 in poles at (-0.007604237335984664+6.2831865631534445j); componentwise 5.01 in ordinary at (0.00272779160881326+1.4207738670775016j)
    ("tanh", "complex128"): (4.0, 6.0),
    # normwise 3.70 in poles_swapped at (-3.1228811740875244+0.12145600467920303j); componentwise 4.28 in ordinary at (-0.006398671306669712-9.037742614746094j)
    ("tan", "complex64"): (4.5, 5.0),
    # normwise 3.79 in poles_swapped at (-1.5713211387749282+0.5702943427041464j); componentwise 3.89 in poles_swapped at (6.283449097830159+0.00011795047334434264j)
    ("tan", "complex128"): (4.5, 4.5),
    # normwise 1.03 in ordinary at (-0.002205655677244067-0.004799004644155502j)
    ("square", "complex64"): (2.0, None),
    # normwise 1.00 in ordinary at (-0.25903651631840646+1.2444714678069277j)
    ("square", "complex128"): (2.0, None),
    # normwise 2.00 in ordinary at (-0.3381306827068329-6.028157711029053j)
    ("cube", "complex64"): (2.5, None),
    # normwise 1.80 in ordinary at (0.06724226896497425+0.003010348560204916j)
    ("cube", "complex128"): (2.5, None),
    # normwise 4.54 in ordinary at (-8.617210388183594+0.0012487360509112477j)
    ("custom_cos", "complex64"): (5.5, None),
    # normwise 3.79 in ordinary at (0.003012098363207765-9.226602260528265j)
    ("custom_cos", "complex128"): (4.5, None),
    # normwise 0.00 in ordinary at (0.05731750279664993+0.0012345960130915046j)
    ("neg", "complex64"): (0.0, None),
    # normwise 0.00 in ordinary at (-1.230228326251561+0.03318995363028112j)
    ("neg", "complex128"): (0.0, None),
    # normwise 0.70 in ordinary/ordinary at (0.07718882709741592+0.056620415300130844j), (6.019308567047119-1.7103959321975708j)
    ("/", "complex64"): (1.5, None),
    # normwise 2.68 in ordinary/ordinary at (0.15147877384162517-0.18060167041828645j), (0.04341262506658525+0.042426519408105934j)
    ("/", "complex128"): (3.5, None),
    # normwise 1.37 in big/big at (2.2637965163364352e+17-1.0841104763479654e+17j), (3.922312225179566e+17-3.788088999621427e+17j)
    ("*", "complex64"): (2.0, None),
    # normwise 1.21 in ordinary/ordinary at (-0.010606355258621487-0.003980129697050578j), (0.1296229792151858-0.24818296584854194j)
    ("*", "complex128"): (2.0, None),
}


@pytest.fixture(scope="module")
def co(tmp_path_factory):
    return complex_oracle.build(str(tmp_path_factory.mktemp("complex_oracle")))


CASES = [(op, dt) for op in list(ca.UNARY) + list(ca.BINARY_REGIONS) for dt in ca.CDTYPES]


@pytest.mark.parametrize("op,dtype", CASES, ids=[f"{op}-{np.dtype(dt).name}" for op, dt in CASES])
def test_oracle_against_mpmath(co, op, dtype):
    pop = ca.population(op, dtype)
    got, _ = ca.oracle_eval(co, pop)
    cap_n, cap_c = CAPS[(op, np.dtype(dtype).name)]
    assert cap_c is not None or op not in ca.COMPONENTWISE
    for region, m in ca.region_maxima(pop, got).items():
        print(f"{op} {np.dtype(dtype).name} {region}: kept {m['kept']:.3f}, normwise {m['norm']:.3f} at {m['norm_at']}, "
              f"componentwise {m['comp']:.3f} at {m['comp_at']}")
        assert m["kept"] >= ca.MIN_KEPT, (region, m["kept"])
        assert m["norm"] <= cap_n, f"{op} {region}: normwise {m['norm']:.3f} ulp at {m['norm_at']} (cap {cap_n})"
        if ca.has_componentwise(op, region):
            assert m["comp"] <= cap_c, f"{op} {region}: componentwise {m['comp']:.3f} ulp at {m['comp_at']} (cap {cap_c})"


@pytest.mark.parametrize("form", ["cx", "xc"])
@pytest.mark.parametrize("op,dtype", [c for c in CASES if c[0] in ca.BINARY_REGIONS],
                         ids=[f"{op}-{np.dtype(dt).name}" for op, dt in CASES if op in ca.BINARY_REGIONS])
def test_oracle_constant_forms_against_mpmath(co, op, dtype, form):
    """c op x and x op c (one tree per constant): the same operator code, so the same caps."""
    pop = ca.population(op, dtype, form)
    got, _ = ca.oracle_eval(co, pop)
    cap_n, _ = CAPS[(op, np.dtype(dtype).name)]
    for region, m in ca.region_maxima(pop, got).items():
        print(f"{op} {form} {np.dtype(dtype).name} {region}: kept {m['kept']:.3f}, normwise {m['norm']:.3f} at {m['norm_at']}")
        assert m["kept"] >= ca.MIN_KEPT, (region, m["kept"])
        assert m["norm"] <= cap_n, f"{op} {form} {region}: normwise {m['norm']:.3f} ulp at {m['norm_at']} (cap {cap_n})"


@pytest.mark.parametrize("dtype", ca.CDTYPES, ids=["cf32", "cf64"])
@pytest.mark.parametrize("op", ["+", "-"])
def test_oracle_add_sub_have_numpy_bits(co, op, dtype):
    """+ and - are componentwise IEEE operations: the bits of numpy's complex arithmetic in that dtype, cancelling pairs included."""
    import dynamicexpressions_jl_amd as de
    a, b = ca.addsub_inputs(op, dtype)
    R = ca.real_of(dtype)
    want = a + b if op == "+" else a - b
    assert (np.abs(want[len(a) // 2:]) < np.abs(a[len(a) // 2:])).mean() > 0.3  # the cancelling half cancels
    ops = ca.operator_enum(op)
    tape, consts = de.flatten(de.Node(1, de.Node(feature=1), de.Node(feature=2)), ops, dtype)
    got, ok = co.eval_tree_array(tape, consts, np.stack([a, b]), dtype, 6, elementwise=True)
    assert ok
    np.testing.assert_array_equal(got.view(R), want.view(R))


@pytest.mark.parametrize("dtype", ca.CDTYPES, ids=["cf32", "cf64"])
def test_tanh_guard_zero_sign_where_twice_the_imaginary_part_overflows(co, dtype):
    """Regression: behind tanh's overflow guard the zero imaginary part has the sign of eta sin(2|eta|).  For |eta| > floatmax / 2 the
    argument 2|eta| is Inf, sin(Inf) is NaN and the oracle took the sign bit of libm's NaN (the device another one).  The sign of
    sin(2a) now comes from sin a cos a there: C99 Annex G's value, numpy's tanh on the host."""
    import dynamicexpressions_jl_amd as de
    z = ca.guard_overflow_points(dtype)
    R = ca.real_of(dtype)
    tape, consts = de.flatten(de.Node(1, de.Node(feature=1)), ca.operator_enum("tanh"), dtype)
    got, _ = co.eval_tree_array(tape, consts, z[None, :], dtype, 6, elementwise=True)
    with np.errstate(all="ignore"):
        want = np.tanh(z)
    assert (want.imag == 0).all() and np.signbit(want.imag).any() and not np.signbit(want.imag).all()
    np.testing.assert_array_equal(got.view(R), want.view(R))
