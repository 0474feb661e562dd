"""The DE_F16 accuracy tables of tests/f16_accuracy.py without a GPU: the references are held to mpmath and to exact rational arithmetic,
the conditions of the acceptance rule are asserted on the reference alone, the CPU Float16 oracle (tests/oracle_f16/) is held to the rule at
every point — all 65536 arguments of every unary opcode, the closed grid and the random pairs of every binary one, the triples and the
cancelling family of every ternary one — the composites to their step models, and four plausible wrong models are shown to fail.
tests/test_gpu_f16_accuracy.py holds the device to the same tables.  DESIGN.md §13.1."""
import numpy as np
import pytest

import f16_accuracy as fa
import f16_oracle
import operator_accuracy as oa

H = np.float16
ONE_STEP = [k for k in fa.OPS if k not in fa.COMPOSITE]


@pytest.fixture(scope="module")
def f16o(tmp_path_factory):
    return f16_oracle.build(str(tmp_path_factory.mktemp("f16_oracle")))


def test_inputs_are_the_closed_sets():
    x = fa.all_patterns()
    assert len(x) == 65536 and np.array_equal(fa.bits(x), np.arange(65536)) and int(np.isnan(x).sum()) == 2046
    g = fa.grid_values()
    assert len(g) == 2 * 31 * 7 + 3 and np.isnan(g).sum() == 1 and np.isinf(g).sum() == 2 and (g == 0).sum() == 2
    a, b = fa.binary_args()
    assert len(a) == len(b) == len(g) ** 2 + 20000
    sg = fa.subgrid_values()
    assert len(sg) == 2 * 11 * 3 + 3
    p, q, r = fa.ternary_args()
    assert len(p) == len(q) == len(r) == len(sg) ** 3 + 7 * (len(sg) ** 2 + 4000)
    # the cancelling family: z is within 3 binary16 steps of -r16(x y)
    n0 = len(sg) ** 3
    with np.errstate(all="ignore"):
        prod = fa.r16(-(p[n0:].astype(np.float64) * q[n0:].astype(np.float64)))
    fin = np.isfinite(prod.astype(np.float32))
    assert (np.abs(fa.ord16(r[n0:]) - fa.ord16(prod))[fin] <= 3).all() and fin.sum() > 30000
    cols = fa.path_columns()
    assert 3000 < len(cols) < 5000 and set(fa.SPECIAL_BITS) <= set(cols.tolist())
    d = fa.direct_columns(2048 + 5)
    assert len(set(d.tolist())) == 2053 and {int(u) >> 10 for u in d} == set(range(64))


def test_float64_libm_is_within_2_pow_minus_20_float32_ulp_of_mpmath():
    """The reference's own error: numpy's float64 functions against mpmath at 160 bits on every 61st argument (and every 211th pair of
    `^`), at every point whose value is finite — the widening of s that the rule grants the reference."""
    import mpmath as mp
    f, _ = oa._mp_tables()
    worst = {}
    with mp.workprec(oa.MP_PREC):
        for key in fa.LIBRARY:
            args = tuple(a[::61 if key[1] == 1 else 211] for a in fa.args_of(key))
            t = fa.truth(key, args)
            keep = np.isfinite(t) & (t != 0)
            err = 0.0
            for i in np.nonzero(keep)[0]:
                v = f[key](*[mp.mpf(float(a[i])) for a in args])
                v = v.real if isinstance(v, mp.mpc) else v
                err = max(err, float(abs(mp.mpf(float(t[i])) - v) / mp.mpf(float(fa.ulp32(t[i])))))
            worst[fa.key_name(key)] = err
            assert keep.sum() > 100, key
    print("[f16 reference] float64 libm against mpmath, worst error in Float32 ulp:", {k: f"{v:.2e}" for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v <= fa.REF_SLACK}
    assert not bad, bad


def test_fma_reference_is_the_contract_in_rational_arithmetic():
    """Float16(muladd(Float32...)): the exact value rounded to Float32, then to binary16 — the error-free float64 model against Fraction,
    on every 499th triple and every 97th point of the cancelling family; the once-rounded model likewise."""
    x, y, z = fa.ternary_args()
    n0 = len(fa.subgrid_values()) ** 3
    idx = np.concatenate([np.arange(0, n0, 499), np.arange(n0, len(x), 97)])
    ref = fa.reference(("fma", 3))
    once = fa.wrong_fma_rounded_once(x[idx], y[idx], z[idx])
    n = 0
    for j, i in enumerate(idx):
        if not all(np.isfinite(float(v[i])) for v in (x, y, z)):
            continue
        assert fa.same_bits(ref.lo[i], fa.fma_fraction(x[i], y[i], z[i])), (float(x[i]), float(y[i]), float(z[i]))
        assert fa.same_bits(once[j], fa.fma_fraction(x[i], y[i], z[i], single=True)), (float(x[i]), float(y[i]), float(z[i]))
        n += 1
    assert n > 1000


@pytest.mark.parametrize("key", ONE_STEP, ids=[fa.key_name(k) for k in ONE_STEP])
def test_conditions_and_oracle_within_the_rule(f16o, key):
    """The conditions on the reference alone (no set of more than two members; at most 0.5 % of the finite-result points two-valued; no
    point dropped), then the CPU oracle inside the rule at every point: NaN exactly where the table says NaN, the infinities and the
    signed zeros of the table, the admissible bits elsewhere."""
    ref = fa.reference(key)
    got, _ = fa.oracle_row(f16o, key, ref.args)
    c = fa.census(ref, got)
    print(f"[f16 oracle] {fa.key_name(key)}: {c['points']} points compared ({c['finite_argument_points']} with finite arguments), "
          f"{c['finite_result_points']} finite results, {c['two_valued']} two-valued sets, oracle not correctly rounded at "
          f"{c['not_correctly_rounded']} (worst {c['worst_ulp16']} binary16 ulp at {c['worst_argument']})")
    assert c["widest_set"] <= 2
    assert c["two_valued"] <= fa.MAX_TWO_VALUED * c["finite_result_points"]
    assert fa.slack(key) == fa.S_LIBRARY or c["two_valued"] == 0
    assert c["compared"] == c["points"] == len(ref.args[0]) and c["compared_finite_argument_points"] == c["finite_argument_points"]
    assert c["outside_rule"] == 0, f"first at (arguments, oracle, lo, hi) {c['first_outside']}"
    assert c["worst_ulp16"] <= 1


def test_composites_equal_their_step_models_in_the_oracle(f16o):
    """cube = square(x) * x, custom_cos = square(cos(x)), pow_abs2 = exp(y * log(abs(x))), +(x, y, z) = (x + y) + z: the oracle's
    composite against the oracle's own single steps chained by numpy binary16 arithmetic (one rounding per operation), bit for bit."""
    xs = fa.all_patterns()
    row = {n: fa.oracle_row(f16o, (n, 1), (xs,))[0] for n in ("square", "cube", "cos", "custom_cos", "log", "exp")}
    assert fa.same_bits(row["cube"], fa.np_mul(row["square"], xs)).all()
    assert fa.same_bits(row["custom_cos"], fa.np_square(row["cos"])).all()
    a, b = fa.binary_args()
    m = fa.np_mul(b, row["log"][fa.bits(np.abs(a))])
    got = fa.oracle_row(f16o, ("pow_abs2", 2), (a, b))[0]
    assert fa.same_bits(got, row["exp"][fa.bits(m)]).all()
    assert fa.composite_accept(("pow_abs2", 2), (a, b), got).all()
    assert fa.composite_accept(("custom_cos", 1), (xs,), row["custom_cos"]).all()
    p, q, r = fa.ternary_args()
    assert fa.same_bits(fa.oracle_row(f16o, ("+", 3), (p, q, r))[0], fa.np_add(fa.np_add(p, q), r)).all()


def test_wrong_models_fail_the_rule():
    """The inputs tell a wrong kernel from a right one: each plausible wrong model is outside the rule at one point or more."""
    xs = fa.all_patterns()
    a, b = fa.binary_args()
    p, q, r = fa.ternary_args()
    fails = {
        "cube with one rounding": ~fa.accept(fa.reference(("cube", 1)), fa.wrong_cube_one_rounding(xs)),
        "custom_cos with one rounding": ~fa.composite_accept(("custom_cos", 1), (xs,), fa.wrong_custom_cos_one_rounding(xs)),
        "pow_abs2 without the middle rounding": ~fa.composite_accept(("pow_abs2", 2), (a, b), fa.wrong_pow_abs2_no_middle_rounding(a, b)),
        "fma rounded once from the exact value": ~fa.accept(fa.reference(("fma", 3)), fa.wrong_fma_rounded_once(p, q, r)),
    }
    counts = {k: int(v.sum()) for k, v in fails.items()}
    print("[f16 discrimination] points at which each wrong model fails the rule:", counts)
    assert all(n >= 1 for n in counts.values()), counts
