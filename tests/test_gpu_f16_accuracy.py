"""Every DE_F16 operator on the MI355X against a high-precision reference, per operator (csrc/de_half.hip, csrc/de_half_ops.h).

The inputs, references and the acceptance rule are those of tests/f16_accuracy.py; tests/test_f16_accuracy_host.py holds the CPU Float16
oracle to the same tables and asserts the rule's conditions on the reference alone, so nothing here rests on the oracle's formulas or on
the device's Float32 library.

a. Values.  Every unary opcode on ALL 65536 binary16 bit patterns (one Population of one-operator trees, early_exit=False, one call);
   every binary opcode on all ordered pairs of the closed grid and 20000 random pairs; every ternary opcode on all triples of the
   sub-grid and the cancelling family.  The device must give an admissible value at every point — almost everywhere the one correctly
   rounded binary16 value, bit for bit — and the oracle's class (NaN, +-Inf, +-0) at NaN / Inf arguments and outside the domains.
b. Composites by transitivity: cube, custom_cos, pow_abs2 and +(x, y, z) equal their written-out trees bit for bit.
c. Paths: the constant forms op(x1, c) and op(c, x1) (every reversed DOP_R* form), op(x1 + 0.0) and op(x1 + x2) with x2 == 0, with folding
   on and with DE_NO_FOLD=1; torch.float16 device buffers against host buffers; an X pointer that is 2 mod 4 (the scalar branch of
   HalfPolicy::stage_x); N = 1, 1023, 1025, 4099; the DIRECT variant (40 features); the early-exit flags against the oracle's.
d. The report ulp_f16.json, written to $DE_ULP_REPORT_DIR, by default build/reports/ of the checkout.

What these tests found on an MI355X (ROCm 7.0), both fixed in csrc/de_half_ops.h: the compiler contracted a Float32
operation and the conversion behind it into v_fma_mixlo_f16, which rounds the exact result to binary16 once — fma was rounded once instead
of exact -> Float32 -> binary16 (408 of 389836 points one ulp off), and cube(x) was +0 instead of -0 for the 2473 negative arguments whose
square underflows (its second product had become fma(r16(x x), x, +0)).  Run with `pytest -m gpu`."""
import json
import os

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import f16_accuracy as fa
import f16_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = np.float16
REPORT, _CACHE = {}, {}
CONSTS = (float(fa.from_bits([0x0155])[0]), 0.5, -3.0, 65504.0)   # a subnormal, 0.5, -3.0, floatmax


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _api.library()
    return _api


@pytest.fixture(scope="module")
def f16o(tmp_path_factory):
    return f16_oracle.build(str(tmp_path_factory.mktemp("f16_oracle")))


def run(api, trees, ops, X, early_exit=False, use_fused=True):
    """(rows, flags, kernel name) of one Population.eval; X a numpy [F, N] binary16 matrix or a torch device tensor."""
    pop = api.Population(trees, ops, H, n_features=int(X.shape[0]), eval_context=api.EvalContext(early_exit=early_exit, use_fused=use_fused))
    try:
        out, ok = pop.eval(X if not isinstance(X, np.ndarray) else np.asfortranarray(X))
        if not isinstance(out, np.ndarray):
            import torch
            torch.cuda.synchronize()
            out, ok = out.cpu().numpy(), ok.cpu().numpy()
        return out, np.asarray(ok, dtype=bool), pop.ctx.last_kernel_name()
    finally:
        pop.close()


def device_rows(api, degree):
    """The device's rows of every opcode of `degree` on its inputs: one call, cached for the module.  name -> row."""
    if degree not in _CACHE:
        names = (fa.UNARY, fa.BINARY, fa.TERNARY)[degree - 1]
        ops = fa.enum_of(degree)
        out, _, kname = run(api, [fa.leaf_tree((n, degree), ops) for n in names], ops, fa.feature_matrix(fa.args_of((names[0], degree))))
        assert "direct" not in kname
        out.setflags(write=False)
        _CACHE[degree] = dict(zip(names, out))
    return _CACHE[degree]


def oracle_rows(f16o, key):
    if ("orc", key) not in _CACHE:
        _CACHE[("orc", key)] = fa.oracle_row(f16o, key, fa.args_of(key))[0]
    return _CACHE[("orc", key)]


def mismatch(got, want, args):
    bad = ~fa.same_bits(got, want)
    i = int(np.argmax(bad))
    return f"{int(bad.sum())} of {len(bad)} columns differ, first at {[float(a[i]) for a in args]}: {float(got[i])!r}, expected {float(want[i])!r}"


# ---- a. values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", fa.OPS, ids=[fa.key_name(k) for k in fa.OPS])
def test_values_within_the_rule(api, f16o, key):
    """Device bits against the admissible set at every point, then the oracle's class at NaN / Inf arguments and outside the domain
    (figures: measured on the GPU; those of the oracle beside them)."""
    got = device_rows(api, key[1])[key[0]]
    orc = oracle_rows(f16o, key)
    args = fa.args_of(key)
    special = ~np.logical_and.reduce([np.isfinite(a.astype(np.float32)) for a in args])
    if key in fa.COMPOSITE:
        ok = fa.composite_accept(key, args, got)
        differs = ~fa.same_bits(got, orc)
        special |= np.isnan(orc)
        REPORT[fa.key_name(key)] = dict(points_compared=len(got), outside_step_sets=int((~ok).sum()), device_differs_from_oracle=int(differs.sum()))
        print(f"[f16] {fa.key_name(key)}: {len(got)} points, {int((~ok).sum())} outside the sets of its steps, {int(differs.sum())} differ from the oracle")
        assert ok.all(), f"{int((~ok).sum())} points outside the step sets, first at {[float(a[np.argmax(~ok)]) for a in args]}: {float(got[np.argmax(~ok)])!r}"
    else:
        ref = fa.reference(key)
        dev, o = fa.census(ref, got), fa.census(ref, orc)
        special |= np.isnan(ref.t)
        REPORT[fa.key_name(key)] = dict(
            points_compared=dev["compared"], finite_result_points=dev["finite_result_points"], two_valued_sets=dev["two_valued"],
            device_not_correctly_rounded=dev["not_correctly_rounded"], device_worst_argument=dev["worst_argument"], device_outside_rule=dev["outside_rule"],
            oracle_not_correctly_rounded=o["not_correctly_rounded"], oracle_worst_argument=o["worst_argument"], oracle_outside_rule=o["outside_rule"])
        print(f"[f16] {fa.key_name(key)}: {dev['compared']} points, {dev['finite_result_points']} finite results, {dev['two_valued']} two-valued sets; "
              f"device not correctly rounded at {dev['not_correctly_rounded']} (worst at {dev['worst_argument']}), outside the rule at {dev['outside_rule']}; "
              f"oracle not correctly rounded at {o['not_correctly_rounded']}")
        assert dev["widest_set"] <= 2 and dev["two_valued"] <= fa.MAX_TWO_VALUED * dev["finite_result_points"]
        assert dev["compared"] == dev["points"] == len(args[0]) and dev["compared_finite_argument_points"] == dev["finite_argument_points"]
        assert dev["outside_rule"] == 0, (f"{dev['outside_rule']} points outside the rule, first at (arguments, device, lo, hi) {dev['first_outside']}; "
                                          f"not correctly rounded at {dev['not_correctly_rounded']} points")
    same_class = fa.klass(got) == fa.klass(orc)
    assert same_class[special].all(), (f"class differs from the oracle's at {int((~same_class & special).sum())} special points, first at "
                                       f"{[float(a[np.argmax(~same_class & special)]) for a in args]}: device {float(got[np.argmax(~same_class & special)])!r}, "
                                       f"oracle {float(orc[np.argmax(~same_class & special)])!r}")


# ---- b. composites by transitivity ----------------------------------------------------------------------------------------------------
def test_composites_equal_their_written_out_trees(api):
    """Both sides on the device, every column, NaN / Inf arguments and overflowing intermediates included.  use_fused=False: a fused
    form of the written-out tree answers Inf for a non-finite inner value (the reference's fused kernels with early_exit=false), which a
    single opcode has no occasion to."""
    ops = de.OperatorEnum(binary_operators=("+", "*", "pow_abs2"), unary_operators=("square", "cube", "cos", "custom_cos", "exp", "log", "abs"),
                          ternary_operators=("+",))
    U = lambda n, a: de.Node(ops.index(n, 1), a)          # noqa: E731
    B = lambda n, a, b: de.Node(ops.index(n, 2), a, b)    # noqa: E731
    x1, x2, x3 = fa.x(1), fa.x(2), fa.x(3)
    xs = fa.all_patterns()
    out, _, _ = run(api, [U("cube", x1), B("*", U("square", x1), x1), U("custom_cos", x1), U("square", U("cos", x1))], ops, fa.feature_matrix((xs,)), use_fused=False)
    assert fa.same_bits(out[0], out[1]).all(), "cube(x) vs square(x) * x: " + mismatch(out[0], out[1], (xs,))
    assert fa.same_bits(out[2], out[3]).all(), "custom_cos(x) vs square(cos(x)): " + mismatch(out[2], out[3], (xs,))
    assert fa.same_bits(out[0], device_rows(api, 1)["cube"]).all() and fa.same_bits(out[2], device_rows(api, 1)["custom_cos"]).all()
    a = fa.binary_args()
    out, _, _ = run(api, [B("pow_abs2", x1, x2), U("exp", B("*", x2, U("log", U("abs", x1))))], ops, fa.feature_matrix(a), use_fused=False)
    assert fa.same_bits(out[0], out[1]).all(), "pow_abs2(x, y) vs exp(y * log(abs(x))): " + mismatch(out[0], out[1], a)
    assert fa.same_bits(out[0], device_rows(api, 2)["pow_abs2"]).all()
    t = fa.ternary_args()
    out, _, _ = run(api, [de.Node(ops.index("+", 3), x1, x2, x3), B("+", B("+", x1, x2), x3)], ops, fa.feature_matrix(t), use_fused=False)
    assert fa.same_bits(out[0], out[1]).all(), "+(x, y, z) vs (x + y) + z: " + mismatch(out[0], out[1], t)
    assert fa.same_bits(out[0], device_rows(api, 3)["+"]).all()


# ---- c. paths -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", ["fold", "DE_NO_FOLD=1"])
def test_constant_forms_carry_the_bits_of_the_feature_form(api, monkeypatch, fold):
    """op(x1, c) and op(c, x1) (the reversed DOP_R* forms of - / ^ mod rem greater pow_abs2) for every binary opcode and
    c in {a subnormal, 0.5, -3.0, 65504}: the bits of op(x1, x2) / op(x2, x1) with x2 == c."""
    if fold != "fold":
        monkeypatch.setenv("DE_NO_FOLD", "1")
    ops = fa.binary_enum()
    xs = fa.from_bits(fa.path_columns())
    X = np.stack([xs] + [np.full_like(xs, H(c)) for c in CONSTS])
    feat, cons, what = [], [], []
    for n in fa.BINARY:
        i = ops.index(n, 2)
        for k, c in enumerate(CONSTS):
            feat += [de.Node(i, fa.x(1), fa.x(k + 2)), de.Node(i, fa.x(k + 2), fa.x(1))]
            cons += [de.Node(i, fa.x(1), de.Node(val=c)), de.Node(i, de.Node(val=c), fa.x(1))]
            what += [f"{n}(x1, {c})", f"{n}({c}, x1)"]
    want, _, _ = run(api, feat, ops, X)
    got, _, _ = run(api, cons, ops, X[:1])
    for t, w in enumerate(what):
        assert fa.same_bits(got[t], want[t]).all(), f"{w} [{fold}]: " + mismatch(got[t], want[t], (xs,))


@pytest.mark.parametrize("fold", ["fold", "DE_NO_FOLD=1"])
def test_accumulator_and_fused_unary_forms_carry_the_bits_of_the_feature_form(api, monkeypatch, fold):
    """op(x1 + 0.0) and op(x1 + x2) with x2 == 0 for every unary opcode: the bits of op at r16(x1 + 0) (-0 + 0 is +0), read from the
    exhaustive row; where x1 + 0 is not finite the fused form answers +Inf (is_valid(x_l) ? op(x_l) : Inf, the reference's fused kernels
    with early_exit=false: DESIGN.md §3)."""
    table = device_rows(api, 1)
    if fold != "fold":
        monkeypatch.setenv("DE_NO_FOLD", "1")
    xs = fa.from_bits(fa.path_columns())
    inner = fa.np_add(xs, np.zeros_like(xs))
    arg, valid = fa.bits(inner), np.isfinite(inner.astype(np.float32))
    X = np.stack([xs, np.zeros_like(xs)])
    for names in fa.unary_groups():
        ops = fa.unary_enum(names)
        plus = ops.index("+", 2)
        trees = [de.Node(ops.index(n, 1), de.Node(plus, fa.x(1), de.Node(val=0.0))) for n in names]
        trees += [de.Node(ops.index(n, 1), de.Node(plus, fa.x(1), fa.x(2))) for n in names]
        got, _, _ = run(api, trees, ops, X)
        for t, n in enumerate(list(names) + list(names)):
            want = np.where(valid, table[n][arg], H(np.inf))
            assert fa.same_bits(got[t], want).all(), f"{n}({'x1 + 0.0' if t < len(names) else 'x1 + x2'}) [{fold}]: " + mismatch(got[t], want, (xs,))


def test_device_buffers_give_the_bits_of_host_buffers(api):
    import torch
    table = device_rows(api, 1)
    ops = fa.unary_enum()
    Xd = torch.from_numpy(fa.all_patterns().copy().reshape(-1, 1)).cuda().t()
    assert tuple(Xd.shape) == (1, 65536)
    out, _, _ = run(api, [fa.leaf_tree((n, 1), ops) for n in fa.UNARY], ops, Xd)
    for t, n in enumerate(fa.UNARY):
        assert fa.same_bits(out[t], table[n]).all(), f"{n}: " + mismatch(out[t], table[n], (fa.all_patterns(),))


def _mixed_trees():
    ops = de.OperatorEnum(binary_operators=fa.BINARY, unary_operators=fa.UNARY, ternary_operators=fa.TERNARY)
    trees = [de.Node(ops.index(n, 1), fa.x(1)) for n in fa.UNARY] + [de.Node(ops.index(n, 2), fa.x(2), fa.x(3)) for n in fa.BINARY]
    trees += [de.Node(ops.index(n, 3), fa.x(1), fa.x(2), fa.x(3)) for n in fa.TERNARY]
    return trees, ops


def test_unaligned_x_pointer_gives_the_bits_of_the_aligned_copy(api):
    """An X whose data pointer is 2 mod 4 with ldX == F (F = 3, N = 2048 + 5: two full tiles and a ragged one): the scalar branch of
    HalfPolicy::stage_x.  All 53 opcodes; the aligned copy and host buffers give the same bits."""
    import torch
    F, N = 3, 2048 + 5
    cols = fa.from_bits(fa.direct_columns(N))
    Xh = np.stack([cols, np.roll(cols, 7), np.roll(cols, 301)])            # [F, N]
    flat = torch.zeros(1 + N * F + 7, dtype=torch.float16, device="cuda")
    flat[1:1 + N * F] = torch.from_numpy(np.ascontiguousarray(Xh.T).reshape(-1)).cuda()
    Xu = flat[1:1 + N * F].view(N, F).t()
    assert Xu.data_ptr() % 4 == 2 and Xu.stride(0) == 1 and Xu.stride(1) == F
    Xa = Xu.t().clone().t()
    assert Xa.data_ptr() % 16 == 0 and Xa.stride(0) == 1 and Xa.stride(1) == F
    trees, ops = _mixed_trees()
    got, _, _ = run(api, trees, ops, Xu)
    want, _, _ = run(api, trees, ops, Xa)
    host, _, _ = run(api, trees, ops, Xh)
    for t in range(len(trees)):
        assert fa.same_bits(got[t], want[t]).all(), f"{de.string_tree(trees[t], ops)}: " + mismatch(got[t], want[t], tuple(Xh))
        assert fa.same_bits(host[t], want[t]).all(), f"{de.string_tree(trees[t], ops)} (host buffers): " + mismatch(host[t], want[t], tuple(Xh))
    table = device_rows(api, 1)
    for t, n in enumerate(fa.UNARY):
        assert fa.same_bits(got[t], table[n][fa.bits(cols)]).all(), n


@pytest.mark.parametrize("n", [1, 1023, 1025, 4099])
def test_shape_does_not_reach_the_bits(api, n):
    table = device_rows(api, 1)
    ops = fa.unary_enum()
    out, _, _ = run(api, [fa.leaf_tree((k, 1), ops) for k in fa.UNARY], ops, fa.feature_matrix((fa.all_patterns()[:n],)))
    for t, k in enumerate(fa.UNARY):
        assert fa.same_bits(out[t], table[k][:n]).all(), f"{k}, N = {n}: " + mismatch(out[t], table[k][:n], (fa.all_patterns()[:n],))


def test_direct_variant_gives_the_bits_of_the_lds_variant(api):
    """40 features, the argument in feature 40, N = 2048 + 5: the kernel gathers from global memory."""
    F, N = 40, 2048 + 5
    u = fa.direct_columns(N)
    cols = fa.from_bits(u)
    X = np.stack([np.roll(cols, 13 * (F - 1 - f)) for f in range(F)])
    assert np.array_equal(fa.bits(X[F - 1]), u)
    ops = fa.unary_enum()
    out, _, kname = run(api, [de.Node(ops.index(k, 1), fa.x(F)) for k in fa.UNARY], ops, X)
    assert "direct" in kname, kname
    table = device_rows(api, 1)
    for t, k in enumerate(fa.UNARY):
        assert fa.same_bits(out[t], table[k][u]).all(), f"{k}: " + mismatch(out[t], table[k][u], (cols,))


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_early_exit_flags_are_the_oracles(api, f16o, degree):
    """One-operator trees with early_exit=True on three column subsets per opcode: all results finite (flag set), one overflow appended,
    one NaN argument appended — the flag is the oracle's element-wise flag."""
    names = (fa.UNARY, fa.BINARY, fa.TERNARY)[degree - 1]
    ops = fa.enum_of(degree)
    full = fa.args_of((names[0], degree))
    pick = fa.path_columns().astype(np.int64) if degree == 1 else np.arange(0, len(full[0]), 53 if degree == 2 else 97)
    args = tuple(a[pick] for a in full)
    fin_args = np.logical_and.reduce([np.isfinite(a.astype(np.float32)) for a in args])
    nan_col = int(np.argmax(np.isnan(args[0])))
    assert np.isnan(args[0][nan_col])
    checked = 0
    for n in names:
        key = (n, degree)
        vals = fa.oracle_row(f16o, key, args)[0]
        finite = np.nonzero(fin_args & np.isfinite(vals.astype(np.float32)))[0][:1500]
        over = np.nonzero(fin_args & np.isinf(vals))[0]
        subsets = {"finite": finite, "nan argument": np.append(finite, nan_col)}
        if len(over):
            subsets["overflow"] = np.append(finite, over[0])
        tree = fa.leaf_tree(key, ops)
        for what, cols in subsets.items():
            sub = tuple(a[cols] for a in args)
            _, want = fa.oracle_row(f16o, key, sub, options=7)
            _, ok, _ = run(api, [tree], ops, fa.feature_matrix(sub), early_exit=True)
            assert bool(ok[0]) == want, f"{fa.key_name(key)}, {what}: flag {bool(ok[0])}, oracle {want}"
            assert want == (what == "finite") or what == "nan argument", f"{fa.key_name(key)}, {what}: oracle flag {want}"
            checked += 1
    assert checked >= 2 * len(names)


# ---- d. the report --------------------------------------------------------------------------------------------------------------------
def test_zz_write_ulp_report():
    """Runs last in this module: the per-opcode figures of DESIGN.md §13.1 / §13.3."""
    assert len(REPORT) == len(fa.OPS)
    import torch
    out_dir = os.environ.get("DE_ULP_REPORT_DIR") or os.path.join(ROOT, "build", "reports")   # (build/ is kept out of git)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "ulp_f16.json"), "w") as fh:
        json.dump(dict(what="DE_F16, per opcode: points compared (unary: all 65536 bit patterns), points whose admissible set has two members, points "
                            "where the device / the CPU oracle is not the correctly rounded binary16 value (with the worst argument) and points "
                            "outside the rule (tests/test_gpu_f16_accuracy.py, tests/f16_accuracy.py)",
                       device=torch.cuda.get_device_name(0), hip=str(torch.version.hip), opcodes=REPORT), fh, indent=1, sort_keys=True)
    print(f"[f16 ulp] {len(REPORT)} opcodes, device not correctly rounded at "
          f"{sum(r.get('device_not_correctly_rounded', 0) for r in REPORT.values())} points in all, outside the rule at "
          f"{sum(r.get('device_outside_rule', 0) for r in REPORT.values())}")
