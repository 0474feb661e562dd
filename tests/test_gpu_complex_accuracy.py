"""The complex operator table on the MI355X (csrc/de_complex_ops.h through csrc/de_complex.hip) against mpmath, per operator.

Every operator of DESIGN.md §14.1 runs as a one-operator tree through the public API with early_exit=False, on the populations of
tests/complex_accuracy.py (input regions aimed at the branches of the formulas: the exponent scaling of ssqs, the log1p condition of
log, the four scalings of the ComplexF64 division, Kahan's tanh around its overflow guard and its poles).  The device is bounded by the
CPU oracle's error ON THE SAME INPUTS, not by a fixed number:

    device_max <= oracle_max + 0.5 + sum over the real library calls feeding one result of (amplification x that function's slack)

per region, normwise for every operator and componentwise where the formula delivers it.  The oracle runs Julia's formulas on glibc, the
device runs them on OCML and fast_exp_f32; 0.5 covers one differently rounded final operation; a real function's slack is the project's
asserted bound for it (2 ulp Float32, 1 ulp Float64) unless REAL_SLACK says otherwise, and test_real_function_feeding_the_complex_formulas
measures every one of them alone, through the complex operator on inputs that isolate it (sin(x + 0i) = sin x, tanh(iy) = i tan y, ...).
The oracle itself is pinned to mpmath by tests/test_complex_accuracy_host.py.

Besides: special values on the grid {+-0, +-subnormal, +-floatmin, +-1, +-floatmax, +-Inf, NaN}^2 against the oracle (NaN pattern,
infinities, signs of zeros, flags), independence of the tile shape (N = 1, 511, 513 and the DIRECT gather variant at F = 17 give the
bits of the 1500-column call), and the report ulp_complex.json (written to $DE_ULP_REPORT_DIR, by default build/reports/ of the checkout).  Run with `pytest -m gpu`."""
import json
import os

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import complex_accuracy as ca
import complex_oracle
from test_complex_accuracy_host import CAPS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
REPORT = {}
REAL_REPORT = {}

# the real library calls feeding one result, each name once per unit of amplification (tan / tanh: the sensitivity to each of tan y and
# sinh x is at most 2; custom_cos: the square doubles the relative error of cos z)
CALLS = {
    "+": (), "-": (), "*": (), "/": (), "inv": (), "sqrt": (), "square": (), "cube": (), "neg": (),
    "exp": ("exp", "sincos"), "sin": ("sincos", "sinhcosh"), "cos": ("sincos", "sinhcosh"), "sinh": ("sincos", "sinhcosh"),
    "cosh": ("sincos", "sinhcosh"),
    "log": ("log", "atan2"),
    "tan": ("tan", "tan", "sinhcosh", "sinhcosh"), "tanh": ("tan", "tan", "sinhcosh", "sinhcosh"),
    "custom_cos": ("sincos", "sincos", "sinhcosh", "sinhcosh"),
}
DEFAULT_SLACK = {np.float32: 2.0, np.float64: 1.0}  # tests/test_gpu_ops.py, tests/test_gpu_ulp_f64.py
# (function group, component type) -> slack in ulp where it differs from the default: the maximum measured for that function alone
# (the three tests below the operator test), rounded up to the next half ulp.  Measured on one MI355X, ROCm 7.0 (HIP 7.0.51831), in ulp:
#   sin 1.36 / 0.71, cos 1.33 / 0.70, sinh 0.76 / 0.78, cosh 0.54 / 0.53, exp 1.04 / 0.80, tan 1.49 / 0.76 (Float32 / Float64),
#   logf 1.85, log1pf 0.53: all within the defaults;
#   atan2f 2.03 at (y, x) = (-0.0036263037, 0.002505339), atan2 1.39 at (0.9922185644151656, 0.7379827810333912): OCML's atan2, which
#   no other test bounds, is past both defaults (the Float64 atan opcode is the library's own de_atan_f64; atan2 is not an opcode).
REAL_SLACK = {("atan2", np.float32): 2.5, ("atan2", np.float64): 1.5}


def slack(group, R):
    return REAL_SLACK.get((group, R), DEFAULT_SLACK[R])


def budget(op, dtype):
    R = ca.real_of(dtype)
    return 0.5 + sum(slack(g, R) for g in CALLS[op])


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _api.library()
    return _api


@pytest.fixture(scope="module")
def co(tmp_path_factory):
    return complex_oracle.build(str(tmp_path_factory.mktemp("complex_oracle")))


def device_eval(api, trees, ops, X, dtype, **ctx):
    pop = api.Population(trees, ops, dtype, n_features=X.shape[0], eval_context=api.EvalContext(**ctx))
    try:
        out, ok = pop.eval(X)
        return out, ok, pop.ctx.last_kernel_name()
    finally:
        pop.close()


def device_population(api, pop):
    trees, X, rows = ca.trees_and_X(pop)
    out, _, _ = device_eval(api, trees, ca.operator_enum(pop.op), X, pop.dtype, early_exit=False)
    return ca.gather(out, rows, X.shape[1], pop.dtype)


# ---- a. per-operator accuracy against mpmath ------------------------------------------------------------------------------------------
CASES = [(op, dt, "xx") for op in list(ca.UNARY) + list(ca.BINARY_REGIONS) for dt in ca.CDTYPES]
CASES += [(op, dt, form) for op in ca.BINARY_REGIONS for dt in ca.CDTYPES for form in ("cx", "xc")]  # c op x1 (DOP_RSUB / DOP_RDIV), x1 op c


@pytest.mark.parametrize("op,dtype,form", CASES, ids=[f"{op}-{np.dtype(dt).name}-{form}" for op, dt, form in CASES])
def test_operator_against_mpmath(api, co, op, dtype, form):
    pop = ca.population(op, dtype, form)
    dev = ca.region_maxima(pop, device_population(api, pop))
    orc = ca.region_maxima(pop, ca.oracle_eval(co, pop)[0])
    extra = budget(op, dtype)
    REPORT[f"{op} {form} {np.dtype(dtype).name}"] = {
        r: dict(kept=dev[r]["kept"], device=dev[r]["norm"], device_at=repr(dev[r]["norm_at"]), oracle=orc[r]["norm"],
                oracle_at=repr(orc[r]["norm_at"]), bound=orc[r]["norm"] + extra,
                **(dict(device_componentwise=dev[r]["comp"], oracle_componentwise=orc[r]["comp"]) if ca.has_componentwise(op, r) else {}))
        for r in dev}
    failures = []
    for r in dev:
        print(f"{op} {form} {np.dtype(dtype).name} {r}: kept {dev[r]['kept']:.3f}; normwise device {dev[r]['norm']:.3f} at {dev[r]['norm_at']}, "
              f"oracle {orc[r]['norm']:.3f}; componentwise device {dev[r]['comp']:.3f} at {dev[r]['comp_at']}, oracle {orc[r]['comp']:.3f}")
        assert dev[r]["kept"] >= ca.MIN_KEPT, (r, dev[r]["kept"])
        if not dev[r]["norm"] <= orc[r]["norm"] + extra:
            failures.append(f"{r}: normwise {dev[r]['norm']:.3f} ulp at {dev[r]['norm_at']} > oracle {orc[r]['norm']:.3f} + {extra}")
        if ca.has_componentwise(op, r) and not dev[r]["comp"] <= orc[r]["comp"] + extra:
            failures.append(f"{r}: componentwise {dev[r]['comp']:.3f} ulp at {dev[r]['comp_at']} > oracle {orc[r]['comp']:.3f} + {extra}")
    assert not failures, f"{op} {form} {np.dtype(dtype).name}: " + "; ".join(failures)


@pytest.mark.parametrize("dtype", ca.CDTYPES, ids=["cf32", "cf64"])
@pytest.mark.parametrize("op", ["+", "-"])
def test_add_sub_have_numpy_bits(api, op, dtype):
    """x1 op x2, c op x1 and x1 op c: the bits of numpy's complex arithmetic in that dtype, on ordinary and on cancelling pairs."""
    a, b = ca.addsub_inputs(op, dtype)
    R = ca.real_of(dtype)
    ops = ca.operator_enum(op)
    f = np.add if op == "+" else np.subtract
    x1, x2 = de.Node(feature=1), de.Node(feature=2)
    out, ok, _ = device_eval(api, [de.Node(1, x1, x2)], ops, np.asfortranarray(np.stack([a, b])), dtype, early_exit=False)
    assert ok[0]
    np.testing.assert_array_equal(out[0].view(R), f(a, b).view(R))
    cs = [a[3], b[len(b) - 2], a[len(a) // 2]]
    trees = [de.Node(1, de.Node(val=complex(c)), x1) for c in cs] + [de.Node(1, x1, de.Node(val=complex(c))) for c in cs]
    out, ok, _ = device_eval(api, trees, ops, np.asfortranarray(b[None, :]), dtype, early_exit=False)
    assert ok.all()
    for t, c in enumerate(cs):
        np.testing.assert_array_equal(out[t].view(R), f(dtype(c), b).view(R), err_msg=f"{c} {op} x1")
        np.testing.assert_array_equal(out[3 + t].view(R), f(b, dtype(c)).view(R), err_msg=f"x1 {op} {c}")


# ---- the real functions inside the formulas, each alone -------------------------------------------------------------------------------
def _near_poles(rng, n):
    return rng.integers(-5, 6, n) * (np.pi / 2) + rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, -1, n)


def _exp_range(rng, n, R):
    top = np.log(float(np.finfo(R).max)) - 1
    return np.concatenate([rng.uniform(-top, top, n), rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 1, n)])


# name -> (slack group, complex operator, which axis carries the argument, which part carries the value, long double reference, sampler)
REAL_FUNCTIONS = {
    "sin": ("sincos", "sin", "re", "re", np.sin, lambda g, R: np.concatenate([g.uniform(-20, 20, 3000), g.uniform(-1e4, 1e4, 3000)])),
    "cos": ("sincos", "cos", "re", "re", np.cos, lambda g, R: np.concatenate([g.uniform(-20, 20, 3000), g.uniform(-1e4, 1e4, 3000)])),
    "sinh": ("sinhcosh", "sin", "im", "im", np.sinh, lambda g, R: _exp_range(g, 3000, R)),
    "cosh": ("sinhcosh", "cos", "im", "re", np.cosh, lambda g, R: _exp_range(g, 3000, R)),
    "exp": ("exp", "exp", "re", "re", np.exp, lambda g, R: _exp_range(g, 3000, R)),
    "tan": ("tan", "tanh", "im", "im", np.tan, lambda g, R: np.concatenate([g.uniform(-10, 10, 3000), _near_poles(g, 3000)])),
}
REAL_CASES = [(n, dt) for n in REAL_FUNCTIONS for dt in ca.CDTYPES]


def _real_ulp(got, want_ld, R):
    w = np.asarray(want_ld, dtype=LD)
    return (np.abs(got.astype(LD) - w) / np.spacing(np.abs(w.astype(R))).astype(LD)).astype(np.float64)


@pytest.mark.parametrize("name,dtype", REAL_CASES, ids=[f"{n}-{np.dtype(dt).name}" for n, dt in REAL_CASES])
def test_real_function_feeding_the_complex_formulas(api, name, dtype):
    """A complex operator on the real or the imaginary axis returns one real library call untouched (c_sin(x + 0i) = (sin x * cosh 0,
    cos x * sinh 0), c_cos(iy) = (cosh y, ...), c_exp(x + 0i) = (exp x, 0), c_tanh(iy) = (0, tan y / 1)): that call's error against a
    long double reference is bounded by its slack, the figure the budget of test_operator_against_mpmath charges per call."""
    group, op, axis_in, part_out, ref, sampler = REAL_FUNCTIONS[name]
    R = ca.real_of(dtype)
    x = sampler(ca._rng("real", name, np.dtype(dtype).name), R).astype(R)
    z = np.zeros(len(x), dtype=dtype)
    if axis_in == "re":
        z.real = x
    else:
        z.imag = x
    out, _, _ = device_eval(api, [de.Node(1, de.Node(feature=1))], ca.operator_enum(op), np.asfortranarray(z[None, :]), dtype, early_exit=False)
    got = out[0].real if part_out == "re" else out[0].imag
    with np.errstate(all="ignore"):
        want = ref(x.astype(LD))
    m = np.isfinite(want.astype(R)) & (np.abs(want.astype(R)) >= np.finfo(R).tiny)
    assert m.mean() > 0.9
    e = _real_ulp(got[m], want[m], R)
    i = int(np.argmax(e))
    REAL_REPORT[f"{name} {np.dtype(R).name}"] = dict(max_ulp=float(e[i]), at=float(x[m][i]), slack=slack(group, R), through=op)
    print(f"{name} {np.dtype(R).name}: {e[i]:.3f} ulp at {x[m][i]!r} (slack {slack(group, R)})")
    assert e[i] <= slack(group, R), f"{name}: {e[i]:.3f} ulp at x = {x[m][i]!r}"


@pytest.mark.parametrize("dtype", ca.CDTYPES, ids=["cf32", "cf64"])
def test_atan2_inside_log(api, dtype):
    """atan2 has no opcode: the imaginary part of log z is atan2(y, x) untouched, measured on every region of log."""
    pop = ca.population("log", dtype)
    R = ca.real_of(dtype)
    got = device_population(api, pop).imag.astype(np.float64)
    with np.errstate(all="ignore"):
        e = np.abs((got - pop.ref.im_hi) - pop.ref.im_lo) / np.spacing(np.abs(pop.ref.im_hi).astype(R)).astype(np.float64)
    e = np.where(np.abs(pop.ref.im_hi) >= float(np.finfo(R).tiny), e, 0.0)
    i = int(np.argmax(e))
    REAL_REPORT[f"atan2 {np.dtype(R).name}"] = dict(max_ulp=float(e[i]), at=repr(complex(pop.args[0][i])), slack=slack("atan2", R), through="log")
    print(f"atan2 {np.dtype(R).name}: {e[i]:.3f} ulp at {pop.args[0][i]!r} (slack {slack('atan2', R)})")
    assert e[i] <= slack("atan2", R), f"atan2: {e[i]:.3f} ulp at z = {pop.args[0][i]!r}"


@pytest.mark.parametrize("name", ["log", "log1p"])
def test_log_and_log1p_f32(api, name):
    """logf / log1pf, the real part of the ComplexF32 log, as real one-operator trees (the Float64 ones: tests/test_gpu_ulp_f64.py).
    log1p over the arguments c_log gives it, (beta - 1)(beta + 1) + theta^2 with 0.5 < beta^2: above -0.5."""
    g = ca._rng("real", name)
    if name == "log":
        x = np.concatenate([10.0 ** g.uniform(-44, 38, 4000), g.uniform(0.5, 2, 4000)])
    else:
        x = np.concatenate([g.uniform(-0.5, 2.7, 4000), g.choice([-1.0, 1.0], 4000) * 10.0 ** g.uniform(-12, -1, 4000)])
    x = x.astype(np.float32)
    ops = de.OperatorEnum(binary_operators=("+",), unary_operators=(name,))
    out, _ = api.eval_tree_array(de.Node(1, de.Node(feature=1)), np.asfortranarray(x[None, :]), ops, eval_context=api.EvalContext(early_exit=False))
    want = (np.log if name == "log" else np.log1p)(x.astype(LD))
    m = np.abs(want.astype(np.float32)) >= np.finfo(np.float32).tiny
    e = _real_ulp(out[m], want[m], np.float32)
    i = int(np.argmax(e))
    REAL_REPORT[f"{name} float32"] = dict(max_ulp=float(e[i]), at=float(x[m][i]), slack=slack("log", np.float32), through=f"{name} (real)")
    print(f"{name} float32: {e[i]:.3f} ulp at {x[m][i]!r}")
    assert e[i] <= slack("log", np.float32), f"{name}: {e[i]:.3f} ulp at x = {x[m][i]!r}"


# ---- b. special values against the oracle ---------------------------------------------------------------------------------------------
def _compare_special(op, dtype, zs, dev, orc, label):
    """Per component: the same NaNs, the same infinities with their signs, the same signs of zeros; finite values within the bound of
    test_operator_against_mpmath taken against the oracle: |device - oracle| <= 2 oracle cap + budget, normwise where both parts are
    finite, else in ulps of the finite part."""
    R = ca.real_of(dtype)
    lim = 2 * CAPS[(op, np.dtype(dtype).name)][0] + budget(op, dtype)
    bad = []
    for k in range(len(dev)):
        d, o = (dev[k].real, dev[k].imag), (orc[k].real, orc[k].imag)
        where = f"{label} {op}({', '.join(repr(complex(z[k])) for z in zs)}): device {dev[k]!r}, oracle {orc[k]!r}"
        if any(np.isnan(a) != np.isnan(b) or (np.isinf(b) or np.isinf(a)) and a != b or (a == 0 and b == 0 and np.signbit(a) != np.signbit(b))
               for a, b in zip(d, o)):
            bad.append(where)
            continue
        fin = [np.isfinite(b) for b in o]
        with np.errstate(all="ignore"):
            if all(fin):  # (in halves: floatmax + floatmax i has no finite modulus)
                scale = 2 * float(np.spacing(R(np.hypot(o[0] / 2, o[1] / 2))))
                err = 2 * np.hypot(float(d[0]) / 2 - float(o[0]) / 2, float(d[1]) / 2 - float(o[1]) / 2) / scale
            else:
                err = max([abs(float(a) - float(b)) / float(np.spacing(R(abs(b)))) for a, b, f in zip(d, o, fin) if f], default=0.0)
        if not err <= lim:
            bad.append(where + f" ({err:.2f} ulp > {lim})")
    return bad


SPECIAL_MODES = {"noee": dict(early_exit=False), "ee": dict(early_exit=True, full_eval=True)}
SPECIAL_CASES = [(op, dt) for op in ca.UNARY for dt in ca.CDTYPES]


@pytest.mark.parametrize("op,dtype", SPECIAL_CASES, ids=[f"{op}-{np.dtype(dt).name}" for op, dt in SPECIAL_CASES])
def test_special_values_unary(api, co, op, dtype):
    z = ca.special_grid(dtype)
    _special(api, co, op, dtype, [de.Node(1, de.Node(feature=1))], (z,))


@pytest.mark.parametrize("dtype", ca.CDTYPES, ids=["cf32", "cf64"])
@pytest.mark.parametrize("op", ["*", "/"])
def test_special_values_binary(api, co, op, dtype):
    a, b = ca.special_pairs(dtype)
    _special(api, co, op, dtype, [de.Node(1, de.Node(feature=1), de.Node(feature=2))], (a, b))


def _special(api, co, op, dtype, trees, zs):
    ops = ca.operator_enum(op)
    R = ca.real_of(dtype)
    tape, consts = de.flatten(trees[0], ops, dtype)
    X = np.asfortranarray(np.stack(zs))
    # the oracle's values: without early exit (with it the reference stops at the first array with a non-finite element, here the
    # feature row itself, and leaves the rest unspecified); the values do not depend on the mode, the flag does
    orc, _ = co.eval_tree_array(tape, consts, X, dtype, 6, elementwise=True)
    fin = np.isfinite(orc) & np.isfinite(X).all(axis=0)
    assert 0 < fin.sum() < len(fin)
    bad = []
    for mode, kw in SPECIAL_MODES.items():
        options = 7 if kw["early_exit"] else 6
        _, orc_ok = co.eval_tree_array(tape, consts, X, dtype, options, elementwise=True)
        out, ok, _ = device_eval(api, trees, ops, X, dtype, **kw)
        if bool(ok[0]) != orc_ok:
            bad.append(f"{mode}: complete flag {bool(ok[0])}, oracle {orc_ok}")
        bad += _compare_special(op, dtype, zs, out[0], orc, mode)
        # the flag in the other direction: finite inputs with finite results, in a call of their own, are a complete tree
        _, orc2_ok = co.eval_tree_array(tape, consts, X[:, fin], dtype, options, elementwise=True)
        out2, ok2, _ = device_eval(api, trees, ops, np.asfortranarray(X[:, fin]), dtype, **kw)
        if not (orc2_ok and bool(ok2[0])):
            bad.append(f"{mode}: finite inputs with finite results alone: complete flag {bool(ok2[0])}, oracle {orc2_ok}")
        if not np.array_equal(out2[0].view(R), out[0][fin].view(R)):
            bad.append(f"{mode}: finite inputs with finite results alone have other bits than inside the grid")
    # plain early exit (rows of an incomplete tree are unspecified): the flag alone
    _, ok, _ = device_eval(api, trees, ops, X, dtype, early_exit=True)
    if ok[0]:
        bad.append("ee without full_eval: complete flag True on a grid with NaN inputs")
    assert not bad, f"{len(bad)} special values differ:\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("dtype", ca.CDTYPES, ids=["cf32", "cf64"])
def test_tanh_guard_zero_sign_where_twice_the_imaginary_part_overflows(api, co, dtype):
    """Regression: behind tanh's overflow guard the zero imaginary part takes the sign of eta sin(2|eta|); for |eta| > floatmax / 2 the
    argument 2|eta| is Inf and sin(Inf) is NaN (Julia throws), so the sign was that of a NaN: +0 on the device, -0 on the oracle's libm at
    tanh(floatmax + floatmax i).  Both now take the sign of sin(2a) from sin a cos a, which is C99 Annex G's value (numpy's tanh on the
    host): DESIGN.md §14.1.  tan is tanh with the parts swapped."""
    R = ca.real_of(dtype)
    tree = de.Node(1, de.Node(feature=1))
    for op, f in (("tanh", np.tanh), ("tan", np.tan)):
        z = ca.guard_overflow_points(dtype)
        if op == "tan":
            z = (z.imag + 1j * z.real).astype(dtype)
        with np.errstate(all="ignore"):
            want = f(z)
        out, _, _ = device_eval(api, [tree], ca.operator_enum(op), np.asfortranarray(z[None, :]), dtype, early_exit=False)
        tape, consts = de.flatten(tree, ca.operator_enum(op), dtype)
        orc, _ = co.eval_tree_array(tape, consts, z[None, :], dtype, 6, elementwise=True)
        np.testing.assert_array_equal(out[0].view(R), want.view(R), err_msg=f"{op}: device")
        np.testing.assert_array_equal(orc.view(R), want.view(R), err_msg=f"{op}: oracle")


# ---- c. the tile shape does not reach the bits ----------------------------------------------------------------------------------------
TILE_CASES = [(op, dt) for op in ("sqrt", "/", "tanh") for dt in ca.CDTYPES]


@pytest.mark.parametrize("op,dtype", TILE_CASES, ids=[f"{op}-{np.dtype(dt).name}" for op, dt in TILE_CASES])
def test_tile_shape_independence(api, op, dtype):
    """ComplexF32 carries two samples per lane and 512 per workgroup (ComplexF64: one and 256): calls of 1, 511 and 513 columns, and the
    DIRECT gather variant (F = 17), give the bits of the head of the 1500-column call."""
    R = ca.real_of(dtype)
    ops = ca.operator_enum(op)
    binary = op in ca.BINARY_REGIONS
    args = ca.binary_region(op, ("ordinary", "ordinary"), dtype) if binary else (ca.unary_region("wide_eq" if op == "sqrt" else "ordinary", dtype),)
    X = np.asfortranarray(np.stack(args))
    assert X.shape[1] == 1500
    tree = de.Node(1, *[de.Node(feature=k + 1) for k in range(len(args))])
    full, _, kernel = device_eval(api, [tree], ops, X, dtype, early_exit=False)
    assert "direct" not in kernel
    for n in (1, 511, 513):
        head, _, _ = device_eval(api, [tree], ops, np.asfortranarray(X[:, :n]), dtype, early_exit=False)
        np.testing.assert_array_equal(head[0].view(R), full[0][:n].view(R), err_msg=f"{op}: N = {n}")
    # F = 17: the operands in rows 17 (and 9), seeded noise in the others
    g = ca._rng("tile", op, np.dtype(dtype).name)
    X17 = np.asfortranarray((g.standard_normal((17, 1500)) + 1j * g.standard_normal((17, 1500))).astype(dtype))
    rows = [17, 9][:len(args)]
    for r, a in zip(rows, args):
        X17[r - 1] = a
    wide, _, kernel = device_eval(api, [de.Node(1, *[de.Node(feature=r) for r in rows])], ops, X17, dtype, early_exit=False)
    assert "direct" in kernel, kernel
    np.testing.assert_array_equal(wide[0].view(R), full[0].view(R), err_msg=f"{op}: F = 17")


# ---- d. the report --------------------------------------------------------------------------------------------------------------------
def test_zz_write_ulp_report():
    """Runs last in this module: the per-operator figures of DESIGN.md §14.3."""
    assert len(REPORT) >= len(CASES)
    import torch
    out_dir = os.environ.get("DE_ULP_REPORT_DIR") or os.path.join(ROOT, "build", "reports")  # (build/ is kept out of git)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "ulp_complex.json"), "w") as fh:
        json.dump(dict(what="max normwise error |got - mpmath| / spacing(|mpmath|) per complex operator, form (xx: features; cx / xc: a constant "
                            "left / right operand), dtype and input region, in ulps of the component type, of the device and of the CPU "
                            "oracle on the same inputs, with the input at the maximum and the share of points kept "
                            "(tests/test_gpu_complex_accuracy.py); real_functions: the real library calls inside the formulas, each alone",
                       device=torch.cuda.get_device_name(0), hip=str(torch.version.hip), operators=REPORT, real_functions=REAL_REPORT),
                  fh, indent=1, sort_keys=True)
    worst = max(((k, r, v["device"]) for k, rs in REPORT.items() for r, v in rs.items()), key=lambda t: t[2])
    print(f"[complex ulp] {len(REPORT)} populations, worst {worst[0]} in {worst[1]}: {worst[2]:.3f} ulp")
