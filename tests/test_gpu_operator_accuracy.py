"""Every real operator on the MI355X against mpmath, per operator: Float32 values and every partial (Float32 and Float64).

The populations, references and bounds are those of tests/operator_accuracy.py; tests/test_operator_accuracy_host.py holds the CPU oracle
to the same tables, so nothing here rests on the oracle's formulas.

a. Float32 values of all 53 opcodes as one-operator trees with early_exit=False through the default eval kernel, the flat-switch kernel
   (DE_EVAL_THREADED=0) and the value output of eval_grad: 0 ulp for exact operators, 0.5 for correctly rounded ones, 2 (+2^-9) for
   library functions (the project's asserted figure: DESIGN.md §5, tests/test_gpu_ops.py), the derived composite bound for cube,
   custom_cos and pow_abs2, 1.5 steps for results below floatmin.  The accumulator form op(x1 + x2) with x2 == 0 and the constant forms
   op(x1 + 0.0), op(x1, c), op(c, x1) give the bits of the leaf form, so accuracy is measured once.  (The Float64 values:
   tests/test_gpu_ulp_f64.py.  Turbo has its own contract and test.)
b. Partials through Population.eval_grad(X, True) on op(x1) / op(x1, x2) / op(x1, x2, x3): the flat-switch kernel (DE_GRAD_THREADED=0)
   and the threaded kernel at one and (Float32) two samples per lane.  E <= B(x; s_device) at every kept point, s_device = 2 ulp
   Float32 / 1 ulp Float64; exact rows and the edge table of DESIGN.md §6 bit for bit; the accumulator form carries the bits of the
   leaf form; flags as the oracle's element-wise flags.
c. The shape does not reach the bits: N = 1, 63, 1025 and 1500 columns against the columns of the whole population (tanh, ^, gamma).
d. The report ulp_real.json, written to $DE_ULP_REPORT_DIR, by default build/reports/ of the checkout.

What these tests found on an MI355X (ROCm 7.0), all fixed in csrc/ (DESIGN.md §5): OCML's asinf 2.41 ulp at 0.50173968 and tgammaf 4.99
ulp at 27.123329 (5.88 next to the poles) against the bound of 2: M<float>::asin / tgamma now round the Float64 function once; with
early_exit=False the threaded eval kernel gave cos(x1 + x2) and sin(x1 + x2) the library's bits and cos(x1) the hot polynomial's (9 % of
60000 points one ulp apart): the injected generic handlers now call the hot function.  Run with `pytest -m gpu`."""
import functools
import json
import os

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import operator_accuracy as oa
from oracle import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUE_REPORT, PARTIAL_REPORT = {}, {}

EVAL_PATHS = ("eval", "eval-flat", "eval_grad")
GRAD_PATHS = {"flat": {"DE_GRAD_THREADED": "0"}, "threaded-1": {"DE_GRAD_VS2_MIN_N": "1000000000000"}, "threaded-2": {"DE_GRAD_VS2_MIN_N": "0"}}


def grad_paths(dtype):   # two samples per lane exist in Float32 only
    return [p for p in GRAD_PATHS if dtype == np.float32 or p != "threaded-2"]


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _api.library()
    return _api


def device_eval(api, key, tree, X, dtype=np.float32):
    pop = api.Population([tree], oa.operator_enum(key), dtype, n_features=X.shape[0], eval_context=api.EvalContext(early_exit=False))
    try:
        out, ok = pop.eval(X)
        return out[0], bool(ok[0])
    finally:
        pop.close()


def device_grad(api, key, tree, X, dtype):
    """(values, Jacobian rows [F, N], flag) of one tree; full_eval: every column is evaluated whatever the flag of the tree becomes."""
    pop = api.Population([tree], oa.operator_enum(key), dtype, n_features=X.shape[0], eval_context=api.EvalContext(full_eval=True))
    try:
        out, grads, ok = pop.eval_grad(X, True)
        return out[0], np.asarray(grads[0]), bool(ok[0])
    finally:
        pop.close()


def set_env(monkeypatch, env):
    for k in ("DE_GRAD_THREADED", "DE_GRAD_VS2_MIN_N", "DE_EVAL_THREADED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@functools.lru_cache(maxsize=None)
def oracle_partials(key, dtype_name):
    pop = oa.partial_population(key, np.dtype(dtype_name).type)
    return oa.oracle_grad(oracle, key, pop.args)


# ---- a. Float32 values ----------------------------------------------------------------------------------------------------------------
VALUE_CASES = [(k, p) for k in oa.OPS for p in EVAL_PATHS]


@pytest.mark.parametrize("key,path", VALUE_CASES, ids=[f"{oa.key_name(k)}-{p}" for k, p in VALUE_CASES])
def test_values_f32(api, monkeypatch, key, path):
    pop = oa.value_population(key)
    X = oa.feature_matrix(pop.args)
    tree = oa.leaf_tree(key)
    set_env(monkeypatch, {"DE_EVAL_THREADED": "0"} if path == "eval-flat" else {})
    got = device_grad(api, key, tree, X, np.float32)[0] if path == "eval_grad" else device_eval(api, key, tree, X)[0]
    tape, consts = de.flatten(tree, oa.operator_enum(key), np.float32)
    orc = oa.value_maxima(pop, oracle.eval_tree_array(tape, consts, X, options=6, elementwise=True)[0], s=oa.S_ORACLE)
    dev = oa.value_maxima(pop, got)
    VALUE_REPORT[f"{oa.key_name(key)} {path}"] = {
        r: dict(kept=m["kept"], device_ulp=m["max_ulp"], device_E=m["max_E"], oracle_ulp=orc[r]["max_ulp"], bound=m["bound"],
                bound_in="E" if oa.value_in_E(key) else "ulp", worst=m["worst"], at=m["at"], subnormal_steps=m["max_subnormal_steps"]) for r, m in dev.items()}
    failures = []
    for r, m in dev.items():
        print(f"{oa.key_name(key)} {path} {r}: kept {m['kept']:.3f}; device {m['max_ulp']:.3f} ulp (E {m['max_E']:.3f}) at {m['at']}, oracle {orc[r]['max_ulp']:.3f} ulp; "
              f"bound {m['bound']:.3f}; subnormal steps {m['max_subnormal_steps']:.2f}")
        assert m["kept"] >= oa.MIN_KEPT, (r, m["kept"])
        if m["bad"]:
            failures.append(f"{r}: {m['bad']} points past the bound {m['bound']:.3f}, worst {m['worst']:.3f} at {m['at']}, first at {m['first_bad']}")
    assert not failures, f"{oa.key_name(key)} {path}: " + "; ".join(failures)
    if path != "eval":
        return
    # the other lowered forms of the operator run the same code
    x1 = de.Node(feature=1)
    if key[1] == 1:
        acc = device_eval(api, key, oa.accumulator_tree(key), oa.feature_matrix(pop.args, extra_zero_row=True))[0]
        assert oa.same_bits(acc, got).all(), "op(x1 + x2), x2 == 0"
        fused = device_eval(api, key, de.Node(1, de.Node(1, x1, de.Node(val=0.0))), X)[0]
        assert oa.same_bits(fused, got).all(), "op(x1 + 0.0)"
    elif key[1] == 2:
        a, b = pop.args
        for c in (b[0], b[len(b) // 2]):
            want = device_eval(api, key, tree, oa.feature_matrix((a, np.full_like(a, c))))[0]
            fused = device_eval(api, key, de.Node(1, x1, de.Node(val=float(c))), oa.feature_matrix((a,)))[0]
            assert oa.same_bits(fused, want).all(), f"op(x1, {c})"
            want = device_eval(api, key, tree, oa.feature_matrix((np.full_like(a, c), a)))[0]
            fused = device_eval(api, key, de.Node(1, de.Node(val=float(c)), x1), oa.feature_matrix((a,)))[0]
            assert oa.same_bits(fused, want).all(), f"op({c}, x1)"


# ---- b. partials ------------------------------------------------------------------------------------------------------------------------
PARTIAL_CASES = [(k, dt, p) for k in oa.BOUNDED for dt in oa.DTYPES for p in grad_paths(dt)]
EXACT_CASES = [(k, dt, p) for k in oa.OPS if k in oa.EXACT for dt in oa.DTYPES for p in grad_paths(dt)]
_ids = lambda cases: [f"{oa.key_name(k)}-{np.dtype(dt).name}-{p}" for k, dt, p in cases]


def _accumulator_rows_match(api, key, args, dtype, leaf_out, leaf_rows):
    out, rows, _ = device_grad(api, key, oa.accumulator_tree(key), oa.feature_matrix(args, extra_zero_row=True), dtype)
    assert oa.same_bits(out, leaf_out).all(), "op(x1 + x2), x2 == 0: values"
    assert oa.same_bits(rows[0], leaf_rows[0]).all(), "op(x1 + x2), x2 == 0: the x1 row"


@pytest.mark.parametrize("key,dtype,path", PARTIAL_CASES, ids=_ids(PARTIAL_CASES))
def test_partials_within_the_pointwise_bound(api, monkeypatch, key, dtype, path):
    pop = oa.partial_population(key, dtype)
    set_env(monkeypatch, GRAD_PATHS[path])
    out, rows, ok = device_grad(api, key, oa.leaf_tree(key), oa.feature_matrix(pop.args), dtype)
    _, orc_rows, orc_ok = oracle_partials(key, np.dtype(dtype).name)
    failures = []
    for k in range(key[1]):
        dev = oa.partial_maxima(pop, k, rows[k], pop.b_dev[k])
        orc = oa.partial_maxima(pop, k, orc_rows[k], pop.b_orc[k])
        for r, m in dev.items():
            PARTIAL_REPORT[f"{oa.key_name(key)} d{k} {np.dtype(dtype).name} {path} {r}"] = dict(
                kept=m["kept"], device_max_E=m["max_E"], oracle_max_E=orc[r]["max_E"], max_B=m["max_B"], worst_E_over_B=m["worst_ratio"], at=m["at"])
            print(f"{oa.key_name(key)} d{k} {np.dtype(dtype).name} {path} {r}: kept {m['kept']:.3f}; device max E {m['max_E']:.3f}, oracle {orc[r]['max_E']:.3f}; "
                  f"max B {m['max_B']:.3f}; worst E / B {m['worst_ratio']:.3f} (E {m['E_at_worst']:.3f}, B {m['B_at_worst']:.3f}) at {m['at']}")
            assert m["kept"] >= oa.MIN_KEPT, (r, m["kept"])
            if not m["worst_ratio"] <= 1.0:
                failures.append(f"d{k} {r}: E = {m['E_at_worst']:.3f} > B = {m['B_at_worst']:.3f} at {m['at']}")
    assert not failures, f"{oa.key_name(key)} {np.dtype(dtype).name} {path}: " + "; ".join(failures)
    assert ok == orc_ok, f"flag {ok}, oracle (element-wise) {orc_ok}"
    if key[1] == 1:
        _accumulator_rows_match(api, key, pop.args, dtype, out, rows)


@pytest.mark.parametrize("key,dtype,path", EXACT_CASES, ids=_ids(EXACT_CASES))
def test_exact_rows(api, monkeypatch, key, dtype, path):
    args, regions, want = oa.exact_population(key, dtype)
    set_env(monkeypatch, GRAD_PATHS[path])
    out, rows, ok = device_grad(api, key, oa.leaf_tree(key), oa.feature_matrix(args), dtype)
    for k in range(key[1]):
        same = oa.same_bits(rows[k], want[k])
        assert same.all(), f"{oa.key_name(key)} d{k}: {(~same).sum()} rows differ, first at {[a[np.argmax(~same)] for a in args]}: {rows[k][np.argmax(~same)]}, expected {want[k][np.argmax(~same)]}"
    _, _, orc_ok = oa.oracle_grad(oracle, key, args)
    assert ok == orc_ok, f"flag {ok}, oracle (element-wise) {orc_ok}"
    if key[1] == 1:
        _accumulator_rows_match(api, key, args, dtype, out, rows)


EDGE_CASES = [(dt, p) for dt in oa.DTYPES for p in grad_paths(dt)]


@pytest.mark.parametrize("dtype,path", EDGE_CASES, ids=[f"{np.dtype(dt).name}-{p}" for dt, p in EDGE_CASES])
def test_edge_table(api, monkeypatch, dtype, path):
    """The Jacobian rows of the one-operator tree at the points of DESIGN.md §6: row k = sum_j g_j (j == k) of the written-out partials
    (a NaN or infinite partial of another argument turns the row into NaN, as in the reference).  One call per operator and per
    finiteness of the arguments."""
    set_env(monkeypatch, GRAD_PATHS[path])
    groups = {}
    for key, args, want in oa.edge_table(dtype):
        groups.setdefault((key, all(np.isfinite(a) for a in args)), []).append((args, want))
    bad = []
    show = lambda v: tuple(float(a) for a in v)
    for (key, finite), rows_in in groups.items():
        args = tuple(np.array([r[0][k] for r in rows_in], dtype=dtype) for k in range(key[1]))
        _, rows, ok = device_grad(api, key, oa.leaf_tree(key), oa.feature_matrix(args), dtype)
        all_finite = True
        for i, (a, want) in enumerate(rows_in):
            exp = oa.jacobian_rows(want)
            all_finite &= all(np.isfinite(e) for e in exp)
            got = tuple(rows[k][i] for k in range(key[1]))
            if not all(oa.same_bits(np.array([g], dtype=dtype), np.array([e], dtype=dtype))[0] for g, e in zip(got, exp)):
                bad.append(f"{oa.key_name(key)}{show(a)}: rows {show(got)}, DESIGN.md §6: {show(exp)}")
        if finite and all_finite and key[0] not in oa.SAFE_OF:   # (a safe_* operator outside its domain: the VALUE is NaN)
            if not ok:
                bad.append(f"{oa.key_name(key)}: finite arguments and finite partials, flag {ok}")
        if not all_finite and ok:
            bad.append(f"{oa.key_name(key)}: a non-finite Jacobian entry, flag {ok}")
    assert not bad, f"{len(bad)} edge rows differ:\n" + "\n".join(bad)


# ---- c. the shape does not reach the bits ---------------------------------------------------------------------------------------------
SHAPE_CASES = [(k, dt, p) for k in (("tanh", 1), ("^", 2), ("gamma", 1)) for dt in oa.DTYPES for p in grad_paths(dt) if p != "flat"]


@pytest.mark.parametrize("key,dtype,path", SHAPE_CASES, ids=_ids(SHAPE_CASES))
def test_shape_independence(api, monkeypatch, key, dtype, path):
    """N = 1, 63, 1025 and 1500 (across a 64-lane wave and a 1024-sample tile) give the bits of those columns of the whole population:
    values and rows of eval_grad at both lanes-per-sample variants, and the values of eval."""
    pop = oa.partial_population(key, dtype)
    X = oa.feature_matrix(pop.args)
    assert X.shape[1] > 1500
    tree = oa.leaf_tree(key)
    set_env(monkeypatch, GRAD_PATHS[path])
    full_out, full_rows, _ = device_grad(api, key, tree, X, dtype)
    full_eval = device_eval(api, key, tree, X, dtype)[0]
    for n in (1, 63, 1025, 1500):
        Xn = np.asfortranarray(X[:, :n])
        out, rows, _ = device_grad(api, key, tree, Xn, dtype)
        assert oa.same_bits(out, full_out[:n]).all(), f"eval_grad values, N = {n}"
        assert oa.same_bits(rows, full_rows[:, :n]).all(), f"eval_grad rows, N = {n}"
        assert oa.same_bits(device_eval(api, key, tree, Xn, dtype)[0], full_eval[:n]).all(), f"eval, N = {n}"


# ---- d. the report --------------------------------------------------------------------------------------------------------------------
def test_zz_write_ulp_report():
    """Runs last in this module: the per-operator figures of DESIGN.md §5."""
    assert len(VALUE_REPORT) >= len(VALUE_CASES) and len(PARTIAL_REPORT) >= len(PARTIAL_CASES)
    import torch
    out_dir = os.environ.get("DE_ULP_REPORT_DIR") or os.path.join(ROOT, "build", "reports")   # (build/ is kept out of git)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "ulp_real.json"), "w") as fh:
        json.dump(dict(what="values_f32: per operator, kernel path and input region, the share of points kept, the max error of the device and of "
                            "the CPU oracle in Float32 ulp (and the device's in E = |got - true| / (eps |true|)), the bound and where the worst "
                            "point is; partials: per operator, argument, dtype, kernel path and region, the kept share, max E of the device and "
                            "of the oracle, max B, the worst E / (1.01 B + 2^-9) and where (tests/test_gpu_operator_accuracy.py)",
                       device=torch.cuda.get_device_name(0), hip=str(torch.version.hip), values_f32=VALUE_REPORT, partials=PARTIAL_REPORT),
                  fh, indent=1, sort_keys=True)
    worst = max(PARTIAL_REPORT.items(), key=lambda kv: kv[1]["worst_E_over_B"])
    print(f"[real ulp] {len(VALUE_REPORT)} value populations, {len(PARTIAL_REPORT)} partial regions, worst E / B {worst[1]['worst_E_over_B']:.3f}: {worst[0]}")
