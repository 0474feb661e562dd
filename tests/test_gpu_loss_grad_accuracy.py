"""The fused loss gradient (de_eval_loss_grad) on the MI355X, per operator and per kernel, against mpmath: every partial of all 53
opcodes through forward duals with the loss reduction ("forward"), the two-samples-per-lane modules ("forward-2", Float32) and reverse
accumulation ("reverse", csrc/de_rev_threaded.hip, whose hot handlers restate the partial functions of csrc/de_grad_common.h).

The vehicle is that of tests/loss_grad_accuracy.py: loss="pullback", dY = 1, N = 1, variable=False, one tree per point of the
populations of tests/operator_accuracy.py with the point in the tree's constants and every feature -0.0; entry k of a tree's gradient
is then the kernel's partial k and its "loss" the operator's value.  tests/test_loss_grad_accuracy_host.py shows on the CPU oracle that
the vehicle adds nothing, that the reverse encoder takes every form, and that the acceptance rule refuses the wrong models.  The tables,
the bound B(x; s_device) and the rule E <= 1.01 B + 2^-9 are those of tests/test_gpu_operator_accuracy.py: no tolerance is added here.

a. Bounded partials: every operator of oa.BOUNDED, dtype, path and form within the bound at every kept point; a kept point's tree is ok.
b. Exact rows: the operators of oa.EXACT and the edge table of DESIGN.md §6 bit for bit; a point with a non-finite argument, partial or
   VALUE (a safe_* operator outside its domain: the value is NaN) has ok False, a NaN loss and NaN entries.  "Bit for bit" leaves out the
   sign of a zero, here and in c and d: every output is a sum over the samples that starts at +0 (same_result below).
c. Values: the pullback "loss" has the bits of eval_grad's `out` on the forward paths, and on the reverse path the bits of the forward
   path at one sample per lane.
d. The sample's position does not reach the bits: N = 65 and 1025, a one-hot dY at sample 0, 63, 64 and N - 1 (tanh, ^, gamma, /).
e. Leaf operands in sum form: op(x1[, x2[, x3]]), variable=True, dY = 1 over the first 257 kept points of a region, each row within
   eps sum_j (1.01 B_j + 2^-9) |p_j| + gamma_256 sum_j |p_j| of the mpmath sum: the bound of a sum in any association.
f. The report loss_grad_accuracy.json, written to $DE_ULP_REPORT_DIR, by default build/reports/ of the checkout.

Found on an MI355X (ROCm 7.0), both fixed in csrc/ (DESIGN.md §5).  By (a): the reverse kernel wrote the second partial of `/` as
-(v * (1 / y)), which rounds twice more than binary_vg's -(v / y): E = 1.10 (Float32) and 1.24 (Float64) against the bound of 1; it now
writes the reference's expression (0.85 / 0.90).  By (b): the lowering evaluates op(leaf, subtree) with its operands swapped and treated
max / min as commutative, which their partials at a tie are not: max(c1, x1 + c2) and min(c1, x1 + c2) gave the tie to the wrong argument
in every gradient kernel; the gradient program now names the swapped forms.  Run with `pytest -m gpu`."""
import json
import os

import numpy as np
import pytest

import dynamicexpressions_jl_amd as de
import loss_grad_accuracy as lga
import operator_accuracy as oa
from oracle import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REVERSE_KERNEL = "de_rev_threaded_kernel"
PATHS = {"forward": {"DE_LOSS_GRAD_REVERSE": "0", "DE_GRAD_VS2_MIN_N": "1000000000000"},
         "forward-2": {"DE_LOSS_GRAD_REVERSE": "0", "DE_GRAD_VS2_MIN_N": "0"},
         "reverse": {"DE_LOSS_GRAD_REVERSE": "1"}}
# forms the reverse encoder refuses (ensure_rev_threaded then runs forward duals silently): (operator, degree, form) -> the reason read
# from encode_grad_reverse.  Empty: tests/test_loss_grad_accuracy_host.py shows that it takes every form.  An entry is asserted to fall back.
REVERSE_REFUSES = {}
REPORT = {}
_RESULTS = {}


def paths(dtype):   # two samples per lane exist in Float32 only
    return [p for p in PATHS if dtype == np.float32 or p != "forward-2"]


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _api.library()
    return _api


def set_env(monkeypatch, path):
    for k in ("DE_LOSS_GRAD_REVERSE", "DE_GRAD_VS2_MIN_N", "DE_GRAD_THREADED", "DE_REV_NO_FUSE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)


def check_kernel(pop, path, what):
    name = pop.ctx.last_kernel_name()
    if path == "reverse" and what not in REVERSE_REFUSES:
        assert name == REVERSE_KERNEL, f"{what}: the reverse path ran {name}"
    else:
        assert name != REVERSE_KERNEL, f"{what}: {path} ran {name}"


def vehicle_call(pop, key, dtype, form, path, N=1, hot=0, with_out=False):
    """(loss[t], rows[k][t], ok[t][, eval_grad's out[t]]) of a population of one-point trees: N equal samples, dY one-hot at `hot`."""
    X = lga.neg_zero_X(lga.form_features(key, form), N, dtype)
    dY = np.zeros(N, dtype=dtype)
    dY[hot] = 1
    loss, dls, ok = pop.eval_loss_grad(X, dY, loss="pullback", variable=False)
    check_kernel(pop, path, (key[0], key[1], form))
    res = (np.asarray(loss), lga.rows_of(dls, key[1], dtype), np.asarray(ok, dtype=bool))
    if with_out:
        out, _, _ = pop.eval_grad(X, False)
        res += (np.asarray(out)[:, hot].copy(),)
    return res


def vehicle(api, monkeypatch, key, dtype, form, args, path, with_out=False):
    set_env(monkeypatch, path)
    pop = api.Population(lga.form_trees(key, form, args), oa.operator_enum(key), dtype, n_features=lga.form_features(key, form))
    try:
        return vehicle_call(pop, key, dtype, form, path, with_out=with_out)
    finally:
        pop.close()


def population_result(api, monkeypatch, key, dtype, form, path):
    """The N = 1 result of the whole population of (operator, dtype), cached per form and path (never modified)."""
    k = (key, np.dtype(dtype).name, form, path)
    if k not in _RESULTS:
        args = oa.exact_population(key, dtype)[0] if key in oa.EXACT else oa.partial_population(key, dtype).args
        _RESULTS[k] = vehicle(api, monkeypatch, key, dtype, form, args, path, with_out=path != "reverse")
    return _RESULTS[k]


def same_result(got, want):
    """The bits, NaN for NaN; a zero for a zero whatever its sign: every output of the fused entry point is a SUM over the samples that
    starts at +0 (the lanes past N and the samples of weight 0 add +0), as the reference's matrix-vector product does, and -0 + 0 = +0."""
    got, want = np.asarray(got), np.asarray(want)
    return oa.same_bits(got, want) | ((got == 0) & (want == 0))


def first_difference(same, args):
    i = int(np.argmax(~same))
    return f"{int((~same).sum())} of {len(same)} differ, first at {[float(a[i]) for a in args]}"


def check_values(api, monkeypatch, key, dtype, form, path, args):
    """c.  Where the tree is ok the loss is the operator's value: the bits of eval_grad's out (forward paths), of the forward path (reverse)."""
    res = population_result(api, monkeypatch, key, dtype, form, path)
    loss, ok = res[0], res[2]
    if path == "reverse":
        want = population_result(api, monkeypatch, key, dtype, form, "forward")
        assert np.array_equal(ok, want[2]), f"{form}: flags, reverse against forward: {first_difference(ok == want[2], args)}"
        ref, what = want[0], "the forward path's loss"
    else:
        ref, what = res[3], "eval_grad's out"
    same = same_result(loss, ref) | ~ok
    assert same.all(), f"{form}: the loss against {what}: {first_difference(same, args)}"
    assert np.isnan(loss[~ok]).all(), f"{form}: an incomplete tree has a NaN loss"


# ---- a. bounded partials ----------------------------------------------------------------------------------------------------------------
PARTIAL_CASES = [(k, dt, p) for k in oa.BOUNDED for dt in oa.DTYPES for p in paths(dt)]
EXACT_CASES = [(k, dt, p) for k in oa.OPS if k in oa.EXACT for dt in oa.DTYPES for p in paths(dt)]
_ids = lambda cases: [f"{oa.key_name(k)}-{np.dtype(dt).name}-{p}" for k, dt, p in cases]


@pytest.mark.parametrize("key,dtype,path", PARTIAL_CASES, ids=_ids(PARTIAL_CASES))
def test_partials_within_the_pointwise_bound(api, monkeypatch, key, dtype, path):
    pop = oa.partial_population(key, dtype)
    failures = []
    for form in lga.forms(key):
        loss, rows, ok = population_result(api, monkeypatch, key, dtype, form, path)[:3]
        form_failures, maxima = lga.accept(pop, rows, pop.b_dev)
        for (k, r), m in maxima.items():
            REPORT[f"{oa.key_name(key)} d{k} {np.dtype(dtype).name} {path} {form} {r}"] = dict(
                kept=m["kept"], max_E=m["max_E"], max_B=m["max_B"], worst_E_over_B=m["worst_ratio"], at=m["at"])
            print(f"{oa.key_name(key)} d{k} {np.dtype(dtype).name} {path} {form} {r}: kept {m['kept']:.3f}; max E {m['max_E']:.3f}; max B {m['max_B']:.3f}; "
                  f"worst E / B {m['worst_ratio']:.3f} (E {m['E_at_worst']:.3f}, B {m['B_at_worst']:.3f}) at {m['at']}")
        failures += [f"{form} {f}" for f in form_failures]
        for k in range(key[1]):
            bad = pop.keep[k] & ~ok
            if bad.any():
                failures.append(f"{form} d{k}: {int(bad.sum())} kept points whose tree is not ok, first at {[float(a[np.argmax(bad)]) for a in pop.args]}")
        assert np.isnan(loss[~ok]).all() and all(np.isnan(r[~ok]).all() for r in rows), f"{form}: an incomplete tree has a NaN loss and NaN entries"
        try:
            check_values(api, monkeypatch, key, dtype, form, path, pop.args)
        except AssertionError as e:
            failures.append(str(e).splitlines()[0])
    assert not failures, f"{oa.key_name(key)} {np.dtype(dtype).name} {path}: " + "; ".join(failures)


# ---- b. exact rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,dtype,path", EXACT_CASES, ids=_ids(EXACT_CASES))
def test_exact_rows(api, monkeypatch, key, dtype, path):
    args, regions, want = oa.exact_population(key, dtype)
    finite = np.logical_and.reduce([np.isfinite(w) for w in want])
    failures = []
    for form in lga.forms(key):
        loss, rows, ok = population_result(api, monkeypatch, key, dtype, form, path)[:3]
        if not np.array_equal(ok, finite):   # (the values of these populations are finite)
            failures.append(f"{form}: flags: {first_difference(ok == finite, args)}")
        for k in range(key[1]):
            same = same_result(rows[k], want[k]) | ~finite
            if not same.all():
                i = int(np.argmax(~same))
                failures.append(f"{form} d{k}: {first_difference(same, args)}: {rows[k][i]!r}, expected {want[k][i]!r}")
            if not np.isnan(rows[k][~finite]).all():
                failures.append(f"{form} d{k}: a NaN partial must make every entry of the tree NaN")
        try:
            check_values(api, monkeypatch, key, dtype, form, path, args)
        except AssertionError as e:
            failures.append(str(e).splitlines()[0])
    assert not failures, f"{oa.key_name(key)} {np.dtype(dtype).name} {path}: " + "; ".join(failures)


EDGE_CASES = [(dt, p) for dt in oa.DTYPES for p in paths(dt)]


def _oracle_value(key, args, R):
    code = de.OPCODES[key]
    return (oracle.unary, oracle.binary, oracle.ternary)[key[1] - 1](code, *[float(a) for a in args], R)


@pytest.mark.parametrize("dtype,path", EDGE_CASES, ids=[f"{np.dtype(dt).name}-{p}" for dt, p in EDGE_CASES])
def test_edge_table(api, monkeypatch, dtype, path):
    """The points of DESIGN.md §6 where the conventions are decided, one tree per point and form: finite rows bit for bit; a non-finite
    argument, a non-finite partial or a non-finite value (safe_* outside its domain) makes the tree incomplete: ok False, NaN loss, NaN entries."""
    groups = {}
    for key, args, want in oa.edge_table(dtype):
        groups.setdefault(key, []).append((args, want))
    bad = []
    show = lambda v: tuple(float(a) for a in v)
    for key, points in groups.items():
        args = tuple(np.array([p[0][k] for p in points], dtype=dtype) for k in range(key[1]))
        for form in lga.forms(key):
            loss, rows, ok = vehicle(api, monkeypatch, key, dtype, form, args, path)
            for i, (a, want) in enumerate(points):
                exp = oa.jacobian_rows(want)
                complete = all(np.isfinite(v) for v in a) and all(np.isfinite(e) for e in exp) and np.isfinite(_oracle_value(key, a, dtype))
                got = tuple(rows[k][i] for k in range(key[1]))
                if complete:
                    if not ok[i] or not all(same_result(np.array([g], dtype=dtype), np.array([e], dtype=dtype))[0] for g, e in zip(got, exp)):
                        bad.append(f"{oa.key_name(key)}{show(a)} {form}: ok {ok[i]}, entries {show(got)}, DESIGN.md §6: {show(exp)}")
                elif ok[i] or not np.isnan(loss[i]) or not all(np.isnan(g) for g in got):
                    bad.append(f"{oa.key_name(key)}{show(a)} {form}: an incomplete tree with ok {ok[i]}, loss {float(loss[i])}, entries {show(got)}")
    assert not bad, f"{len(bad)} edge rows differ:\n" + "\n".join(bad)


JACOBIAN_PATHS = {"flat": {"DE_GRAD_THREADED": "0"}, "threaded-1": {"DE_GRAD_VS2_MIN_N": "1000000000000"}, "threaded-2": {"DE_GRAD_VS2_MIN_N": "0"}}
SWAPPED_CASES = [(op, dt, p) for op in ("max", "min") for dt in oa.DTYPES for p in JACOBIAN_PATHS if dt == np.float32 or p != "threaded-2"]


@pytest.mark.parametrize("op,dtype,path", SWAPPED_CASES, ids=[f"{op}-{np.dtype(dt).name}-{p}" for op, dt, p in SWAPPED_CASES])
def test_swapped_max_min_keep_their_argument_order_in_eval_grad(api, monkeypatch, op, dtype, path):
    """Found by (b): the lowering evaluates op(leaf, subtree) as op'(subtree, leaf) and treated max / min as commutative, which their
    partials at a tie are not: max(c1, x1 + c2) gave the tie to the FIRST argument in every gradient kernel.  The fused
    paths are covered by test_exact_rows (form const-left); this is the Jacobian of eval_grad, the flat-switch kernel included."""
    key = (op, 2)
    args, regions, want = oa.exact_population(key, dtype)
    sl = dict(regions)["ties"]
    args, want = tuple(a[sl] for a in args), tuple(w[sl] for w in want)
    assert (args[0] == args[1]).sum() > 100
    for k in ("DE_GRAD_THREADED", "DE_GRAD_VS2_MIN_N"):
        monkeypatch.delenv(k, raising=False)
    for k, v in JACOBIAN_PATHS[path].items():
        monkeypatch.setenv(k, v)
    for form in ("const-left", "const-right"):
        pop = api.Population(lga.form_trees(key, form, args), oa.operator_enum(key), dtype, n_features=1)
        try:
            _, grads, ok = pop.eval_grad(lga.neg_zero_X(1, 1, dtype), False)
        finally:
            pop.close()
        assert np.asarray(ok).all()
        rows = lga.rows_of([np.asarray(g)[:, 0] for g in grads], 2, dtype)
        for k in range(2):
            same = oa.same_bits(rows[k], want[k])
            assert same.all(), f"{op}, {form}, d{k}: {first_difference(same, args)}"


# ---- d. the sample's position does not reach the bits ----------------------------------------------------------------------------------
POSITION_CASES = [(k, dt, p) for k in (("tanh", 1), ("^", 2), ("gamma", 1), ("/", 2)) for dt in oa.DTYPES for p in paths(dt)]


@pytest.mark.parametrize("key,dtype,path", POSITION_CASES, ids=_ids(POSITION_CASES))
def test_sample_position_independence(api, monkeypatch, key, dtype, path):
    """N = 65 and 1025 equal samples (past a wave, past a 1024-sample tile) with a one-hot dY at sample 0, 63, 64 and N - 1 give the bits of
    N = 1: loss and entries (zeros by value: the samples with dY = 0 are excluded, and a sum that starts at +0 loses the sign of -0)."""
    pop = oa.partial_population(key, dtype)
    for form in lga.forms(key):
        loss1, rows1, ok1 = population_result(api, monkeypatch, key, dtype, form, path)[:3]
        set_env(monkeypatch, path)
        trees = api.Population(lga.form_trees(key, form, pop.args), oa.operator_enum(key), dtype, n_features=lga.form_features(key, form))
        try:
            for N in (65, 1025):
                for hot in (0, 63, 64, N - 1):
                    loss, rows, ok = vehicle_call(trees, key, dtype, form, path, N=N, hot=hot)
                    assert np.array_equal(ok, ok1), f"{form} N = {N}, sample {hot}: flags: {first_difference(ok == ok1, pop.args)}"
                    for what, got, want in [("loss", loss, loss1)] + [(f"d{k}", rows[k], rows1[k]) for k in range(key[1])]:
                        same = same_result(got, want)
                        assert same.all(), f"{form} N = {N}, sample {hot}, {what}: {first_difference(same, pop.args)}"
        finally:
            trees.close()


# ---- e. leaf operands, in sum form ------------------------------------------------------------------------------------------------------
LEAF_CASES = [(k, dt, p) for k in oa.OPS for dt in oa.DTYPES for p in paths(dt)]


@pytest.mark.parametrize("key,dtype,path", LEAF_CASES, ids=_ids(LEAF_CASES))
def test_leaf_operands_in_sum_form(api, monkeypatch, key, dtype, path):
    set_env(monkeypatch, path)
    pop = api.Population([oa.leaf_tree(key)], oa.operator_enum(key), dtype, n_features=key[1])
    failures = []
    try:
        for name, args, parts in lga.leaf_sum_cases(key, dtype):
            loss, dls, ok = pop.eval_loss_grad(oa.feature_matrix(args), np.ones(lga.LEAF_N, dtype=dtype), loss="pullback", variable=True)
            check_kernel(pop, path, (key[0], key[1], "leaf"))
            assert bool(ok[0]), f"{name}: the tree of {lga.LEAF_N} kept points is not ok"
            for k, (hi, lo, slack) in enumerate(parts):
                err, bound = lga.leaf_sum_error(dls[0][k], hi, lo, slack, dtype)
                print(f"{oa.key_name(key)} d{k} {np.dtype(dtype).name} {path} {name}: |sum error| {err:.3e}, bound {bound:.3e}")
                if not err <= bound:
                    failures.append(f"{name} d{k}: {float(dls[0][k])!r} is {err:.3e} from the sum, bound {bound:.3e}")
    finally:
        pop.close()
    assert not failures, f"{oa.key_name(key)} {np.dtype(dtype).name} {path}: " + "; ".join(failures)


# ---- f. the report --------------------------------------------------------------------------------------------------------------------
def test_zz_write_loss_grad_report():
    """Runs last in this module: the per-operator figures of the fused loss gradient of DESIGN.md §5."""
    assert len(REPORT) >= len(PARTIAL_CASES)
    import torch
    out_dir = os.environ.get("DE_ULP_REPORT_DIR") or os.path.join(ROOT, "build", "reports")   # (build/ is kept out of git)
    os.makedirs(out_dir, exist_ok=True)
    per_path = {}
    for name, m in REPORT.items():
        p = name.split(" ")[3]
        if p not in per_path or m["worst_E_over_B"] > per_path[p][1]["worst_E_over_B"]:
            per_path[p] = (name, m)
    with open(os.path.join(out_dir, "loss_grad_accuracy.json"), "w") as fh:
        json.dump(dict(what="de_eval_loss_grad, loss = pullback, dY = 1, N = 1, one tree per point: per operator, partial, dtype, kernel path, form and "
                            "region, the kept share, max E = |got - true| / (eps |true|), max B(x; s_device), the worst E / (1.01 B + 2^-9) and where "
                            "(tests/test_gpu_loss_grad_accuracy.py)",
                       device=torch.cuda.get_device_name(0), hip=str(torch.version.hip), worst_per_path={p: dict(where=n, **m) for p, (n, m) in per_path.items()},
                       partials=REPORT), fh, indent=1, sort_keys=True)
    for p, (n, m) in sorted(per_path.items()):
        print(f"[loss grad accuracy] {p}: worst E / B {m['worst_E_over_B']:.3f}: {n} at {m['at']}")
