"""CPU tests of the parameterised loss kinds (include/de_hip.h de_loss_kind_t values >= 16): the float64 reference the GPU tests compare
against (tests/loss_reference.py) is checked against itself — l' against central differences of l, l'' against those of l', the stable
forms against the naive formulas —, de_loss_spec_check accepts every kind with a good parameter and refuses every bad one, and the
Python name table carries the header's enum values."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from loss_reference import KINDS, MARGIN, PARAMS, kink_samples, loss_terms, naive_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    _api.library()
    return _api


def _samples(kind, n=4000, seed=5):
    g = np.random.Generator(np.random.PCG64(seed))
    yhat = 3.0 * g.standard_normal(n)
    y = g.standard_normal(n)
    if kind in MARGIN:
        y = np.where(y > 0, 1.0, -1.0) * (1.0 + 0.5 * g.random(n))
    return yhat, y


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_reference_derivatives_match_central_differences(kind):
    p = PARAMS[kind]
    yhat, y = _samples(kind)
    h = 1e-6
    l, lp, lpp = loss_terms(kind, yhat, y, p)
    assert np.all(l >= 0) and np.all(np.isfinite(l)) and np.all(np.isfinite(lp)) and np.all(np.isfinite(lpp))
    # away from the points where l' jumps or bends: |e| = delta / eps, e = 0, a = 1
    e, a = yhat - y, y * yhat
    away = np.ones(len(e), dtype=bool)
    if kind in ("huber", "l1_eps", "l2_eps"):
        away = np.abs(np.abs(e) - p) > 1e-3
    if kind in ("quantile", "lp", "l1_eps"):
        away &= np.abs(e) > 1e-3
    if kind == "l1_hinge":
        away = np.abs(a - 1.0) > 1e-3 * np.abs(y)
    assert away.mean() > 0.99
    lh, lph, _ = loss_terms(kind, yhat + h, y, p)
    ll, lpl, _ = loss_terms(kind, yhat - h, y, p)
    d1, d2 = (lh - ll) / (2 * h), (lph - lpl) / (2 * h)
    assert np.allclose(d1[away], lp[away], rtol=1e-6, atol=1e-8)
    assert np.allclose(d2[away], lpp[away], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("kind", ["logcosh", "logit_dist", "logit_margin"])
def test_stable_forms_equal_the_naive_formulas_where_those_work(kind):
    yhat, y = _samples(kind, seed=6)
    yhat = np.concatenate([yhat, 40.0 * yhat])  # |e| up to ~ 500: cosh and exp still finite in float64
    y = np.concatenate([y, y])
    l = loss_terms(kind, yhat, y)[0]
    naive = naive_loss(kind, yhat, y)
    ok = np.isfinite(naive) & (np.abs(yhat - y) > 1e-3 if kind != "logit_margin" else np.ones(len(y), dtype=bool))  # (the naive forms cancel near 0)
    assert ok.mean() > 0.9
    assert np.all(np.abs(l[ok] - naive[ok]) <= 2e-15 * np.maximum(1.0, np.abs(naive[ok])) + 1e-9 * (np.abs(naive[ok]) < 1e-6))
    # and where the naive ones fail: no overflow far out, no cancellation close to 0
    assert abs(float(loss_terms("logcosh", 1e4, 0.0)[0]) - (1e4 - np.log(2.0))) < 1e-9
    assert abs(float(loss_terms("logcosh", 1e-5, 0.0)[0]) - 0.5e-10) < 1e-20
    assert float(loss_terms("logit_margin", -1e4, 1.0)[0]) == 1e4
    assert abs(float(np.float32(1e4 - np.log(2.0))) - 9999.3069) < 1e-3


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_few_samples_sit_on_a_kink_with_the_parameters_of_the_gpu_tests(kind):
    """The GPU gradient tests let a sample within 4 eps max(|yhat|, |y|) of a jump of l' take either side and cap such samples at
    1 %: with continuous random targets and these parameters the float64 reference alone stays far below the cap."""
    yhat, y = _samples(kind, n=20000, seed=7)
    near, jump = kink_samples(kind, yhat, y, PARAMS[kind], float(np.finfo(np.float32).eps))
    assert near.mean() < 0.01 and np.all(jump >= 0)
    near1, jump1 = kink_samples("lp", yhat, y, 1.0, float(np.finfo(np.float32).eps))
    assert near1.mean() < 0.01 and np.all(jump1 == 2.0)


def test_python_names_carry_the_enum_values_of_the_header(api):
    src = open(os.path.join(ROOT, "include", "de_hip.h")).read()
    enum = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"\bDE_LOSS_(\w+)\s*=\s*(\d+)", src))
    assert enum["L2"] == 0 and enum["L1"] == 1 and enum["PULLBACK"] == 2 and len(enum) == 12
    assert {k.upper(): v for k, v in api.LOSS_KINDS.items()} == enum
    assert {k: api.LOSS_KINDS[k] for k in KINDS} == KINDS
    assert "huber" in api.LOSS_KINDS and set(("de_loss_spec_check", "de_eval_loss_ex", "de_eval_loss_grad_ex",
                                              "de_eval_loss_grad_by_class_ex")) <= set(api.EXPORTS)
    assert C.sizeof(api.LossSpec) == 16 and api.LossSpec.param.offset == 8
    assert api.ABI_VERSION == 3


def test_spec_check_accepts_good_and_refuses_bad_parameters(api):
    lib = api.library()

    def check(kind, param, with_gradient=1):
        spec = api.LossSpec(kind, 0, param)
        return lib.de_loss_spec_check(C.byref(spec), with_gradient)

    for name, kind in KINDS.items():
        for wg in (0, 1):
            assert check(kind, PARAMS[name], wg) == 0, name
    for kind in (0, 1):
        assert check(kind, 0.0, 0) == 0 and check(kind, float("nan"), 1) == 0  # (no parameter: ignored)
    assert check(2, 0.0, 1) == 0 and check(2, 0.0, 0) == 1  # DE_LOSS_PULLBACK belongs to the gradient entry points
    for name in ("logcosh", "logit_dist", "logit_margin", "l1_hinge"):
        assert check(KINDS[name], -5.0) == 0  # ignored as well
    bad = [("huber", 0.0), ("huber", -1.0), ("l1_eps", -1e-9), ("l2_eps", -0.5), ("quantile", -0.01), ("quantile", 1.01), ("lp", 0.99),
           ("lp", 0.0)]
    for name in ("huber", "l1_eps", "l2_eps", "quantile", "lp"):
        bad += [(name, float("nan")), (name, float("inf")), (name, -float("inf"))]
    for name, v in bad:
        for wg in (0, 1):
            assert check(KINDS[name], v, wg) == 1, (name, v)
    # the ends of the closed ranges are good
    assert check(KINDS["l1_eps"], 0.0) == 0 and check(KINDS["quantile"], 0.0) == 0 and check(KINDS["quantile"], 1.0) == 0 and check(KINDS["lp"], 1.0) == 0
    for kind in (3, 7, 15, 25, 31, 32, -1, 1 << 20):
        assert check(kind, 1.0) == 1, kind
    assert lib.de_loss_spec_check(None, 1) == 1
    for kind in (0, KINDS["huber"]):  # `reserved` must be 0 (the header says so: the field can be given a meaning later)
        bad_reserved = api.LossSpec(kind, 1, 1.3)
        assert lib.de_loss_spec_check(C.byref(bad_reserved), 1) == 1
    # the Python layer: KeyError for a name it does not know, ValueError for a parameter the library refuses
    with pytest.raises(KeyError):
        api.loss_spec("hubert", 1.0)
    with pytest.raises(KeyError):
        api.loss_spec("pullback", 0.0, with_gradient=False)
    with pytest.raises(ValueError):
        api.loss_spec("huber", 0.0)
    with pytest.raises(ValueError):
        api.loss_spec("quantile", float("nan"))
    assert api.loss_spec("lp", 1.5).kind == 21 and api.loss_spec("pullback").kind == 2
