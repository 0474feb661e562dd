"""CPU tests of the generalised Gauss-Newton fit (include/de_hip.h de_gn_spec_check / de_eval_loss_gn_ex / de_fit_consts_lm_ex, DESIGN.md
§4.4.5): which specs and residual floors the host-only check admits, the float64 reference of the curvature weights
(tests/gn_kinds_reference.py) against l' and l'' of tests/loss_reference.py, the Python keywords, and the numpy model of the loop on a
line with 10 % gross outliers."""
import ctypes as C
import inspect

import numpy as np
import pytest

import gn_kinds_reference as gk
import loss_reference as lr
from dynamicexpressions_jl_amd import api

OK, INVALID, UNSUPPORTED = 0, 1, 7
GOOD_PARAM = {"L2": 0.0, "L1": 0.0, "huber": 1.3, "logcosh": 0.0, "l1_eps": 0.4, "l2_eps": 0.4, "quantile": 0.3, "lp": 1.5,
              "logit_dist": 0.0, "logit_margin": 0.0}
BAD_FLOORS = (0.0, -1.0, float("nan"), float("inf"), -float("inf"))


def check(kind, param=0.0, floor=1e-4, reserved=0):
    spec = api.LossSpec(kind, reserved, float(param))
    return api.library().de_gn_spec_check(C.byref(spec), float(floor))


def test_every_kind_is_admitted_or_refused_as_documented():
    assert set(gk.KINDS) | {"pullback", "l1_hinge"} == set(api.LOSS_KINDS)
    for name, kind in api.LOSS_KINDS.items():
        want = UNSUPPORTED if name == "l1_hinge" else INVALID if name == "pullback" else OK
        assert check(kind, GOOD_PARAM.get(name, 0.0)) == want, name
    assert api.library().de_gn_spec_check(None, 1e-4) == INVALID  # a null spec
    for kind in (-1, 3, 15, 25, 99):
        assert check(kind) == INVALID
    assert check(api.LOSS_KINDS["huber"], 1.3, reserved=1) == INVALID


@pytest.mark.parametrize("name,bad", [("huber", 0.0), ("huber", -1.0), ("huber", float("nan")), ("huber", float("inf")), ("l1_eps", -0.1),
                                      ("l2_eps", -0.1), ("quantile", 1.5), ("quantile", -0.1), ("lp", 0.5), ("lp", float("inf"))])
def test_a_bad_parameter_is_refused(name, bad):
    assert check(api.LOSS_KINDS[name], bad) == INVALID


@pytest.mark.parametrize("name", sorted(gk.KINDS))
def test_the_floor_is_checked_for_the_kinds_that_read_it(name):
    kind, p = api.LOSS_KINDS[name], GOOD_PARAM[name]
    reads = gk.reads_floor(name, p)
    assert reads == (name in ("L1", "l1_eps", "quantile", "lp"))
    for f in BAD_FLOORS:
        assert check(kind, p, f) == (INVALID if reads else OK), (name, f)
    for f in (1e-4, 1.0, 1e-300):
        assert check(kind, p, f) == OK, (name, f)
    # 1e-60 is a good floor in Float64 and rounds to 0 in Float32: this check knows no element type and admits it; the entry points refuse
    # it for a DE_F32 program (tests/test_gpu_gn_kinds.py)
    assert np.float32(1e-60) == 0 and check(kind, p, 1e-60) == OK


def test_lp_reads_the_floor_below_two_only():
    lp = api.LOSS_KINDS["lp"]
    for p, reads in ((1.0, True), (1.5, True), (np.nextafter(2.0, 0.0), True), (2.0, False), (3.0, False)):
        assert check(lp, p, 0.0) == (INVALID if reads else OK), p
        assert check(lp, p, 1e-4) == OK


def residuals():
    g = np.random.default_rng(3)
    e = np.concatenate([g.standard_normal(400) * 3, g.standard_normal(200) * 1e-3, [1.3, -1.3, 0.4, -0.4, 5e-4, -5e-4, 30.0, -30.0, 400.0]])
    y = g.standard_normal(e.size)
    return e + y - y, y  # (e as yhat - y reproduces it: the reference forms it the same way)


DISTANCE = [(n, GOOD_PARAM[n]) for n in sorted(set(gk.KINDS) - {"logit_margin", "lp"})] + [("lp", 1.0), ("lp", 1.5), ("lp", 2.0), ("lp", 3.0)]


@pytest.mark.parametrize("name,p", DISTANCE, ids=[f"{n}-{p}" for n, p in DISTANCE])
def test_twice_c_e_is_the_derivative_of_the_loss(name, p):
    f, tau = 1e-4, 2.0 ** -27
    e, y = residuals()
    yhat = y + e
    e = yhat - y
    c = gk.curvature(name, e, y, yhat, p, f, tau)
    assert np.isfinite(c).all() and (c >= 0).all()
    lp = gk.loss_terms(name, yhat, y, p)[1]
    sel = (np.abs(e) >= f) & (np.abs(e) >= tau)
    assert sel.sum() > 500
    assert (np.abs(2.0 * c * e - lp)[sel] <= 1e-12 * np.abs(lp[sel])).all()
    if name == "L2" or (name == "lp" and p == 2.0):
        assert (c == 1.0).all()
    if gk.reads_floor(name, p):  # below the floor the weight is the floor's: it stays bounded
        at_floor = gk.curvature(name, np.array([f, -f]), 0.0, 0.0, p, f, tau).max()
        assert c[np.abs(e) < f].size == 0 or c[np.abs(e) < f].max() <= at_floor


def test_twice_c_is_the_second_derivative_of_the_logistic_margin():
    g = np.random.default_rng(4)
    y = np.where(g.random(500) < 0.5, -1.0, 1.0) * np.concatenate([np.ones(400), g.uniform(0.5, 2, 100)])
    yhat = np.concatenate([g.standard_normal(480) * 4, [0.0, 1e-9, 40.0, -40.0, 800.0, -800.0], g.standard_normal(14)])
    c = gk.curvature("logit_margin", yhat - y, y, yhat)
    lpp = lr.loss_terms("logit_margin", yhat, y)[2]
    assert np.isfinite(c).all() and (c >= 0).all()
    assert (np.abs(2.0 * c - lpp) <= 1e-12 * lpp).all()


def test_the_python_keywords_exist_and_refuse_unknown_kinds():
    for fn in (api.Population.eval_gauss_newton, api.Population.fit_constants_lm, api.Population.fit_constants_lm_device):
        prm = inspect.signature(fn).parameters
        assert (prm["loss"].default, prm["loss_param"].default, prm["e_floor"].default) == ("L2", 0.0, 1e-4), fn.__name__
    for fn in (api.GaussNewton.lm_step, api.GaussNewton.lm_step_device):  # unchanged
        assert "loss" not in inspect.signature(fn).parameters
    assert api.gn_loss_spec("huber", 1.3).kind == 16 and api.gn_loss_spec("L2", 0.0, 0.0).kind == 0
    with pytest.raises(KeyError):
        api.gn_loss_spec("no_such_loss")
    for bad in (("l1_hinge", 0.0, 1e-4), ("pullback", 0.0, 1e-4), ("huber", -1.0, 1e-4), ("L1", 0.0, 0.0), ("quantile", 0.5, float("nan"))):
        with pytest.raises(ValueError):
            api.gn_loss_spec(*bad)
    for name in ("de_gn_spec_check", "de_eval_loss_gn_ex", "de_fit_consts_lm_ex"):
        assert name in api.EXPORTS and hasattr(api.library(), name)
    assert api.library().de_abi_version() == 3


# (c0, c1) the float64 loop reaches from (0.5, -0.5) in 20 iterations with the default options; the line is y = 2 x + 1
FITS = {"huber": (1.3, 1.987, 1.146), "logcosh": (0.0, 1.990, 1.112), "logit_dist": (0.0, 1.980, 1.225), "L1": (0.0, 2.0001, 1.0002),
        "quantile": (0.5, 2.0001, 1.0002), "L2": (0.0, 1.839, 3.02)}


@pytest.mark.parametrize("name", sorted(FITS))
def test_the_numpy_loop_recovers_the_line_under_the_robust_kinds(name):
    p, c0, c1 = FITS[name]
    x, y = gk.outlier_line()
    c, hist = gk.lm_fit(gk.line_model(x), [0.5, -0.5], y, name, p, iters=20)
    assert (np.diff(hist) <= 0).all() and hist[-1] < hist[0]
    assert abs(c[0] - c0) < 5e-3 and abs(c[1] - c1) < 5e-3, c  # (the figures above are rounded)
    if name == "L2":
        assert c[1] > 2.5  # squared error follows the outliers
    else:
        assert abs(c[0] - 2) < 0.05 and abs(c[1] - 1) < 0.3
