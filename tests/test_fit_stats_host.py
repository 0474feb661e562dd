"""CPU tests of the fit statistics (include/de_hip.h de_eval_fit_stats): the quantities `FitStats` derives on the host against numpy's
closed forms over the samples themselves, the rule for trees without variance, the validation that needs no device, the ctypes
prototype against the header, and the internal loss kind staying out of reach of a de_loss_spec_t."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def api():
    from dynamicexpressions_jl_amd import api as _api
    _api.library()
    return _api


def moments(p, y, w):
    W = w.sum()
    mp, my = (w * p).sum() / W, (w * y).sum() / W
    return mp, (w * (p - mp) ** 2).sum(), (w * (p - mp) * (y - my)).sum(), W, my, (w * (y - my) ** 2).sum()


def test_derived_quantities_match_closed_forms(api):
    g = np.random.Generator(np.random.PCG64(3))
    N, n = 500, 6
    y = 2.0 + g.standard_normal(N)
    w = g.uniform(0.5, 2.0, N)
    P = np.stack([y * s + g.standard_normal(N) * 0.3 + o for s, o in ((1, 0), (-2, 5), (0.1, -3), (0, 1), (3, 3), (-1, 0))])
    rows = [moments(p, y, w) for p in P]
    fs = api.FitStats([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], rows[0][3], rows[0][4], rows[0][5])
    assert len(fs) == n
    sw = np.sqrt(w)
    for t, p in enumerate(P):
        # weighted least squares y ~ a + b p, solved directly
        A = np.stack([np.ones(N), p], axis=1) * sw[:, None]
        (a, b), res = np.linalg.lstsq(A, y * sw, rcond=None)[:2]
        assert abs(fs.slope[t] - b) <= 1e-11 * max(1, abs(b)) and abs(fs.intercept[t] - a) <= 1e-11 * max(1, abs(a))
        assert abs(fs.scaled_sse[t] - res[0]) <= 1e-10 * fs.m2_y
        assert abs(fs.sse[t] - (w * (p - y) ** 2).sum()) <= 1e-11 * (w * (p - y) ** 2).sum()
        r = np.cov(p, y, aweights=w)[0, 1] / np.sqrt(np.cov(p, p, aweights=w)[0, 1] * np.cov(y, y, aweights=w)[0, 1])
        assert abs(fs.pearson_r[t] - r) <= 1e-12
        assert abs(fs.r2[t] - (1 - (w * (p - y) ** 2).sum() / fs.m2_y)) <= 1e-11 * max(1, abs(fs.r2[t]))
        assert abs((1 - fs.scaled_sse[t] / fs.m2_y) - r * r) <= 1e-12  # the R^2 of the scaled fit is r^2


def test_trees_without_variance_and_incomplete_trees(api):
    nan = float("nan")
    fs = api.FitStats([1.5, nan, 0.25], [0.0, nan, 4.0], [0.0, nan, -2.0], 10.0, 3.0, 8.0)
    assert np.isnan(fs.pearson_r[0]) and fs.slope[0] == 0.0 and fs.intercept[0] == 3.0 and fs.scaled_sse[0] == 8.0
    assert fs.sse[0] == 8.0 + 10.0 * 1.5 ** 2
    for v in (fs.pearson_r, fs.slope, fs.intercept, fs.scaled_sse, fs.sse, fs.r2):  # an incomplete tree stays NaN everywhere
        assert np.isnan(v[1])
    assert fs.slope[2] == -0.5 and fs.intercept[2] == 3.0 + 0.5 * 0.25 and fs.scaled_sse[2] == 8.0 - 1.0
    assert abs(fs.pearson_r[2] - (-2.0 / np.sqrt(32.0))) < 1e-15
    # W == 0 (no sample counts): the means are NaN, the sums 0
    z = api.FitStats([nan], [0.0], [0.0], 0.0, nan, 0.0)
    assert np.isnan(z.pearson_r[0]) and z.slope[0] == 0.0 and np.isnan(z.intercept[0]) and z.scaled_sse[0] == 0.0


def test_argument_validation_needs_no_device(api):
    with pytest.raises(ValueError):
        api.FitStats([1.0, 2.0], [1.0], [1.0, 2.0], 1.0, 0.0, 1.0)
    with pytest.raises(ValueError):
        api.FitStats([[1.0]], [[1.0]], [[1.0]], 1.0, 0.0, 1.0)
    with pytest.raises((TypeError, ValueError)):
        api.FitStats([1.0], [1.0], [1.0], "many", 0.0, 1.0)
    # the internal kind of a fit-statistics launch is no loss kind: de_loss_spec_check refuses it with and without a gradient
    lib = api.library()
    for with_gradient in (0, 1):
        assert lib.de_loss_spec_check(C.byref(api.LossSpec(25, 0, 0.0)), with_gradient) == 1
    assert 25 not in api.LOSS_KINDS.values()
    # null handles are refused before anything else is looked at
    assert lib.de_eval_fit_stats(None, None, None, 0, 0, None, None, None, None, None, None) == 1


def test_ctypes_prototype_matches_the_header(api):
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "de_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+de_eval_fit_stats\s*\(([^;]*?)\)\s*;", src)
    assert m, "include/de_hip.h declares de_eval_fit_stats"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["ctx", "prog", "X", "N", "ldX", "pargs", "y", "w", "stats", "ystats", "ok"]
    want = []
    for p in params:
        if "*" in p:
            want.append(C.POINTER(api.ParamArgs) if "de_param_args_t" in p else C.c_void_p)
        else:
            assert p.split()[0] == "int64_t", p
            want.append(C.c_int64)
    fn = api.library().de_eval_fit_stats
    assert list(fn.argtypes) == want and fn.restype is C.c_int
    assert "double *stats" in m.group(1) and "double *ystats" in m.group(1) and "uint8_t *ok" in m.group(1)
    assert "de_eval_fit_stats" in api.EXPORTS and api.ABI_VERSION == 3 and re.search(r"#define\s+DE_HIP_ABI_VERSION\s+3\b", src)
