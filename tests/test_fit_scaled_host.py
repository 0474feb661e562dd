"""CPU tests of the objective of the matrix-free fits under linear scaling (include/de_hip.h de_scaled_objective_host, DESIGN.md
§4.4.14): the host-only hook runs csrc/de_fit_scaled.h, the code de_fit_scaled_objective_kernel runs behind every evaluation of
de_fit_consts_bfgs_scaled / de_fit_consts_nm_scaled.

The header states two formulas in one association, in float64 and without contraction:
    sse = m2_y - (cov * cov) / m2_p,      g_k = (2 * b) * (b * P_k - Q_k)   with   b = cov / m2_p.
Every operation is one IEEE-754 double operation on both sides, so the hook equals numpy's float64 evaluation BIT FOR BIT — no tolerance —
and, for G <= 8, the `sse` and `g` of de_lm_project_host, which writes the same formulas out."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dynamicexpressions_jl_amd import api
import test_fit_stats_grad_host as FSG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QNAN = np.array([np.nan]).tobytes()  # the quiet NaN 0x7ff8000000000000


def numpy_objective(st, ys, P, Q):
    """The two formulas in the stated association, one float64 operation at a time."""
    m2p, cov, m2y = np.float64(st[1]), np.float64(st[2]), np.float64(ys[2])
    sse = m2y - (cov * cov) / m2p
    b = cov / m2p
    tb = np.float64(2.0) * b
    return sse, tb * (b * np.asarray(P, dtype=np.float64) - np.asarray(Q, dtype=np.float64))


def draw(g, G):
    st = [g.standard_normal(), np.exp(g.uniform(-6.0, 6.0)), g.standard_normal() * np.exp(g.uniform(-3.0, 3.0))]
    ys = [np.exp(g.uniform(0.0, 6.0)), g.standard_normal(), np.exp(g.uniform(-6.0, 6.0))]
    D, P, Q = (g.standard_normal(G) * np.exp(g.uniform(-3.0, 3.0, G)) for _ in range(3))
    return st, ys, D, P, Q


@pytest.mark.parametrize("seed", range(3))
def test_bit_equal_to_numpy_on_random_statistics(seed):
    g = np.random.default_rng(seed)
    n = 0
    for G in list(range(1, 33)) * 3:
        st, ys, D, P, Q = draw(g, G)
        sse, grad, formed = api.scaled_objective_host(st, ys, D, P, Q)
        want_sse, want_g = numpy_objective(st, ys, P, Q)
        assert formed and grad.shape == (G,)
        assert np.float64(sse).tobytes() == np.float64(want_sse).tobytes(), (G, st, ys)
        assert grad.tobytes() == want_g.tobytes(), (G, st, ys)
        # ... which is what the Python classes compute
        fs = api.FitStats([st[0]], [st[1]], [st[2]], *ys)
        fg = api.FitStatsGrad(fs, [D], [P], [Q], [np.full((G, G), np.nan)], np.ones(1, dtype=bool))
        assert np.float64(fs.scaled_sse[0]).tobytes() == np.float64(sse).tobytes() and fg.scaled_sse_grad()[0].tobytes() == grad.tobytes()
        # D is not read
        assert api.scaled_objective_host(st, ys, D * np.nan, P, Q)[1].tobytes() == grad.tobytes()
        n += 1
    assert n == 96


@pytest.mark.parametrize("seed", range(2))
def test_agrees_with_lm_project_host_up_to_8_rows(seed):
    g = np.random.default_rng(100 + seed)
    for G in list(range(1, 9)) * 4:
        st, ys, D, P, Q = draw(g, G)
        A = g.standard_normal((G, G))
        sse_p, g_p, _, formed_p = api.lm_project_host(st, ys, D, P, Q, A @ A.T)
        sse, grad, formed = api.scaled_objective_host(st, ys, D, P, Q)
        assert formed and formed_p
        assert np.float64(sse).tobytes() == np.float64(sse_p).tobytes() and grad.tobytes() == g_p.tobytes(), G
    # ... and where nothing is formed
    D, P, Q = np.array([1.0, 2.0]), np.array([0.5, 0.2]), np.array([0.3, 0.1])
    for st, ys in (([3.0, 0.0, 0.5], [10.0, 0.5, 4.0]), ([3.0, 2.0, 0.5], [0.0, 0.5, 4.0]), ([3.0, 0.0, np.nan], [10.0, 0.5, 4.0])):
        sse_p, g_p, _, formed_p = api.lm_project_host(st, ys, D, P, Q, np.eye(2))
        sse, grad, formed = api.scaled_objective_host(st, ys, D, P, Q)
        assert not formed and not formed_p and grad.tobytes() == g_p.tobytes() == np.zeros(2).tobytes()
        assert np.float64(sse).tobytes() == np.float64(sse_p).tobytes()


def test_edge_cases():
    nan = np.nan
    D, P, Q = np.array([1.0, 2.0]), np.array([0.5, 0.2]), np.array([0.3, 0.1])
    ys = [10.0, 0.5, 4.0]
    # M2_p == 0 (a tree constant over the samples): sse = M2_y, g = 0, not formed
    sse, g, formed = api.scaled_objective_host([3.0, 0.0, 0.0], ys, D, P, Q)
    assert sse == 4.0 and g.tolist() == [0.0, 0.0] and not formed
    sse, g, formed = api.scaled_objective_host([3.0, -0.0, 0.7], ys, D, P, Q)
    assert sse == 4.0 and g.tolist() == [0.0, 0.0] and not formed
    # W == 0 (no sample counts): the same, whatever the other statistics hold
    sse, g, formed = api.scaled_objective_host([nan, 2.0, 1.0], [0.0, nan, 4.0], D, P, Q)
    assert sse == 4.0 and g.tolist() == [0.0, 0.0] and not formed
    sse, g, formed = api.scaled_objective_host([nan, 0.0, 0.0], [0.0, nan, 0.0], D, P, Q)  # (what N == 0 gives)
    assert sse == 0.0 and g.tolist() == [0.0, 0.0] and not formed
    # a NaN C: sse is THE quiet NaN, formed or not
    for m2p in (0.0, 2.0):
        for c in (nan, -nan, np.frombuffer(np.uint64(0x7ff8000000000123).tobytes(), dtype=np.float64)[0],
                  np.frombuffer(np.uint64(0xfff0000000000001).tobytes(), dtype=np.float64)[0]):
            sse, g, formed = api.scaled_objective_host([0.1, m2p, c], ys, D, P, Q)
            assert np.float64(sse).tobytes() == QNAN and formed == (m2p != 0.0)
            assert (np.isnan(g).all() if formed else g.tolist() == [0.0, 0.0])
    # NaN statistics (an incomplete tree) propagate
    sse, g, formed = api.scaled_objective_host([nan, nan, nan], ys, D * nan, P * nan, Q * nan)
    assert np.float64(sse).tobytes() == QNAN and np.isnan(g).all() and formed
    sse, g, formed = api.scaled_objective_host([0.1, 2.0, 1.0], ys, D, [nan, 0.2], Q)
    assert sse == 3.5 and np.isnan(g[0]) and g[1] == (2.0 * 0.5) * (0.5 * 0.2 - 0.1) and formed
    # an infinite slope: what the formulas give
    with np.errstate(all="ignore"):
        want_sse, want_g = numpy_objective([0.1, 1e-320, 1e300], ys, P, Q)
    sse, g, formed = api.scaled_objective_host([0.1, 1e-320, 1e300], ys, D, P, Q)
    assert formed and np.float64(sse).tobytes() == np.float64(want_sse).tobytes() and g.tobytes() == want_g.tobytes()
    # G = 0: the objective alone; G = 1 and G = 32: formed; G = 33 (beyond de_bfgs_max_rows()): not formed, g zero-filled
    lib = api.library()
    assert lib.de_bfgs_max_rows() == 32 == api.BFGS_MAX_ROWS
    st3, ys3, one, sse1 = np.array([0.1, 2.0, 1.0]), np.array(ys), np.full(1, 7.0), np.full(1, 7.0)
    assert lib.de_scaled_objective_host(0, st3.ctypes.data, ys3.ctypes.data, one.ctypes.data, sse1.ctypes.data, one.ctypes.data) == 0
    assert one[0] == 7.0 and sse1[0] == 3.5
    sse, g, formed = api.scaled_objective_host(st3, ys, np.zeros(0), np.zeros(0), np.zeros(0))
    assert sse == 3.5 and g.size == 0 and not formed
    sse, g, formed = api.scaled_objective_host(st3, ys, [1.0], [0.5], [0.3])
    assert formed and g.tolist() == [(2.0 * 0.5) * (0.5 * 0.5 - 0.3)]
    rows = np.arange(1.0, 33.0)
    sse, g, formed = api.scaled_objective_host(st3, ys, rows, rows / 8, rows / 32)
    assert formed and g.tobytes() == numpy_objective(st3, ys, rows / 8, rows / 32)[1].tobytes() and g.all()
    rows = np.arange(1.0, 34.0)
    sse, g, formed = api.scaled_objective_host(st3, ys, rows, rows / 8, rows / 32)
    assert not formed and g.shape == (33,) and not g.any() and sse == 3.5
    # null pointers and a negative G: nothing is written, nothing is formed
    assert lib.de_scaled_objective_host(2, None, None, None, None, None) == 0
    g2 = np.full(2, 7.0)
    assert lib.de_scaled_objective_host(-1, st3.ctypes.data, ys3.ctypes.data, one.ctypes.data, None, g2.ctypes.data) == 0 and (g2 == 7.0).all()
    assert lib.de_scaled_objective_host(2, st3.ctypes.data, ys3.ctypes.data, None, None, g2.ctypes.data) == 0 and not g2.any()
    with pytest.raises(ValueError):
        api.scaled_objective_host([0.1, 2.0], ys, D, P, Q)
    with pytest.raises(ValueError):
        api.scaled_objective_host(st3, ys, D, P[:1], Q)


def test_prototypes_and_null_contexts():
    text = open(os.path.join(ROOT, "include", "de_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    lib = api.library()
    for name, n_args in (("de_scaled_objective_host", 6), ("de_fit_consts_bfgs_scaled", 15), ("de_fit_consts_nm_scaled", 15)):
        m = re.search(r"^int %s\(([^;]*)\);" % name, src, re.M)
        assert m, f"include/de_hip.h declares {name}"
        assert len(m.group(1).split(",")) == n_args == len(getattr(lib, name).argtypes)
        assert name in api.EXPORTS
    assert api.ABI_VERSION == 3 == lib.de_abi_version() and re.search(r"\(r\) de_fit_consts_bfgs_scaled", text)
    # the refusals that need no device: a null context or program
    none15 = (None, None, None, 0, 0, None, None, None, None, None, None, None, None, None, None)
    assert lib.de_fit_consts_bfgs_scaled(*none15) == 1 and lib.de_fit_consts_nm_scaled(*none15) == 1
    # the existing entry points keep their prototypes
    assert len(lib.de_fit_consts_bfgs.argtypes) == 14 == len(lib.de_fit_consts_nm.argtypes)


def test_scaled_fits_take_l2_only_before_anything_is_touched():
    class Touched(Exception):
        pass

    class Dummy:  # any attribute access would mean the population was looked at before the refusal
        def __getattr__(self, name):
            raise Touched(name)

    P = api.Population
    for fit in (P.fit_constants_bfgs, P.fit_constants_bfgs_device, P.fit_constants_nm, P.fit_constants_nm_device):
        for kw in (dict(loss="huber", loss_param=1.0), dict(loss="L1"), dict(loss="l1_hinge"), dict(loss="pullback"), dict(loss="nonsense")):
            with pytest.raises(ValueError, match=r"scaled=True"):
                fit(Dummy(), None, None, np.zeros(2), scaled=True, **kw)
        with pytest.raises(Touched):  # L2 goes on ...
            fit(Dummy(), None, None, np.zeros(2), scaled=True)
        with pytest.raises(Touched):  # ... and so does every kind without the keyword
            fit(Dummy(), None, None, np.zeros(2), loss="huber", loss_param=1.0)
    # scaled_fit_stats before any scaled fit
    class Bare:
        n_trees = 1
    with pytest.raises(AttributeError, match="scaled_fit_stats"):
        P.scaled_fit_stats.fget(Bare())


def test_host_nm_loop_keeps_a_double_objective():
    """api.nm_fit(loss_dtype=float64) — the loop behind fit_constants_nm(scaled=True) — keeps the objective's double where the default
    rounds it to the element type: on a float32 tree an objective that differs below float32's resolution is still ordered."""
    target = np.float32(0.3)

    def make(calls):
        def evaluate(consts):
            calls.append(np.array(consts, copy=True))
            d = np.float64(consts[0]) - np.float64(target)
            return np.array([1.0 + 1e-12 * d * d]), np.array([True])
        return evaluate

    for ldt, moves in ((None, False), (np.float64, True)):
        hist = []
        consts, lo, ok, imp = api.nm_fit(make([]), lambda c: None, np.array([1.0], dtype=np.float32), [1], np.float32, iters=12, history=hist,
                                         loss_dtype=ldt)
        assert lo.dtype == (np.float64 if moves else np.float32) and consts.dtype == np.float32 and ok.all() and len(hist) == 13
        assert (imp[0] > 0) == moves and (consts[0] != np.float32(1.0)) == moves
        assert all(b[0] <= a[0] for a, b in zip(hist, hist[1:]))


# ---- the host loops over a numpy model of one tree: what chose the data and starts of tests/test_gpu_fit_scaled.py --------------------------------
class Model:
    """One tree on numpy standing in for a Population in `fit_constants_bfgs(scaled=True)` / `fit_constants_nm(scaled=True)`: the loops
    are the library's, the evaluation is `f(c, x) -> (values, Jacobian)` with the values rounded through the element type."""

    def __init__(self, f, x, dtype):
        self.f, self.x, self.dtype = f, x, np.dtype(dtype)
        self.n_trees, self.n_consts, self.c = 1, np.array([3]), None

    def _refuse_f16(self, what):
        pass

    def set_constants(self, c):
        self.c = np.array(c, dtype=self.dtype).copy()

    def eval_fit_stats_grad(self, X, y, weights=None, **kw):
        yh, J = self.f(self.c.astype(np.float64), self.x)
        return FSG.moments(yh.astype(self.dtype).astype(np.float64), J, y, weights)

    def eval_fit_stats(self, X, y, weights=None, **kw):
        return self.eval_fit_stats_grad(X, y, weights).stats, np.ones(1, dtype=bool)


def redundant(c, x):  # c0 + c1 cos(c2 x): c0 and c1 are redundant under scaling
    v = np.cos(c[2] * x)
    return c[0] + c[1] * v, np.stack([np.ones_like(x), v, -c[1] * x * np.sin(c[2] * x)])


def rounded(c, x):  # c0 round(c1 x) + c2 x: the row of c1 is zero
    r = np.rint(c[1] * x)
    return c[0] * r + c[2] * x, np.stack([r, 0.0 * x, x])


def model_data(N=1025):
    g = np.random.Generator(np.random.PCG64(404))
    x = g.uniform(-2.0, 2.0, N)
    return x, g.choice(np.array([0.0, 0.5, 1.0, 2.0]), N)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_loops_on_a_model_fit_what_the_scaled_lm_step_cannot(dtype):
    x, w = model_data()
    P = api.Population
    # constants that are redundant under scaling: both loops lower scaled_sse, BFGS to rounding
    y = (2.5 * np.cos(1.3 * x) - 0.7).astype(dtype).astype(np.float64)
    start = [0.5, 1.0, 1.0]
    hb, hn = [], []
    m = Model(redundant, x, dtype)
    cb, lb, okb = P.fit_constants_bfgs(m, None, y, start, weights=w, iters=12, history=hb, scaled=True)
    assert lb.dtype == np.float64 and cb.dtype == dtype and okb[0] and m.bfgs_accepts[0] > 0 and m.c.tobytes() == cb.tobytes()
    assert lb[0] < 1e-6 * hb[0][0] and abs(float(cb[2]) - 1.3) < 1e-3 and all(b[0] <= a[0] for a, b in zip(hb, hb[1:]))
    st = P.scaled_fit_stats.fget(m)
    assert np.float64(st.scaled_sse[0]).tobytes() == lb.tobytes() == hb[-1].tobytes() and abs(st.slope[0] * float(cb[1]) - 2.5) < 1e-2
    m = Model(redundant, x, dtype)
    cn, ln, okn = P.fit_constants_nm(m, None, y, start, weights=w, iters=40, history=hn, scaled=True)
    assert ln.dtype == np.float64 and cn.dtype == dtype and okn[0] and m.nm_improves[0] > 0 and m.c.tobytes() == cn.tobytes()
    assert ln[0] < 1e-3 * hn[0][0] and hn[0][0] == hb[0][0] and all(b[0] <= a[0] for a, b in zip(hn, hn[1:]))
    assert np.float64(P.scaled_fit_stats.fget(m).scaled_sse[0]).tobytes() == ln.tobytes() == hn[-1].tobytes()
    # a zero gradient row: BFGS leaves the constant's bits, Nelder-Mead moves it
    y = (2.0 * np.rint(3.0 * x) + 0.5 * x).astype(dtype).astype(np.float64)
    start = np.array([1.5, 2.6, 0.2], dtype=dtype)
    m = Model(rounded, x, dtype)
    hb, hn = [], []
    cb, lb, _ = P.fit_constants_bfgs(m, None, y, start, weights=w, iters=12, history=hb, scaled=True)
    assert cb[1:2].tobytes() == start[1:2].tobytes() and lb[0] < 0.5 * hb[0][0] and m.bfgs_accepts[0] > 0
    m = Model(rounded, x, dtype)
    cn, ln, _ = P.fit_constants_nm(m, None, y, start, weights=w, iters=40, history=hn, scaled=True)
    assert cn[1] != start[1] and ln[0] < 0.5 * hn[0][0] and m.nm_improves[0] > 0
    print(f"[fit scaled host] {np.dtype(dtype).name}: model of the rounded tree {hn[0][0]:.6g} -> BFGS {lb[0]:.6g}, Nelder-Mead {ln[0]:.6g}")
