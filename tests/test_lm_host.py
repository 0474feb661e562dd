"""CPU tests of the arithmetic of the device-side Levenberg-Marquardt step (include/de_hip.h de_lm_solve_host): the
host-only hook runs csrc/de_lm_solve.h, the code de_lm_step_kernel runs — a Cholesky solve of  A delta = -g / 2,
A = H + lam diag(diag H), in float64.

Bounds (u = 2^-53), for systems H = (J w) J^T with badly scaled rows:
    residual   |A delta - b|_2 <= 4 G^2 u (|A|_2 |delta|_2 + |b|_2)       Cholesky's backward error, gamma_{3G+1} G < 4 G^2 u
                                                                         (Higham, Accuracy and Stability, Thm 10.4): a worst case
    forward    |delta - delta_np| <= 8 G^2 u cond_2(A) |delta_np|          against numpy.linalg.solve where cond_2(A) < 10^12: the two
                                                                         forward errors added
The residual is formed in long double.  The zero step is returned exactly where a float64 Cholesky in the documented order
(d = A_jj - sum_k L_jk^2) meets a pivot with !(d > 0)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from dynamicexpressions_jl_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53


def damped(H, lam):
    A = np.array(H, dtype=np.float64)
    for j in range(A.shape[0]):
        A[j, j] = A[j, j] + np.float64(lam) * A[j, j]
    return A


def cholesky_pivots_positive(A):
    """The factorisation of csrc/de_lm_solve.h in float64 scalars, same order of operations: False at the first pivot with !(d > 0)."""
    G = A.shape[0]
    L = np.zeros((G, G), dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(G):
            s = np.float64(0.0)
            for k in range(j):
                s = s + L[j, k] * L[j, k]
            d = A[j, j] - s
            if not d > 0.0:
                return False
            l = np.sqrt(d)
            L[j, j] = l
            for i in range(j + 1, G):
                r = np.float64(0.0)
                for k in range(j):
                    r = r + L[i, k] * L[j, k]
                L[i, j] = (A[i, j] - r) / l
    return True


def draw(seed):
    """(G, N, dtype, H, g) over G = 1 .. 8, N in {64, 300}, the matrix rounded through float32 or float64."""
    g = np.random.default_rng(seed)
    for G in range(1, 9):
        for N in (64, 300):
            for dtype in (np.float32, np.float64):
                J = g.standard_normal((G, N)) * np.exp(g.uniform(-6.0, 6.0, (G, 1)))
                w = g.uniform(0.25, 2.0, N)
                H = ((J * w) @ J.T).astype(dtype).astype(np.float64)
                H = np.tril(H) + np.tril(H, -1).T  # both triangles present, exactly symmetric (as de_eval_loss_gn writes them)
                grad = (2.0 * (J * w) @ g.standard_normal(N)).astype(dtype).astype(np.float64)
                yield G, N, dtype, H, grad


@pytest.mark.parametrize("seed", range(5))
def test_residual_and_forward_bounds(seed):
    L = np.longdouble
    worst_res = worst_fwd = 0.0
    n_fwd = n_zero = n = 0
    for G, N, dtype, H, grad in draw(seed):
        for lam in (1e-3, 1.0, 1e3):
            step, produced = api.lm_solve_host(H, grad, lam)
            A = damped(H, lam)
            assert produced == cholesky_pivots_positive(A), (G, N, dtype, lam)
            n += 1
            if not produced:
                assert not step.any()
                n_zero += 1
                continue
            b = -0.5 * grad
            res = float(np.sqrt(np.sum((A.astype(L) @ step.astype(L) - b.astype(L)) ** 2)))
            bound = 4 * G * G * U64 * (np.linalg.norm(A, 2) * np.linalg.norm(step) + np.linalg.norm(b))
            worst_res = max(worst_res, res / bound)
            assert res <= bound, (G, N, dtype, lam, res / bound)
            cond = np.linalg.cond(A, 2)
            if cond < 1e12:
                ref = np.linalg.solve(A, b)
                err, fb = np.linalg.norm(step - ref), 8 * G * G * U64 * cond * np.linalg.norm(ref)
                worst_fwd = max(worst_fwd, err / fb)
                assert err <= fb, (G, N, dtype, lam, err / fb)
                n_fwd += 1
    print(f"[lm host] seed {seed}: {n} systems, {n_zero} zero steps, worst residual {worst_res:.3f} of the bound, "
          f"worst forward error {worst_fwd:.3g} of the bound over {n_fwd} systems with cond < 1e12")
    assert n == 8 * 2 * 2 * 3 and n_fwd >= n // 4 and n_zero <= n // 10


def test_the_answer_is_the_zero_step_exactly_where_a_pivot_is_not_positive():
    # lam = 0 on nearly rank-deficient matrices: both outcomes occur, and the hook agrees with the float64 factorisation on every one
    g = np.random.default_rng(11)
    seen = {True: 0, False: 0}
    for G in range(2, 9):
        for rep in range(20):
            J = g.standard_normal((G, 40))
            J[-1] = J[0] * (1.0 + (0.0 if rep % 2 else 1e-9 * g.standard_normal()))  # a repeated row: H is singular to rounding
            H = (J @ J.T).astype(np.float32 if rep % 4 < 2 else np.float64).astype(np.float64)
            H = np.tril(H) + np.tril(H, -1).T
            grad = g.standard_normal(G)
            step, produced = api.lm_solve_host(H, grad, 0.0)
            assert produced == cholesky_pivots_positive(damped(H, 0.0)), (G, rep)
            assert produced or not step.any()
            seen[produced] += 1
    assert seen[True] >= 10 and seen[False] >= 10, seen


def test_zero_step_cases():
    lib = api.library()
    # H = [[N, N], [N, N]] (one repeated row of ones over N samples), lam = 0.  N = 64: sqrt(64) and 64 / 8 are exact, the second pivot is
    # exactly 0 and the answer is the zero step.  N = 300: sqrt(300) rounds, the pivot 300 - fl(300 / fl(sqrt(300)))^2 is a rounding
    # error of either sign, and the answer is whatever the float64 factorisation in the documented order meets.
    H = np.array([[64.0, 64.0], [64.0, 64.0]])
    step, produced = api.lm_solve_host(H, np.array([1.0, -2.0]), 0.0)
    assert not produced and step.tolist() == [0.0, 0.0] and not cholesky_pivots_positive(H)
    H300 = np.full((2, 2), 300.0)
    step, produced = api.lm_solve_host(H300, np.array([1.0, -2.0]), 0.0)
    assert produced == cholesky_pivots_positive(H300) and (produced or not step.any())
    step, produced = api.lm_solve_host(H, np.array([1.0, -2.0]), 0.5)  # ... and the damped system is regular
    assert produced and np.allclose(damped(H, 0.5) @ step, [-0.5, 1.0], rtol=1e-14)
    good = np.array([[4.0, 1.0], [1.0, 3.0]])
    for Hb, gb, lam in ((np.array([[4.0, np.nan], [np.nan, 3.0]]), [1.0, 1.0], 1e-3), (np.array([[np.nan, 1.0], [1.0, 3.0]]), [1.0, 1.0], 1e-3),
                        (np.array([[4.0, 1.0], [1.0, np.inf]]), [1.0, 1.0], 1e-3), (good, [np.nan, 1.0], 1e-3), (good, [1.0, -np.inf], 1e-3),
                        (good, [1.0, 1.0], np.inf), (good, [1.0, 1.0], np.nan), (-good, [1.0, 1.0], 1e-3)):
        step, produced = api.lm_solve_host(Hb, gb, lam)
        assert not produced and step.tolist() == [0.0, 0.0], (Hb, gb, lam)
    step, produced = api.lm_solve_host(good, [1.0, 1.0], 1e-3)
    assert produced and np.isfinite(step).all() and step.any()
    # G = 0 and G > 8: return value 0; the wide system's step is zero-filled
    assert lib.de_lm_solve_host(0, None, None, 1e-3, None) == 0
    sentinel = np.full(3, 7.0)
    assert lib.de_lm_solve_host(0, good.ctypes.data, sentinel.ctypes.data, 1e-3, sentinel.ctypes.data) == 0 and (sentinel == 7).all()
    wide, gw, sw = np.asfortranarray(np.eye(9)), np.ones(9), np.full(9, 7.0)
    assert lib.de_lm_solve_host(9, wide.ctypes.data, gw.ctypes.data, 1e-3, sw.ctypes.data) == 0 and not sw.any()


def test_matches_lm_step_on_a_well_conditioned_system():
    g = np.random.default_rng(5)
    for G in (1, 3, 8):
        a = g.standard_normal((G + 3, G))
        H, grad = a.T @ a, g.standard_normal(G)
        gn = api.GaussNewton(np.zeros(1), [grad], [H], np.ones(1, dtype=bool))
        for lam in (0.0, 1e-3, 2.5):
            step, produced = api.lm_solve_host(H, grad, lam)
            want = gn.lm_step(lam, tree=0)
            cond = np.linalg.cond(damped(H, lam), 2)
            assert produced and np.linalg.norm(step - want) <= 8 * G * G * U64 * cond * np.linalg.norm(want)


def test_prototypes_and_struct():
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "de_hip.h")).read(), flags=re.S)
    for name, n_args in (("de_gn_lm_step", 11), ("de_fit_consts_lm", 13), ("de_lm_solve_host", 5)):
        m = re.search(r"^int %s\(([^;]*)\);" % name, src, re.M)
        assert m, f"include/de_hip.h declares {name}"
        assert len(m.group(1).split(",")) == n_args == len(getattr(api.library(), name).argtypes)
        assert name in api.EXPORTS
    m = re.search(r"typedef\s+struct\s+de_lm_opts\s*\{([^}]*)\}\s*de_lm_opts_t\s*;", src)
    fields = [f.strip() for decl in m.group(1).split(";") if decl.strip() for f in decl.split(",")]
    assert [f.split()[-1] for f in fields] == [n for n, _ in api.LmOpts._fields_] and C.sizeof(api.LmOpts) == 40
    assert api.ABI_VERSION == 3 and re.search(r"#define\s+DE_HIP_ABI_VERSION\s+3\b", src)
    assert re.search(r"\(h\) de_gn_lm_step", open(os.path.join(ROOT, "include", "de_hip.h")).read())
