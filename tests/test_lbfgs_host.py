"""CPU tests of the L-BFGS fit's arithmetic (include/de_hip.h de_lbfgs_direction_host / de_lbfgs_update_host): the two
host-only hooks instantiate the templates of csrc/de_lbfgs.h, the code the kernels of de_fit_consts_lbfgs / de_fit_tree_params_lbfgs run.

THE REFERENCE of the direction is independent of the two-loop recursion: the dense BFGS update
    H <- (I - rho s y^T) H (I - rho y s^T) + rho s s^T          from H_0 = (s . y / y . y of the newest pair) I, oldest pair first,
applied to g as an operator (H itself would be 4096^2 entries) in mpmath at 50 digits, from the pairs the ring holds.  The pairs are
y = A s for a seeded SPD A = Q D Q (Q a Householder reflection, D in [1, 100]: condition <= 100), so every H is positive definite and no
case takes the reset.  The comparison is norm-wise: |p - p_ref| / |p_ref|.

DIRECTION_TOL is 4 x the worst relative error measured HERE, on the CPU, over every seeded case below (G x memory x ring shape).  The
margin is over a deterministic host computation — division and sqrt are correctly rounded — so x 4 only guards compiler differences.

THE HOST LOOP END TO END: api.lbfgs_fit (through api.tree_params_fit_lbfgs) over tests/test_tree_params_host.py's oracle_evaluator, one
member that is linear in its G = 51 unknowns (3 parameters x 16 classes + 3 real constants), Float64, memory 8, 200 iterations, against
the numpy.linalg.lstsq optimum."""
import ctypes as C

import mpmath
import numpy as np
import pytest

from dynamicexpressions_jl_amd import api
from test_tree_params_host import O_, OPS, P_, V_, X_, oracle_evaluator

MAX_ROWS, MAX_MEMORY = 4096, 16
WIDTHS = (1, 2, 63, 64, 65, 200, MAX_ROWS)
MEMORIES = (1, 3, 16)
SHAPES = ("short", "full", "wrapped")  # count < m, count == m, a ring that has wrapped
# measured: the worst |p - p_ref| / |p_ref| over WIDTHS x MEMORIES x SHAPES is 7.33e-16 (G = 63, memory = 16, count < m); x 4
DIRECTION_TOL = 2.94e-15
# measured: (final - opt) / (start - opt) after 200 iterations of the end-to-end case is 1.41e-15 — loss 112.926 -> 72.616285537841492
# against the lstsq optimum 72.616285537841435 (4 ulps apart), 57 accepted steps, then no trial lowers the loss any more; x 10
GAP_MEASURED, GAP_BOUND = 1.41e-15, 1.41e-14


def test_limits():
    lib = api.library()
    assert lib.de_lbfgs_max_rows() == MAX_ROWS == api.LBFGS_MAX_ROWS and lib.de_lbfgs_max_memory() == MAX_MEMORY == api.LBFGS_MAX_MEMORY
    assert MAX_ROWS >= 8 * 511 + 8  # P = 8 with 511 classes and 8 real constants
    assert C.sizeof(api.LbfgsOpts) == 48
    for name in ("de_lbfgs_max_rows", "de_lbfgs_max_memory", "de_lbfgs_direction_host", "de_lbfgs_update_host", "de_fit_consts_lbfgs",
                 "de_fit_tree_params_lbfgs"):
        assert hasattr(lib, name) and name in api.EXPORTS


# ---- the seeded pairs ------------------------------------------------------------------------------------------------------------------
def spd_apply(G, seed):
    """s -> A s for A = Q D Q, Q = I - 2 v v^T, D = diag(d), 1 <= d <= 100."""
    g = np.random.Generator(np.random.PCG64(seed))
    v = g.standard_normal(G)
    v /= np.linalg.norm(v)
    d = np.exp(g.uniform(0.0, np.log(100.0), G))

    def apply(s):
        q = s - 2.0 * v * (v @ s)
        q = d * q
        return q - 2.0 * v * (v @ q)

    return apply


def filled_state(G, m, shape, seed):
    """A ring of `shape` filled through lbfgs_update_host, and the number of pairs that went in."""
    n = {"short": m - 1, "full": m, "wrapped": m + 2}[shape]
    A = spd_apply(G, seed)
    g = np.random.Generator(np.random.PCG64(seed + 1))
    st = api.LbfgsState(G, m)
    for _ in range(n):
        s = g.standard_normal(G)
        assert api.lbfgs_update_host(st, s, A(s))
    assert st.count == min(n, m) and st.head == n % m
    return st, n


def mp_direction(st, g):
    """-H g by the dense BFGS recursion as an operator, in mpmath."""
    mp = mpmath.mp
    pairs = [([mpmath.mpf(v) for v in st.S[j, :st.G].tolist()], [mpmath.mpf(v) for v in st.Y[j, :st.G].tolist()])
             for j in reversed(st.newest_first())]  # oldest first
    gv = [mpmath.mpf(v) for v in g.tolist()]
    if not pairs:
        return [-v for v in gv]
    sn, yn = pairs[-1]
    gamma = mp.fdot(sn, yn) / mp.fdot(yn, yn)

    def H(k, v):  # H_k v, H_0 = gamma I
        if k == 0:
            return [gamma * e for e in v]
        s, y = pairs[k - 1]
        rho = 1 / mp.fdot(s, y)
        sv = mp.fdot(s, v)
        w = H(k - 1, [e - rho * sv * yy for e, yy in zip(v, y)])
        c = rho * (sv - mp.fdot(y, w))
        return [e + c * ss for e, ss in zip(w, s)]

    return [-e for e in H(len(pairs), gv)]


@pytest.fixture(scope="module")
def direction_errors():
    """|p - p_ref| / |p_ref| of every seeded case, computed once."""
    errs = {}
    with mpmath.workdps(50):
        for G in WIDTHS:
            for m in MEMORIES:
                for k, shape in enumerate(SHAPES):
                    st, _ = filled_state(G, m, shape, 1000 * m + 10 * k + G)
                    g = np.random.Generator(np.random.PCG64(7 * G + m)).standard_normal(G)
                    cnt, al = st.count, st.alpha
                    p, slope, produced = api.lbfgs_direction_host(st, g)
                    assert produced and slope < 0 and st.count == cnt and st.alpha == al  # (no reset: H is positive definite)
                    ref = mp_direction(st, g)
                    num = mpmath.sqrt(mpmath.fsum((mpmath.mpf(a) - b) ** 2 for a, b in zip(p.tolist(), ref)))
                    errs[(G, m, shape)] = float(num / mpmath.sqrt(mpmath.fsum(b * b for b in ref)))
                    assert slope == api.lbfgs_dot(g, p)
    return errs


def test_direction_against_the_dense_recursion(direction_errors):
    worst = max(direction_errors, key=direction_errors.get)
    print(f"[lbfgs direction] worst relative error {direction_errors[worst]:.3g} at (G, memory, ring) = {worst}; bound {DIRECTION_TOL:.3g}")
    assert len(direction_errors) == len(WIDTHS) * len(MEMORIES) * len(SHAPES)
    assert direction_errors[worst] <= DIRECTION_TOL, (worst, direction_errors[worst])


# ---- exact semantics -------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("G", [1, 5, 64, 130])
def test_an_empty_ring_gives_minus_g(G):
    g = np.random.Generator(np.random.PCG64(G)).standard_normal(G) * 3.0
    st = api.LbfgsState(G, 4, alpha=0.125)
    p, slope, produced = api.lbfgs_direction_host(st, g)
    assert produced and bits(p) == bits(-g) and slope == -api.lbfgs_dot(g, g)
    assert st.count == 0 and st.alpha == 0.125  # (a descent direction: the step the line search has reached stays)
    # the first step's length is a0 in the dot product's order
    n = np.sqrt(api.lbfgs_dot(g, g))
    assert api._lbfgs_a0(g, 1.0) == (1.0 / n if n > 1.0 else 1.0) and api._lbfgs_a0(g * 1e-3, 1.0) == 1.0


def test_no_descent_resets_the_state():
    """A ring whose pair has negative curvature (put there by hand: the update refuses such a pair) gives no descent direction: count = 0,
    p = -g bit for bit, slope = -g . g, alpha = a0(g)."""
    G = 70
    g = np.random.Generator(np.random.PCG64(5)).standard_normal(G) * 2.0
    st = api.LbfgsState(G, 3, alpha=0.25)
    st.S[0], st.Y[0] = g, -g
    st.rho[0], st.count, st.head = 1.0 / float(st.S[0] @ st.Y[0]), 1, 1
    p, slope, produced = api.lbfgs_direction_host(st, g, step0=1.0)
    assert produced and bits(p) == bits(-g) and slope == -api.lbfgs_dot(g, g)
    assert st.count == 0 and st.head == 1 and st.alpha == api._lbfgs_a0(g, 1.0) != 0.25


def test_non_finite_entries_and_a_zero_gradient_produce_nothing():
    G, m = 67, 3
    st, _ = filled_state(G, m, "full", 11)
    g = np.random.Generator(np.random.PCG64(2)).standard_normal(G)
    assert api.lbfgs_direction_host(st, g)[2]
    for where in ("g", "S", "Y"):
        bad, gb = api.LbfgsState(G, m), g.copy()
        bad.S[:], bad.Y[:], bad.rho[:], bad.count, bad.head = st.S, st.Y, st.rho, st.count, st.head
        if where == "g":
            gb[66] = np.nan
        else:
            getattr(bad, where)[1, 65] = np.nan
        p, slope, produced = api.lbfgs_direction_host(bad, gb)
        assert not produced and np.all(p == 0) and bits(p) == bits(np.zeros(G)), where
    p, slope, produced = api.lbfgs_direction_host(st, np.zeros(G))
    assert not produced and bits(p) == bits(np.zeros(G)) and st.count == 0 and st.alpha == 1.0
    # a NaN in a slot that is NOT stored is not read
    st2, _ = filled_state(G, m, "short", 12)
    st2.S[m - 1, 0] = np.nan
    assert api.lbfgs_direction_host(st2, g)[2]


@pytest.mark.parametrize("G", [0, MAX_ROWS + 1])
def test_a_width_outside_the_limit_touches_nothing(G):
    lib, m, SENT = api.library(), 2, 7.0
    n = max(G, 1)
    S, Y, rho = np.full((m, n), SENT), np.full((m, n), SENT), np.full(m, SENT)
    cnt, head = np.array([1], dtype=np.int32), np.array([1], dtype=np.int32)
    al, g, p, slope = np.full(1, SENT), np.full(n, SENT), np.full(n, SENT), np.full(1, SENT)
    rc = lib.de_lbfgs_direction_host(G, m, S.ctypes.data, Y.ctypes.data, rho.ctypes.data, cnt.ctypes.data, head.ctypes.data, al.ctypes.data,
                                     g.ctypes.data, 1.0, p.ctypes.data, slope.ctypes.data)
    assert rc == 0
    rc = lib.de_lbfgs_update_host(G, m, S.ctypes.data, Y.ctypes.data, rho.ctypes.data, cnt.ctypes.data, head.ctypes.data, g.ctypes.data,
                                  g.ctypes.data, 1e-8)
    assert rc == 0
    for a in (S, Y, rho, al, g, p, slope):
        assert np.all(a == SENT)
    assert cnt[0] == 1 and head[0] == 1
    # ... and so does a memory outside 1 .. 16 at a good width
    for mem in (0, MAX_MEMORY + 1):
        rc = lib.de_lbfgs_direction_host(1, mem, S.ctypes.data, Y.ctypes.data, rho.ctypes.data, cnt.ctypes.data, head.ctypes.data,
                                         al.ctypes.data, g.ctypes.data, 1.0, p.ctypes.data, slope.ctypes.data)
        assert rc == 0 and np.all(p == SENT) and np.all(slope == SENT) and np.all(al == SENT)


def test_a_pair_without_curvature_leaves_every_byte():
    G, m = 66, 3
    st, _ = filled_state(G, m, "wrapped", 21)
    before = (bits(st.S), bits(st.Y), bits(st.rho), st.count, st.head)
    g = np.random.Generator(np.random.PCG64(3)).standard_normal(G)
    for s, yv in ((g, -g), (g, np.zeros(G)), (g, np.full(G, np.nan)), (np.full(G, np.inf), g)):
        assert not api.lbfgs_update_host(st, s, yv)
        assert (bits(st.S), bits(st.Y), bits(st.rho), st.count, st.head) == before
    # curv: s . yv > curv |s| |yv| is the whole test
    e0, e1 = np.eye(G)[0], np.eye(G)[1]
    assert not api.lbfgs_update_host(st, e0, 0.5 * e0 + e1, curv=0.5) and api.lbfgs_update_host(st, e0, 0.5 * e0 + e1, curv=0.4)


@pytest.mark.parametrize("m", [1, 3, 16])
def test_the_ring_wraps(m):
    """After m + 1 stored pairs the oldest slot (0) holds the newest pair, head = 1 mod m and count = m."""
    G = 65
    A = spd_apply(G, 31)
    g = np.random.Generator(np.random.PCG64(32))
    st, pairs = api.LbfgsState(G, m), []
    for k in range(m + 1):
        s = g.standard_normal(G)
        pairs.append((s, A(s)))
        assert api.lbfgs_update_host(st, *pairs[-1])
        assert st.count == min(k + 1, m) and st.head == (k + 1) % m
    s, yv = pairs[-1]
    assert bits(st.S[0]) == bits(s) and bits(st.Y[0]) == bits(yv) and st.rho[0] == 1.0 / api.lbfgs_dot(s, yv)
    for j in range(1, m):  # the others: pairs 1 .. m - 1, untouched
        assert bits(st.S[j]) == bits(pairs[j][0]) and bits(st.Y[j]) == bits(pairs[j][1])
    assert st.newest_first()[0] == 0


# ---- the host loop end to end ----------------------------------------------------------------------------------------------------------
def linear_case():
    """One member, linear in its 51 unknowns: c1 x1 x2 + c2 x1 x1 + c3 x2 x2 + p1 + p2 x1 + p3 x2 with 16 classes of 8 samples."""
    P, NCLS, per = 3, 16, 8
    N = NCLS * per
    g = np.random.Generator(np.random.PCG64(41))
    X = np.asfortranarray(g.uniform(-1.0, 1.0, (2, N)))
    y = g.standard_normal(N)
    classes = np.repeat(np.arange(1, NCLS + 1), per)
    x1, x2 = X_(1), X_(2)
    tree = O_("+", O_("+", O_("+", O_("*", V_(0.0), O_("*", x1, x2)), O_("*", V_(0.0), O_("*", x1, x1))), O_("*", V_(0.0), O_("*", x2, x2))),
              O_("+", O_("+", P_(1), O_("*", P_(2), x1)), O_("*", P_(3), x2)))
    # the design matrix in the combined vector's order: constants, then parameters[:] column-major over [P, NCLS]
    D = np.zeros((N, 3 + P * NCLS))
    D[:, 0], D[:, 1], D[:, 2] = X[0] * X[1], X[0] * X[0], X[1] * X[1]
    for j in range(N):
        c = classes[j] - 1
        D[j, 3 + c * P:3 + c * P + P] = (1.0, X[0, j], X[1, j])
    return tree, X, y, classes, D, P, NCLS


def test_lbfgs_fit_reaches_the_least_squares_optimum():
    tree, X, y, classes, D, P, NCLS = linear_case()
    ev = oracle_evaluator([tree], OPS, X, y, classes)
    hist = []
    cs, ps, lo, ok, acc = api.tree_params_fit_lbfgs(ev, [np.zeros(3)], np.zeros((1, P, NCLS)), iters=200, memory=8, history=hist)
    assert ok[0] and len(hist) == 201 and len(cs[0]) + ps[0].size == 51 == D.shape[1]
    sol = np.linalg.lstsq(D, y, rcond=None)[0]
    opt = float(np.sum((D @ sol - y) ** 2))
    start, final = float(hist[0][0]), float(lo[0])
    gap = (final - opt) / (start - opt)
    print(f"[lbfgs_fit, oracle] G = 51: loss {start:.6g} -> {final:.17g}, lstsq optimum {opt:.17g}, gap {gap:.3g} (measured {GAP_MEASURED:.3g}), "
          f"{int(acc[0])} accepted steps of 200")
    assert all(b[0] <= a[0] for a, b in zip(hist, hist[1:]))
    assert final < start and start == float(np.sum(y * y))
    assert final >= opt * (1 - 1e-12)  # not below the optimum (lstsq's own rounding)
    assert gap <= GAP_BOUND
    # the same member under tree_params_fit_bfgs keeps every bit: 51 unknowns > 32
    cs_b, ps_b, lo_b, _, acc_b = api.tree_params_fit_bfgs(ev, [np.zeros(3)], np.zeros((1, P, NCLS)), iters=3)
    assert acc_b[0] == 0 and not ps_b.any() and lo_b[0] == start


# ---- a stand-alone program under the sanitizers ----------------------------------------------------------------------------------------
MAIN = r"""
#include <cstdio>
#include <vector>
#include "de_lbfgs.h"
// argv[1]: G, memory, n, curv, alpha, step0, then n pairs (s, yv: G doubles each) and g, raw.  Every pair goes through lbfgs_update, then
// one lbfgs_direction.  Prints the updates' results, then count and head with the bit patterns of rho, then produced and the count
// behind the direction with those of p, slope and alpha.
static void bits(const std::vector<double> &v) {
    for (double d : v) {
        unsigned long long u;
        __builtin_memcpy(&u, &d, 8);
        std::printf(" %016llx", u);
    }
    std::printf("\n");
}
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    double head6[6];
    if (std::fread(head6, 8, 6, f) != 6) return 2;
    const int G = (int)head6[0], m = (int)head6[1], n = (int)head6[2];
    // exactly the documented sizes: a sanitizer sees any overrun
    std::vector<double> S((size_t)m * G), Y((size_t)m * G), rho((size_t)m), s((size_t)G), yv((size_t)G), g((size_t)G), p((size_t)G);
    int32_t count = 0, head = 0;
    de::LbfgsHostTeam tm;
    for (int i = 0; i < n; i++) {
        if (std::fread(s.data(), 8, s.size(), f) != s.size() || std::fread(yv.data(), 8, yv.size(), f) != yv.size()) return 2;
        std::printf("%d", de::lbfgs_update(tm, G, m, S.data(), Y.data(), rho.data(), &count, &head, s.data(), yv.data(), head6[3]));
    }
    if (std::fread(g.data(), 8, g.size(), f) != g.size()) return 2;
    std::fclose(f);
    std::printf("\n%d %d", (int)count, (int)head);
    bits(rho);
    const de::LbfgsDir r = de::lbfgs_direction(tm, G, m, S.data(), Y.data(), rho.data(), count, head, head6[4], g.data(), head6[5], p.data());
    std::printf("%d %d", r.produced, r.count);
    bits(p);
    bits({r.slope, r.alpha});
    return 0;
}
"""


def test_the_shared_header_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The shapes of the direction test (the ring short — empty at memory 1 —, full and wrapped, a refused pair in between) through a
    program of its own built with -fsanitize=address,undefined: clean, and the library's bits."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed (the oracle is built with one)"
    (tmp_path / "main.cpp").write_text(MAIN)
    exe = tmp_path / "lbfgs_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(root, "dynamicexpressions.jl_amd", "csrc"), str(tmp_path / "main.cpp"), "-o", str(exe)], check=True)
    hexes = lambda v: [f"{x:016x}" for x in np.ascontiguousarray(v, dtype=np.float64).reshape(-1).view(np.uint64)]
    cases = [(G, m, shape) for G in (1, 65, 200, MAX_ROWS) for m, shape in ((1, "wrapped"), (3, "short"), (16, "full"), (3, "wrapped"))]
    cases.append((70, 1, "short"))  # an empty ring
    for k, (G, m, shape) in enumerate(cases):
        rng = np.random.Generator(np.random.PCG64(100 + k))
        A = spd_apply(G, 200 + k)
        n = {"short": m - 1, "full": m, "wrapped": m + 2}[shape]
        g = rng.standard_normal(G) * 2.0
        pairs = [(s, A(s)) for s in (rng.standard_normal(G) for _ in range(n))]
        if shape == "wrapped":
            pairs.insert(1, (pairs[0][0], -pairs[0][1]))  # a pair the curvature test refuses
        st, results = api.LbfgsState(G, m, alpha=0.25), []
        for s, yv in pairs:
            results.append(int(api.lbfgs_update_host(st, s, yv)))
        path = tmp_path / f"case{k}.bin"
        blob = np.array([float(G), float(m), float(len(pairs)), 1e-8, 0.25, 0.5]).tobytes()
        path.write_bytes(blob + b"".join(s.tobytes() + yv.tobytes() for s, yv in pairs) + g.tobytes())
        out = subprocess.run([str(exe), str(path)], check=True, capture_output=True, text=True).stdout.split("\n")
        assert out[0] == "".join(map(str, results)) and sum(results) == n
        rho = st.rho.copy()
        stored = st.newest_first()
        line = out[1].split()
        assert line[:2] == [str(st.count), str(st.head)] and [line[2 + j] for j in stored] == [hexes(rho)[j] for j in stored]
        p, slope, produced = api.lbfgs_direction_host(st, g, 0.5)
        line = out[2].split()
        assert produced and line[:2] == ["1", str(st.count)] and line[2:] == hexes(p)
        assert out[3].split() == hexes([slope, st.alpha])
