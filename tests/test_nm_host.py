"""CPU tests of the Nelder-Mead fit's arithmetic (include/de_hip.h de_nm_ask_host / de_nm_tell_host): the two
host-only hooks run csrc/de_nm.h, the code the kernels of de_fit_consts_nm run.

The method is stated in the header as a rule set with a fixed order of every sum, so the check is BITS, not bounds: `Model` below is that
rule set again in plain Python floats (float64 loops, sums in the stated order, `rnd` the one rounding to the element type) — no call into
the library — and after every one of 300 rounds every vertex, every f, the phase and the trial of the hooks equal the model's bit for
bit, for T = float32 and float64.  The objectives are analytic and evaluated by the test (a quadratic bowl at G = 1, 2, 3, 8, 32,
Rosenbrock at G = 2, a bowl with a forbidden half-space whose evaluations fail).  The model counts the outcomes it takes; every one of
reflect-accept, expand-taken, expand-refused, contract-out, contract-in, shrink and DONE occurs over the set (the starts were chosen on
the CPU so that the model alone does that).

`Model`, `rnd` and `model_fit` are shared with tests/test_gpu_nm.py."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from dynamicexpressions_jl_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
BUILD, REFLECT, EXPAND, CONTRACT_OUT, CONTRACT_IN, SHRINK, DONE = range(7)
OUTCOMES = ("reflect-accept", "expand-taken", "expand-refused", "contract-out", "contract-in", "shrink", "DONE")


# ---- the rule set in plain Python ----------------------------------------------------------------------------------------------------------
def rnd(dtype, v: float) -> float:
    """T(v) as a float64."""
    if np.dtype(dtype) == np.float64:
        return float(v)
    with np.errstate(over="ignore"):
        return float(np.float32(v))


class Model:
    """One tree: include/de_hip.h's rule set, one evaluation per round."""

    def __init__(self, x0, f0, dtype, a=0.025, b=0.5, f_tol=0.0):
        self.T, self.a, self.b, self.f_tol = dtype, a, b, f_tol
        G = self.G = len(x0)
        self.V = [[rnd(dtype, v) for v in x0]] + [[0.0] * G for _ in range(G)]
        self.f = [f0 if math.isfinite(f0) else INF] + [INF] * G
        self.phase, self.cur, self.l0 = BUILD, 1, 0
        self.c, self.xr, self.fr = [0.0] * G, [0.0] * G, 0.0
        if G >= 2:
            self.alpha, self.beta, self.gamma, self.delta = 1.0, 1.0 + 2.0 / G, 0.75 - 1.0 / (2.0 * G), 1.0 - 1.0 / G
        else:
            self.alpha, self.beta, self.gamma, self.delta = 1.0, 2.0, 0.5, 0.5
        self.counts = dict.fromkeys(OUTCOMES, 0)

    def order(self):
        f, G = self.f, self.G
        l = h = 0
        for i in range(1, G + 1):
            if f[i] < f[l]:
                l = i
            if f[i] >= f[h]:
                h = i
        s = -1
        for i in range(G + 1):
            if i != h and (s < 0 or f[i] >= f[s]):
                s = i
        return l, s, h

    def second(self, j):
        c, x = self.c[j], self.xr[j]
        if self.phase == EXPAND:
            return rnd(self.T, c + self.beta * (x - c))
        if self.phase == CONTRACT_OUT:
            return rnd(self.T, c + self.gamma * (x - c))
        return rnd(self.T, c - self.gamma * (x - c))

    def ask(self):
        G, V, T = self.G, self.V, self.T
        if self.phase == BUILD:
            k = self.cur
            V[k] = [rnd(T, (1.0 + self.b) * V[0][j] + self.a) if j == k - 1 else V[0][j] for j in range(G)]
            return list(V[k])
        if self.phase == REFLECT:
            l, s, h = self.order()
            if self.f[h] - self.f[l] <= self.f_tol * abs(self.f[l]):
                self.phase = DONE
                self.counts["DONE"] += 1
                return list(V[l])
            for j in range(G):
                acc = 0.0
                for i in range(G + 1):
                    if i != h:
                        acc = acc + V[i][j]
                self.c[j] = acc / G
                self.xr[j] = rnd(T, self.c[j] + self.alpha * (self.c[j] - V[h][j]))
            return list(self.xr)
        if self.phase in (EXPAND, CONTRACT_OUT, CONTRACT_IN):
            return [self.second(j) for j in range(G)]
        if self.phase == SHRINK:
            i, l0 = self.cur, self.l0
            V[i] = [rnd(T, V[l0][j] + self.delta * (V[i][j] - V[l0][j])) for j in range(G)]
            return list(V[i])
        return list(V[self.order()[0]])  # DONE

    def tell(self, F):
        """F: the trial's loss as stored (+inf: failed)."""
        G, V, f = self.G, self.V, self.f
        if self.phase == DONE:
            return
        if self.phase in (BUILD, SHRINK):
            f[self.cur] = F
            nxt = self.cur + 1
            if self.phase == SHRINK and nxt == self.l0:
                nxt += 1
            if nxt > G:
                self.phase = REFLECT
            else:
                self.cur = nxt
            return
        l, s, h = self.order()
        trial = [self.second(j) for j in range(G)] if self.phase != REFLECT else None
        shrink = False
        if self.phase == REFLECT:
            self.fr = F
            if F < f[l]:
                self.phase = EXPAND
            elif F < f[s]:
                V[h], f[h] = list(self.xr), F
                self.counts["reflect-accept"] += 1
            elif F < f[h]:
                self.phase = CONTRACT_OUT
            else:
                self.phase = CONTRACT_IN
            return
        if self.phase == EXPAND:
            if F < self.fr:
                V[h], f[h] = trial, F
                self.counts["expand-taken"] += 1
            else:
                V[h], f[h] = list(self.xr), self.fr
                self.counts["expand-refused"] += 1
        elif self.phase == CONTRACT_OUT:
            if F <= self.fr:
                V[h], f[h] = trial, F
                self.counts["contract-out"] += 1
            else:
                shrink = True
        else:
            if F < f[h]:
                V[h], f[h] = trial, F
                self.counts["contract-in"] += 1
            else:
                shrink = True
        if shrink:
            self.counts["shrink"] += 1
            self.phase, self.l0, self.cur = SHRINK, l, (1 if l == 0 else 0)
        else:
            self.phase = REFLECT


def model_fit(objective, x0, dtype, rounds, **kw):
    """The model alone on `objective(list of float) -> (loss, ok)`: (accepted constants, accepted loss, history, model)."""
    f0, ok0 = objective([rnd(dtype, v) for v in x0])
    assert ok0
    m = Model(x0, rnd(dtype, f0), dtype, **kw)
    hist = [m.f[0]]
    for _ in range(rounds):
        F, ok = objective(m.ask())
        F = rnd(dtype, F)
        m.tell(F if ok and math.isfinite(F) else INF)
        hist.append(m.f[m.order()[0]])
    l = m.order()[0]
    return m.V[l], m.f[l], hist, m


# ---- the analytic objectives ---------------------------------------------------------------------------------------------------------------
def bowl(G, wall=None):
    """sum_j (1 + j / 2) (x_j - m_j)^2 with m_j = 0.3 j - 1; evaluations with x_0 > wall fail."""
    def f(x):
        if wall is not None and x[0] > wall:
            return math.nan, False
        acc = 0.0
        for j in range(G):
            d = x[j] - (0.3 * j - 1.0)
            acc = acc + (1.0 + 0.5 * j) * (d * d)
        return acc, True
    return f


def rosenbrock(x):
    p, q = 1.0 - x[0], x[1] - x[0] * x[0]
    return p * p + 100.0 * (q * q), True


def cases():
    """(name, objective, start, options)"""
    out = [(f"bowl{G}", bowl(G), [0.7 + 0.11 * j for j in range(G)], {}) for G in (1, 2, 3, 8, 32)]
    out.append(("bowl3 f_tol", bowl(3), [2.0, -1.5, 0.25], dict(f_tol=1e-9)))
    out.append(("bowl2 a only", bowl(2), [0.0, 0.0], dict(a=0.5, b=0.0)))
    out.append(("rosenbrock", rosenbrock, [-1.2, 1.0], {}))
    out.append(("rosenbrock far", rosenbrock, [3.0, -2.0], dict(a=0.1, b=0.25)))
    out.append(("wall2", bowl(2, wall=-0.6), [-2.0, 1.5], {}))
    out.append(("wall8", bowl(8, wall=-0.8), [-1.5 - 0.1 * j for j in range(8)], {}))
    return out


def state_bits(s):
    return s.V.tobytes(), s.f.tobytes(), int(s.st[0])


def model_bits(m):
    return np.array(m.V, dtype=np.float64).tobytes(), np.array(m.f, dtype=np.float64).tobytes(), m.phase


# ---- 1. exports ----------------------------------------------------------------------------------------------------------------------------
def test_prototypes_and_null_arguments():
    raw = open(os.path.join(ROOT, "include", "de_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    lib = api.library()
    for name, n_args in (("de_nm_max_rows", 0), ("de_nm_ask_host", 9), ("de_nm_tell_host", 10), ("de_fit_consts_nm", 14)):
        m = re.search(r"^int %s\(([^;]*)\);" % name, src, re.M)
        assert m, f"include/de_hip.h declares {name}"
        assert (0 if m.group(1).strip() == "void" else len(m.group(1).split(","))) == n_args
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == n_args and name in api.EXPORTS
    assert re.search(r"typedef struct de_nm_opts \{\s*int32_t iters;\s*int32_t reserved;\s*double a, b;\s*double f_tol;\s*\} de_nm_opts_t;", src)
    assert [n for n, _ in api.NmOpts._fields_] == ["iters", "reserved", "a", "b", "f_tol"]
    assert api.ABI_VERSION == 3 == lib.de_abi_version() and re.search(r"#define\s+DE_HIP_ABI_VERSION\s+3\b", src)
    assert lib.de_nm_max_rows() == 32 == api.NM_MAX_ROWS
    assert re.search(r"\(q\) de_nm_max_rows", raw)
    assert lib.de_fit_consts_nm(None, None, None, 0, 0, None, None, None, None, None, None, None, None, None) == 1  # no context
    assert lib.de_nm_ask_host(3, 0, None, None, None, None, None, None, None) == 0
    assert lib.de_nm_tell_host(3, 0, None, None, None, None, None, None, 1.0, 1) == 0
    # one null pointer among good ones, another dtype, a phase outside 0 .. 6: 0, the state untouched
    s = api.NmState([1.0, 2.0, 3.0], 5.0, np.float64)
    before = state_bits(s)
    trial = np.zeros(3)
    good = [s.V.ctypes.data, s.f.ctypes.data, s.st.ctypes.data, s.c.ctypes.data, s.xr.ctypes.data, trial.ctypes.data]
    for k in range(6):
        assert lib.de_nm_ask_host(3, 1, None, *[None if i == k else p for i, p in enumerate(good)]) == 0
    tgood = good[:5] + [s.fr.ctypes.data]
    for k in range(6):
        assert lib.de_nm_tell_host(3, 1, *[None if i == k else p for i, p in enumerate(tgood)], 1.0, 1) == 0
    assert lib.de_nm_ask_host(3, 2, None, *good) == 0 and lib.de_nm_tell_host(3, 5, *tgood, 1.0, 1) == 0  # DE_F16, no dtype
    s.st[0] = 9
    assert lib.de_nm_ask_host(3, 1, None, *good) == 0 and lib.de_nm_tell_host(3, 1, *tgood, 1.0, 1) == 0
    s.st[0] = 0
    assert state_bits(s) == before and not trial.any()
    assert lib.de_nm_ask_host(3, 1, None, *good) == 1 and trial.tolist() == [1.5 * 1.0 + 0.025, 2.0, 3.0]  # null options: a = 0.025, b = 0.5


# ---- 2. + 3. the hooks against the model, and the invariants ---------------------------------------------------------------------------------
def run_case(objective, x0, dtype, rounds, kw, totals):
    T = np.dtype(dtype)
    x0r = [rnd(dtype, v) for v in x0]
    f0, ok0 = objective(x0r)
    assert ok0 and math.isfinite(f0)
    f0 = rnd(dtype, f0)
    m = Model(x0r, f0, dtype, **kw)
    s = api.NmState(np.array(x0r, dtype=T), f0, T)
    assert state_bits(s) == model_bits(m)
    accepted, failed_trials = f0, 0
    for r in range(rounds):
        want = m.ask()
        got = api.nm_ask_host(s, **kw)
        assert got.dtype == T and got.astype(np.float64).tobytes() == np.array(want).tobytes(), (r, m.phase)
        assert state_bits(s) == model_bits(m), (r, "ask")
        F, ok = objective(want)
        F = rnd(dtype, F) if ok else math.nan
        assert api.nm_tell_host(s, F, ok)
        m.tell(F if ok and math.isfinite(F) else INF)
        assert state_bits(s) == model_bits(m), (r, "tell")
        assert s.c.tobytes() == np.array(m.c).tobytes() and s.xr.tobytes() == np.array(m.xr).tobytes() and s.fr[0] == m.fr
        # invariants: no NaN is stored; a failed trial never becomes the accepted vertex; the accepted loss never increases; every
        # stored coordinate is a value of T
        assert not np.isnan(s.f).any()
        if not (ok and math.isfinite(F)):
            failed_trials += 1
            assert s.V[s.best].tobytes() != np.array(want).tobytes()  # (an expansion that fails hands the reflected point over)
        now = s.f[s.best]
        assert now <= accepted and math.isfinite(now)
        accepted = now
        with np.errstate(over="ignore"):
            assert np.array_equal(s.V.astype(T).astype(np.float64), s.V) and np.array_equal(s.xr.astype(T).astype(np.float64), s.xr)
    for k, v in m.counts.items():
        totals[k] = totals.get(k, 0) + v
    return f0, accepted, failed_trials, m


@DTYPES
def test_hooks_equal_the_model_bit_for_bit_over_300_rounds(dtype):
    totals, failed = {}, 0
    for name, objective, x0, kw in cases():
        f0, f1, nfail, m = run_case(objective, x0, dtype, 300, kw, totals)
        failed += nfail
        print(f"[nm host] {np.dtype(dtype).name} {name}: loss {f0:.4g} -> {f1:.4g}, phase {m.phase}, {m.counts}")
        assert f1 < f0
    assert all(totals[k] >= 1 for k in OUTCOMES), totals
    assert failed >= 1  # the +Inf handling ran
    print(f"[nm host] {np.dtype(dtype).name}: outcomes over the set {totals}, {failed} failed trials")


def test_widths_outside_the_range_leave_a_sentinel_state_untouched():
    lib = api.library()
    for G in (0, 33, -1):
        n = max(G, 1)
        V, f, c, xr, fr = np.full((n + 1) * n, 7.0), np.full(n + 1, 7.0), np.full(n, 7.0), np.full(n, 7.0), np.full(1, 7.0)
        st, trial = np.array([1, 7, 7], dtype=np.int32), np.full(n, 7.0)
        for dt in (0, 1):
            assert lib.de_nm_ask_host(G, dt, None, V.ctypes.data, f.ctypes.data, st.ctypes.data, c.ctypes.data, xr.ctypes.data, trial.ctypes.data) == 0
            assert lib.de_nm_tell_host(G, dt, V.ctypes.data, f.ctypes.data, st.ctypes.data, c.ctypes.data, xr.ctypes.data, fr.ctypes.data, 0.5, 1) == 0
        assert all((v == 7.0).all() for v in (V, f, c, xr, fr, trial)) and st.tolist() == [1, 7, 7]
    for G in (0, 33):  # the Python surface: None / False
        s = api.NmState(np.zeros(G), 1.0, np.float32)
        assert api.nm_ask_host(s) is None and api.nm_tell_host(s, 0.5) is False


def test_a_start_whose_loss_is_not_finite_is_stored_as_inf_and_recovers():
    """f[0] = +Inf (the start overflowed, say): the simplex is built, the first finite trial becomes the accepted vertex."""
    obj = bowl(2)
    m = Model([0.5, 0.5], math.nan, np.float64)
    s = api.NmState([0.5, 0.5], math.nan, np.float64)
    assert s.f[0] == INF and state_bits(s) == model_bits(m)
    for r in range(40):
        want = m.ask()
        assert api.nm_ask_host(s).tolist() == want
        F, _ = obj(want)
        api.nm_tell_host(s, F)
        m.tell(F)
        assert state_bits(s) == model_bits(m)
        assert math.isfinite(s.f[s.best])


# ---- 4. a stand-alone program under the sanitizers -------------------------------------------------------------------------------------------
MAIN = r"""
#include <cstdio>
#include <vector>
#include "de_nm.h"
// For G = 1, 2, 9, 32 and both element types: 150 rounds on sum_j (1 + j / 2) (x_j - (0.3 j - 1))^2 from x_j = 0.7 + 0.11 j, the state in
// vectors of exactly the documented sizes (a sanitizer sees any overrun).  Prints the bit patterns of V and f.
template <typename T> static void run(int G) {
    std::vector<double> V((size_t)(G + 1) * G, 0.0), f((size_t)G + 1, de::nm_inf()), c((size_t)G, 0.0), xr((size_t)G, 0.0);
    std::vector<T> trial((size_t)G);
    int32_t st[3] = {de::NM_BUILD, 1, 0};
    double fr = 0.0;
    auto loss = [&](const T *x) {
        double acc = 0.0;
        for (int j = 0; j < G; j++) {
            const double d = (double)x[j] - (0.3 * j - 1.0);
            acc = acc + (1.0 + 0.5 * j) * (d * d);
        }
        return (double)(T)acc;
    };
    for (int j = 0; j < G; j++) { trial[j] = (T)(0.7 + 0.11 * j); V[j] = (double)trial[j]; }
    f[0] = loss(trial.data());
    for (int r = 0; r < 150; r++) {
        de::nm_ask_tree<T>(G, 0, G, true, 0.025, 0.5, 0.0, V.data(), f.data(), st, c.data(), xr.data(), trial.data());
        de::nm_tell_tree<T>(G, 0, G, true, V.data(), f.data(), st, c.data(), xr.data(), &fr, de::nm_loss(loss(trial.data()), true));
    }
    std::printf("%d", (int)st[0]);
    for (const std::vector<double> *v : {&V, &f})
        for (double d : *v) {
            unsigned long long u;
            __builtin_memcpy(&u, &d, 8);
            std::printf(" %016llx", u);
        }
    std::printf("\n");
}
int main() {
    for (int G : {1, 2, 9, 32}) { run<float>(G); run<double>(G); }
    return 0;
}
"""


def test_the_shared_header_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed (the oracle is built with one)"
    (tmp_path / "main.cpp").write_text(MAIN)
    exe = tmp_path / "nm_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "dynamicexpressions.jl_amd", "csrc"), str(tmp_path / "main.cpp"), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    at = 0
    for G in (1, 2, 9, 32):
        for dtype in (np.float32, np.float64):
            obj = bowl(G)
            x0 = np.array([0.7 + 0.11 * j for j in range(G)], dtype=dtype)
            s = api.NmState(x0, rnd(dtype, obj(x0.astype(np.float64).tolist())[0]), dtype)
            for _ in range(150):
                trial = api.nm_ask_host(s)
                api.nm_tell_host(s, rnd(dtype, obj(trial.astype(np.float64).tolist())[0]))
            words = lines[at].split()
            at += 1
            hexes = [f"{x:016x}" for x in np.concatenate([s.V.reshape(-1), s.f]).view(np.uint64)]
            assert words[0] == str(s.phase) and words[1:] == hexes, (G, dtype)  # the library's bits


# ---- 5. the Python surface -----------------------------------------------------------------------------------------------------------------
def test_python_surface():
    class Touched(Exception):
        pass

    class Dummy:  # any attribute access beyond the dtype refusal would mean the population was looked at before the refusal
        def _refuse_f16(self, what):
            pass

        def __getattr__(self, name):
            raise Touched(name)

    P = api.Population
    nan, inf = float("nan"), float("inf")
    for fit in (P.fit_constants_nm, P.fit_constants_nm_device):
        for kw in (dict(iters=-1), dict(a=nan), dict(a=inf), dict(b=nan), dict(b=-inf), dict(a=0.0, b=0.0), dict(f_tol=-1e-9), dict(f_tol=nan),
                   dict(f_tol=inf), dict(loss="pullback"), dict(loss="huber", loss_param=-1.0)):
            with pytest.raises(ValueError):
                fit(Dummy(), None, None, np.zeros(2), **kw)
        with pytest.raises(KeyError):
            fit(Dummy(), None, None, np.zeros(2), loss="no such kind")
        with pytest.raises(Touched):  # good options go on to the population; the hinge is an objective here
            fit(Dummy(), None, None, np.zeros(2), loss="l1_hinge", a=0.0, b=0.25)

    # nm_fit, the loop itself, on an analytic population: two bowls, a tree without constants and one of 33
    def evaluate(consts):
        c = np.asarray(consts, dtype=np.float64)
        return np.array([bowl(2)(c[0:2].tolist())[0], 4.0, bowl(3)(c[2:5].tolist())[0], 9.0], dtype=np.float32), np.ones(4, dtype=bool)

    installed = []
    c0 = np.concatenate([[0.5, 0.25, 2.0, -1.0, 0.125], np.arange(33.0)]).astype(np.float32)
    hist = []
    consts, lo, ok, improve = api.nm_fit(evaluate, installed.append, c0, [2, 0, 3, 33], np.float32, iters=120, history=hist)
    assert len(hist) == 121 and consts.dtype == lo.dtype == np.float32 and improve.dtype == np.int32
    assert installed[-1].tobytes() == consts.tobytes() and consts[5:].tobytes() == c0[5:].tobytes()
    assert evaluate(consts)[0].tobytes() == lo.tobytes() and hist[-1].tobytes() == lo.astype(np.float64).tobytes()
    assert all((b <= a).all() for a, b in zip(hist, hist[1:])) and improve[1] == improve[3] == 0 and improve[0] > 5 and improve[2] > 5
    assert lo[0] < 1e-6 * hist[0][0] and lo[2] < 1e-6 * hist[0][2] and lo[1] == 4.0 and lo[3] == 9.0
    want, wf, _, _ = model_fit(bowl(2), [0.5, 0.25], np.float32, 120)
    assert consts[:2].astype(np.float64).tolist() == want and float(lo[0]) == wf
