"""CPU tests of the scaled Levenberg-Marquardt fit for trees of 9 to 32 constants (include/de_hip.h de_eval_fit_stats_grad_wide /
de_lm_project_host_wide / de_fit_stats_lm_step_wide / de_fit_consts_lm_scaled_wide): the declarations, the arithmetic
of the projection at a run-time width — the host-only hook runs csrc/de_lm_project_wide.h, the code de_lm_step_scaled_wide_kernel runs —
and the Python surface.

    G <= 8     the bytes of de_lm_project_host on the systems of tests/test_lm_scaled_host.py
    G > 8      bit for bit numpy's FitStatsGrad.projected() / FitStats.scaled_sse, both triangles
    the step   lm_solve_host_wide of the hook's system against projected().lm_step:
               |delta - delta_np| <= 8 G^2 u cond_2(A) |delta_np|, u = 2^-53, every system with cond_2(A) < 10^12 (asserted: none exempt)

The header is plain C++: a stand-alone program around it and de_lm_solve_wide.h is also built with -fsanitize=address,undefined on the host
and run at G = 32 and G = 9; its g, Ht and step are the library's bit for bit.

THE RECOVERY SCENARIO (shared with tests/test_gpu_lm_scaled_wide.py): cos_sum(12) = sum_i cos(c_i x_{1 + i mod 3}), c*_i = 0.6 + 0.17 i,
target 2 - 3 tree(c*), N = 513 with a zero-weight tail of 37 samples, start c0 = c* + PERTURB (a ramp of -0.12 .. +0.12 over the twelve
constants) and ITERS = 20 iterations.  Chosen here on the CPU: the numpy emulation below then ends at about 0.06 of the bound in Float64
and far below it in Float32 (whose start lies 10 x above the bound's noise floor), where e.g. an alternating perturbation of the same size
needs more than 80 iterations in Float64.  Four cosines per feature on [-2, 2) are nearly dependent: the valley is narrow and flat, the
objective reaches the bound with the constants still several per cent from c*, so the scenario bounds the objective alone."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from dynamicexpressions_jl_amd import api
import test_fit_stats_grad_host as FSG
import test_lm_scaled_host as LSH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53
WIDTHS = (9, 12, 16, 17, 31, 32)
NAN_BITS = struct.pack("<Q", 0x7FF8000000000000)

# the recovery scenario
K = 12
C_STAR = np.array([0.6 + 0.17 * i for i in range(K)])
PERTURB = 0.12 * (np.arange(K) - 5.5) / 5.5
ITERS = 20


def recovery_data(dtype, seed=11, N=513):
    g = np.random.default_rng(seed)
    x = g.uniform(-2.0, 2.0, (3, N)).astype(dtype)
    w = g.uniform(0.5, 1.5, N).astype(dtype)
    w[-37:] = 0
    y = (2.0 - 3.0 * cos_sum_model(C_STAR.astype(dtype).astype(np.float64), x.astype(np.float64))[0]).astype(dtype)
    return x, y, w


def cos_sum_model(theta, x):
    """yhat = sum_i cos(theta_i x_{i mod 3}) and its Jacobian [K, N]"""
    xs = np.stack([x[i % 3] for i in range(theta.size)])
    a = theta[:, None] * xs
    return np.cos(a).sum(axis=0), -xs * np.sin(a)


def draw_wide(seed):
    """tests/test_lm_scaled_host.py's systems at the wide widths: rows scaled by exp(U(-3, 3)), N in {64, 300}, weights with some zeros,
    H rounded through float32 or float64; has_jtj set (the default of a hand-made FitStatsGrad stops at 8 rows)"""
    g = np.random.default_rng(1000 + seed)
    for G in WIDTHS:
        for N in (64, 300):
            for dtype in (np.float32, np.float64):
                J = g.standard_normal((G, N)) * np.exp(g.uniform(-3.0, 3.0, (G, 1)))
                yh, y = g.standard_normal(N) * 1.5 + 0.3, g.standard_normal(N) - 0.7
                w = g.uniform(0.25, 2.0, N)
                w[g.integers(0, N, N // 8)] = 0.0
                fg = FSG.moments(yh, J, y, w)
                H = fg.jtj[0].astype(dtype).astype(np.float64)
                fg.jtj[0] = np.tril(H) + np.tril(H, -1).T
                fg.has_jtj = np.ones(1, dtype=bool)
                yield G, N, dtype, fg


def hook_wide(fg, t=0):
    st = fg.stats
    D, P, Q = fg._dpq(t)
    return api.lm_project_host_wide([st.mean_p[t], st.m2_p[t], st.cov[t]], [st.W, st.mean_y, st.m2_y], D, P, Q, fg.jtj[t])


# ---- 1. prototypes ---------------------------------------------------------------------------------------------------------------------
def test_prototypes_and_null_contexts():
    raw = open(os.path.join(ROOT, "include", "de_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    lib = api.library()
    norm = lambda a: [re.sub(r"\s+", " ", x).strip() for x in a.split(",")]
    for name, twin, n_args in (("de_eval_fit_stats_grad_wide", "de_eval_fit_stats_grad", 16), ("de_lm_project_host_wide", "de_lm_project_host", 8),
                               ("de_fit_stats_lm_step_wide", "de_fit_stats_lm_step", 14), ("de_fit_consts_lm_scaled_wide", "de_fit_consts_lm_scaled", 15)):
        m, m2 = (re.search(r"^int %s\(([^;]*)\);" % n, src, re.M) for n in (name, twin))
        assert m and m2, f"include/de_hip.h declares {name}"
        assert norm(m.group(1)) == norm(m2.group(1)) and len(norm(m.group(1))) == n_args  # the twin's argument list
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == n_args and name in api.EXPORTS
    assert api.ABI_VERSION == 3 == lib.de_abi_version() and re.search(r"#define\s+DE_HIP_ABI_VERSION\s+3\b", src)
    assert lib.de_gn_max_rows() == 8 and lib.de_gn_wide_max_rows() == 32
    assert re.search(r"\(m\) de_eval_fit_stats_grad_wide", raw)
    # null contexts are refused without a device
    assert lib.de_eval_fit_stats_grad_wide(None, None, None, 0, 0, None, 1, None, None, None, None, None, None, None, None, None) == 1
    assert lib.de_fit_stats_lm_step_wide(None, 0, 1, None, None, None, None, None, None, None, None, None, None, None) == 1
    assert lib.de_fit_consts_lm_scaled_wide(None, None, None, 0, 0, None, None, None, None, None, None, None, None, None, None) == 1


# ---- 2. the hook -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(3))
def test_narrow_systems_get_the_bytes_of_de_lm_project_host(seed):
    n = 0
    for G, N, dtype, fg in LSH.draw(seed):
        a, b = LSH.hook(fg), hook_wide(fg)
        assert np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes() and a[3] == b[3]
        assert a[1].tobytes() == b[1].tobytes() and np.ascontiguousarray(a[2]).tobytes() == np.ascontiguousarray(b[2]).tobytes(), (G, N, dtype)
        n += 1
    assert n == 8 * 2 * 2


@pytest.mark.parametrize("seed", range(2))
def test_wide_systems_bit_equal_to_numpy_and_forward_bound(seed):
    worst, n = 0.0, 0
    for G, N, dtype, fg in draw_wide(seed):
        gn = fg.projected()
        sse, g, Ht, formed = hook_wide(fg)
        assert formed, (G, N, dtype)
        assert np.float64(sse).tobytes() == np.float64(fg.stats.scaled_sse[0]).tobytes() == np.float64(gn.loss[0]).tobytes()
        assert g.tobytes() == fg.scaled_sse_grad()[0].tobytes() == np.asarray(gn.grad[0]).tobytes(), (G, N, dtype)
        assert np.ascontiguousarray(Ht).tobytes() == np.ascontiguousarray(gn.jtj[0]).tobytes(), (G, N, dtype)  # both triangles
        assert np.array_equal(Ht, Ht.T)
        # ---- 3. the step: lm_solve_host_wide of the hook's system against numpy's solve of projected()'s
        for lam in (1e-3, 1.0, 1e3):
            step, produced = api.lm_solve_host_wide(Ht, g, lam)
            assert produced, (G, N, dtype, lam)
            ref = gn.lm_step(lam, tree=0)
            cond = np.linalg.cond(LSH.damped(gn.jtj[0], lam), 2)  # (numpy's own system)
            assert np.isfinite(cond) and cond < 1e12, (G, N, dtype, lam, cond)  # the generator keeps every system under the cap: none exempt
            err, bound = np.linalg.norm(step - ref), 8 * G * G * U64 * cond * np.linalg.norm(ref)
            assert ref.any() and err <= bound, (G, N, dtype, lam, err, bound)
            worst, n = max(worst, err / bound), n + 1
    assert n == len(WIDTHS) * 2 * 2 * 3
    print(f"[lm scaled wide host] seed {seed}: {n} systems of {WIDTHS} rows bit-equal to projected(); worst forward error {worst:.3g} of the bound")


def test_not_formed_rules_and_limits():
    G = 12
    g0 = np.random.default_rng(3)
    J = g0.standard_normal((G, 80))
    D, P, Q = J.sum(axis=1), J @ g0.standard_normal(80), J @ g0.standard_normal(80)
    H = J @ J.T
    H = np.tril(H) + np.tril(H, -1).T
    ys = [80.0, 0.5, 4.0]
    sse, g, Ht, formed = api.lm_project_host_wide([0.1, 2.0, 1.0], ys, D, P, Q, H)
    assert formed and sse == 4.0 - 1.0 / 2.0 and g.all() and Ht.all()
    # M2_p == 0 (a tree constant over the samples) and W == 0: not formed, zeros, sse = M2_y — or NaN where C is NaN
    for st, y3, want in (([3.0, 0.0, 0.0], ys, 4.0), ([3.0, 0.0, np.nan], ys, np.nan), ([np.nan, 0.0, 0.0], [0.0, np.nan, 0.0], 0.0),
                         ([np.nan, 2.0, 1.0], [0.0, np.nan, 4.0], 4.0)):
        sse, g, Ht, formed = api.lm_project_host_wide(st, y3, D, P, Q, H)
        assert not formed and not g.any() and not Ht.any() and (sse == want or (np.isnan(want) and np.isnan(sse))), (st, y3)
        if np.isnan(want):
            assert np.float64(sse).tobytes() == NAN_BITS  # THE quiet NaN
        step, produced = api.lm_solve_host_wide(Ht, g, 1e-3)
        assert not produced and not step.any()
    # ... as projected() has it
    fg = api.FitStatsGrad(api.FitStats([3.0], [0.0], [0.0], *ys), [D], [P], [Q], [H], np.ones(1, dtype=bool), np.ones(1, dtype=bool))
    gn = fg.projected()
    assert gn.loss[0] == 4.0 and not gn.grad[0].any() and not gn.jtj[0].any()
    # NaN statistics (an incomplete tree) propagate, the objective is the canonical NaN (also for a negated NaN operand) and the solve
    # answers the zero step
    nan = np.nan
    for c in (nan, -nan, np.float64(np.frombuffer(struct.pack("<Q", 0xFFF8000000000123), dtype=np.float64)[0])):
        sse, g, Ht, formed = api.lm_project_host_wide([nan, c, c], ys, D * nan, P * nan, Q * nan, H * nan)
        assert np.float64(sse).tobytes() == NAN_BITS and np.isnan(g).all() and np.isnan(Ht).all()
        step, produced = api.lm_solve_host_wide(Ht, g, 1e-3)
        assert not produced and step.tolist() == [0.0] * G
    Pn = P.copy()
    Pn[G - 1] = nan
    sse, g, Ht, formed = api.lm_project_host_wide([0.1, 2.0, 1.0], ys, D, Pn, Q, H)
    assert formed and not api.lm_solve_host_wide(Ht, g, 1e-3)[1]
    # G = 0, G = 33 (zero-filled), G < 0, null buffers
    lib = api.library()
    st3, ys3, one, sse1 = np.array([0.1, 2.0, 1.0]), np.array(ys), np.full(1, 7.0), np.full(1, 7.0)
    assert lib.de_lm_project_host_wide(0, st3.ctypes.data, ys3.ctypes.data, one.ctypes.data, one.ctypes.data, sse1.ctypes.data, one.ctypes.data,
                                       one.ctypes.data) == 0 and one[0] == 7.0 and sse1[0] == 3.5
    assert lib.de_lm_project_host_wide(-1, st3.ctypes.data, ys3.ctypes.data, one.ctypes.data, one.ctypes.data, sse1.ctypes.data, one.ctypes.data,
                                       one.ctypes.data) == 0 and one[0] == 7.0
    sse, g, Ht, formed = api.lm_project_host_wide([0.1, 2.0, 1.0], ys, np.ones(33), np.ones(33), np.ones(33), np.eye(33))
    assert not formed and g.shape == (33,) and Ht.shape == (33, 33) and not g.any() and not Ht.any() and sse == 3.5
    assert lib.de_lm_project_host_wide(12, None, None, None, None, None, None, None) == 0
    # the widest system is formed
    sse, g, Ht, formed = api.lm_project_host_wide([0.1, 2.0, 1.0], ys, np.ones(32), np.ones(32), np.ones(32), np.eye(32) * 5)
    assert formed and g.all()


# ---- 4. a stand-alone program under the sanitizers ---------------------------------------------------------------------------------------
MAIN = r"""
#include <cstdio>
#include <vector>
#include "de_lm_project_wide.h"
// argv[1]: G, lam, stats[3], ystats[3], then dmom (3 G doubles) and H (G * G doubles, column-major), raw.  Prints `formed` with the bit
// patterns of g and Ht, then the solve's return value with the step's.
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
    double head[8];
    if (std::fread(head, 8, 8, f) != 8) return 2;
    const int G = (int)head[0];
    std::vector<double> dmom((size_t)3 * G), H((size_t)G * G);
    if (std::fread(dmom.data(), 8, dmom.size(), f) != dmom.size() || std::fread(H.data(), 8, H.size(), f) != H.size()) return 2;
    std::fclose(f);
    // exactly the documented sizes: a sanitizer sees any overrun
    std::vector<double> g((size_t)G), Ht((size_t)G * G), x((size_t)G), work((size_t)de::LMW_WORK);
    const int formed = de::lm_project_wide(G, head + 2, head + 5, dmom.data(), H.data(), g.data(), Ht.data());
    std::printf("%d", formed);
    bits(g);
    std::printf("%d", formed);
    bits(Ht);
    const int rc = de::lm_solve_wide<double>(G, Ht.data(), g.data(), head[1], x.data(), work.data());
    std::printf("%d", rc);
    bits(x);
    return 0;
}
"""


def test_the_shared_headers_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed (the oracle is built with one)"
    (tmp_path / "main.cpp").write_text(MAIN)
    exe = tmp_path / "lm_project_wide_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "dynamicexpressions.jl_amd", "csrc"), str(tmp_path / "main.cpp"), "-o", str(exe)], check=True)
    systems = {(G, N): fg for G, N, dtype, fg in draw_wide(5) if dtype == np.float64}
    for G, N, lam in ((32, 64, 1e-3), (9, 300, 1.0)):
        fg = systems[(G, N)]
        st, (D, P, Q) = fg.stats, fg._dpq(0)
        path = tmp_path / f"g{G}.bin"
        path.write_bytes(struct.pack("8d", float(G), lam, st.mean_p[0], st.m2_p[0], st.cov[0], st.W, st.mean_y, st.m2_y) +
                         np.concatenate([D, P, Q]).tobytes() + np.asfortranarray(fg.jtj[0]).tobytes(order="F"))
        out = [line.split() for line in subprocess.run([str(exe), str(path)], check=True, capture_output=True, text=True).stdout.split("\n")[:3]]
        sse, g, Ht, formed = hook_wide(fg)
        step, produced = api.lm_solve_host_wide(Ht, g, lam)
        assert formed and produced and step.any()
        assert out[0][0] == "1" and out[0][1:] == [f"{v:016x}" for v in g.view(np.uint64)]  # the library's bits
        assert out[1][1:] == [f"{v:016x}" for v in np.asfortranarray(Ht).reshape(-1, order="F").view(np.uint64)]
        assert out[2][0] == "1" and out[2][1:] == [f"{v:016x}" for v in step.view(np.uint64)]


# ---- 5. the scaled loop, emulated in numpy with the hook's steps -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_scaled_loop_emulation_driven_by_the_wide_hook_recovers(dtype):
    """tests/test_fit_stats_grad_host.py::test_scaled_lm_loop_emulation_recovers for cos_sum(12), with the step and the objective from
    the wide hooks (what the device loop runs): final scaled_sse <= max(1e-9 initial, 4 * 1024 u m2_y)."""
    x, y, w = recovery_data(dtype)
    u = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53

    def ev(th):
        yh, J = cos_sum_model(th.astype(dtype), x)
        fg = FSG.moments(yh.astype(dtype), J.astype(dtype), y, w)
        fg.jtj[0] = fg.jtj[0].astype(dtype).astype(np.float64)  # (the matrix has the population's element type)
        sse, gr, Ht, formed = hook_wide(fg)
        assert formed
        return fg, sse, gr, Ht

    th = (C_STAR + PERTURB).astype(dtype)
    fg, loss, gr, Ht = ev(th)
    first, lam, m2y, accepted = loss, 1e-3, fg.stats.m2_y, 0
    bound = max(1e-9 * first, 4 * 1024 * u * m2y)
    assert first >= 10 * bound  # the start lies well above what the fit has to reach
    for _ in range(ITERS):
        step, produced = api.lm_solve_host_wide(Ht, gr, lam)
        trial = (th.astype(np.float64) + step).astype(dtype) if produced else th
        fgt, loss_t, gr_t, Ht_t = ev(trial)
        if loss_t < loss:
            th, fg, loss, gr, Ht, lam, accepted = trial, fgt, loss_t, gr_t, Ht_t, max(lam * 0.1, 1e-12), accepted + 1
        else:
            lam *= 10.0
    print(f"{np.dtype(dtype).name}: initial / bound = {first / bound:.3g}, final scaled_sse / bound = {loss / bound:.3g}, {accepted} accepted steps")
    assert loss <= bound, (loss, bound)
    # (no bound on the slope or the constants: four cosines per feature on [-2, 2) are nearly dependent, and the objective reaches
    # 1e-13 m2_y with the constants several per cent from c* and the slope at -3.05 — the narrow recovery case's tolerance on the slope
    # presumes a well-conditioned minimum)
    assert accepted >= 3 and np.isfinite(fg.stats.slope[0])


# ---- 6. the Python surface -------------------------------------------------------------------------------------------------------------
def test_python_surface():
    class Touched(Exception):
        pass

    class Dummy:  # any attribute access would mean the population was looked at before the refusal
        def __getattr__(self, name):
            raise Touched(name)

    with pytest.raises(ValueError, match="scaled") as e:
        api.Population.fit_constants_lm_device(Dummy(), None, None, np.zeros(2), scaled=True, wide=True)
    assert "fit_constants_lm_scaled_device" in str(e.value)  # the message names the method that serves the pair
    with pytest.raises(ValueError, match="scaled"):
        api.Population.fit_constants_lm(Dummy(), None, None, np.zeros(2), scaled=True, wide=True, loss="huber")
    with pytest.raises(Touched):  # scaled and wide is admitted by the host loop
        api.Population.fit_constants_lm(Dummy(), None, None, np.zeros(2), scaled=True, wide=True)

    class Forward:  # wide=False is fit_constants_lm_device(scaled=True), nothing else
        def fit_constants_lm_device(self, *a, **kw):
            self.got = (a, kw)
            return "forwarded"

    f, hist = Forward(), []
    out = api.Population.fit_constants_lm_scaled_device(f, "X", "y", "c0", weights="w", iters=7, lam0=0.5, up=3.0, down=0.25, history=hist)
    assert out == "forwarded" and f.got[0] == ("X", "y", "c0")
    assert f.got[1] == dict(weights="w", iters=7, lam0=0.5, up=3.0, down=0.25, history=hist, params=None, classes=None, class_base=1, scaled=True)
    assert f.got[1]["history"] is hist
    with pytest.raises(ValueError, match="lam_min"):
        api.Population.fit_constants_lm_scaled_device(f, "X", "y", lam_min=1e-9)
    with pytest.raises(Touched):  # wide=True goes on to the population
        api.Population.fit_constants_lm_scaled_device(Dummy(), None, None, np.zeros(2), wide=True)
    assert api.lm_project_host_wide([0.0, 1.0, 0.5], [2.0, 0.0, 1.0], [1.0], [0.5], [0.25], [[2.0]])[3]
