"""CPU tests of the wide Gauss-Newton route (include/de_hip.h de_eval_loss_gn_wide / de_lm_solve_host_wide / de_gn_lm_step_wide /
de_fit_consts_lm_wide): the declarations, and the arithmetic of the wide Levenberg-Marquardt step — the host-only hook
runs csrc/de_lm_solve_wide.h, the code de_lm_step_wide_kernel runs: a Cholesky solve of  A delta = -g / 2,  A = H + lam diag(diag H), in
float64 for G up to 32.

    G <= 8     the bytes of de_lm_solve_host on the systems of tests/test_lm_host.py
    G > 8      |delta - delta_np| <= 8 G^2 u cond_2(A) |delta_np|, u = 2^-53 (that file's forward bound), for cond_2(A) < 10^12, lam >= 1e-3
    zero step  G = 0, G = 33, a non-finite entry, a non-finite lam, a rank-deficient H with lam = 0

The header is plain C++: a stand-alone program around it is also built with -fsanitize=address,undefined on the host and run at G = 32;
its steps are the library's bit for bit."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from dynamicexpressions_jl_amd import api
import test_lm_host as LMH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53


def spd(G, seed):
    """H = B B^T + I and a gradient, seeded; both triangles present, exactly symmetric."""
    g = np.random.default_rng(seed)
    B = g.standard_normal((G, G + 3)) * np.exp(g.uniform(-2.0, 2.0, (G, 1)))
    H = B @ B.T + np.eye(G)
    H = np.tril(H) + np.tril(H, -1).T
    return H, g.standard_normal(G) * 3.0


def test_declarations_and_limits():
    lib = api.library()
    assert lib.de_gn_wide_max_rows() == 32 == api.GN_WIDE_MAX_ROWS
    assert lib.de_gn_max_rows() == 8 == api.GN_MAX_ROWS and lib.de_abi_version() == 3 == api.ABI_VERSION
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "de_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+DE_HIP_ABI_VERSION\s+3\b", src)
    for name, twin, n_args in (("de_eval_loss_gn_wide", "de_eval_loss_gn_ex", 17), ("de_lm_solve_host_wide", "de_lm_solve_host", 5),
                               ("de_gn_lm_step_wide", "de_gn_lm_step", 11), ("de_fit_consts_lm_wide", "de_fit_consts_lm_ex", 15)):
        m, m2 = (re.search(r"^int %s\(([^;]*)\);" % n, src, re.M) for n in (name, twin))
        assert m and m2, f"include/de_hip.h declares {name}"
        norm = lambda a: [re.sub(r"\s+", " ", x).strip() for x in a.split(",")]
        assert norm(m.group(1)) == norm(m2.group(1)) and len(norm(m.group(1))) == n_args  # the twin's argument list
        assert len(getattr(lib, name).argtypes) == n_args and name in api.EXPORTS
    assert re.search(r"^int de_gn_wide_max_rows\(void\);", src, re.M) and "de_gn_wide_max_rows" in api.EXPORTS


@pytest.mark.parametrize("seed", range(3))
def test_narrow_systems_get_the_bytes_of_de_lm_solve_host(seed):
    n = 0
    for G, N, dtype, H, grad in LMH.draw(seed):
        for lam in (0.0, 1e-3, 1.0, 1e3):
            a, pa = api.lm_solve_host(H, grad, lam)
            b, pb = api.lm_solve_host_wide(H, grad, lam)
            assert pa == pb and a.tobytes() == b.tobytes(), (G, N, dtype, lam)
            n += 1
    assert n == 8 * 2 * 2 * 4


@pytest.mark.parametrize("G", [9, 16, 31, 32])
def test_forward_bound_on_wide_systems(G):
    worst, n = 0.0, 0
    for seed in range(6):
        H, grad = spd(G, 100 * G + seed)
        for lam in (1e-3, 1.0, 1e3):
            step, produced = api.lm_solve_host_wide(H, grad, lam)
            A = LMH.damped(H, lam)
            assert produced == LMH.cholesky_pivots_positive(A) and produced
            cond = np.linalg.cond(A, 2)
            assert cond < 1e12
            ref = np.linalg.solve(A, -0.5 * grad)
            err, fb = np.linalg.norm(step - ref), 8 * G * G * U64 * cond * np.linalg.norm(ref)
            assert err <= fb, (G, seed, lam, err / fb)
            worst, n = max(worst, err / fb), n + 1
    print(f"[lm host wide] G = {G}: worst forward error {worst:.3g} of the bound over {n} systems")
    assert n == 18


def test_zero_step_cases():
    lib = api.library()
    assert lib.de_lm_solve_host_wide(0, None, None, 1e-3, None) == 0
    H33, g33, s33 = np.asfortranarray(np.eye(33)), np.ones(33), np.full(33, 7.0)
    assert lib.de_lm_solve_host_wide(33, H33.ctypes.data, g33.ctypes.data, 1e-3, s33.ctypes.data) == 0 and not s33.any()
    for G in (9, 32):
        H, grad = spd(G, G)
        step, produced = api.lm_solve_host_wide(H, grad, 1e-3)
        assert produced and step.any() and np.isfinite(step).all()
        for i, k, v in ((0, 0, np.nan), (G - 1, 2, np.inf), (1, G - 1, -np.inf)):  # either triangle: every entry is tested
            Hb = H.copy()
            Hb[i, k] = v
            step, produced = api.lm_solve_host_wide(Hb, grad, 1e-3)
            assert not produced and step.shape == (G,) and not step.any()
        gb = grad.copy()
        gb[G - 1] = np.nan
        for Hc, gc, lam in ((H, gb, 1e-3), (H, grad, np.inf), (H, grad, np.nan), (-H, grad, 1e-3)):
            step, produced = api.lm_solve_host_wide(Hc, gc, lam)
            assert not produced and not step.any()
        # one repeated row of ones over 64 samples: sqrt(64) and 64 / 8 are exact, the second pivot is exactly 0
        ones = np.full((G, G), 64.0)
        step, produced = api.lm_solve_host_wide(ones, grad, 0.0)
        assert not produced and not step.any() and not LMH.cholesky_pivots_positive(ones)
        step, produced = api.lm_solve_host_wide(ones, grad, 0.5)  # ... and the damped system is regular
        assert produced and np.allclose(LMH.damped(ones, 0.5) @ step, -0.5 * grad, rtol=1e-10)


MAIN = r"""
#include <cstdio>
#include <vector>
#include "de_lm_solve_wide.h"
// argv[1]: G, lam, then H (G * G doubles, column-major) and g (G doubles), raw.  Prints the return value and the step's bit patterns.
template <typename T> static int run(int G, double lam, const std::vector<double> &H, const std::vector<double> &g) {
    std::vector<T> Ht(H.begin(), H.end()), gt(g.begin(), g.end());
    std::vector<double> x((size_t)G), work((size_t)de::LMW_WORK);  // exactly the documented sizes: a sanitizer sees any overrun
    const int rc = de::lm_solve_wide<T>(G, Ht.data(), gt.data(), lam, x.data(), work.data());
    std::printf("%d", rc);
    for (int k = 0; k < G; k++) {
        unsigned long long u;
        __builtin_memcpy(&u, &x[(size_t)k], 8);
        std::printf(" %016llx", u);
    }
    std::printf("\n");
    return rc;
}
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    double head[2];
    if (std::fread(head, 8, 2, f) != 2) return 2;
    const int G = (int)head[0];
    std::vector<double> H((size_t)G * G), g((size_t)G);
    if (std::fread(H.data(), 8, H.size(), f) != H.size() || std::fread(g.data(), 8, g.size(), f) != g.size()) return 2;
    std::fclose(f);
    run<double>(G, head[1], H, g);
    run<float>(G, head[1], H, g);
    return 0;
}
"""


def test_the_shared_header_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed (the oracle is built with one)"
    (tmp_path / "main.cpp").write_text(MAIN)
    exe = tmp_path / "lm_solve_wide_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "dynamicexpressions.jl_amd", "csrc"), str(tmp_path / "main.cpp"), "-o", str(exe)], check=True)
    G = 32
    H, grad = spd(G, 7)
    singular = np.full((G, G), 64.0)
    for name, Hm, lam, want in (("regular", H, 1e-3, True), ("singular", singular, 0.0, False)):
        path = tmp_path / f"{name}.bin"
        path.write_bytes(struct.pack("2d", float(G), lam) + np.asfortranarray(Hm).tobytes(order="F") + grad.tobytes())
        out = subprocess.run([str(exe), str(path)], check=True, capture_output=True, text=True).stdout.split("\n")
        f64, f32 = out[0].split(), out[1].split()
        assert (f64[0] == "1") == want and (f32[0] == "1") == want
        step, produced = api.lm_solve_host_wide(Hm, grad, lam)
        assert produced == want and [f"{v:016x}" for v in step.view(np.uint64)] == f64[1:]  # the library's bits
        # the Float32 instantiation: the system rounded to float32, solved in double
        s32, p32 = api.lm_solve_host_wide(Hm.astype(np.float32).astype(np.float64), grad.astype(np.float32).astype(np.float64), lam)
        assert p32 == want and [f"{v:016x}" for v in s32.view(np.uint64)] == f32[1:]
