// de_lm_solve.h — the per-tree arithmetic of the device-side Levenberg-Marquardt step, one function for both sides:
// de_lm_step_kernel (de_lm.hip) and the host-only hook de_lm_solve_host (de_api_grad.cpp) run this code, so they give the same bits
// (every translation unit is built with -ffp-contract=off; double division and square root are correctly rounded on both sides).
//   A = H + lam diag(diag H),  b = -g / 2,  A = L L^T (Cholesky, no pivoting, pivot d = A_jj - sum_k L_jk^2),  delta = A^-1 b
// The G x G system is padded to 8 x 8 with the identity and every loop is fully unrolled: all subscripts are compile-time constants,
// so on the device the matrix lives in registers (no private memory, no dynamically indexed register array).
#ifndef DE_LM_SOLVE_H
#define DE_LM_SOLVE_H
#include <cmath>

#if defined(__HIPCC__) || defined(__HIP__)
#define DE_LM_HD __host__ __device__ __forceinline__
#else
#define DE_LM_HD inline
#endif

namespace de {

constexpr int LM_MAX_ROWS = 8; // = DE_GN_MAX_ROWS (de_kernels.h): the widest tree de_eval_loss_gn forms the matrix of

DE_LM_HD bool lm_finite(double v) { return v - v == 0.0; } // (false for NaN and +-inf; the same instruction sequence on both sides)

// H: column-major G x G, both triangles present (the lower is used, every entry is tested for finiteness); g: G entries.
// Returns 1 and the step in x[0 .. G) (x[G .. 8) = 0), or 0 and x = 0: G outside 1 .. 8, lam / an entry of H, g or the step not
// finite, or a pivot with !(d > 0).
template <typename T>
DE_LM_HD int lm_solve8(int G, const T *H, const T *g, double lam, double (&x)[LM_MAX_ROWS]) {
    constexpr int M = LM_MAX_ROWS;
#pragma unroll
    for (int k = 0; k < M; k++) x[k] = 0.0;
    if (G <= 0 || G > M || !lm_finite(lam)) return 0;
    double a[M][M], b[M];
    bool fin = true;
#pragma unroll
    for (int j = 0; j < M; j++) {
#pragma unroll
        for (int i = 0; i < M; i++) {
            double v = i == j ? 1.0 : 0.0;
            if (i < G && j < G) v = (double)H[i + G * j];
            fin = fin && lm_finite(v);
            a[i][j] = v;
        }
    }
#pragma unroll
    for (int i = 0; i < M; i++) {
        double v = 0.0;
        if (i < G) v = -0.5 * (double)g[i];
        fin = fin && lm_finite(v);
        b[i] = v;
    }
    if (!fin) return 0;
#pragma unroll
    for (int j = 0; j < M; j++)
        if (j < G) a[j][j] = a[j][j] + lam * a[j][j]; // Marquardt's scaling
    bool pos = true;
#pragma unroll
    for (int j = 0; j < M; j++) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < j; k++) s = s + a[j][k] * a[j][k];
        const double d = a[j][j] - s;
        pos = pos && (d > 0.0);
        const double l = sqrt(d);
        a[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < M; i++) {
            double r = 0.0;
#pragma unroll
            for (int k = 0; k < j; k++) r = r + a[i][k] * a[j][k];
            a[i][j] = (a[i][j] - r) / l;
        }
    }
    if (!pos) return 0;
#pragma unroll
    for (int i = 0; i < M; i++) { // L y = b
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < i; k++) s = s + a[i][k] * b[k];
        b[i] = (b[i] - s) / a[i][i];
    }
#pragma unroll
    for (int i = M - 1; i >= 0; i--) { // L^T delta = y
        double s = 0.0;
#pragma unroll
        for (int k = i + 1; k < M; k++) s = s + a[k][i] * b[k];
        b[i] = (b[i] - s) / a[i][i];
    }
    fin = true;
#pragma unroll
    for (int i = 0; i < M; i++) fin = fin && lm_finite(b[i]);
    if (!fin) return 0;
#pragma unroll
    for (int i = 0; i < M; i++) x[i] = b[i];
    return 1;
}

} // namespace de
#endif
