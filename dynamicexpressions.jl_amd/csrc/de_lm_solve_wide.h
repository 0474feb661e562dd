// de_lm_solve_wide.h — the Levenberg-Marquardt step of a tree of 9 .. 32 gradient rows: the arithmetic of de_lm_solve.h
//   A = H + lam diag(diag H),  b = -g / 2,  A = L L^T (Cholesky, no pivoting, pivot d = A_jj - sum_k L_jk^2),  delta = A^-1 b
// without the padding to 8 x 8: the matrix lives in a caller-supplied work array (LDS on the device, the stack on the host), row i at
// a + i * LMW_LD.  Every sum runs over k ascending from 0.0, one product at a time (s = s + p q): the summation order of lm_solve8, so a
// system of G <= 8 rows gets lm_solve8's bits (the identity padding never enters rows < G).  Plain C++: the row primitives below are the
// only arithmetic, and both sides call them — de_lm_step_wide_kernel (de_gn_wide.hip) with one lane per row of a column step, the host hook
// de_lm_solve_host_wide (de_api_grad.cpp) through lm_solve_wide with a loop over the rows.  Every translation unit is built with
// -ffp-contract=off; double division and square root are correctly rounded on both sides: the same bits.
#ifndef DE_LM_SOLVE_WIDE_H
#define DE_LM_SOLVE_WIDE_H
#include "de_lm_solve.h"

namespace de {

constexpr int LM_WIDE_MAX_ROWS = 32;            // = DE_GN_WIDE_MAX_ROWS (de_gn_wide.h)
constexpr int LMW_LD = LM_WIDE_MAX_ROWS + 1;    // doubles between two rows of the work matrix (odd: a column walk changes LDS bank every row)
constexpr int LMW_WORK = LM_WIDE_MAX_ROWS * LMW_LD; // doubles of the work matrix

// sum_{k < n} p[k] q[k], k ascending
DE_LM_HD double lmw_dot(const double *p, const double *q, int n) {
    double s = 0.0;
    for (int k = 0; k < n; k++) s = s + p[k] * q[k];
    return s;
}
// sum_{i < k < G} a[k][i] b[k], k ascending (the back substitution walks a column of L)
DE_LM_HD double lmw_dot_col(const double *a, int i, const double *b, int G) {
    double s = 0.0;
    for (int k = i + 1; k < G; k++) s = s + a[k * LMW_LD + i] * b[k];
    return s;
}
// Marquardt's scaling of pivot j
DE_LM_HD double lmw_damp(double ajj, double lam) { return ajj + lam * ajj; }
// column step j: the pivot's d, then row i > j of column j given l = sqrt(d)
DE_LM_HD double lmw_pivot(const double *a, int j) { return a[j * LMW_LD + j] - lmw_dot(a + j * LMW_LD, a + j * LMW_LD, j); }
DE_LM_HD double lmw_below(const double *a, int i, int j, double l) { return (a[i * LMW_LD + j] - lmw_dot(a + i * LMW_LD, a + j * LMW_LD, j)) / l; }
// L y = b, then L^T delta = y, in place; returns whether every entry of delta is finite
DE_LM_HD bool lmw_substitute(const double *a, double *b, int G) {
    for (int i = 0; i < G; i++) b[i] = (b[i] - lmw_dot(a + i * LMW_LD, b, i)) / a[i * LMW_LD + i];
    for (int i = G - 1; i >= 0; i--) b[i] = (b[i] - lmw_dot_col(a, i, b, G)) / a[i * LMW_LD + i];
    bool fin = true;
    for (int i = 0; i < G; i++) fin = fin && lm_finite(b[i]);
    return fin;
}

// One system on one thread.  H: column-major G x G, both triangles present (the lower is used, every entry is tested for finiteness);
// g: G entries; a: LMW_WORK doubles of scratch.  Returns 1 and the step in x[0 .. G), or 0 and x[0 .. G) = 0: G outside 1 .. 32, lam / an
// entry of H, g or the step not finite, or a pivot with !(d > 0).
template <typename T>
DE_LM_HD int lm_solve_wide(int G, const T *H, const T *g, double lam, double *x, double *a) {
    if (G <= 0 || G > LM_WIDE_MAX_ROWS) return 0;
    for (int k = 0; k < G; k++) x[k] = 0.0;
    if (!lm_finite(lam)) return 0;
    bool fin = true;
    for (int j = 0; j < G; j++)
        for (int i = 0; i < G; i++) {
            const double v = (double)H[i + G * j];
            fin = fin && lm_finite(v);
            a[i * LMW_LD + j] = v;
        }
    double b[LM_WIDE_MAX_ROWS];
    for (int i = 0; i < G; i++) {
        b[i] = -0.5 * (double)g[i];
        fin = fin && lm_finite(b[i]);
    }
    if (!fin) return 0;
    for (int j = 0; j < G; j++) a[j * LMW_LD + j] = lmw_damp(a[j * LMW_LD + j], lam);
    for (int j = 0; j < G; j++) {
        const double d = lmw_pivot(a, j);
        if (!(d > 0.0)) return 0;
        const double l = sqrt(d);
        a[j * LMW_LD + j] = l;
        for (int i = j + 1; i < G; i++) a[i * LMW_LD + j] = lmw_below(a, i, j, l);
    }
    if (!lmw_substitute(a, b, G)) return 0;
    for (int i = 0; i < G; i++) x[i] = b[i];
    return 1;
}

} // namespace de
#endif
