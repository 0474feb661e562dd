// de_bfgs.h — the per-tree arithmetic of the device-side BFGS fit, one source for both sides: the kernels of
// de_bfgs.hip and the host-only hooks de_bfgs_direction_host / de_bfgs_update_host (de_api_grad.cpp) run this code, so they give the same
// bits (every translation unit is built with -ffp-contract=off; double division and square root are correctly rounded on both sides).
//   B: the inverse-Hessian approximation of one tree, G x G doubles, row-major (exactly symmetric), 1 <= G <= 32
//   direction  p = -B g, slope = g . p; !(slope < 0): B = I, fresh = 1, p = -g, slope = -g . g, alpha = a0(g)
//   update     s = c_trial - c, yv = g_trial - g, only where s . yv > curv |s| |yv|; from a fresh state B = (s . yv / yv . yv) I first;
//              u = B yv, B_ik += (s.yv + yv.u) / (s.yv)^2 s_i s_k - (u_i s_k + s_i u_k) / s.yv
// Everything is in double.  Every sum runs over k ascending from 0.0, one product at a time (s = s + p q).  The row primitives below are
// the only arithmetic: the kernels call them with one lane per row of B, bfgs_direction / bfgs_update with a loop over the rows.
#ifndef DE_BFGS_H
#define DE_BFGS_H
#include "de_lm_solve.h"

namespace de {

constexpr int BFGS_MAX_ROWS = 32; // the widest tree that is fitted

// sum_{k < n} p[k] q[k], k ascending
DE_LM_HD double bfgs_dot(const double *p, const double *q, int n) {
    double s = 0.0;
    for (int k = 0; k < n; k++) s = s + p[k] * q[k];
    return s;
}
// the first trial step's length: a0 = |g| > step0 ? step0 / |g| : 1, from gg = g . g (a NaN norm compares false: 1)
DE_LM_HD double bfgs_a0(double gg, double step0) {
    const double n = sqrt(gg);
    return n > step0 ? step0 / n : 1.0;
}
DE_LM_HD bool bfgs_row_finite(const double *row, int G) {
    bool fin = true;
    for (int k = 0; k < G; k++) fin = fin && lm_finite(row[k]);
    return fin;
}
// p_i of row i of B
DE_LM_HD double bfgs_dir_row(const double *row, const double *g, int G) { return -bfgs_dot(row, g, G); }
DE_LM_HD void bfgs_identity_row(double *row, int i, int G, double d) {
    for (int k = 0; k < G; k++) row[k] = k == i ? d : 0.0;
}
// whether the pair (s, yv) has enough curvature for an update (a NaN compares false)
DE_LM_HD bool bfgs_curvature(double sy, double ss, double yy, double curv) {
    return lm_finite(sy) && lm_finite(ss) && lm_finite(yy) && sy > curv * sqrt(ss) * sqrt(yy);
}
DE_LM_HD double bfgs_coef(double sy, double yBy) { return (sy + yBy) / (sy * sy); }
// row i of the rank-two update, given u = B yv (of the B before the update)
DE_LM_HD void bfgs_update_row(double *row, int i, int G, const double *s, const double *u, double coef, double sy) {
    for (int k = 0; k < G; k++) row[k] = row[k] + (coef * (s[i] * s[k]) - (u[i] * s[k] + s[i] * u[k]) / sy);
}
// the trial constant of one entry, and the Armijo test of the accept rule
DE_LM_HD double bfgs_trial(double c, double alpha, double p) { return c + alpha * p; }
DE_LM_HD bool bfgs_armijo(double f_trial, double f, double c1, double alpha, double slope) {
    return lm_finite(f_trial) && f_trial < f && f_trial <= f + (c1 * alpha) * slope;
}

// One tree on one thread.  Returns `produced` (1: p is a descent direction of slope *slope < 0; 0: p = 0 — G outside 1 .. 32, an entry of g
// or B not finite, or g = 0).  B, *fresh and *alpha are reset as described above where the quasi-Newton direction is no descent direction.
// G outside 1 .. 32: nothing is read or written.
DE_LM_HD int bfgs_direction(int G, double *B, unsigned char *fresh, double *alpha, const double *g, double step0, double *p, double *slope) {
    if (G < 1 || G > BFGS_MAX_ROWS) return 0;
    bool fin = bfgs_row_finite(g, G);
    for (int i = 0; i < G; i++) {
        fin = fin && bfgs_row_finite(B + i * G, G);
        p[i] = bfgs_dir_row(B + i * G, g, G);
    }
    double sl = bfgs_dot(g, p, G);
    if (!(sl < 0.0)) {
        const double gg = bfgs_dot(g, g, G);
        for (int i = 0; i < G; i++) {
            bfgs_identity_row(B + i * G, i, G, 1.0);
            p[i] = -g[i];
        }
        *fresh = 1;
        *alpha = bfgs_a0(gg, step0);
        sl = -gg;
    }
    const int produced = fin && sl < 0.0 ? 1 : 0;
    if (!produced)
        for (int i = 0; i < G; i++) p[i] = 0.0;
    *slope = sl;
    return produced;
}

// Returns `updated`; otherwise B and *fresh are unchanged.
DE_LM_HD int bfgs_update(int G, double *B, unsigned char *fresh, const double *s, const double *yv, double curv) {
    if (G < 1 || G > BFGS_MAX_ROWS) return 0;
    const double sy = bfgs_dot(s, yv, G), ss = bfgs_dot(s, s, G), yy = bfgs_dot(yv, yv, G);
    if (!bfgs_curvature(sy, ss, yy, curv)) return 0;
    if (*fresh) {
        const double d = sy / yy;
        for (int i = 0; i < G; i++) bfgs_identity_row(B + i * G, i, G, d);
        *fresh = 0;
    }
    double u[BFGS_MAX_ROWS];
    for (int i = 0; i < G; i++) u[i] = bfgs_dot(B + i * G, yv, G);
    const double coef = bfgs_coef(sy, bfgs_dot(yv, u, G));
    for (int i = 0; i < G; i++) bfgs_update_row(B + i * G, i, G, s, u, coef, sy);
    return 1;
}

} // namespace de
#endif
