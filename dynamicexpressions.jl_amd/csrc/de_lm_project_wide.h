// de_lm_project_wide.h — de_lm_project.h's arithmetic at a run-time width of 9 .. 32 rows: the system of a
// Levenberg-Marquardt step under Keijzer's linear scaling, from what de_eval_fit_stats_grad_wide returns for a tree,
//   b     = C / M2_p
//   g_k   = (2 * b) * (b * P_k - Q_k)
//   Ht_ik = (b * b) * ((H_ik - (D_i * D_k) / W) - (P_i * P_k) / M2_p)      the lower triangle computed, mirrored
// in double and in exactly de_lm_project.h's association (so a system of G <= 8 rows would get lm_project's bits).  Plain C++: the
// per-tree and per-entry primitives below are the only arithmetic, and both sides call them — de_lm_step_scaled_wide_kernel
// (de_lm_scaled_wide.hip) with the lanes of a wave spread over the entries while it loads H into the LDS work matrix of
// de_lm_solve_wide.h, the host hook de_lm_project_host_wide (de_api_grad.cpp) through lm_project_wide with loops.  Every translation
// unit is built with -ffp-contract=off and double division is correctly rounded on both sides: the same bits.
#ifndef DE_LM_PROJECT_WIDE_H
#define DE_LM_PROJECT_WIDE_H
#include "de_lm_project.h"
#include "de_lm_solve_wide.h"

namespace de {

// what every entry of a tree's system shares
struct LmProjectCoef {
    double b, b2, tb; // C / M2_p, b * b, 2 * b
    double W, m2p;
    int formed;       // 0: M2_p == 0 or W == 0 — g = 0, Ht = 0, nothing below is called
};
DE_LM_HD LmProjectCoef lmpw_coef(double m2p, double cov, double W) {
    LmProjectCoef c;
    c.formed = (m2p == 0.0 || W == 0.0) ? 0 : 1;
    c.b = c.formed ? cov / m2p : 0.0;
    c.b2 = c.b * c.b;
    c.tb = 2.0 * c.b;
    c.W = W;
    c.m2p = m2p;
    return c;
}
// row k of the gradient
DE_LM_HD double lmpw_grad(const LmProjectCoef &c, double Pk, double Qk) { return c.tb * (c.b * Pk - Qk); }
// entry (i, k), i >= k, of the projected matrix from entry h = H_ik
DE_LM_HD double lmpw_entry(const LmProjectCoef &c, double h, double Di, double Dk, double Pi, double Pk) {
    return c.b2 * ((h - (Di * Dk) / c.W) - (Pi * Pk) / c.m2p);
}

// One tree on one thread.  dmom: D | P | Q (3 G doubles); H: column-major G x G doubles, both triangles present (the lower is read);
// g: G entries, Ht: column-major G x G, both triangles written.  Returns 1 (formed) or 0 (g = 0, Ht = 0).  G in 1 .. 32.
DE_LM_HD int lm_project_wide(int G, const double *stats, const double *ystats, const double *dmom, const double *H, double *g, double *Ht) {
    const LmProjectCoef c = lmpw_coef(stats[1], stats[2], ystats[0]);
    const double *D = dmom, *P = dmom + G, *Q = dmom + 2 * G;
    if (!c.formed) {
        for (int k = 0; k < G; k++) g[k] = 0.0;
        for (int k = 0; k < G * G; k++) Ht[k] = 0.0;
        return 0;
    }
    for (int k = 0; k < G; k++) g[k] = lmpw_grad(c, P[k], Q[k]);
    for (int k = 0; k < G; k++)
        for (int i = k; i < G; i++) {
            const double v = lmpw_entry(c, H[i + G * k], D[i], D[k], P[i], P[k]);
            Ht[i + G * k] = v;
            Ht[k + G * i] = v;
        }
    return 1;
}

} // namespace de
#endif
