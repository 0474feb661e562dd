// de_lm_project.h — the per-tree arithmetic of a Levenberg-Marquardt step under Keijzer's linear scaling a + b * yhat,
// one function for both sides: de_lm_step_scaled_kernel (de_lm_scaled.hip) and the host-only hook de_lm_project_host (de_api_grad.cpp)
// run this code, so they give the same bits (every translation unit is built with -ffp-contract=off; double division is correctly
// rounded on both sides).  From what de_eval_fit_stats_grad returns for a tree of G <= 8 rows —
//   stats = (mean_p, M2_p, C), ystats = (W, mean_y, M2_y), D, P, Q (G doubles each), H (G x G, the element type, converted to double)
// — it forms, in double and in exactly this association (FitStats.scaled_sse, FitStatsGrad.scaled_sse_grad and .projected() written out):
//   b     = C / M2_p
//   sse   = M2_y - (C * C) / M2_p
//   g_k   = (2 * b) * (b * P_k - Q_k)
//   Ht_ik = (b * b) * ((H_ik - (D_i * D_k) / W) - (P_i * P_k) / M2_p)      the lower triangle computed, mirrored
// M2_p == 0 or W == 0: g = 0, Ht = 0, sse = M2_y (NaN where C is NaN), "not formed".  NaN statistics (an incomplete tree) propagate:
// lm_solve8 then answers the zero step by its non-finite test.
// G is a template argument and every loop is fully unrolled: all subscripts are compile-time constants, so on the device g and Ht live in
// registers and lm_solve8 reads them there (no private memory).
#ifndef DE_LM_PROJECT_H
#define DE_LM_PROJECT_H
#include "de_lm_solve.h"

namespace de {

// the objective of the scaled fit from a tree's statistics alone.  A NaN result is THE quiet NaN 0x7ff8000000000000 on both sides: which
// operand's sign and payload a NaN result takes is the one thing the two instruction sets do not agree on (a negated operand).
DE_LM_HD double lm_scaled_sse(double m2p, double cov, double W, double m2y) {
    const double e = (m2p == 0.0 || W == 0.0) ? (cov != cov ? cov : m2y) : m2y - (cov * cov) / m2p;
    return e != e ? __builtin_nan("") : e;
}

// D, P, Q: G doubles each; H: column-major G x G of HT, both triangles present (the lower is read).  g: G entries, Ht: column-major G x G
// doubles.  Returns 1 (formed) or 0 (not formed: g = 0, Ht = 0).
template <int G, typename HT>
DE_LM_HD int lm_project(double m2p, double cov, double W, const double *D, const double *P, const double *Q, const HT *H,
                        double (&g)[G], double (&Ht)[G * G]) {
    if (m2p == 0.0 || W == 0.0) {
#pragma unroll
        for (int k = 0; k < G; k++) g[k] = 0.0;
#pragma unroll
        for (int k = 0; k < G * G; k++) Ht[k] = 0.0;
        return 0;
    }
    const double b = cov / m2p, b2 = b * b, tb = 2.0 * b;
    double d[G], p[G];
#pragma unroll
    for (int k = 0; k < G; k++) {
        d[k] = D[k];
        p[k] = P[k];
        g[k] = tb * (b * p[k] - Q[k]);
    }
#pragma unroll
    for (int k = 0; k < G; k++) {
#pragma unroll
        for (int i = k; i < G; i++) {
            const double v = b2 * (((double)H[i + G * k] - (d[i] * d[k]) / W) - (p[i] * p[k]) / m2p);
            Ht[i + G * k] = v;
            Ht[k + G * i] = v;
        }
    }
    return 1;
}

// The whole scaled step of one tree of G rows at lam: x = the step (x[G .. 8) = 0), *sse = the objective; returns 1 where a step was
// produced (formed and solved), else 0 and x = 0.  dmom: the tree's D | P | Q (3 G doubles, de_eval_fit_stats_grad's layout).
template <int G, typename HT>
DE_LM_HD int lm_step_scaled(const double *stats, const double *ystats, const double *dmom, const HT *H, double lam, double (&x)[LM_MAX_ROWS],
                            double *sse) {
    const double m2p = stats[1], cov = stats[2], W = ystats[0];
    *sse = lm_scaled_sse(m2p, cov, W, ystats[2]);
    double g[G], Ht[G * G];
    const int formed = lm_project<G, HT>(m2p, cov, W, dmom, dmom + G, dmom + 2 * G, H, g, Ht);
    const int solved = lm_solve8<double>(G, Ht, g, lam, x); // (x = 0 where it answers 0)
    return formed && solved;
}

// lm_project on buffers in memory (the host hook): g[G] and the column-major Ht[G * G] are written through local copies
template <int G>
DE_LM_HD int lm_project_mem(const double *stats, const double *ystats, const double *dmom, const double *H, double *g, double *Ht) {
    double gg[G], hh[G * G];
    const int formed = lm_project<G, double>(stats[1], stats[2], ystats[0], dmom, dmom + G, dmom + 2 * G, H, gg, hh);
    for (int k = 0; k < G; k++) g[k] = gg[k];
    for (int k = 0; k < G * G; k++) Ht[k] = hh[k];
    return formed;
}

// CALL with the constant GG = G_ for a run-time G_ of 1 .. 8 (nothing for any other)
#define DE_LM_FOR_G(G_, CALL)                \
    switch (G_) {                            \
    case 1: { constexpr int GG = 1; CALL; } break; \
    case 2: { constexpr int GG = 2; CALL; } break; \
    case 3: { constexpr int GG = 3; CALL; } break; \
    case 4: { constexpr int GG = 4; CALL; } break; \
    case 5: { constexpr int GG = 5; CALL; } break; \
    case 6: { constexpr int GG = 6; CALL; } break; \
    case 7: { constexpr int GG = 7; CALL; } break; \
    case 8: { constexpr int GG = 8; CALL; } break; \
    default: break;                          \
    }

} // namespace de
#endif
