// de_fit_scaled.h — the objective of the matrix-free fits under Keijzer's linear scaling a + b * yhat, one source for
// both sides: de_fit_scaled_objective_kernel (de_fit_scaled.hip) and the host-only hook de_scaled_objective_host (de_api_fit.cpp) run this
// code, so they give the same bits (every translation unit is built with -ffp-contract=off; double division is correctly rounded on both
// sides).  From a tree's statistics stats = (mean_p, M2_p, C), ystats = (W, mean_y, M2_y) and moments D | P | Q (G doubles each; D is not
// read) it forms, in double and in exactly this association (FitStats.scaled_sse and FitStatsGrad.scaled_sse_grad written out):
//   sse = lm_scaled_sse (de_lm_project.h): M2_y - (C * C) / M2_p, a NaN THE quiet NaN
//   b   = C / M2_p
//   g_k = (2 * b) * (b * P_k - Q_k)                                  lm_project's g, entry by entry
// M2_p == 0 or W == 0: sse = M2_y (NaN where C is NaN), g = 0, "not formed".  NaN statistics (an incomplete tree) propagate.  No matrix is
// read or formed, so G has no limit of its own: the limit is that of the optimiser that reads g.
#ifndef DE_FIT_SCALED_H
#define DE_FIT_SCALED_H
#include "de_lm_project.h"

namespace de {

constexpr int FIT_SCALED_MAX_ROWS = 32; // = BFGS_MAX_ROWS: the widest tree de_scaled_objective_host forms the gradient of

// whether a gradient is formed from these statistics (a NaN compares false: formed, and it propagates)
DE_LM_HD bool fit_scaled_formed(double m2p, double W) { return !(m2p == 0.0 || W == 0.0); }
DE_LM_HD double fit_scaled_slope(double m2p, double cov) { return cov / m2p; }
// g_k from b, tb = 2 * b and the entry's P_k and Q_k
DE_LM_HD double fit_scaled_grad_entry(double b, double tb, double P, double Q) { return tb * (b * P - Q); }

// One tree on one thread.  dmom: the tree's D | P | Q (3 G doubles, de_eval_fit_stats_grad's layout).  *sse and g[0 .. G) are written;
// returns 1 (formed) or 0 (g = 0).
DE_LM_HD int fit_scaled_objective(int G, const double *stats, const double *ystats, const double *dmom, double *sse, double *g) {
    const double m2p = stats[1], cov = stats[2], W = ystats[0];
    *sse = lm_scaled_sse(m2p, cov, W, ystats[2]);
    if (!fit_scaled_formed(m2p, W)) {
        for (int k = 0; k < G; k++) g[k] = 0.0;
        return 0;
    }
    const double b = fit_scaled_slope(m2p, cov), tb = 2.0 * b;
    for (int k = 0; k < G; k++) g[k] = fit_scaled_grad_entry(b, tb, dmom[G + k], dmom[2 * G + k]);
    return 1;
}

} // namespace de
#endif
