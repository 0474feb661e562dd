// de_fit_scaled.hip — the device glue of de_fit_consts_bfgs_scaled / de_fit_consts_nm_scaled: between an evaluation
// that returns fit statistics (de_eval_fit_stats_grad without a matrix, de_eval_fit_stats) and the BFGS / Nelder-Mead kernels that read an
// objective and a gradient, without the host seeing either.
//   de_fit_scaled_objective_kernel  sse[t] = scaled_sse of the tree's statistics and, where the moments are given, g = its gradient
// One wave per tree, lane k owns entries k, k + 64, ... of g (the arithmetic: de_fit_scaled.h, the code the host hook runs).  On the
// context's stream, plain vector stores only, no atomics, no LDS.
#include "de_fit_scaled_dev.h"
#include "de_fit_scaled.h"

namespace de {

__global__ void __launch_bounds__(64) de_fit_scaled_objective_kernel(FitScaledArgs a) {
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const double m2p = a.stats[3 * t + 1], cov = a.stats[3 * t + 2], W = a.ystats[0];
    if (lane == 0) a.sse[t] = lm_scaled_sse(m2p, cov, W, a.ystats[2]);
    if (!a.dmom) return; // (uniform)
    const int G = a.n_grad[t];
    double *g = a.grad + a.coff[t];
    if (!fit_scaled_formed(m2p, W)) { // (uniform)
        for (int k = lane; k < G; k += 64) g[k] = 0.0;
        return;
    }
    const double *P = a.dmom + a.moff[t] + G, *Q = P + G;
    const double b = fit_scaled_slope(m2p, cov), tb = 2.0 * b;
    for (int k = lane; k < G; k += 64) g[k] = fit_scaled_grad_entry(b, tb, P[k], Q[k]);
}

hipError_t launch_fit_scaled_objective(const FitScaledArgs &a, hipStream_t stream) {
    if (a.n_trees <= 0) return hipSuccess;
    hipLaunchKernelGGL(de_fit_scaled_objective_kernel, dim3((unsigned)a.n_trees), dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace de
