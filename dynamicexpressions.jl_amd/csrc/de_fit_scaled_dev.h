// de_fit_scaled_dev.h — launcher of de_fit_scaled.hip: the adapter between the fit statistics and the BFGS / Nelder-Mead kernels of
// de_fit_consts_bfgs_scaled / de_fit_consts_nm_scaled.
#ifndef DE_FIT_SCALED_DEV_H
#define DE_FIT_SCALED_DEV_H
#include <hip/hip_runtime.h>
#include <cstdint>

namespace de {

// One wave per tree.  Tree t: its statistics at stats[3 t], the target's at ystats; where dmom is not null its D | P | Q (3 G doubles, G =
// n_grad[t]) at moff[t] and its G gradient slots at coff[t].  sse[t] = the scaled objective; grad[coff[t] + k] = g_k (de_fit_scaled.h).
struct FitScaledArgs {
    int64_t n_trees;
    const int32_t *n_grad;
    const int64_t *moff, *coff;
    const double *stats, *ystats, *dmom; // dmom null (de_fit_consts_nm_scaled): the objective alone
    double *sse, *grad;
};
hipError_t launch_fit_scaled_objective(const FitScaledArgs &a, hipStream_t stream);

} // namespace de
#endif
