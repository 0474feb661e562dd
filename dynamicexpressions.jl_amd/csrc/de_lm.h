// de_lm.h — launchers of de_lm.hip: the device side of de_gn_lm_step / de_fit_consts_lm.
#ifndef DE_LM_H
#define DE_LM_H
#include <hip/hip_runtime.h>
#include <cstdint>

namespace de {

// One thread per tree: step[doff[t] .. + n_grad[t]) = the Levenberg-Marquardt step of the tree (de_lm_solve.h lm_solve8), or zeros.
// dloss / jtj: the element type `dtype`, at doff[t] / joff[t] (column-major n_grad[t]^2 block).  consts / trial (may both be null): the
// element type, tree t at coff[t]: trial = T(double(consts) + step) where a step was produced, else the bits of consts.
struct LmStepArgs {
    int64_t n_trees;
    const int32_t *n_grad;
    const int64_t *doff, *joff;
    const void *dloss, *jtj;
    const uint8_t *has;
    const double *lam;
    double *step;
    const int64_t *coff;
    const void *consts;
    void *trial;
};
hipError_t launch_lm_step(int dtype, const LmStepArgs &a, hipStream_t stream);

// One thread per tree: the accept rule of Population.fit_constants_lm.  *_acc: the accepted state, *_trial: the evaluation at the trial
// constants; ok and G <= row_limit make `has` (8: de_fit_consts_lm, 32: de_fit_consts_lm_wide).  history_row / n_accept may be null.
struct LmAcceptArgs {
    int64_t n_trees;
    const int32_t *n_grad;
    const int64_t *doff, *joff, *coff;
    void *consts_acc, *loss_acc, *dloss_acc, *jtj_acc;
    uint8_t *ok_acc;
    const void *consts_trial, *loss_trial, *dloss_trial, *jtj_trial;
    const uint8_t *ok_trial;
    double *lam;
    double up, down, lam_min;
    double *history_row; // n_trees entries: the accepted losses after this iteration
    int32_t *n_accept;
    int32_t row_limit;
};
hipError_t launch_lm_accept(int dtype, const LmAcceptArgs &a, hipStream_t stream);

// lam[t] = lam0 and n_accept[t] = 0 (either may be null)
hipError_t launch_lm_init(int64_t n_trees, double lam0, double *lam, int32_t *n_accept, hipStream_t stream);
// row[t] = double(loss[t])
hipError_t launch_lm_history(int dtype, const void *loss, int64_t n_trees, double *row, hipStream_t stream);

} // namespace de
#endif
