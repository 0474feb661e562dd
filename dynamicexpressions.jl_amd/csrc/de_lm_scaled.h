// de_lm_scaled.h — launchers of de_lm_scaled.hip: the device side of de_fit_stats_lm_step / de_fit_consts_lm_scaled.
#ifndef DE_LM_SCALED_H
#define DE_LM_SCALED_H
#include <hip/hip_runtime.h>
#include <cstdint>

namespace de {

// One thread per tree: step[soff[t] .. + n_grad[t]) = the Levenberg-Marquardt step of the tree under linear scaling (de_lm_project.h
// lm_step_scaled), or zeros; sse[t] (may be null) = its scaled_sse.  stats: 3 doubles per tree, ystats: 3 doubles; dmom: D | P | Q of
// tree t at moff[t] (3 n_grad[t] doubles); jtj: the element type `dtype`, the column-major block of tree t at joff[t].  consts / trial
// (may both be null): the element type, tree t at soff[t]: trial = T(double(consts) + step) where a step was produced, else the bits of
// consts.
struct LmScaledStepArgs {
    int64_t n_trees;
    const int32_t *n_grad;
    const int64_t *moff, *joff, *soff;
    const double *stats, *ystats, *dmom;
    const void *jtj;
    const uint8_t *has;
    const double *lam;
    double *step, *sse;
    const void *consts;
    void *trial;
};
hipError_t launch_lm_step_scaled(int dtype, const LmScaledStepArgs &a, hipStream_t stream);
// One wave per tree with 8 < n_grad <= 32 (de_lm_scaled_wide.hip): the same contract with the projection of de_lm_project_wide.h folded
// into the load of the matrix and lm_solve_wide's arithmetic (de_lm_solve_wide.h); every other tree is left alone (launch_lm_step_scaled
// has served it, and has given the wide trees the zero step and their sse).
hipError_t launch_lm_step_scaled_wide(int dtype, const LmScaledStepArgs &a, hipStream_t stream);

// One thread per tree: the accept rule of Population.fit_constants_lm(scaled=True) on scaled_sse, in double.  *_acc: the accepted state,
// *_trial: the evaluation at the trial constants; ok and G <= row_limit make `has` (8: de_fit_consts_lm_scaled, 32:
// de_fit_consts_lm_scaled_wide).  history_row / n_accept may be null.
struct LmScaledAcceptArgs {
    int64_t n_trees;
    const int32_t *n_grad;
    const int64_t *moff, *joff, *coff;
    const double *ystats;
    void *consts_acc, *jtj_acc;
    double *stats_acc, *dmom_acc, *sse_acc;
    uint8_t *ok_acc;
    const void *consts_trial, *jtj_trial;
    const double *stats_trial, *dmom_trial;
    const uint8_t *ok_trial;
    double *lam;
    double up, down, lam_min;
    double *history_row; // n_trees entries: the accepted scaled_sse after this iteration
    int32_t *n_accept;
    int32_t row_limit;
};
hipError_t launch_lm_accept_scaled(int dtype, const LmScaledAcceptArgs &a, hipStream_t stream);

// sse[t] = the scaled_sse of stats[3 t ..] against ystats, and row[t] (may be null) the same value
hipError_t launch_lm_sse_scaled(const double *stats, const double *ystats, int64_t n_trees, double *sse, double *row, hipStream_t stream);

} // namespace de
#endif
