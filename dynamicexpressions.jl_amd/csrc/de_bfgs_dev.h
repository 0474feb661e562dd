// de_bfgs_dev.h — launchers of de_bfgs.hip: the device side of de_fit_consts_bfgs.
#ifndef DE_BFGS_DEV_H
#define DE_BFGS_DEV_H
#include <hip/hip_runtime.h>
#include <cstdint>

namespace de {

// One wave per tree.  Tree t has G = n_grad[t] constants at coff[t] (constants, gradients and p alike: packed) and, where 1 <= G <= 32,
// its G x G doubles of B at boff[t] (row-major).  *_acc: the accepted state, *_trial: the evaluation at the trial constants, both in the
// element type `dtype`; has = ok_acc && 1 <= G <= 32.  f64_objective (de_fit_consts_bfgs_scaled): the losses and gradients
// (loss_*, dloss_*) are doubles whatever `dtype` is — the kernels' second template argument; the constants stay `dtype`.
struct BfgsArgs {
    int64_t n_trees;
    const int32_t *n_grad;
    const int64_t *coff, *boff;
    void *consts_acc, *loss_acc, *dloss_acc;
    uint8_t *ok_acc;
    void *consts_trial;
    const void *loss_trial, *dloss_trial;
    const uint8_t *ok_trial;
    double *B, *alpha, *p, *slope; // alpha, slope: n_trees entries
    uint8_t *fresh, *produced;     // n_trees entries
    double step0, shrink, c1, curv;
    double *history_row; // n_trees entries: the accepted losses after this iteration (may be null)
    int32_t *n_accept;   // may be null
};
// B = I, fresh = 1, alpha = a0(dloss_acc), n_accept = 0
hipError_t launch_bfgs_init(int dtype, const BfgsArgs &a, hipStream_t stream, bool f64_objective = false);
// p, slope, produced (de_bfgs.h bfgs_direction; the state is reset where B gives no descent direction) and
// consts_trial = T(double(consts_acc) + alpha p) where a direction was produced, else the bits of consts_acc
hipError_t launch_bfgs_direction(int dtype, const BfgsArgs &a, hipStream_t stream, bool f64_objective = false);
// the accept rule: Armijo on the trial loss; an accepted tree takes the trial constants, loss, gradient and flag, B takes bfgs_update
// of the step actually taken, alpha = fresh ? a0(g) : 1; a rejected tree's alpha shrinks
hipError_t launch_bfgs_accept(int dtype, const BfgsArgs &a, hipStream_t stream, bool f64_objective = false);

} // namespace de
#endif
