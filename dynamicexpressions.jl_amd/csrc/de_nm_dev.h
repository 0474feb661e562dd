// de_nm_dev.h — launchers of de_nm.hip: the device side of de_fit_consts_nm.
#ifndef DE_NM_DEV_H
#define DE_NM_DEV_H
#include <hip/hip_runtime.h>
#include <cstdint>

namespace de {

// One wave per tree.  Tree t has G = n_grad[t] constants at coff[t] (constants, c and xr alike: packed) and, where 1 <= G <= 32, its
// (G + 1) x G vertices followed by its G + 1 losses at voff[t] (doubles).  *_acc: the accepted state, *_trial: the evaluation at the trial
// constants, both in the element type `dtype`; a tree is fitted where ok_acc && 1 <= G <= 32 at the start (st[3 t] != NM_OFF afterwards).
// f64_objective (de_fit_consts_nm_scaled): the losses (loss_*) are doubles whatever `dtype` is — the kernels' second
// template argument; the constants stay `dtype`.
struct NmArgs {
    int64_t n_trees;
    const int32_t *n_grad;
    const int64_t *coff, *voff;
    void *consts_acc, *loss_acc;
    const uint8_t *ok_acc;
    void *consts_trial;
    const void *loss_trial;
    const uint8_t *ok_trial;
    double *V, *c, *xr, *fr; // fr: n_trees entries
    int32_t *st;             // 3 per tree: phase, cursor, l0
    double a, b, f_tol;
    double *history_row; // n_trees entries: the accepted losses after this round (may be null)
    int32_t *n_improve;  // may be null
};
// V_0 = the accepted constants, f_0 = their loss, every other f +Inf, phase BUILD(1) (NM_OFF where the tree is not fitted), n_improve = 0
hipError_t launch_nm_init(int dtype, const NmArgs &a, hipStream_t stream, bool f64_objective = false);
// consts_trial = the trial of the tree's phase (de_nm.h nm_ask_tree); the bits of consts_acc where the tree is not fitted
hipError_t launch_nm_ask(int dtype, const NmArgs &a, hipStream_t stream, bool f64_objective = false);
// de_nm.h nm_tell_tree with the trial's loss; then the accepted constants and loss are vertex l of the simplex (where its loss is finite),
// n_improve += 1 where the accepted loss became strictly smaller, and the history row is the accepted loss
hipError_t launch_nm_tell(int dtype, const NmArgs &a, hipStream_t stream, bool f64_objective = false);

} // namespace de
#endif
