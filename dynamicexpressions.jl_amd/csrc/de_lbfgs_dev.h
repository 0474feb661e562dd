// de_lbfgs_dev.h — launchers of de_lbfgs.hip: the device side of de_fit_consts_lbfgs / de_fit_tree_params_lbfgs.
#ifndef DE_LBFGS_DEV_H
#define DE_LBFGS_DEV_H
#include "de_bfgs_dev.h"
#include "de_lbfgs.h"

namespace de {

// One wave per tree, on the packed vectors of BfgsArgs (b.B, b.boff and b.fresh are not used).  Where 1 <= G <= 4096 the tree owns
// memory x G doubles of S and of Y at roff[t] (slot j at roff[t] + j G), rho[t memory + j], count[t], head[t]; tmp: as long as b.p (the
// accept kernel forms s in b.p and yv in tmp before a pair is stored).  has = ok_acc && 1 <= G <= 4096.
struct LbfgsArgs {
    BfgsArgs b;
    const int64_t *roff;
    double *S, *Y, *rho, *tmp;
    int32_t *count, *head; // n_trees entries
    int32_t memory;
};
// count = head = 0, alpha = a0(dloss_acc), n_accept = 0
hipError_t launch_lbfgs_init(int dtype, const LbfgsArgs &a, hipStream_t stream);
// p, slope, produced (de_lbfgs.h lbfgs_direction; count = 0 where the ring gives no descent direction) and
// consts_trial = T(double(consts_acc) + alpha p) where a direction was produced, else the bits of consts_acc
hipError_t launch_lbfgs_direction(int dtype, const LbfgsArgs &a, hipStream_t stream);
// the accept rule: Armijo on the trial loss; an accepted tree takes the trial constants, loss, gradient and flag, the ring takes
// lbfgs_update of the step actually taken, alpha = count == 0 ? a0(g) : 1; a rejected tree's alpha shrinks
hipError_t launch_lbfgs_accept(int dtype, const LbfgsArgs &a, hipStream_t stream);

// The quasi-Newton kernels of a fit on packed vectors — de_bfgs.hip (memory = 0) or de_lbfgs.hip (memory = the ring's length) — and what
// their per-tree state takes: the loops of de_api_fit.cpp and de_api_tree_params.cpp are written once over this.
struct QnKernels {
    int memory = 0;
    LbfgsArgs x; // x.b: what both kernel sets read
    int max_rows() const { return memory ? LBFGS_MAX_ROWS : BFGS_MAX_ROWS; }
    // the doubles of B, or of each of S and Y, that a tree of g unknowns owns: none where it is not fitted
    int64_t state_doubles(int64_t g) const { return g < 1 || g > max_rows() ? 0 : memory ? memory * g : g * g; }
    hipError_t init(int dtype, hipStream_t s) const { return memory ? launch_lbfgs_init(dtype, x, s) : launch_bfgs_init(dtype, x.b, s); }
    hipError_t direction(int dtype, hipStream_t s) const { return memory ? launch_lbfgs_direction(dtype, x, s) : launch_bfgs_direction(dtype, x.b, s); }
    hipError_t accept(int dtype, hipStream_t s) const { return memory ? launch_lbfgs_accept(dtype, x, s) : launch_bfgs_accept(dtype, x.b, s); }
};

} // namespace de
#endif
