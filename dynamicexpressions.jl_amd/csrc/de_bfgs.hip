// de_bfgs.hip — the device side of de_fit_consts_bfgs: BFGS on the constants of a whole population without the host
// seeing a constant, a gradient or a matrix.
//   de_bfgs_init_kernel       B = I, fresh = 1, alpha = a0(g), n_accept = 0
//   de_bfgs_direction_kernel  p = -B g (or the reset to -g), its slope, and the trial constants
//   de_bfgs_accept_kernel     the Armijo accept rule, the rank-two update of B and a row of the loss history
// One wave per tree, lane i < G owns row i of B (the arithmetic: de_bfgs.h, the code the host hooks run); the scalars are summed in index
// order from LDS by every lane.  All on the context's stream, plain vector stores only, no atomics.
// T: the element type of the constants; LT: the type of the loss and gradient slots — T itself for de_fit_consts_bfgs, double whatever T is
// for de_fit_consts_bfgs_scaled (the scaled objective is never rounded to Float32).
#include "../../include/de_hip.h"

#include "de_bfgs_dev.h"
#include "de_bfgs.h"

namespace de {

template <typename T, typename LT = T>
__global__ void __launch_bounds__(64) de_bfgs_init_kernel(BfgsArgs a) {
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const int G = a.n_grad[t];
    if (lane == 0 && a.n_accept) a.n_accept[t] = 0;
    if (G < 1 || G > BFGS_MAX_ROWS) return; // (the whole workgroup: one wave)
    __shared__ double g[BFGS_MAX_ROWS];
    if (lane < G) {
        g[lane] = (double)(static_cast<const LT *>(a.dloss_acc) + a.coff[t])[lane];
        bfgs_identity_row(a.B + a.boff[t] + (int64_t)lane * G, lane, G, 1.0);
    }
    __syncthreads();
    if (lane == 0) {
        a.fresh[t] = 1;
        a.alpha[t] = bfgs_a0(bfgs_dot(g, g, G), a.step0);
    }
}

template <typename T, typename LT = T>
__global__ void __launch_bounds__(64) de_bfgs_direction_kernel(BfgsArgs a) {
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const int G = a.n_grad[t];
    if (G <= 0) {
        if (lane == 0) { a.produced[t] = 0; a.slope[t] = 0.0; }
        return;
    }
    const int64_t off = a.coff[t];
    const T *c = static_cast<const T *>(a.consts_acc) + off;
    T *tr = static_cast<T *>(a.consts_trial) + off;
    if (G > BFGS_MAX_ROWS || !a.ok_acc[t]) { // (uniform) not fitted: the bits of the constants, -0 and NaN payloads stay
        for (int k = lane; k < G; k += 64) {
            tr[k] = c[k];
            a.p[off + k] = 0.0;
        }
        if (lane == 0) { a.produced[t] = 0; a.slope[t] = 0.0; }
        return;
    }
    __shared__ double g[BFGS_MAX_ROWS], p[BFGS_MAX_ROWS];
    double al = a.alpha[t];
    double *row = a.B + a.boff[t] + (int64_t)lane * G;
    if (lane < G) g[lane] = (double)(static_cast<const LT *>(a.dloss_acc) + off)[lane];
    __syncthreads();
    bool fin = true;
    double pv = 0.0;
    if (lane < G) {
        fin = lm_finite(g[lane]) && bfgs_row_finite(row, G);
        pv = bfgs_dir_row(row, g, G);
        p[lane] = pv;
    }
    const bool all_fin = __syncthreads_and(fin ? 1 : 0) != 0;
    double sl = bfgs_dot(g, p, G);
    if (!(sl < 0.0)) { // (uniform: every lane summed the same entries in the same order) no descent direction: the state is reset
        const double gg = bfgs_dot(g, g, G);
        al = bfgs_a0(gg, a.step0);
        sl = -gg;
        if (lane < G) {
            bfgs_identity_row(row, lane, G, 1.0);
            pv = -g[lane];
        }
        if (lane == 0) {
            a.fresh[t] = 1;
            a.alpha[t] = al;
        }
    }
    const bool produced = all_fin && sl < 0.0;
    if (lane == 0) {
        a.produced[t] = produced ? 1 : 0;
        a.slope[t] = sl;
    }
    if (lane >= G) return;
    a.p[off + lane] = produced ? pv : 0.0;
    tr[lane] = produced ? (T)bfgs_trial((double)c[lane], al, pv) : c[lane];
}

template <typename T, typename LT = T>
__global__ void __launch_bounds__(64) de_bfgs_accept_kernel(BfgsArgs a) {
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const int G = a.n_grad[t];
    LT *la = static_cast<LT *>(a.loss_acc);
    const double f = (double)la[t], ft = (double)static_cast<const LT *>(a.loss_trial)[t];
    const double al = a.alpha[t];
    const bool has = a.ok_acc[t] != 0 && G >= 1 && G <= BFGS_MAX_ROWS;
    const bool accept = has && a.produced[t] != 0 && a.ok_trial[t] != 0 && bfgs_armijo(ft, f, a.c1, al, a.slope[t]);
    uint8_t fr = a.fresh[t];
    __syncthreads(); // (every lane has read the tree's scalars before lane 0 writes them)
    if (lane == 0 && a.history_row) a.history_row[t] = accept ? ft : f;
    if (!accept) { // (uniform)
        if (lane == 0) a.alpha[t] = al * a.shrink;
        return;
    }
    __shared__ double s[BFGS_MAX_ROWS], yv[BFGS_MAX_ROWS], u[BFGS_MAX_ROWS], gn[BFGS_MAX_ROWS];
    const int64_t off = a.coff[t];
    T *ca = static_cast<T *>(a.consts_acc) + off;
    LT *ga = static_cast<LT *>(a.dloss_acc) + off;
    const T *ct = static_cast<const T *>(a.consts_trial) + off;
    const LT *gt = static_cast<const LT *>(a.dloss_trial) + off;
    if (lane < G) {
        s[lane] = (double)ct[lane] - (double)ca[lane]; // the rounded step actually taken
        gn[lane] = (double)gt[lane];
        yv[lane] = gn[lane] - (double)ga[lane];
    }
    __syncthreads();
    const double sy = bfgs_dot(s, yv, G), ss = bfgs_dot(s, s, G), yy = bfgs_dot(yv, yv, G);
    if (bfgs_curvature(sy, ss, yy, a.curv)) { // (uniform)
        double *row = a.B + a.boff[t] + (int64_t)lane * G;
        if (lane < G) {
            if (fr) bfgs_identity_row(row, lane, G, sy / yy);
            u[lane] = bfgs_dot(row, yv, G);
        }
        __syncthreads();
        const double coef = bfgs_coef(sy, bfgs_dot(yv, u, G));
        if (lane < G) bfgs_update_row(row, lane, G, s, u, coef, sy);
        fr = 0;
    }
    if (lane < G) {
        ca[lane] = ct[lane];
        ga[lane] = gt[lane];
    }
    if (lane == 0) {
        la[t] = static_cast<const LT *>(a.loss_trial)[t];
        a.ok_acc[t] = a.ok_trial[t];
        a.fresh[t] = fr;
        a.alpha[t] = fr ? bfgs_a0(bfgs_dot(gn, gn, G), a.step0) : 1.0;
        if (a.n_accept) a.n_accept[t] += 1;
    }
}

#define DE_BFGS_LAUNCH(KERNEL)                                                                                         \
    if (a.n_trees <= 0) return hipSuccess;                                                                             \
    if (dtype == DE_F32 && f64_objective)                                                                              \
        hipLaunchKernelGGL((KERNEL<float, double>), dim3((unsigned)a.n_trees), dim3(64), 0, stream, a);                \
    else if (dtype == DE_F32) hipLaunchKernelGGL(KERNEL<float>, dim3((unsigned)a.n_trees), dim3(64), 0, stream, a);    \
    else hipLaunchKernelGGL(KERNEL<double>, dim3((unsigned)a.n_trees), dim3(64), 0, stream, a);                        \
    return hipGetLastError()

hipError_t launch_bfgs_init(int dtype, const BfgsArgs &a, hipStream_t stream, bool f64_objective) { DE_BFGS_LAUNCH(de_bfgs_init_kernel); }
hipError_t launch_bfgs_direction(int dtype, const BfgsArgs &a, hipStream_t stream, bool f64_objective) { DE_BFGS_LAUNCH(de_bfgs_direction_kernel); }
hipError_t launch_bfgs_accept(int dtype, const BfgsArgs &a, hipStream_t stream, bool f64_objective) { DE_BFGS_LAUNCH(de_bfgs_accept_kernel); }

} // namespace de
