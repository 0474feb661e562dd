// de_lm.hip — the device side of de_gn_lm_step / de_fit_consts_lm: Levenberg-Marquardt on the constants of a whole
// population without the host seeing a constant, a gradient or a matrix.
//   de_lm_step_kernel    one thread per tree: the damped normal equations of de_eval_loss_gn solved by Cholesky (de_lm_solve.h)
//   de_lm_accept_kernel  one thread per tree: the accept rule of Population.fit_constants_lm
//   de_lm_init_kernel / de_lm_history_kernel: lam = lam0, n_accept = 0; a row of the loss history
// All on the context's stream, plain vector stores only.  The 8 x 8 system of a thread stays in registers: the padded matrix is
// indexed by compile-time constants throughout (the code object's private segment is 0 bytes).
#include "de_lm.h"
#include "de_lm_solve.h"

#include "../../include/de_hip.h"

namespace de {

template <typename T>
__global__ void __launch_bounds__(64) de_lm_step_kernel(LmStepArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= a.n_trees) return;
    const int G = a.n_grad[t];
    if (G <= 0) return;
    const int64_t off = a.doff[t];
    double x[LM_MAX_ROWS];
    int solved = 0;
    if (G <= LM_MAX_ROWS && a.has[t])
        solved = lm_solve8<T>(G, static_cast<const T *>(a.jtj) + a.joff[t], static_cast<const T *>(a.dloss) + off, a.lam[t], x);
    if (G <= LM_MAX_ROWS) {
#pragma unroll
        for (int k = 0; k < LM_MAX_ROWS; k++)
            if (k < G) a.step[off + k] = solved ? x[k] : 0.0;
    } else {
        for (int k = 0; k < G; k++) a.step[off + k] = 0.0;
    }
    if (!a.trial) return;
    const T *c = static_cast<const T *>(a.consts) + a.coff[t];
    T *tr = static_cast<T *>(a.trial) + a.coff[t];
    if (solved) {
#pragma unroll
        for (int k = 0; k < LM_MAX_ROWS; k++)
            if (k < G) tr[k] = (T)((double)c[k] + x[k]);
    } else {
        for (int k = 0; k < G; k++) tr[k] = c[k]; // (the bits: -0 and NaN payloads stay)
    }
}

template <typename T>
__global__ void __launch_bounds__(256) de_lm_accept_kernel(LmAcceptArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n_trees) return;
    const int G = a.n_grad[t];
    T *loss_acc = static_cast<T *>(a.loss_acc);
    const T *loss_trial = static_cast<const T *>(a.loss_trial);
    const bool narrow = G <= a.row_limit;
    const bool has_acc = narrow && a.ok_acc[t], has_trial = narrow && a.ok_trial[t];
    const bool accept = has_acc && has_trial && (double)loss_trial[t] < (double)loss_acc[t]; // (a NaN compares false)
    if (accept) {
        const int64_t co = a.coff[t], d0 = a.doff[t], j0 = a.joff[t];
        T *ca = static_cast<T *>(a.consts_acc), *da = static_cast<T *>(a.dloss_acc), *ja = static_cast<T *>(a.jtj_acc);
        const T *ct = static_cast<const T *>(a.consts_trial), *dt = static_cast<const T *>(a.dloss_trial), *jt = static_cast<const T *>(a.jtj_trial);
        for (int k = 0; k < G; k++) {
            ca[co + k] = ct[co + k];
            da[d0 + k] = dt[d0 + k];
        }
        for (int k = 0; k < G * G; k++) ja[j0 + k] = jt[j0 + k];
        loss_acc[t] = loss_trial[t];
        a.ok_acc[t] = a.ok_trial[t];
    }
    const double lam = a.lam[t];
    a.lam[t] = accept ? fmax(lam * a.down, a.lam_min) : lam * a.up;
    if (a.history_row) a.history_row[t] = (double)loss_acc[t];
    if (a.n_accept) a.n_accept[t] += accept ? 1 : 0;
}

__global__ void __launch_bounds__(256) de_lm_init_kernel(int64_t n_trees, double lam0, double *lam, int32_t *n_accept) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_trees) return;
    if (lam) lam[t] = lam0;
    if (n_accept) n_accept[t] = 0;
}

template <typename T>
__global__ void __launch_bounds__(256) de_lm_history_kernel(const T *__restrict__ loss, int64_t n_trees, double *__restrict__ row) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n_trees) row[t] = (double)loss[t];
}

static inline dim3 grid_of(int64_t n, int block) { return dim3((unsigned)((n + block - 1) / block)); }

hipError_t launch_lm_step(int dtype, const LmStepArgs &a, hipStream_t stream) {
    if (a.n_trees <= 0) return hipSuccess;
    if (dtype == DE_F32) hipLaunchKernelGGL(de_lm_step_kernel<float>, grid_of(a.n_trees, 64), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL(de_lm_step_kernel<double>, grid_of(a.n_trees, 64), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_lm_accept(int dtype, const LmAcceptArgs &a, hipStream_t stream) {
    if (a.n_trees <= 0) return hipSuccess;
    if (dtype == DE_F32) hipLaunchKernelGGL(de_lm_accept_kernel<float>, grid_of(a.n_trees, 256), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(de_lm_accept_kernel<double>, grid_of(a.n_trees, 256), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_lm_init(int64_t n_trees, double lam0, double *lam, int32_t *n_accept, hipStream_t stream) {
    if (n_trees <= 0 || (!lam && !n_accept)) return hipSuccess;
    hipLaunchKernelGGL(de_lm_init_kernel, grid_of(n_trees, 256), dim3(256), 0, stream, n_trees, lam0, lam, n_accept);
    return hipGetLastError();
}

hipError_t launch_lm_history(int dtype, const void *loss, int64_t n_trees, double *row, hipStream_t stream) {
    if (n_trees <= 0 || !row) return hipSuccess;
    if (dtype == DE_F32)
        hipLaunchKernelGGL(de_lm_history_kernel<float>, grid_of(n_trees, 256), dim3(256), 0, stream, static_cast<const float *>(loss), n_trees, row);
    else
        hipLaunchKernelGGL(de_lm_history_kernel<double>, grid_of(n_trees, 256), dim3(256), 0, stream, static_cast<const double *>(loss), n_trees, row);
    return hipGetLastError();
}

} // namespace de
