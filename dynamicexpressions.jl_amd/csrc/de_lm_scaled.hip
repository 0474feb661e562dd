// de_lm_scaled.hip — the device side of de_fit_stats_lm_step / de_fit_consts_lm_scaled: Levenberg-Marquardt on the
// constants of a whole population under Keijzer's linear scaling, without the host seeing a statistic, a moment or a matrix.
//   de_lm_step_scaled_kernel    one thread per tree: the system of de_eval_fit_stats_grad projected (de_lm_project.h) and solved
//                               (de_lm_solve.h) in registers
//   de_lm_accept_scaled_kernel  one thread per tree: the accept rule of Population.fit_constants_lm(scaled=True)
//   de_lm_sse_scaled_kernel     scaled_sse of the first evaluation: the accepted objective and row 0 of the history
// All on the context's stream, plain vector stores only.  A thread branches on its tree's width into code whose subscripts are all
// compile-time constants: the projected system never leaves the registers (the code object's private segment is 0 bytes).
#include "de_lm_scaled.h"
#include "de_lm_project.h"

#include "../../include/de_hip.h"

namespace de {

template <typename T>
__global__ void __launch_bounds__(64) de_lm_step_scaled_kernel(LmScaledStepArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= a.n_trees) return;
    const int G = a.n_grad[t];
    const double *st = a.stats + 3 * t;
    if (a.sse) a.sse[t] = lm_scaled_sse(st[1], st[2], a.ystats[0], a.ystats[2]);
    if (G <= 0) return;
    const int64_t off = a.soff[t];
    double x[LM_MAX_ROWS];
#pragma unroll
    for (int k = 0; k < LM_MAX_ROWS; k++) x[k] = 0.0;
    int solved = 0;
    if (G <= LM_MAX_ROWS && a.has[t]) {
        const double *dm = a.dmom + a.moff[t];
        const T *H = static_cast<const T *>(a.jtj) + a.joff[t];
        const double lam = a.lam[t];
        double sse;
        DE_LM_FOR_G(G, (solved = lm_step_scaled<GG, T>(st, a.ystats, dm, H, lam, x, &sse)));
    }
    if (G <= LM_MAX_ROWS) {
#pragma unroll
        for (int k = 0; k < LM_MAX_ROWS; k++)
            if (k < G) a.step[off + k] = solved ? x[k] : 0.0;
    } else {
        for (int k = 0; k < G; k++) a.step[off + k] = 0.0;
    }
    if (!a.trial) return;
    const T *c = static_cast<const T *>(a.consts) + off;
    T *tr = static_cast<T *>(a.trial) + off;
    if (solved) {
#pragma unroll
        for (int k = 0; k < LM_MAX_ROWS; k++)
            if (k < G) tr[k] = (T)((double)c[k] + x[k]);
    } else {
        for (int k = 0; k < G; k++) tr[k] = c[k]; // (the bits: -0 and NaN payloads stay)
    }
}

template <typename T>
__global__ void __launch_bounds__(256) de_lm_accept_scaled_kernel(LmScaledAcceptArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n_trees) return;
    const int G = a.n_grad[t];
    const bool fitted = G <= a.row_limit;
    const bool has_acc = fitted && a.ok_acc[t], has_trial = fitted && a.ok_trial[t];
    const double *stt = a.stats_trial + 3 * t;
    const double sse_trial = lm_scaled_sse(stt[1], stt[2], a.ystats[0], a.ystats[2]);
    const bool accept = has_acc && has_trial && sse_trial < a.sse_acc[t]; // (a NaN compares false)
    if (accept) {
        const int64_t co = a.coff[t], m0 = a.moff[t], j0 = a.joff[t];
        T *ca = static_cast<T *>(a.consts_acc), *ja = static_cast<T *>(a.jtj_acc);
        const T *ct = static_cast<const T *>(a.consts_trial), *jt = static_cast<const T *>(a.jtj_trial);
        for (int k = 0; k < G; k++) ca[co + k] = ct[co + k];
        for (int k = 0; k < 3 * G; k++) a.dmom_acc[m0 + k] = a.dmom_trial[m0 + k];
        for (int k = 0; k < G * G; k++) ja[j0 + k] = jt[j0 + k];
        for (int k = 0; k < 3; k++) a.stats_acc[3 * t + k] = stt[k];
        a.sse_acc[t] = sse_trial;
        a.ok_acc[t] = a.ok_trial[t];
    }
    const double lam = a.lam[t];
    a.lam[t] = accept ? fmax(lam * a.down, a.lam_min) : lam * a.up;
    if (a.history_row) a.history_row[t] = a.sse_acc[t];
    if (a.n_accept) a.n_accept[t] += accept ? 1 : 0;
}

__global__ void __launch_bounds__(256) de_lm_sse_scaled_kernel(const double *__restrict__ stats, const double *__restrict__ ystats,
                                                                int64_t n_trees, double *__restrict__ sse, double *__restrict__ row) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_trees) return;
    const double v = lm_scaled_sse(stats[3 * t + 1], stats[3 * t + 2], ystats[0], ystats[2]);
    sse[t] = v;
    if (row) row[t] = v;
}

static inline dim3 grid_of(int64_t n, int block) { return dim3((unsigned)((n + block - 1) / block)); }

hipError_t launch_lm_step_scaled(int dtype, const LmScaledStepArgs &a, hipStream_t stream) {
    if (a.n_trees <= 0) return hipSuccess;
    if (dtype == DE_F32) hipLaunchKernelGGL(de_lm_step_scaled_kernel<float>, grid_of(a.n_trees, 64), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL(de_lm_step_scaled_kernel<double>, grid_of(a.n_trees, 64), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_lm_accept_scaled(int dtype, const LmScaledAcceptArgs &a, hipStream_t stream) {
    if (a.n_trees <= 0) return hipSuccess;
    if (dtype == DE_F32) hipLaunchKernelGGL(de_lm_accept_scaled_kernel<float>, grid_of(a.n_trees, 256), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(de_lm_accept_scaled_kernel<double>, grid_of(a.n_trees, 256), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_lm_sse_scaled(const double *stats, const double *ystats, int64_t n_trees, double *sse, double *row, hipStream_t stream) {
    if (n_trees <= 0 || !sse) return hipSuccess;
    hipLaunchKernelGGL(de_lm_sse_scaled_kernel, grid_of(n_trees, 256), dim3(256), 0, stream, stats, ystats, n_trees, sse, row);
    return hipGetLastError();
}

} // namespace de
