// de_lm_scaled_wide.hip — the device side of de_fit_stats_lm_step_wide / de_fit_consts_lm_scaled_wide: the
// Levenberg-Marquardt step under Keijzer's linear scaling of a tree of 9 .. 32 constants.
//   de_lm_step_scaled_wide_kernel   one wave per wide tree: the system of de_eval_fit_stats_grad_wide projected (de_lm_project_wide.h)
//                                   WHILE its matrix is loaded into the LDS work matrix, then de_lm_step_wide_kernel's Cholesky
//                                   (de_lm_solve_wide.h), a lane per row
// On the context's stream, plain vector stores only.  D, P, the right-hand side and the 32 x 33 work matrix live in LDS (8 448 + 768
// bytes): there is no thread-private array, no second copy of the matrix and the projected matrix never travels through memory.
#include "../../include/de_hip.h"

#include "de_lm_scaled.h"
#include "de_lm_project_wide.h"

namespace de {

template <typename T>
__global__ void __launch_bounds__(64) de_lm_step_scaled_wide_kernel(LmScaledStepArgs a) {
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const int G = a.n_grad[t];
    if (G <= LM_MAX_ROWS || G > LM_WIDE_MAX_ROWS) return; // (the whole workgroup: one wave; launch_lm_step_scaled has served the tree)
    __shared__ double A[LMW_WORK];
    __shared__ double D[LM_WIDE_MAX_ROWS], P[LM_WIDE_MAX_ROWS], b[LM_WIDE_MAX_ROWS];
    __shared__ int positive, solved;
    const double *st = a.stats + 3 * t;
    const LmProjectCoef pc = lmpw_coef(st[1], st[2], a.ystats[0]);
    if (a.sse && lane == 0) a.sse[t] = lm_scaled_sse(st[1], st[2], a.ystats[0], a.ystats[2]);
    const int64_t off = a.soff[t];
    const double lam = a.lam[t];
    const double *__restrict__ dm = a.dmom + a.moff[t];
    const T *__restrict__ H = static_cast<const T *>(a.jtj) + a.joff[t];
    bool fin = true;
    if (lane < G) {
        D[lane] = dm[lane];
        P[lane] = dm[G + lane];
        const double v = -0.5 * lmpw_grad(pc, dm[G + lane], dm[2 * G + lane]); // (not formed: never read)
        fin = fin && lm_finite(v);
        b[lane] = v;
    }
    if (lane == 0) { positive = 1; solved = 0; }
    __syncthreads();
    for (int x = lane; x < G * G; x += 64) { // H[i + G k], i >= k -> the projected entry, into rows i and k of the work matrix
        const int i = x % G, k = x / G;
        if (i < k) continue;
        const double v = lmpw_entry(pc, (double)H[x], D[i], D[k], P[i], P[k]);
        fin = fin && lm_finite(v);
        A[i * LMW_LD + k] = v;
        A[k * LMW_LD + i] = v;
    }
    const bool go = __syncthreads_and(fin ? 1 : 0) != 0 && pc.formed != 0 && a.has[t] != 0 && lm_finite(lam);
    if (go) { // (uniform) — from here on de_lm_step_wide_kernel
        if (lane < G) A[lane * LMW_LD + lane] = lmw_damp(A[lane * LMW_LD + lane], lam);
        __syncthreads();
        for (int j = 0; j < G; j++) {
            if (lane == j) {
                const double d = lmw_pivot(A, j);
                A[j * LMW_LD + j] = sqrt(d);
                if (!(d > 0.0)) positive = 0;
            }
            __syncthreads();
            if (!positive) break;
            if (lane > j && lane < G) A[lane * LMW_LD + j] = lmw_below(A, lane, j, A[j * LMW_LD + j]);
            __syncthreads();
        }
        if (lane == 0 && positive) solved = lmw_substitute(A, b, G) ? 1 : 0;
    }
    __syncthreads();
    const bool sv = solved != 0;
    if (lane >= G) return;
    a.step[off + lane] = sv ? b[lane] : 0.0;
    if (!a.trial) return;
    const T *c = static_cast<const T *>(a.consts) + off;
    T *tr = static_cast<T *>(a.trial) + off;
    tr[lane] = sv ? (T)((double)c[lane] + b[lane]) : c[lane]; // (no step: the bits, -0 and NaN payloads stay)
}

hipError_t launch_lm_step_scaled_wide(int dtype, const LmScaledStepArgs &a, hipStream_t stream) {
    if (a.n_trees <= 0) return hipSuccess;
    if (dtype == DE_F32) hipLaunchKernelGGL(de_lm_step_scaled_wide_kernel<float>, dim3((unsigned)a.n_trees), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL(de_lm_step_scaled_wide_kernel<double>, dim3((unsigned)a.n_trees), dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace de
