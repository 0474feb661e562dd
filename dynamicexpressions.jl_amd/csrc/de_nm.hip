// de_nm.hip — the device side of de_fit_consts_nm: Nelder-Mead on the constants of a whole population, from the
// fused loss alone, without the host seeing a constant or a loss.
//   de_nm_init_kernel  V_0 = the constants, f_0 = their loss, phase BUILD(1), n_improve = 0
//   de_nm_ask_kernel   the trial constants of the tree's phase
//   de_nm_tell_kernel  the phase's decision on the trial's loss, the accepted vertex, n_improve and a row of the loss history
// One wave per tree, lane j < G owns coordinate j of every vertex (the arithmetic: de_nm.h, the code the host hooks run); the ordering of
// the G + 1 <= 33 losses is scanned by every lane, so every decision is wave-uniform: no LDS, no atomics, plain vector stores only.  A
// tree that is not fitted leaves at once.  All on the context's stream.
// T: the element type of the constants; LT: the type of the loss slots — T itself for de_fit_consts_nm, double whatever T is for
// de_fit_consts_nm_scaled (the scaled objective is never rounded to Float32).
#include "../../include/de_hip.h"

#include "de_nm_dev.h"
#include "de_nm.h"

namespace de {

template <typename T, typename LT = T>
__global__ void __launch_bounds__(64) de_nm_init_kernel(NmArgs a) {
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const int G = a.n_grad[t];
    const bool has = a.ok_acc[t] != 0 && G >= 1 && G <= NM_MAX_ROWS;
    if (lane == 0) {
        if (a.n_improve) a.n_improve[t] = 0;
        a.st[3 * t] = has ? NM_BUILD : NM_OFF;
        a.st[3 * t + 1] = 1;
        a.st[3 * t + 2] = 0;
        a.fr[t] = 0.0;
    }
    if (!has) return; // (the whole workgroup: one wave)
    const int64_t off = a.coff[t];
    double *V = a.V + a.voff[t], *f = V + (G + 1) * G;
    if (lane < G) {
        V[lane] = (double)(static_cast<const T *>(a.consts_acc) + off)[lane];
        a.c[off + lane] = 0.0;
        a.xr[off + lane] = 0.0;
    }
    if (lane <= G) f[lane] = lane == 0 ? nm_loss((double)static_cast<const LT *>(a.loss_acc)[t], true) : nm_inf();
}

template <typename T, typename LT = T>
__global__ void __launch_bounds__(64) de_nm_ask_kernel(NmArgs a) {
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const int G = a.n_grad[t];
    if (G <= 0) return;
    const int64_t off = a.coff[t];
    T *tr = static_cast<T *>(a.consts_trial) + off;
    if (a.st[3 * t] == NM_OFF) { // (uniform) not fitted: the bits of the constants, -0 and NaN payloads stay
        const T *c = static_cast<const T *>(a.consts_acc) + off;
        for (int k = lane; k < G; k += 64) tr[k] = c[k];
        return;
    }
    double *V = a.V + a.voff[t];
    nm_ask_tree<T>(G, lane, lane < G ? lane + 1 : lane, lane == 0, a.a, a.b, a.f_tol, V, V + (G + 1) * G, a.st + 3 * t, a.c + off, a.xr + off, tr);
}

template <typename T, typename LT = T>
__global__ void __launch_bounds__(64) de_nm_tell_kernel(NmArgs a) {
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const int G = a.n_grad[t];
    LT *la = static_cast<LT *>(a.loss_acc);
    if (a.st[3 * t] == NM_OFF) { // (uniform)
        if (lane == 0 && a.history_row) a.history_row[t] = (double)la[t];
        return;
    }
    const int64_t off = a.coff[t];
    double *V = a.V + a.voff[t], *f = V + (G + 1) * G;
    const double F = nm_loss((double)static_cast<const LT *>(a.loss_trial)[t], a.ok_trial[t] != 0);
    const double before = f[nm_order(f, G).l];
    nm_tell_tree<T>(G, lane, lane < G ? lane + 1 : lane, lane == 0, V, f, a.st + 3 * t, a.c + off, a.xr + off, a.fr + t, F);
    __syncthreads(); // (lane 0 has written the tree's losses before every lane orders them)
    const int l = nm_order(f, G).l;
    const double now = f[l];
    if (now < nm_inf()) { // (uniform) the accepted state is vertex l
        if (lane < G) (static_cast<T *>(a.consts_acc) + off)[lane] = (T)V[l * G + lane];
        if (lane == 0) {
            la[t] = (LT)now;
            if (a.n_improve && now < before) a.n_improve[t] += 1;
        }
    }
    if (lane == 0 && a.history_row) a.history_row[t] = now < nm_inf() ? now : (double)la[t];
}

#define DE_NM_LAUNCH(KERNEL)                                                                                           \
    if (a.n_trees <= 0) return hipSuccess;                                                                             \
    if (dtype == DE_F32 && f64_objective)                                                                              \
        hipLaunchKernelGGL((KERNEL<float, double>), dim3((unsigned)a.n_trees), dim3(64), 0, stream, a);                \
    else if (dtype == DE_F32) hipLaunchKernelGGL(KERNEL<float>, dim3((unsigned)a.n_trees), dim3(64), 0, stream, a);    \
    else hipLaunchKernelGGL(KERNEL<double>, dim3((unsigned)a.n_trees), dim3(64), 0, stream, a);                        \
    return hipGetLastError()

hipError_t launch_nm_init(int dtype, const NmArgs &a, hipStream_t stream, bool f64_objective) { DE_NM_LAUNCH(de_nm_init_kernel); }
hipError_t launch_nm_ask(int dtype, const NmArgs &a, hipStream_t stream, bool f64_objective) { DE_NM_LAUNCH(de_nm_ask_kernel); }
hipError_t launch_nm_tell(int dtype, const NmArgs &a, hipStream_t stream, bool f64_objective) { DE_NM_LAUNCH(de_nm_tell_kernel); }

} // namespace de
