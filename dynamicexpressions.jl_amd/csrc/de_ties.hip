// de_ties.hip — the device side of the tied fits de_fit_consts_{bfgs,lbfgs,nm,lm}_tied: a shared GraphNode constant
// is ONE unknown of the optimiser kernels, which run unchanged on packed vectors of unknowns; these kernels sit around every evaluation.
//   de_ties_pack_kernel         unique[u] = slots[first slot of u]                       one thread per unknown
//   de_ties_unpack_kernel       slots[s] = unique[slot_unk[s]]                            one thread per slot
//   de_ties_fold_kernel         g_u = the occurrence rows of u, summed ascending from +0  one thread per unknown, over its own slot list
//   de_ties_fold_matrix_kernel  Hu = S H S^T, rows first then columns                     one workgroup per tree, one thread per entry
// Every output entry is owned by one thread: plain vector stores, no atomics, no LDS; the cost is linear in the slots (the matrix: in the
// S^2 entries of the occurrence block).  The arithmetic is de_ties.h, the code the host hooks run.  All on the context's stream.
#include "../../include/de_hip.h"

#include "de_ties_dev.h"
#include "de_ties.h"

namespace de {

template <typename T>
__global__ void __launch_bounds__(256) de_ties_pack_kernel(TieArgs a, const T *__restrict__ slots, T *__restrict__ unique) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= a.n_unknowns) return;
    unique[u] = slots[a.unk_slots[a.unk_off[u]]]; // (a checked map: every unknown has a slot)
}

template <typename T>
__global__ void __launch_bounds__(256) de_ties_unpack_kernel(TieArgs a, const T *__restrict__ unique, T *__restrict__ slots) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n_slots) return;
    slots[s] = unique[a.slot_unk[s]];
}

template <typename T>
__global__ void __launch_bounds__(256) de_ties_fold_kernel(TieArgs a, const T *__restrict__ g_slots, T *__restrict__ g_unique) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= a.n_unknowns) return;
    const int64_t k0 = a.unk_off[u];
    g_unique[u] = ties_fold<T>(g_slots, a.unk_slots + k0, a.unk_off[u + 1] - k0);
}

template <typename T>
__global__ void __launch_bounds__(64) de_ties_fold_matrix_kernel(TieArgs a, const T *__restrict__ H, T *__restrict__ Hu) {
    const int64_t t = blockIdx.x;
    const int64_t s0 = a.slot_off[t], S = a.slot_off[t + 1] - s0, u0 = a.unk_tree_off[t], U = a.unk_tree_off[t + 1] - u0;
    if (U <= 0) return;
    T *out = Hu + a.huoff[t];
    if (S > a.max_slots) { // the evaluation formed no occurrence block
        if (U <= a.max_slots)
            for (int64_t e = threadIdx.x; e < U * U; e += 64) out[e] = (T)__builtin_nan("");
        return;
    }
    const T *block = H + a.hoff[t];
    for (int64_t e = threadIdx.x; e < U * U; e += 64) {
        const int64_t u = u0 + e % U, v = u0 + e / U; // (column-major: consecutive threads store consecutive entries)
        const int64_t ku = a.unk_off[u], kv = a.unk_off[v];
        out[e] = ties_fold_matrix<T>(block, S, s0, a.unk_slots + ku, a.unk_off[u + 1] - ku, a.unk_slots + kv, a.unk_off[v + 1] - kv);
    }
}

#define DE_TIES_LAUNCH(KERNEL, COUNT, BLOCK, IN, OUT)                                                                                    \
    const int64_t n_ = (COUNT);                                                                                                         \
    if (n_ <= 0) return hipSuccess;                                                                                                     \
    const dim3 grid_((unsigned)((n_ + (BLOCK) - 1) / (BLOCK)));                                                                         \
    if (dtype == DE_F32) hipLaunchKernelGGL(KERNEL<float>, grid_, dim3(BLOCK), 0, stream, a, static_cast<const float *>(IN), static_cast<float *>(OUT)); \
    else hipLaunchKernelGGL(KERNEL<double>, grid_, dim3(BLOCK), 0, stream, a, static_cast<const double *>(IN), static_cast<double *>(OUT)); \
    return hipGetLastError()

hipError_t launch_ties_pack(int dtype, const TieArgs &a, const void *slots, void *unique, hipStream_t stream) {
    DE_TIES_LAUNCH(de_ties_pack_kernel, a.n_unknowns, 256, slots, unique);
}
hipError_t launch_ties_unpack(int dtype, const TieArgs &a, const void *unique, void *slots, hipStream_t stream) {
    DE_TIES_LAUNCH(de_ties_unpack_kernel, a.n_slots, 256, unique, slots);
}
hipError_t launch_ties_fold(int dtype, const TieArgs &a, const void *g_slots, void *g_unique, hipStream_t stream) {
    DE_TIES_LAUNCH(de_ties_fold_kernel, a.n_unknowns, 256, g_slots, g_unique);
}
hipError_t launch_ties_fold_matrix(int dtype, const TieArgs &a, const void *H, void *Hu, hipStream_t stream) {
    if (a.n_trees <= 0 || a.n_unknowns <= 0) return hipSuccess;
    const dim3 grid((unsigned)a.n_trees);
    if (dtype == DE_F32)
        hipLaunchKernelGGL(de_ties_fold_matrix_kernel<float>, grid, dim3(64), 0, stream, a, static_cast<const float *>(H), static_cast<float *>(Hu));
    else
        hipLaunchKernelGGL(de_ties_fold_matrix_kernel<double>, grid, dim3(64), 0, stream, a, static_cast<const double *>(H), static_cast<double *>(Hu));
    return hipGetLastError();
}

} // namespace de
