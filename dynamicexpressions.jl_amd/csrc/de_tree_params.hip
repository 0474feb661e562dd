// de_tree_params.hip — the device side of de_eval_tree_params / de_eval_loss_tree_params / de_eval_loss_grad_tree_params (DESIGN.md
// §4.4.11): a population whose trees each own their parameter matrix, served one class segment at a time.
//   de_tree_params_scatter_kernel     the constant vector of one class: base values in real slots, the tree's own column in parameter slots
//   de_tree_params_accumulate_kernel  one class's per-tree results added into double accumulators, its dparams cells formed, flags ANDed
//   de_tree_params_finish_kernel      the accumulators in the element type, NaN where the tree's flag is 0
//   de_tree_params_pack_kernel        de_fit_tree_params_bfgs (§4.4.12): the packed unknowns gathered from (slot vector, parameter cells) —
//                                     pack_x from (constants, parameter block), pack_g from (dloss, dparams)
//   de_tree_params_unpack_kernel      ... and scattered back: real constant slots and parameter cells, nothing else
// One thread per entry, every entry owned by one thread: plain vector stores, no atomics; the order of the additions is the stream
// order of the launches (classes ascending).  The arithmetic is de_tree_params.h, the code the host hook runs.
#include "../../include/de_hip.h"

#include "de_tree_params_dev.h"
#include "de_tree_params.h"
#include "de_tree_params_fit.h"

namespace de {

template <typename T>
__global__ void __launch_bounds__(256) de_tree_params_scatter_kernel(TreeParamsArgs a) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n_consts) return;
    const int32_t p = a.slot_param[s];
    T v;
    if (p < 0) v = static_cast<const T *>(a.base)[s];
    else v = static_cast<const T *>(a.params)[p + a.ld_params * (a.cls + a.n_classes * (int64_t)a.slot_tree[s])];
    static_cast<T *>(a.cvec)[s] = v;
}

template <typename T>
__global__ void __launch_bounds__(256) de_tree_params_accumulate_kernel(TreeParamsArgs a) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n_trees) {
        if (a.loss_c) a.acc_loss[i] = tp_add(a.acc_loss[i], static_cast<const T *>(a.loss_c)[i]);
        a.acc_ok[i] = (a.acc_ok[i] && a.ok_c[i]) ? 1 : 0;
        return;
    }
    if (!a.dloss_c) return;
    i -= a.n_trees;
    const T *d = static_cast<const T *>(a.dloss_c);
    if (i < a.n_consts) {
        const int64_t t = a.slot_tree[i];
        a.acc_dloss[i] = tp_add(a.acc_dloss[i], d[a.doff[t] + (i - a.coff[t])]);
        return;
    }
    i -= a.n_consts;
    if (i >= a.n_trees * a.n_params) return;
    const int64_t t = i / a.n_params;
    const int32_t p = (int32_t)(i % a.n_params);
    a.acc_dparams[(t * a.n_classes + a.cls) * a.n_params + p] = tp_cell(d + a.doff[t], a.slot_param + a.coff[t], a.coff[t + 1] - a.coff[t], p);
}

template <typename T>
__global__ void __launch_bounds__(256) de_tree_params_finish_kernel(TreeParamsArgs a) {
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n_trees) {
        const uint8_t k = a.acc_ok[i];
        a.ok[i] = k;
        if (a.loss) static_cast<T *>(a.loss)[i] = tp_finish<T>(a.acc_loss[i], k);
        return;
    }
    if (!a.dloss) return;
    i -= a.n_trees;
    if (i < a.n_consts) {
        const int64_t t = a.slot_tree[i];
        static_cast<T *>(a.dloss)[a.doff[t] + (i - a.coff[t])] = tp_finish<T>(a.acc_dloss[i], a.acc_ok[t]);
        return;
    }
    i -= a.n_consts;
    const int64_t per_tree = a.n_classes * a.n_params;
    if (i >= a.n_trees * per_tree) return;
    static_cast<T *>(a.dparams)[i] = tp_finish<T>(a.acc_dparams[i], a.acc_ok[i / per_tree]);
}

// (consecutive threads read consecutive table entries and packed elements; the other side is slot order / cell order, so it is
// consecutive too inside a tree's constants and inside its matrix)
template <typename T>
__global__ void __launch_bounds__(256) de_tree_params_pack_kernel(TreeParamsFitArgs a) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= a.n_unknowns) return;
    static_cast<T *>(a.packed)[u] = tpf_load(a.map[u], static_cast<const T *>(a.slots), static_cast<const T *>(a.cells), a.n_params, a.ld);
}

template <typename T>
__global__ void __launch_bounds__(256) de_tree_params_unpack_kernel(TreeParamsFitArgs a) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= a.n_unknowns) return;
    tpf_store(a.map[u], static_cast<const T *>(a.packed)[u], static_cast<T *>(a.slots), static_cast<T *>(a.cells), a.n_params, a.ld);
}

#define DE_TP_LAUNCH(KERNEL, COUNT)                                                                                     \
    const int64_t n_ = (COUNT);                                                                                         \
    if (n_ <= 0) return hipSuccess;                                                                                     \
    const dim3 grid_((unsigned)((n_ + 255) / 256));                                                                     \
    if (dtype == DE_F32) hipLaunchKernelGGL(KERNEL<float>, grid_, dim3(256), 0, stream, a);                             \
    else hipLaunchKernelGGL(KERNEL<double>, grid_, dim3(256), 0, stream, a);                                            \
    return hipGetLastError()

hipError_t launch_tree_params_scatter(int dtype, const TreeParamsArgs &a, hipStream_t stream) {
    DE_TP_LAUNCH(de_tree_params_scatter_kernel, a.n_consts);
}
hipError_t launch_tree_params_accumulate(int dtype, const TreeParamsArgs &a, hipStream_t stream) {
    DE_TP_LAUNCH(de_tree_params_accumulate_kernel, a.n_trees + (a.dloss_c ? a.n_consts + a.n_trees * a.n_params : 0));
}
hipError_t launch_tree_params_finish(int dtype, const TreeParamsArgs &a, hipStream_t stream) {
    DE_TP_LAUNCH(de_tree_params_finish_kernel, a.n_trees + (a.dloss ? a.n_consts + a.n_trees * a.n_classes * a.n_params : 0));
}
hipError_t launch_tree_params_pack(int dtype, const TreeParamsFitArgs &a, hipStream_t stream) {
    DE_TP_LAUNCH(de_tree_params_pack_kernel, a.n_unknowns);
}
hipError_t launch_tree_params_unpack(int dtype, const TreeParamsFitArgs &a, hipStream_t stream) {
    DE_TP_LAUNCH(de_tree_params_unpack_kernel, a.n_unknowns);
}

} // namespace de
