// de_const_patch.hip — the device side of de_program_set_consts_device: new constants go from a device buffer into every
// record of the program's device streams that carries one, the constant subtrees are re-evaluated by de_fold_kernel (de_kernels.hip) and
// the per-tree flags recomputed — three small data-parallel kernels, all on the context's stream, nothing read back.
//   de_const_gather_kernel   the fold kernel's constant images from the constants
//   de_const_scatter_kernel  one thread per (source, site): constants and fold results into the streams
//   de_const_flags_kernel    one thread per tree: recompute_host_ok (de_api_program.cpp)
// The tables (sites, sources, per-tree fold lists) are made on the host from the bookkeeping de_program_set_consts patches by
// (de_api_program.cpp build_const_patch_tables); a site's address was bounds-checked there against the stream it lies in.
#include "de_const_patch.h"
#include "de_lower.h"

#include "../../include/de_hip.h"

namespace de {

template <typename T>
__global__ void __launch_bounds__(256) de_const_gather_kernel(const T *__restrict__ consts, const int64_t *__restrict__ idx, int64_t n0,
                                                              T *__restrict__ dst0, int64_t n1, T *__restrict__ dst1) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n0 + n1) return;
    const T v = consts[idx[k]];
    if (k < n0) dst0[k] = v;
    else dst1[k - n0] = v;
}

template <typename T>
__global__ void __launch_bounds__(256) de_const_scatter_kernel(const T *__restrict__ vals, const uint64_t *__restrict__ addr,
                                                               const uint32_t *__restrict__ src, int64_t n_sites) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_sites) return;
    const uint64_t a = addr[i];
    const T v = vals[src[i]];
    if constexpr (sizeof(T) == 4) {
        const uint32_t bits = __float_as_uint(v);
        if (a & CONST_SITE_32) *reinterpret_cast<uint32_t *>(a & ~(uint64_t)3) = bits; // (the `.arg` word of a chained record)
        else *reinterpret_cast<uint64_t *>(a) = (uint64_t)bits;                            // (.lo = the bits, .hi = 0: write_imm)
    } else {
        *reinterpret_cast<uint64_t *>(a) = (uint64_t)__double_as_longlong(v);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) de_const_flags_kernel(const T *__restrict__ vals, const int64_t *__restrict__ const_off,
                                                             const uint8_t *__restrict__ const_checks, const int32_t *__restrict__ tfold_off,
                                                             const uint32_t *__restrict__ tfold, const uint8_t *__restrict__ fold_ok,
                                                             int64_t n_trees, int ee, uint8_t *__restrict__ ok_eval, uint8_t *__restrict__ ok_grad) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_trees) return;
    bool eval = true, grad = true;
    for (int64_t k = const_off[t]; k < const_off[t + 1]; k++) {
        const bool fin = isfinite(vals[k]);
        grad = grad && fin;
        const uint8_t ch = const_checks[k];
        if (!fin && ((ch & CONST_CHECK_ALWAYS) || (ee && (ch & CONST_CHECK_EE)))) eval = false;
    }
    // a constant subtree with a non-finite value: tested whatever the options (dispatch_constant_tree) or only under early exit
    for (int32_t q = tfold_off[t]; q < tfold_off[t + 1]; q++) {
        const uint32_t e = tfold[q];
        if (!fold_ok[e >> 1] && ((e & 1u) || ee)) eval = false;
    }
    ok_eval[t] = eval ? 1 : 0;
    if (ok_grad) ok_grad[t] = grad ? 1 : 0;
}

static inline dim3 grid_of(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

hipError_t launch_const_gather(int dtype, const void *consts, const int64_t *idx, int64_t n0, void *dst0, int64_t n1, void *dst1, hipStream_t stream) {
    if (n0 + n1 <= 0) return hipSuccess;
    if (dtype == DE_F32)
        hipLaunchKernelGGL(de_const_gather_kernel<float>, grid_of(n0 + n1), dim3(256), 0, stream, static_cast<const float *>(consts), idx, n0,
                           static_cast<float *>(dst0), n1, static_cast<float *>(dst1));
    else
        hipLaunchKernelGGL(de_const_gather_kernel<double>, grid_of(n0 + n1), dim3(256), 0, stream, static_cast<const double *>(consts), idx, n0,
                           static_cast<double *>(dst0), n1, static_cast<double *>(dst1));
    return hipGetLastError();
}

hipError_t launch_const_scatter(int dtype, const void *vals, const uint64_t *addr, const uint32_t *src, int64_t n_sites, hipStream_t stream) {
    if (n_sites <= 0) return hipSuccess;
    if (dtype == DE_F32)
        hipLaunchKernelGGL(de_const_scatter_kernel<float>, grid_of(n_sites), dim3(256), 0, stream, static_cast<const float *>(vals), addr, src, n_sites);
    else
        hipLaunchKernelGGL(de_const_scatter_kernel<double>, grid_of(n_sites), dim3(256), 0, stream, static_cast<const double *>(vals), addr, src, n_sites);
    return hipGetLastError();
}

hipError_t launch_const_flags(int dtype, const void *vals, const int64_t *const_off, const uint8_t *const_checks, const int32_t *tfold_off,
                              const uint32_t *tfold, const uint8_t *fold_ok, int64_t n_trees, bool early_exit, uint8_t *ok_eval, uint8_t *ok_grad,
                              hipStream_t stream) {
    if (n_trees <= 0) return hipSuccess;
    if (dtype == DE_F32)
        hipLaunchKernelGGL(de_const_flags_kernel<float>, grid_of(n_trees), dim3(256), 0, stream, static_cast<const float *>(vals), const_off,
                           const_checks, tfold_off, tfold, fold_ok, n_trees, early_exit ? 1 : 0, ok_eval, ok_grad);
    else
        hipLaunchKernelGGL(de_const_flags_kernel<double>, grid_of(n_trees), dim3(256), 0, stream, static_cast<const double *>(vals), const_off,
                           const_checks, tfold_off, tfold, fold_ok, n_trees, early_exit ? 1 : 0, ok_eval, ok_grad);
    return hipGetLastError();
}

} // namespace de
