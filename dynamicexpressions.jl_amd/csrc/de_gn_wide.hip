// de_gn_wide.hip — the device side of de_eval_loss_gn_wide / de_gn_lm_step_wide (contract and scratch: de_gn_wide.h).
//   de_gnw_gather_kernel     the wide trees' constants out of the population's (the hidden sub-program's device set)
//   de_gnw_gram_kernel       one workgroup per (slice of GNW_SLICE samples, wide tree): the lower triangle of sum (w c) d d^T over the slice
//   de_gnw_fold_kernel       the slices of a chunk into the running totals, in order; behind the last chunk the blocks themselves
//   de_lm_step_wide_kernel   one wave per wide tree: Cholesky in double with the matrix in LDS (de_lm_solve_wide.h), a lane per row
// All on the context's stream, plain vector stores only.
//
// The Gram kernel.  A thread owns up to three entries (i, k), i <= k, of the triangle (528 entries at G = 32, 256 threads) and walks the
// slice's samples in order.  A tile of GNW_TILE samples is staged in LDS exactly as it lies in memory — G contiguous values per sample, so the
// load is one contiguous, coalesced range — with w c per sample beside it.  In the inner loop every lane reads rows[j G + i] and
// rows[j G + k] of the SAME sample j: lanes that share an index broadcast, the others hit G <= 32 consecutive dwords, so the reads are free
// of bank conflicts.  The product ((w c) d_i) d_k is formed in the element type, the association order of the narrow tree ends
// (g_epilogue_gn), and summed in double: a chain of at most GNW_TILE = 64 terms per tile, then the tiles of the slice.  A sample of
// weight zero is skipped as a whole (a select: its rows may hold anything).
#include "../../include/de_hip.h"

#include "de_gn_wide.h"
#include "de_lm_solve_wide.h"
#include "de_loss_kinds.h"

namespace de {

__device__ __forceinline__ void gnw_entry(int e, int *i, int *k) { // e = k (k + 1) / 2 + i, i <= k
    int kk = 0;
    while ((kk + 1) * (kk + 2) / 2 <= e) kk++;
    *k = kk;
    *i = e - kk * (kk + 1) / 2;
}

template <typename T>
__global__ void __launch_bounds__(256) de_gnw_gather_kernel(const T *__restrict__ full, const int64_t *__restrict__ idx, int64_t n, T *__restrict__ sub) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) sub[k] = full[idx[k]];
}

template <typename T>
__global__ void __launch_bounds__(256) de_gnw_gram_kernel(GnWideGramArgs a) {
    constexpr int PER = (DE_GN_WIDE_MAX_ROWS * (DE_GN_WIDE_MAX_ROWS + 1) / 2 + 255) / 256; // entries per thread: 3
    __shared__ T rows[GNW_TILE * DE_GN_WIDE_MAX_ROWS];
    __shared__ T wc[GNW_TILE];
    __shared__ int keep[GNW_TILE];
    const int tid = threadIdx.x, s = blockIdx.y;
    const GnWideTree tr = a.trees[s];
    const int G = tr.G, ntri = G * (G + 1) / 2;
    const T *__restrict__ jac = static_cast<const T *>(a.jac) + tr.row0 * a.n;
    const T *__restrict__ vals = static_cast<const T *>(a.vals) + (int64_t)s * a.n;
    const T *__restrict__ y = static_cast<const T *>(a.y), *__restrict__ w = static_cast<const T *>(a.w);
    const T p = (T)a.param, f = (T)a.e_floor;
    int ei[PER], ek[PER];
    double acc[PER];
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int e = tid + 256 * q;
        gnw_entry(e < ntri ? e : 0, &ei[q], &ek[q]);
        acc[q] = 0.0;
    }
    // a narrow triangle leaves whole waves and whole rounds q without an entry: they stage and wait, and skip the products
    const int nq = (ntri + 255) / 256;
    const bool idle = (tid & ~63) >= ntri;
    const int64_t j0 = (int64_t)blockIdx.x * GNW_SLICE, j1 = j0 + GNW_SLICE < a.n ? j0 + GNW_SLICE : a.n;
    for (int64_t jt = j0; jt < j1; jt += GNW_TILE) {
        const int m = (int)(j1 - jt < GNW_TILE ? j1 - jt : GNW_TILE);
        const T *__restrict__ src = jac + jt * G;
        for (int x = tid; x < m * G; x += 256) rows[x] = src[x];
        if (tid < m) {
            const int64_t j = jt + tid;
            const T wv = w ? w[j] : T(1);
            const T c = a.kind == DE_LOSS_L2 ? T(1) : loss_kind_curv_term<T>(a.kind, vals[j], y[j], p, f);
            wc[tid] = wv * c;
            keep[tid] = wv == T(0) ? 0 : 1;
        }
        __syncthreads();
        double ts[PER];
#pragma unroll
        for (int q = 0; q < PER; q++) ts[q] = 0.0;
        for (int j = 0; j < m && !idle; j++) {
            if (!keep[j]) continue; // (the same for every thread)
            const T wcj = wc[j];
            const T *r = rows + j * G;
#pragma unroll
            for (int q = 0; q < PER; q++)
                if (q < nq) ts[q] = ts[q] + (double)((wcj * r[ei[q]]) * r[ek[q]]);
        }
#pragma unroll
        for (int q = 0; q < PER; q++) acc[q] = acc[q] + ts[q];
        __syncthreads();
    }
    double *__restrict__ out = a.partial + (int64_t)blockIdx.x * a.tri_total + tr.tri0;
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int e = tid + 256 * q;
        if (e < ntri) out[e] = acc[q];
    }
}

template <typename T>
__global__ void __launch_bounds__(256) de_gnw_fold_kernel(const GnWideTree *__restrict__ trees, const double *__restrict__ partial, int64_t n_slices,
                                                          int64_t tri_total, double *__restrict__ total, int first, int last, T *__restrict__ jtj,
                                                          const uint8_t *__restrict__ ok) {
    const GnWideTree tr = trees[blockIdx.x];
    const int G = tr.G, ntri = G * (G + 1) / 2;
    for (int e = threadIdx.x; e < ntri; e += 256) {
        double t = first ? 0.0 : total[tr.tri0 + e];
        for (int64_t sl = 0; sl < n_slices; sl++) t = t + partial[sl * tri_total + tr.tri0 + e];
        total[tr.tri0 + e] = t;
        if (last) {
            int i, k;
            gnw_entry(e, &i, &k);
            const T v = ok[tr.tree] ? (T)t : (T)__builtin_nan("");
            jtj[tr.joff + i + (int64_t)G * k] = v;
            jtj[tr.joff + k + (int64_t)G * i] = v;
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(64) de_lm_step_wide_kernel(LmStepArgs a) {
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const int G = a.n_grad[t];
    if (G <= LM_MAX_ROWS || G > LM_WIDE_MAX_ROWS) return; // (the whole workgroup: one wave)
    __shared__ double A[LMW_WORK];
    __shared__ double b[LM_WIDE_MAX_ROWS];
    __shared__ int positive, solved;
    const int64_t off = a.doff[t];
    const double lam = a.lam[t];
    const T *__restrict__ H = static_cast<const T *>(a.jtj) + a.joff[t];
    const T *__restrict__ g = static_cast<const T *>(a.dloss) + off;
    bool fin = true;
    for (int x = lane; x < G * G; x += 64) { // H[i + G j] -> row i of the work matrix
        const double v = (double)H[x];
        fin = fin && lm_finite(v);
        A[(x % G) * LMW_LD + x / G] = v;
    }
    if (lane < G) {
        const double v = -0.5 * (double)g[lane];
        fin = fin && lm_finite(v);
        b[lane] = v;
    }
    if (lane == 0) { positive = 1; solved = 0; }
    const bool go = __syncthreads_and(fin ? 1 : 0) != 0 && a.has[t] != 0 && lm_finite(lam);
    if (go) { // (uniform)
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
    if (lane < G) a.step[off + lane] = sv ? b[lane] : 0.0;
    if (!a.trial || lane >= G) return;
    const T *c = static_cast<const T *>(a.consts) + a.coff[t];
    T *tr = static_cast<T *>(a.trial) + a.coff[t];
    tr[lane] = sv ? (T)((double)c[lane] + b[lane]) : c[lane]; // (no step: the bits, -0 and NaN payloads stay)
}

hipError_t launch_gnw_gather(int dtype, const void *full, const int64_t *idx, int64_t n, void *sub, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (dtype == DE_F32) hipLaunchKernelGGL(de_gnw_gather_kernel<float>, grid, dim3(256), 0, stream, static_cast<const float *>(full), idx, n, static_cast<float *>(sub));
    else hipLaunchKernelGGL(de_gnw_gather_kernel<double>, grid, dim3(256), 0, stream, static_cast<const double *>(full), idx, n, static_cast<double *>(sub));
    return hipGetLastError();
}

hipError_t launch_gnw_gram(int dtype, const GnWideGramArgs &a, hipStream_t stream) {
    if (a.n_wide <= 0 || a.n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.n + GNW_SLICE - 1) / GNW_SLICE), (unsigned)a.n_wide);
    if (dtype == DE_F32) hipLaunchKernelGGL(de_gnw_gram_kernel<float>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(de_gnw_gram_kernel<double>, grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_gnw_fold(int dtype, const GnWideTree *trees, int32_t n_wide, const double *partial, int64_t n_slices, int64_t tri_total,
                           double *total, bool first, bool last, void *jtj, const uint8_t *ok, hipStream_t stream) {
    if (n_wide <= 0) return hipSuccess;
    if (dtype == DE_F32)
        hipLaunchKernelGGL(de_gnw_fold_kernel<float>, dim3((unsigned)n_wide), dim3(256), 0, stream, trees, partial, n_slices, tri_total, total, first ? 1 : 0,
                           last ? 1 : 0, static_cast<float *>(jtj), ok);
    else
        hipLaunchKernelGGL(de_gnw_fold_kernel<double>, dim3((unsigned)n_wide), dim3(256), 0, stream, trees, partial, n_slices, tri_total, total, first ? 1 : 0,
                           last ? 1 : 0, static_cast<double *>(jtj), ok);
    return hipGetLastError();
}

hipError_t launch_lm_step_wide(int dtype, const LmStepArgs &a, hipStream_t stream) {
    if (a.n_trees <= 0) return hipSuccess;
    if (dtype == DE_F32) hipLaunchKernelGGL(de_lm_step_wide_kernel<float>, dim3((unsigned)a.n_trees), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL(de_lm_step_wide_kernel<double>, dim3((unsigned)a.n_trees), dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace de
