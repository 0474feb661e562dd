// de_grad_kernels.hip — forward-mode gradient of a population of trees on gfx950: the Float32 / Float64 arithmetic policy of the tape
// interpreter (de_grad_tape.h: the kernel, its semantics and the one launch path), the finish kernels of the fused reductions, and the
// launch of the threaded and reverse kernels (de_grad_threaded.hip, de_rev_threaded.hip).
// Partial derivatives restate ChainRules' scalar rules (same table as oracle/de_oracle_ops.h).
#include "de_grad_tape.h"
#include <memory>
#include <mutex>
#include <utility>
#include <vector>
#include <algorithm>
#include <cstdlib>

namespace de {

// The real policy of de_grad_tape_kernel: a value is a T, in memory, in registers and in LDS; plain IEEE arithmetic.
template <typename T> struct RealGrad {
    typedef T Elem;
    typedef T V;
    static constexpr bool TREE_ENDS = true;
    static constexpr const char *NAMES[3] = {"de_grad_tape_kernel", "de_grad_tape_kernel<GN>", "de_grad_tape_kernel<FIT>"};

    static __device__ __forceinline__ void stage_x(T *rows, const T *X, int64_t ldX, uint32_t F, int64_t base, int64_t N, int) {
        stage_x_rows<T>(rows, X, ldX, F, GBLK, base, N - 1, [](uint32_t j, uint32_t f) { return f * GRAD_TAPE_ROW + j; });
    }
    static __device__ __forceinline__ T imm(U32x4 w) { return gimm<T>(w.z, w.w); }

    template <int K> static __device__ __forceinline__ BG<T> bin(T lx, T ly) {
        BG<T> r;
        if (K == 0) { r.v = lx + ly; r.gx = T(1); r.gy = T(1); }
        else if (K == 1 || K == 2) { r.v = lx - ly; r.gx = T(1); r.gy = T(-1); }
        else if (K == 3) { r.v = lx * ly; r.gx = ly; r.gy = lx; }
        else { r.v = lx / ly; r.gx = T(1) / ly; r.gy = -(r.v / ly); }
        return r;
    }
    template <int K> static __device__ __forceinline__ T bin_dual(T gl, T dl, T gr, T dr) { return gl * dl + gr * dr; }
    template <int K> static __device__ __forceinline__ UG<T> un(T xin) {
        UG<T> r;
        if (sizeof(T) == 4) {
            if (K == 1) { r.y = (T)fast_exp_f32((float)xin); r.g = r.y; }
            else {
                float sn, cs;
                fast_sincos_f32((float)xin, &sn, &cs);
                if (K == 0) { r.y = (T)cs; r.g = (T)-sn; } else { r.y = (T)sn; r.g = (T)cs; }
                // per ELEMENT: a sample's value must not depend on its wave neighbours
                if (__ballot(M<T>::abs(xin) > T(DE_TRIG_FAST_BOUND)) != 0ull) {
                    const UG<T> slow = unary_vg<T>(K == 0 ? DE_U_COS : DE_U_SIN, xin);
                    if (M<T>::abs(xin) > T(DE_TRIG_FAST_BOUND)) r = slow;
                }
            }
        } else r = unary_vg<T>(K == 0 ? DE_U_COS : (K == 1 ? DE_U_EXP : DE_U_SIN), xin);
        return r;
    }
    static __device__ __forceinline__ T scale(T g, T d) { return g * d; }
    static __device__ __forceinline__ T chain2(T g1, T d1, T g2, T d2) { return g1 * d1 + g2 * d2; }
    static __device__ __forceinline__ T chain3(T g0, T a, T g1, T b, T g2, T c) { return (g0 * a + g1 * b) + g2 * c; }
    static __device__ __forceinline__ UG<T> unary(uint32_t op, T x) { return unary_vg<T>(op, x); }
    static __device__ __forceinline__ BG<T> binary(uint32_t op, T x, T y) { return binary_vg<T>(op, x, y); }
    static __device__ __forceinline__ TG<T> ternary(uint32_t op, T x, T y, T z) { return ternary_vg<T>(op, x, y, z); }
};

// Pass 3 of the fused loss+pullback reduction: thread = one reduction column (a tree's loss or one of its
// gradient rows; the owner is found by bisection in col_off); fixed summation order.  NaN where the evaluation
// was incomplete (src/ChainRules.jl:62-64 `dX_constants_dY .= NaN`).
template <typename T>
__global__ void __launch_bounds__(256) de_loss_grad_finish_kernel(const double *__restrict__ seg_sum, int64_t n_trees, int64_t n_cols,
                                                                 int32_t n_segs, const int64_t *__restrict__ col_off,
                                                                 const uint8_t *__restrict__ ok,
                                                                 T *__restrict__ loss, T *__restrict__ dloss,
                                                                 const int64_t *__restrict__ dloss_off) {
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= n_cols) return;
    int64_t lo = 0, hi = n_trees; // col_off[lo] <= col < col_off[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (col_off[mid] <= col) lo = mid;
        else hi = mid;
    }
    const int64_t t = lo;
    const int c = (int)(col - col_off[t]);
    double s = 0.0;
    for (int32_t g = 0; g < n_segs; ++g)
        for (int w = 0; w < 4; ++w) s += seg_sum[((int64_t)g * n_cols + col) * 4 + w];
    const T v = ok[t] != 0 ? (T)s : M<T>::nan();
    if (c == 0) { if (loss) loss[t] = v; }
    else dloss[dloss_off[t] + c - 1] = v;
}

// ... of de_eval_loss_gn: a tree of G <= gn_max rows owns G (G + 1) / 2 more columns, entry (i, k), i <= k, of its Gauss-Newton matrix at
// 1 + G + k (k + 1) / 2 + i.  Loss and gradient exactly as above (same segment order, same bits); every triangle entry goes into both halves of
// the tree's column-major G x G block at jtj_off[t]; the thread of a wider tree's loss column fills its block with NaN.
template <typename T>
__global__ void __launch_bounds__(256) de_loss_gn_finish_kernel(const double *__restrict__ seg_sum, int64_t n_trees, int64_t n_cols,
                                                               int32_t n_segs, const int64_t *__restrict__ col_off,
                                                               const int32_t *__restrict__ n_grad, const uint8_t *__restrict__ ok,
                                                               T *__restrict__ loss, T *__restrict__ dloss,
                                                               const int64_t *__restrict__ dloss_off, T *__restrict__ jtj,
                                                               const int64_t *__restrict__ jtj_off, int32_t gn_max) {
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= n_cols) return;
    int64_t lo = 0, hi = n_trees; // col_off[lo] <= col < col_off[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (col_off[mid] <= col) lo = mid;
        else hi = mid;
    }
    const int64_t t = lo;
    const int c = (int)(col - col_off[t]);
    const int G = n_grad[t];
    double s = 0.0;
    for (int32_t g = 0; g < n_segs; ++g)
        for (int w = 0; w < 4; ++w) s += seg_sum[((int64_t)g * n_cols + col) * 4 + w];
    const T v = ok[t] != 0 ? (T)s : M<T>::nan();
    if (c == 0) {
        if (loss) loss[t] = v;
        if (G > gn_max) {
            T *__restrict__ blk = jtj + jtj_off[t];
            for (int64_t e = 0; e < (int64_t)G * G; e++) blk[e] = M<T>::nan();
        }
    } else if (c <= G) dloss[dloss_off[t] + c - 1] = v;
    else {
        const int e = c - 1 - G;
        int k = 0;
        while ((k + 1) * (k + 2) / 2 <= e) ++k;
        const int i = e - k * (k + 1) / 2;
        T *__restrict__ blk = jtj + jtj_off[t];
        blk[i + (int64_t)G * k] = v;
        blk[k + (int64_t)G * i] = v;
    }
}

// ---- de_eval_fit_stats_grad: the recombination of the per-wave columns of g_epilogue_fit, everything in double, every sum
// in a fixed order.  Two passes over the partials, because the shift of a wave's sums, m - mu, needs the tree's mean mu first.
struct FitGradReduce {
    const void *partial;        // [n_tiles][n_cols][4 waves], element type
    int64_t n_trees, n_cols, n_tiles, tiles_per_seg;
    int32_t n_segs, gn_max, want_j;
    const int64_t *col_off;
    const int32_t *n_grad;
    const uint8_t *ok;
    const double *ystats;       // {W, mean_y, M2_y}
    double *seg_a;              // [n_segs][n_trees]: sum over the segment's waves of m W_wave + S1
    double *seg_b;              // [n_segs][n_cols][4 waves]
    const double *tile_r;       // [n_tiles]: sum w yc per 256 samples, in double (the pre-pass over y / w, launch_fit_ystats)
    double *rsum;               // their sum R = W (mean_y - T(mean_y)), the mean of y to more than a double's precision
    double *stats, *dmom;
    const int64_t *dmom_off;
    void *jtj;
    const int64_t *jtj_off;
};
// Pass 1: thread = one tree, block row = one segment of tiles: the numerator of the tree's mean.
template <typename T> __global__ void __launch_bounds__(256) de_fit_grad_reduce_mu_kernel(const FitGradReduce a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n_trees) return;
    const T *__restrict__ partial = static_cast<const T *>(a.partial);
    const int64_t r0 = (int64_t)blockIdx.y * a.tiles_per_seg;
    const int64_t r1 = r0 + a.tiles_per_seg < a.n_tiles ? r0 + a.tiles_per_seg : a.n_tiles;
    double s = 0.0;
    for (int64_t r = r0; r < r1; ++r) {
        const T *__restrict__ q = partial + (r * a.n_cols + a.col_off[t]) * 4;
        for (int w = 0; w < 4; ++w) s += (double)q[w] * (double)q[16 + w] + (double)q[4 + w];
    }
    a.seg_a[(int64_t)blockIdx.y * a.n_trees + t] = s;
}
__device__ __forceinline__ int64_t fit_grad_owner(const int64_t *__restrict__ col_off, int64_t n_trees, int64_t col) {
    int64_t lo = 0, hi = n_trees; // col_off[lo] <= col < col_off[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (col_off[mid] <= col) lo = mid;
        else hi = mid;
    }
    return lo;
}
// Pass 2, with mu known: thread = one column, block row = one segment; per wave slot, over the segment's tiles,
//   B: B + 2 (m - mu) S1 + W_wave (m - mu)^2      Cc: Cc + (m - mu) R_wave      P'_k: P'_k + (m - mu) D_k,wave      D_k, Q'_k, triangle: as they are
// — identities for any shift m.  The triangle's sums are de_loss_reduce_tiles_kernel's: the same bits as de_eval_loss_gn's.
template <typename T> __global__ void __launch_bounds__(256) de_fit_grad_reduce_cols_kernel(const FitGradReduce a) {
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= a.n_cols) return;
    const int64_t t = fit_grad_owner(a.col_off, a.n_trees, col);
    const int c = (int)(col - a.col_off[t]), G = a.n_grad[t];
    const T *__restrict__ partial = static_cast<const T *>(a.partial);
    double mu = 0.0;
    for (int32_t g = 0; g < a.n_segs; ++g) mu += a.seg_a[(int64_t)g * a.n_trees + t];
    mu /= a.ystats[0];
    const int kind = c == 2 ? 1 : (c == 3 ? 2 : (c >= FIT_COLS + G && c < FIT_COLS + 2 * G ? 3 : 0));
    const int64_t r0 = (int64_t)blockIdx.y * a.tiles_per_seg;
    const int64_t r1 = r0 + a.tiles_per_seg < a.n_tiles ? r0 + a.tiles_per_seg : a.n_tiles;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t r = r0; r < r1; ++r) {
        const T *__restrict__ q = partial + (r * a.n_cols + a.col_off[t]) * 4;
        for (int w = 0; w < 4; ++w) {
            double v = (double)q[c * 4 + w];
            if (kind) {
                const double dm = (double)q[w] - mu;
                if (kind == 1) v = (v + (2.0 * dm) * (double)q[4 + w]) + ((double)q[16 + w] * dm) * dm;
                else if (kind == 2) v = v + dm * (double)q[20 + w];
                else v = v + dm * (double)q[(c - G) * 4 + w];
            }
            s[w] += v;
        }
    }
    for (int w = 0; w < 4; ++w) a.seg_b[(((int64_t)blockIdx.y * a.n_cols) + col) * 4 + w] = s[w];
}
// R = sum_tiles tile_r, one block, a fixed order
__global__ void __launch_bounds__(256) de_fit_grad_rsum_kernel(const double *__restrict__ tile_r, int64_t n_tiles, double *__restrict__ rsum) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n_tiles; i += 256) s += tile_r[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) rsum[0] = sh[0];
}
// Pass 3: thread = one column: segments in order, the four wave slots inside (de_loss_gn_finish_kernel's order).  NaN where the evaluation
// was incomplete; W == 0: the mean is NaN, everything else 0.  Q_k = sum Q'_k + (T(mean_y) - mean_y) D_k: unlike C, Q is not invariant under
// the shift of y — and D_k (W for an additive constant) multiplies whatever error the shift carries, so mean_y is taken as T(mean_y) + R / W
// with R = sum w (y - T(mean_y)) in double, not as the double ystats[1] (whose rounding alone, times W, exceeds Q's bound for a Float64
// target with an offset): the shift is -R / W.  The thread of a tree's column 0 writes its mean and, where the tree is wider than
// gn_max, the NaN block.
template <typename T> __global__ void __launch_bounds__(256) de_fit_grad_finish_kernel(const FitGradReduce a) {
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= a.n_cols) return;
    const int64_t t = fit_grad_owner(a.col_off, a.n_trees, col);
    const int c = (int)(col - a.col_off[t]), G = a.n_grad[t];
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const double W = a.ystats[0];
    const bool good = a.ok[t] != 0, empty = W == 0.0;
    auto total = [&](int64_t cc) {
        double s = 0.0;
        for (int32_t g = 0; g < a.n_segs; ++g)
            for (int w = 0; w < 4; ++w) s += a.seg_b[(((int64_t)g * a.n_cols) + cc) * 4 + w];
        return s;
    };
    if (c == 0) {
        double mu = 0.0;
        for (int32_t g = 0; g < a.n_segs; ++g) mu += a.seg_a[(int64_t)g * a.n_trees + t];
        mu /= W;
        a.stats[3 * t] = good && !empty ? mu : nan;
        if (a.want_j && G > a.gn_max) {
            T *__restrict__ blk = static_cast<T *>(a.jtj) + a.jtj_off[t];
            for (int64_t e = 0; e < (int64_t)G * G; e++) blk[e] = M<T>::nan();
        }
        return;
    }
    if (c == 1 || c == 4 || c == 5) return;
    double v = empty ? 0.0 : total(col);
    if (c == 2 || c == 3) {
        if (c == 2 && v < 0.0) v = 0.0; // (a sum of squares: only the roundings of a constant tree can take it below 0)
        a.stats[3 * t + (c - 1)] = good ? v : nan;
    } else if (c < FIT_COLS + 3 * G) {
        if (c >= FIT_COLS + 2 * G && !empty) {
            v -= (a.rsum[0] / W) * total(col - 2 * G);
        }
        a.dmom[a.dmom_off[t] + (c - FIT_COLS)] = good ? v : nan;
    } else {
        const int e = c - FIT_COLS - 3 * G;
        int k = 0;
        while ((k + 1) * (k + 2) / 2 <= e) ++k;
        const int i = e - k * (k + 1) / 2;
        T *__restrict__ blk = static_cast<T *>(a.jtj) + a.jtj_off[t];
        const T vj = good ? (T)v : M<T>::nan();
        blk[i + (int64_t)G * k] = vj;
        blk[k + (int64_t)G * i] = vj;
    }
}
size_t fit_grad_seg_bytes(int64_t n_trees, int64_t n_cols, int64_t N) {
    const int64_t n_tiles = (N + GBLK - 1) / GBLK;
    return ((size_t)loss_segments(n_tiles) * ((size_t)n_trees + 4 * (size_t)n_cols) + 1) * sizeof(double);
}
template <typename T> static hipError_t fit_grad_finish_t(const GradArgs &ga, int64_t n_tiles, hipStream_t stream) {
    FitGradReduce a;
    a.partial = ga.loss->partial;
    a.n_trees = ga.e.n_trees;
    a.n_cols = ga.n_cols;
    a.n_tiles = n_tiles;
    a.n_segs = loss_segments(n_tiles);
    a.tiles_per_seg = (n_tiles + a.n_segs - 1) / a.n_segs;
    a.gn_max = DE_GN_MAX_ROWS;
    a.want_j = ga.fit_jtj ? 1 : 0;
    a.col_off = ga.col_off;
    a.n_grad = ga.n_grad;
    a.ok = ga.e.ok;
    a.ystats = ga.loss->ystats;
    a.seg_a = ga.fit_seg;
    a.seg_b = ga.fit_seg + (int64_t)a.n_segs * a.n_trees;
    a.rsum = a.seg_b + (int64_t)a.n_segs * a.n_cols * 4;
    a.tile_r = ga.fit_seg - 2 * n_tiles; // (GradArgs::fit_seg: behind the pre-pass's three per-tile arrays {W, R, Q})
    a.stats = ga.loss->stats;
    a.dmom = static_cast<double *>(ga.dloss);
    a.dmom_off = ga.dloss_off;
    a.jtj = ga.jtj;
    a.jtj_off = ga.jtj_off;
    hipLaunchKernelGGL(de_fit_grad_rsum_kernel, dim3(1), dim3(256), 0, stream, a.tile_r, n_tiles, a.rsum);
    hipLaunchKernelGGL(de_fit_grad_reduce_mu_kernel<T>, dim3((unsigned)((a.n_trees + 255) / 256), (unsigned)a.n_segs), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(de_fit_grad_reduce_cols_kernel<T>, dim3((unsigned)((a.n_cols + 255) / 256), (unsigned)a.n_segs), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(de_fit_grad_finish_kernel<T>, dim3((unsigned)((a.n_cols + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}


// passes 2 and 3 of the deterministic loss-gradient reduction (pass 2 is shared with de_eval_loss)
template <typename T> static hipError_t loss_grad_finish_t(const GradArgs &ga, int64_t n_tiles, hipStream_t stream) {
    if (ga.fit) return fit_grad_finish_t<T>(ga, n_tiles, stream);
    int32_t n_segs = 1;
    hipError_t st = launch_loss_reduce_tiles(sizeof(T) == 4 ? DE_F32 : DE_F64, ga.loss->partial, ga.n_cols * 4, n_tiles, ga.loss->seg_sum,
                                             &n_segs, stream);
    if (st != hipSuccess) return st;
    if (ga.gn) {
        hipLaunchKernelGGL(de_loss_gn_finish_kernel<T>, dim3((unsigned)((ga.n_cols + 255) / 256)), dim3(256), 0, stream,
                           static_cast<const double *>(ga.loss->seg_sum), (int64_t)ga.e.n_trees, ga.n_cols, n_segs, ga.col_off, ga.n_grad,
                           ga.e.ok, static_cast<T *>(ga.loss->loss), static_cast<T *>(ga.dloss), ga.dloss_off, static_cast<T *>(ga.jtj),
                           ga.jtj_off, (int32_t)DE_GN_MAX_ROWS);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(de_loss_grad_finish_kernel<T>, dim3((unsigned)((ga.n_cols + 255) / 256)), dim3(256), 0, stream,
                       static_cast<const double *>(ga.loss->seg_sum), (int64_t)ga.e.n_trees, ga.n_cols, n_segs, ga.col_off,
                       ga.e.ok, static_cast<T *>(ga.loss->loss), static_cast<T *>(ga.dloss), ga.dloss_off);
    return hipGetLastError();
}
hipError_t launch_loss_grad_finish_range(int dtype, const GradArgs &ga, int64_t tile0, int64_t n_tiles, void *loss, void *dloss, hipStream_t stream) {
    LossArgs la = *ga.loss;
    GradArgs g = ga;
    la.partial = static_cast<char *>(la.partial) + (size_t)tile0 * (size_t)ga.n_cols * 4 * (dtype == DE_F32 ? 4 : 8);
    la.loss = loss;
    g.loss = &la;
    g.dloss = dloss;
    return dtype == DE_F32 ? loss_grad_finish_t<float>(g, n_tiles, stream) : loss_grad_finish_t<double>(g, n_tiles, stream);
}
hipError_t launch_loss_grad_finish(int dtype, const GradArgs &ga, int64_t n_tiles, hipStream_t stream) {
    return dtype == DE_F32 ? loss_grad_finish_t<float>(ga, n_tiles, stream) : loss_grad_finish_t<double>(ga, n_tiles, stream);
}

// ---- de_eval_loss_grad_by_class: fold the per-class passes into the outputs ---------------------------
// One thread per tree; classes are added in index order, in double: reproducible.
template <typename T>
__global__ void __launch_bounds__(256) de_by_class_combine_kernel(const ByClassArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n_trees) return;
    const T *loss_c = static_cast<const T *>(a.loss_c), *dloss_c = static_cast<const T *>(a.dloss_c);
    T *dloss = static_cast<T *>(a.dloss), *dparams = static_cast<T *>(a.dparams);
    const int C = a.n_classes, P = a.n_params, G = a.n_grad[t];
    const int64_t off = a.dloss_off[t];
    bool ok = true;
    for (int c = 0; c < C; c++) ok = ok && a.ok_c[(int64_t)c * a.ok_stride + t] != 0;
    a.ok[t] = ok ? 1 : 0;
    const T nan = T(__builtin_nan(""));
    if (a.loss) {
        double s = 0.0;
        for (int c = 0; c < C; c++) s += (double)loss_c[(int64_t)c * a.n_trees + t];
        static_cast<T *>(a.loss)[t] = ok ? (T)s : nan; // incomplete evaluations are NaN-filled (src/EvaluationHelpers.jl:29-33)
    }
    for (int k = 0; k < G; k++) {
        double s = 0.0;
        for (int c = 0; c < C; c++) {
            const T v = dloss_c[(int64_t)c * a.span + off + k];
            s += (double)v;
            if (k < P) dparams[((int64_t)t * C + c) * P + k] = ok ? v : nan;
        }
        dloss[off + k] = ok ? (T)s : nan;
    }
}
// EvalPullback's `dX = dX_dY .* reshape(dY, 1, :)` (src/ChainRules.jl:74) on the Jacobians de_eval_grad just wrote:
// tree t's [G, N] block (gradient index fastest) is scaled column j by dY[j]; an incomplete tree is NaN-filled
// (`dX_constants_dY .= NaN`, :62-64).  blockIdx.y = tree, 16-byte accesses where the block is aligned.
template <typename T>
__global__ void __launch_bounds__(256) de_pullback_scale_kernel(T *__restrict__ grad, const int64_t *__restrict__ grad_off,
                                                               const int32_t *__restrict__ n_grad, const uint8_t *__restrict__ ok,
                                                               const T *__restrict__ dY, int64_t N, int64_t n_trees) {
    for (int64_t t = blockIdx.y; t < n_trees; t += gridDim.y) { // (gridDim.y <= 65535: larger populations stride)
        const uint32_t G = (uint32_t)n_grad[t];
        if (G == 0) continue;
        T *__restrict__ g = grad + grad_off[t];
        const bool complete = ok[t] != 0;
        const int64_t total = (int64_t)G * N;
        for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
            const int64_t j = e / G;
            g[e] = complete ? g[e] * dY[j] : M<T>::nan();
        }
    }
}
hipError_t launch_pullback_scale(int dtype, void *grad, const int64_t *grad_off, const int32_t *n_grad, const uint8_t *ok,
                                 const void *dY, int64_t N, int64_t n_trees, int32_t max_grad, hipStream_t stream) {
    if (n_trees <= 0 || N <= 0 || max_grad <= 0) return hipSuccess;
    int64_t bx = ((int64_t)max_grad * N + 256 * 8 - 1) / (256 * 8);
    if (bx > 4096) bx = 4096;
    const dim3 grid((unsigned)bx, (unsigned)(n_trees < 65535 ? n_trees : 65535)); // HIP limits gridDim.y: the kernel strides over trees
    if (dtype == DE_F32)
        hipLaunchKernelGGL(de_pullback_scale_kernel<float>, grid, dim3(256), 0, stream, static_cast<float *>(grad), grad_off, n_grad, ok,
                           static_cast<const float *>(dY), N, n_trees);
    else
        hipLaunchKernelGGL(de_pullback_scale_kernel<double>, grid, dim3(256), 0, stream, static_cast<double *>(grad), grad_off, n_grad, ok,
                           static_cast<const double *>(dY), N, n_trees);
    return hipGetLastError();
}

hipError_t launch_by_class_combine(int dtype, const ByClassArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.n_trees + 255) / 256));
    if (dtype == DE_F32) hipLaunchKernelGGL(de_by_class_combine_kernel<float>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(de_by_class_combine_kernel<double>, grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

// ---- threaded variants: one module per (type, window, samples per lane) — de_grad_threaded.hip — and, for reverse accumulation, one
// per element type — de_rev_threaded.hip.  DE_GT_ALL is THE list of the former: build.sh reads its entries from this file.
// (Float64: windows of <= 5 rows — wider states than 16 dwords would be passed through scratch memory)
#define DE_GT_ALL(X)                                                                                     \
    X(f, 1, 1) X(f, 2, 1) X(f, 3, 1) X(f, 4, 1) X(f, 5, 1) X(f, 6, 1) X(f, 8, 1)                          \
    X(f, 1, 2) X(f, 2, 2) X(f, 3, 2) X(f, 4, 2) X(f, 5, 2) X(f, 6, 2)                                     \
    X(d, 1, 1) X(d, 2, 1) X(d, 3, 1) X(d, 4, 1) X(d, 5, 1)
#define DE_GT_DECL(TAG, GC, V) GradModule grad_thr_module_##TAG##GC##v##V();
DE_GT_ALL(DE_GT_DECL)
GradModule rev_thr_module_f();
GradModule rev_thr_module_d();

static bool grad_thr_module(int dtype, int GC, int VS, GradModule *m) {
    static const struct { int dtype, GC, VS; GradModule (*get)(); } all[] = {
#define DE_GT_ROW(TAG, GC, V) {#TAG[0] == 'f' ? DE_F32 : DE_F64, GC, V, grad_thr_module_##TAG##GC##v##V},
        DE_GT_ALL(DE_GT_ROW)};
    for (const auto &r : all)
        if (r.dtype == dtype && r.GC == GC && r.VS == VS) { if (m) *m = r.get(); return true; }
    return false;
}
bool grad_threaded_has(int dtype, int GC, int VS) { return grad_thr_module(dtype, GC, VS, nullptr); }

hipError_t grad_handler_table(int dtype, int GC, int VS, uint64_t *table) {
    GradModule m;
    if (!grad_thr_module(dtype, GC, VS, &m)) return hipErrorInvalidValue;
    return handler_table(m.fill, gop_count(GC), table);
}
hipError_t rev_handler_table(int dtype, uint64_t *table) {
    return handler_table((dtype == DE_F32 ? rev_thr_module_f() : rev_thr_module_d()).fill, ROP_COUNT, table);
}

// Side streams of a caller's stream: the buckets of one gradient call (one launch — with its probe launch in front — per window width and
// samples-per-lane class: 2 ... 9 per call) are independent of each other, and each is short enough (0.2 ... 1.7 ms at 10^6 samples)
// that its ramp and tail are a tenth of it; spread over DE_GRAD_STREAMS streams (default 3; 1 = all on the caller's stream) the tail of
// one bucket runs beside the next.  Fork / join by events (legal under stream capture); one set per caller stream, made on first use.
struct SideStreams {
    hipStream_t s[3] = {nullptr, nullptr, nullptr};
    hipEvent_t fork = nullptr, join[3] = {nullptr, nullptr, nullptr};
    int n = 0;
};
static SideStreams *side_streams_of(hipStream_t main, int want) {
    static std::mutex mu;
    static std::vector<std::pair<std::pair<int, hipStream_t>, std::unique_ptr<SideStreams>>> all;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    const std::lock_guard<std::mutex> lock(mu);
    for (auto &e : all) if (e.first.first == dev && e.first.second == main) return e.second->n >= want ? e.second.get() : nullptr;
    if (all.size() >= 32) return nullptr; // a caller that makes a new stream per call: no side streams for the later ones (nothing is ever freed here)
    std::unique_ptr<SideStreams> ss(new SideStreams());
    if (hipEventCreateWithFlags(&ss->fork, hipEventDisableTiming) != hipSuccess) return nullptr;
    for (int i = 0; i < 3; i++) {
        if (hipStreamCreateWithFlags(&ss->s[i], hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&ss->join[i], hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            break;
        }
        ss->n = i + 1;
    }
    all.emplace_back(std::make_pair(dev, main), std::move(ss));
    SideStreams *r = all.back().second.get();
    return r->n >= want ? r : nullptr;
}

// n_launches independent launch sequences of one call over the caller's stream and its side streams: fork(), next() per sequence, join()
struct ForkJoin {
    hipStream_t main;
    SideStreams *ss = nullptr;
    int n_side = 0, slot = 0;
    ForkJoin(hipStream_t m, int n_launches) : main(m) {
        static const int n_env = [] { const char *v = getenv("DE_GRAD_STREAMS"); const int n = v ? atoi(v) : 3; return n < 1 ? 1 : (n > 4 ? 4 : n); }();
        n_side = n_launches >= 2 ? std::min(n_env, n_launches) - 1 : 0;
        ss = n_side > 0 ? side_streams_of(m, n_side) : nullptr;
        if (!ss) n_side = 0;
    }
    hipError_t fork() {
        if (!ss) return hipSuccess;
        hipError_t st = hipEventRecord(ss->fork, main);
        for (int i = 0; i < n_side && st == hipSuccess; i++) st = hipStreamWaitEvent(ss->s[i], ss->fork, 0);
        return st;
    }
    hipStream_t next() {
        const int k = slot++ % (n_side + 1);
        return k == 0 ? main : ss->s[k - 1];
    }
    hipError_t join() { // (also after an error: the side streams must not run on behind the caller's back)
        hipError_t err = hipSuccess;
        for (int i = 0; i < n_side; i++) {
            hipError_t st = hipEventRecord(ss->join[i], ss->s[i]);
            if (st == hipSuccess) st = hipStreamWaitEvent(main, ss->join[i], 0);
            if (st != hipSuccess && err == hipSuccess) err = st;
        }
        return err;
    }
};

// de_eval_loss_grad_by_class: the pair of finish passes of every class over its own tiles (class k: tiles [tile0[k], tile0[k + 1])) — 2 C
// launches of ~25 us each, independent of each other except for the segment sums they stage: spread over the caller's stream and its side
// streams, each with a region of its own in `seg_sum` (seg_stride bytes apart; classes of one stream run in order).  Same launches, same
// reduction order per class: the same bits as one call per class.
hipError_t launch_loss_grad_finish_ranges(int dtype, const GradArgs &ga, int64_t n_classes, const int64_t *tile0, void *loss, size_t loss_stride,
                                          void *dloss, size_t dloss_stride, size_t seg_stride, int seg_regions, hipStream_t stream) {
    ForkJoin fj(stream, seg_regions > 1 ? (int)std::min<int64_t>(n_classes, seg_regions) : 1);
    hipError_t first_err = fj.fork();
    if (first_err != hipSuccess) return first_err;
    for (int64_t k = 0; k < n_classes; k++) {
        const int slot = fj.slot % (fj.n_side + 1);
        const hipStream_t ks = fj.next();
        LossArgs la = *ga.loss;
        GradArgs g = ga;
        la.partial = static_cast<char *>(la.partial) + (size_t)tile0[k] * (size_t)ga.n_cols * 4 * (dtype == DE_F32 ? 4 : 8);
        la.seg_sum = static_cast<char *>(la.seg_sum) + (size_t)slot * seg_stride;
        la.loss = static_cast<char *>(loss) + (size_t)k * loss_stride;
        g.loss = &la;
        g.dloss = static_cast<char *>(dloss) + (size_t)k * dloss_stride;
        const hipError_t st = dtype == DE_F32 ? loss_grad_finish_t<float>(g, tile0[k + 1] - tile0[k], ks) : loss_grad_finish_t<double>(g, tile0[k + 1] - tile0[k], ks);
        if (st != hipSuccess) { first_err = st; break; }
    }
    { const hipError_t js = fj.join(); if (first_err == hipSuccess) first_err = js; }
    return first_err;
}

static hipError_t grad_prio_prepass(int dtype, const GradArgs &a, hipStream_t stream, GradArgs *with);
// one bucket of a gradient call: the forward threaded kernel of the module built for its window width and samples per lane
template <typename T> static hipError_t launch_grad_bucket(const GradArgs &ga, const GradArgs::Bucket &bk, hipStream_t stream) {
    const EvalArgs &e = ga.e;
    GradModule m;
    if (!grad_thr_module(sizeof(T) == 4 ? DE_F32 : DE_F64, bk.GC, bk.VS, &m)) return hipErrorInvalidValue;
    const int GC = bk.GC, VS = bk.VS;
    GArgs<T> a = make_gargs<T>(ga);
    a.code = ga.threaded_code;
    a.code_off = e.code_off;
    a.tree_ids = bk.ids;
    a.n_trees = bk.n;
    a.n_slots = bk.n_slots; // spill slots the trees of this bucket need
    a.F += e.uses_params ? ga.P : 0; // leaf rows: X, then the parameters gathered by class
    const bool share = ga.gt_share;
    a.share = share ? 1 : 0;
    a.var_stride = share ? ga.gt_var_stride : 0;
    const int tile_samples = share ? 64 * VS : GBLK * VS;
    // (shared rows: whole groups of four tiles — a fused-loss launch must write every (tile of 256 x VS samples, wave) entry of the partial
    // sums, also the all-padding quarter tiles behind N, as the four-wave workgroup did)
    a.n_tiles = share ? 4 * ((e.N + GBLK * VS - 1) / (GBLK * VS)) : (e.N + tile_samples - 1) / tile_samples;
    const size_t slot_rows = std::max<size_t>((size_t)a.n_slots * (1 + GC), (size_t)GC);
    const size_t lds = (share ? (size_t)a.F + 4 * slot_rows : 4 * ((size_t)a.F + slot_rows)) * 64 * VS * sizeof(T); // 4 waves x rows x one wave's samples (shared leaf rows: once)
    return launch_grad_kernel((ga.fit ? m.kernel_fit : ga.gn ? m.kernel_gn : m.kernel)[e.uses_params ? 1 : 0][share ? 1 : 0], a, bk.windows, lds, ga.prio_ready ? e.prio_keys : nullptr, tile_samples,
                              ga.prio_ready, bk.handler_base, bk.param_handler_off, stream); // the loss reduction passes run once, after the last bucket
}
hipError_t launch_grad_threaded(int dtype, const GradArgs &a0, hipStream_t stream, const char **kernel_name) {
    if (kernel_name) *kernel_name = a0.fit ? "de_grad_threaded_kernel<FIT>" : a0.gn ? "de_grad_threaded_kernel<GN>" : "de_grad_threaded_kernel";
    GradArgs a;
    { const hipError_t ps = grad_prio_prepass(dtype, a0, stream, &a); if (ps != hipSuccess) return ps; }
    if (a.loss) { // two-sample modules use 512-sample tiles: the 256-sample tile slots they never write must read as 0
        bool wide = false;
        for (int b = 0; b < a.n_buckets; b++) wide = wide || (a.buckets[b].n > 0 && a.buckets[b].VS > 1);
        if (wide) {
            const size_t bytes = (size_t)((a.e.N + GBLK - 1) / GBLK) * (size_t)a.n_cols * 4 * (dtype == DE_F32 ? 4 : 8);
            hipError_t st = hipMemsetAsync(a.loss->partial, 0, bytes, stream);
            if (st != hipSuccess) return st;
        }
    }
    int n_active = 0;
    for (int b = 0; b < a.n_buckets; b++) n_active += a.buckets[b].n > 0;
    ForkJoin fj(stream, n_active);
    hipError_t first_err = fj.fork();
    if (first_err != hipSuccess) return first_err;
    for (int b = 0; b < a.n_buckets; b++) {
        const GradArgs::Bucket &bk = a.buckets[b];
        if (bk.n <= 0) continue;
        const hipStream_t bs = fj.next();
        const hipError_t st = dtype == DE_F32 ? launch_grad_bucket<float>(a, bk, bs) : launch_grad_bucket<double>(a, bk, bs);
        if (st != hipSuccess) { first_err = st; break; }
    }
    { const hipError_t js = fj.join(); if (first_err == hipSuccess) first_err = js; }
    if (first_err != hipSuccess) return first_err;
    if (!a.loss) return hipSuccess;
    return launch_loss_grad_finish(dtype, a, (a.e.N + GBLK - 1) / GBLK, stream);
}

// ---- reverse accumulation: one module per element type (de_rev_threaded.hip) --------------------------
// one LDS-need group of trees
template <typename T> static hipError_t launch_rev_group(const GradArgs &ga, const GradArgs::RevGroup &grp, hipStream_t stream) {
    const EvalArgs &e = ga.e;
    if (grp.n <= 0) return hipSuccess;
    const GradModule m = sizeof(T) == 4 ? rev_thr_module_f() : rev_thr_module_d();
    GArgs<T> a = make_gargs<T>(ga);
    a.code = ga.rev_code;
    a.code_off = ga.rev_code_off;
    a.rev_mid = ga.rev_code_mid;
    a.rev_rows = grp.rows;
    a.rev_stage_cols = ga.rev_stage_cols;
    a.rev_stage_rows = (int32_t)(((size_t)ga.rev_stage_cols * sizeof(T) + 64 * sizeof(T) - 1) / (64 * sizeof(T)));
    a.tree_ids = ga.rev_ids + grp.first;
    a.n_trees = grp.n;
    a.n_slots = e.n_slots;
    a.F += e.uses_params ? ga.P : 0; // leaf rows: X, then the parameters gathered by class
    a.n_tiles = ga.rev_tile_range ? ga.rev_n_tiles : (e.N + GBLK - 1) / GBLK;
    a.tile_range = ga.rev_tile_range;
    const size_t lds = 4 * (size_t)a.rev_rows * 64 * sizeof(T);
    return launch_grad_kernel(m.kernel[e.uses_params ? 1 : 0][0], a, 1, lds, ga.prio_ready && !ga.rev_tile_range ? e.prio_keys : nullptr, GBLK, // (class-aligned tiles: no priority tiles)
                              false, ga.rev_handler_base, ga.rev_param_off, stream);
}
// the priority tiles of a gradient / reverse launch: one pre-pass over X for all its buckets (de_kernels.hip de_tile_extremes_kernel)
static hipError_t grad_prio_prepass(int dtype, const GradArgs &a, hipStream_t stream, GradArgs *with) {
    *with = a;
    with->prio_ready = false;
    if (!a.e.skip_flagged || !a.e.prio_keys || !a.e.X || !prio_tiles_wanted(a.e.N, a.e.F, a.e.n_trees)) return hipSuccess;
    const hipError_t st = a.e.prio_keys_ready ? hipSuccess : launch_tile_extremes(dtype, a.e.X, a.e.N, a.e.ldX, a.e.F, a.e.prio_keys, stream);
    if (st == hipSuccess) with->prio_ready = true;
    return st;
}
hipError_t launch_rev_threaded(int dtype, const GradArgs &a0, hipStream_t stream, const char **kernel_name) {
    if (kernel_name) *kernel_name = "de_rev_threaded_kernel";
    GradArgs a;
    { const hipError_t ps = a0.rev_tile_range ? (a = a0, a.prio_ready = false, hipSuccess) : grad_prio_prepass(dtype, a0, stream, &a); if (ps != hipSuccess) return ps; }
    const int64_t n_tiles = (a.e.N + GBLK - 1) / GBLK;
    ForkJoin fj(stream, a.rev_n_groups);
    hipError_t first_err = fj.fork();
    if (first_err != hipSuccess) return first_err;
    for (int k = 0; k < a.rev_n_groups; k++) { // one launch per LDS-need group of trees, spread over the side streams
        const hipError_t st = dtype == DE_F32 ? launch_rev_group<float>(a, a.rev_groups[k], fj.next()) : launch_rev_group<double>(a, a.rev_groups[k], fj.next());
        if (st != hipSuccess) { first_err = st; break; }
    }
    { const hipError_t js = fj.join(); if (first_err == hipSuccess) first_err = js; }
    if (first_err != hipSuccess) return first_err;
    if (a.rev_tile_range) return hipSuccess; // by-class: the caller reduces every class's tile range itself
    return launch_loss_grad_finish(dtype, a, n_tiles, stream);
}

hipError_t launch_grad(int dtype, const GradArgs &a, hipStream_t stream, const char **kernel_name) {
    if (a.threaded_code && a.diff_direction < 0) return launch_grad_threaded(dtype, a, stream, kernel_name);
    // (eval_diff — diff_direction >= 0: launch_grad_dt's window of 1 — comes from grad_impl alone, which sets neither fit nor gn: the plain kernel)
    if (kernel_name) *kernel_name = RealGrad<float>::NAMES[a.fit ? 2 : a.gn ? 1 : 0];
    if (a.fit) return dtype == DE_F32 ? launch_grad_dt<RealGrad<float>, false, true>(a, stream) : launch_grad_dt<RealGrad<double>, false, true>(a, stream);
    if (a.gn) return dtype == DE_F32 ? launch_grad_dt<RealGrad<float>, true>(a, stream) : launch_grad_dt<RealGrad<double>, true>(a, stream);
    return dtype == DE_F32 ? launch_grad_dt<RealGrad<float>>(a, stream) : launch_grad_dt<RealGrad<double>>(a, stream);
}

} // namespace de
