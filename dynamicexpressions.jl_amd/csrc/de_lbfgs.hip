// de_lbfgs.hip — the device side of de_fit_consts_lbfgs / de_fit_tree_params_lbfgs: L-BFGS on the unknowns of a whole
// population, for the trees of more than 32 unknowns that de_bfgs.hip leaves alone.
//   de_lbfgs_init_kernel       count = head = 0, alpha = a0(g), n_accept = 0
//   de_lbfgs_direction_kernel  the two-loop recursion (or the reset to -g), its slope, and the trial constants
//   de_lbfgs_accept_kernel     the Armijo accept rule, the pair stored in the ring and a row of the loss history
// One wave per tree; lane l owns the entries k = l mod 64 of every vector, a dot product is 64 partial sums added in lane order from LDS by
// every lane (the arithmetic: de_lbfgs.h, the templates the host hooks instantiate).  q and r of the recursion live in p.  All on the
// context's stream, plain vector stores only, no atomics.
// T: the element type of the constants; LT: the type of the loss and gradient slots (T itself for both entry points).
#include "../../include/de_hip.h"

#include "de_lbfgs_dev.h"
#include "de_lbfgs.h"

namespace de {

struct LbfgsWaveTeam { // the 64 lanes of de_lbfgs.h as one wave
    double *part, *av;
    int lane;
    template <class F> __device__ void each(F f) { f(lane); }
    template <class F> __device__ bool all(F f) { return __syncthreads_and(f(lane) ? 1 : 0) != 0; }
    template <class F> __device__ void one(F f) {
        if (lane == 0) f();
    }
    template <class A, class B> __device__ double dot(const A *p, const B *q, int n) {
        part[lane] = lbfgs_dot_part(p, q, n, lane);
        __syncthreads();
        const double s = lbfgs_sum(part);
        __syncthreads(); // (every lane has read the partials before the next dot writes them)
        return s;
    }
    __device__ void set_a(int i, double v) {
        if (lane == 0) av[i] = v; // (read behind the barriers of a later dot)
    }
    __device__ double a(int i) const { return av[i]; }
    __device__ void sync() { __syncthreads(); }
};

template <typename T, typename LT = T>
__global__ void __launch_bounds__(LBFGS_LANES) de_lbfgs_init_kernel(LbfgsArgs x) {
    const BfgsArgs &a = x.b;
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const int G = a.n_grad[t];
    if (lane == 0 && a.n_accept) a.n_accept[t] = 0;
    if (G < 1 || G > LBFGS_MAX_ROWS) return; // (the whole workgroup: one wave)
    __shared__ double part[LBFGS_LANES];
    LbfgsWaveTeam tm{part, nullptr, lane};
    const LT *g = static_cast<const LT *>(a.dloss_acc) + a.coff[t];
    const double gg = tm.dot(g, g, G);
    if (lane == 0) {
        x.count[t] = 0;
        x.head[t] = 0;
        a.alpha[t] = bfgs_a0(gg, a.step0);
    }
}

template <typename T, typename LT = T>
__global__ void __launch_bounds__(LBFGS_LANES) de_lbfgs_direction_kernel(LbfgsArgs x) {
    const BfgsArgs &a = x.b;
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
    double *p = a.p + off;
    if (G > LBFGS_MAX_ROWS || !a.ok_acc[t]) { // (uniform) not fitted: the bits of the constants, -0 and NaN payloads stay
        for (int k = lane; k < G; k += LBFGS_LANES) {
            tr[k] = c[k];
            p[k] = 0.0;
        }
        if (lane == 0) { a.produced[t] = 0; a.slope[t] = 0.0; }
        return;
    }
    __shared__ double part[LBFGS_LANES], av[LBFGS_MAX_MEMORY];
    LbfgsWaveTeam tm{part, av, lane};
    const int m = x.memory;
    const int count = x.count[t], head = x.head[t];
    const double al0 = a.alpha[t];
    __syncthreads(); // (every lane has read the tree's scalars before lane 0 writes them)
    const LbfgsDir r = lbfgs_direction(tm, G, m, x.S + x.roff[t], x.Y + x.roff[t], x.rho + t * m, count, head, al0,
                                       static_cast<const LT *>(a.dloss_acc) + off, a.step0, p);
    if (lane == 0) {
        x.count[t] = r.count;
        a.alpha[t] = r.alpha;
        a.produced[t] = (uint8_t)r.produced;
        a.slope[t] = r.slope;
    }
    for (int k = lane; k < G; k += LBFGS_LANES) // (p[k]: this lane's own store)
        tr[k] = r.produced ? (T)bfgs_trial((double)c[k], r.alpha, p[k]) : c[k];
}

template <typename T, typename LT = T>
__global__ void __launch_bounds__(LBFGS_LANES) de_lbfgs_accept_kernel(LbfgsArgs x) {
    const BfgsArgs &a = x.b;
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const int G = a.n_grad[t];
    LT *la = static_cast<LT *>(a.loss_acc);
    const double f = (double)la[t], ft = (double)static_cast<const LT *>(a.loss_trial)[t];
    const double al = a.alpha[t];
    const bool has = a.ok_acc[t] != 0 && G >= 1 && G <= LBFGS_MAX_ROWS;
    const bool accept = has && a.produced[t] != 0 && a.ok_trial[t] != 0 && bfgs_armijo(ft, f, a.c1, al, a.slope[t]);
    __syncthreads(); // (every lane has read the tree's scalars before lane 0 writes them)
    if (lane == 0 && a.history_row) a.history_row[t] = accept ? ft : f;
    if (!accept) { // (uniform)
        if (lane == 0) a.alpha[t] = al * a.shrink;
        return;
    }
    __shared__ double part[LBFGS_LANES];
    LbfgsWaveTeam tm{part, nullptr, lane};
    const int64_t off = a.coff[t];
    const int m = x.memory;
    T *ca = static_cast<T *>(a.consts_acc) + off;
    LT *ga = static_cast<LT *>(a.dloss_acc) + off;
    const T *ct = static_cast<const T *>(a.consts_trial) + off;
    const LT *gt = static_cast<const LT *>(a.dloss_trial) + off;
    double *s = a.p + off, *yv = x.tmp + off; // (the direction is spent)
    for (int k = lane; k < G; k += LBFGS_LANES) {
        s[k] = (double)ct[k] - (double)ca[k]; // the rounded step actually taken
        yv[k] = (double)gt[k] - (double)ga[k];
    }
    const int n = x.count[t];
    const int updated = lbfgs_update(tm, G, m, x.S + x.roff[t], x.Y + x.roff[t], x.rho + t * m, x.count + t, x.head + t, s, yv, a.curv);
    const int n_new = updated && n < m ? n + 1 : n;
    const double gg = n_new == 0 ? tm.dot(gt, gt, G) : 0.0; // (uniform)
    for (int k = lane; k < G; k += LBFGS_LANES) {
        ca[k] = ct[k];
        ga[k] = gt[k];
    }
    if (lane == 0) {
        la[t] = static_cast<const LT *>(a.loss_trial)[t];
        a.ok_acc[t] = a.ok_trial[t];
        a.alpha[t] = n_new == 0 ? bfgs_a0(gg, a.step0) : 1.0;
        if (a.n_accept) a.n_accept[t] += 1;
    }
}

#define DE_LBFGS_LAUNCH(KERNEL)                                                                                             \
    if (a.b.n_trees <= 0) return hipSuccess;                                                                                \
    if (dtype == DE_F32) hipLaunchKernelGGL(KERNEL<float>, dim3((unsigned)a.b.n_trees), dim3(LBFGS_LANES), 0, stream, a);   \
    else hipLaunchKernelGGL(KERNEL<double>, dim3((unsigned)a.b.n_trees), dim3(LBFGS_LANES), 0, stream, a);                  \
    return hipGetLastError()

hipError_t launch_lbfgs_init(int dtype, const LbfgsArgs &a, hipStream_t stream) { DE_LBFGS_LAUNCH(de_lbfgs_init_kernel); }
hipError_t launch_lbfgs_direction(int dtype, const LbfgsArgs &a, hipStream_t stream) { DE_LBFGS_LAUNCH(de_lbfgs_direction_kernel); }
hipError_t launch_lbfgs_accept(int dtype, const LbfgsArgs &a, hipStream_t stream) { DE_LBFGS_LAUNCH(de_lbfgs_accept_kernel); }

} // namespace de
