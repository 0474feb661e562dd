// de_loss_kinds.h — the parameterised element-wise losses of the fused reductions (include/de_hip.h de_loss_kind_t, values >= 16;
// DESIGN.md §4.4.1): l and l' = dl/dyhat of ONE sample, unweighted, formed in T.  One table for the four kernels that carry a loss
// epilogue: the threaded eval kernel (de_kernels.hip h_tree_end_loss) and, through loss_term (de_grad_common.h), the three gradient
// kernels.  `kind` is wave-uniform: the switch is a scalar branch.
//   x = the tree's value yhat, y = the target, p = the kind's parameter (already converted to T on the host);
//   distance kinds: e = x - y; margin kinds: a = y * x; sign(0) = 0.
#pragma once
#include "de_device_ops.h"

namespace de {

template <typename T> struct LossKindTerm { T l, lp; };

// OCML's own exp / pow (1-2 ulp): the losses claim no bit parity with a CPU library, so none of M<T>'s Julia-parity repairs is needed
__device__ __forceinline__ float lk_exp(float x) { return expf(x); }
__device__ __forceinline__ double lk_exp(double x) { return ::exp(x); }
__device__ __forceinline__ float lk_pow(float x, float y) { return powf(x, y); }
__device__ __forceinline__ double lk_pow(double x, double y) { return ::pow(x, y); }

// log(cosh(e)) without overflow (large |e|) and without cancellation (small |e|):
//   |e| < 1 : log1p(2 sinh^2(|e| / 2))          (cosh e = 1 + 2 sinh^2(e / 2); every step is relatively accurate)
//   else    : (|e| + log1p(exp(-2 |e|))) - ln 2  (the terms are >= 1, the result >= 0.43: no cancellation left)
template <typename T> __device__ __forceinline__ T lk_logcosh(T e) {
    const T a = M<T>::abs(e);
    if (a < T(1)) {
        const T s = M<T>::sinh(T(0.5) * a);
        return M<T>::log1p(T(2) * (s * s));
    }
    return (a + M<T>::log1p(lk_exp(T(-2) * a))) - T(0.693147180559945309417232121458);
}

// one sample of kind KIND (a compile-time constant: the callers dispatch once per wave, outside their loops over samples)
template <int KIND, typename T> __device__ __forceinline__ LossKindTerm<T> loss_kind_one(T x, T y, T p) {
    const T e = x - y, ae = M<T>::abs(e);
    LossKindTerm<T> r;
    if constexpr (KIND == DE_LOSS_HUBER) { // p = delta > 0
        if (ae <= p) { r.l = T(0.5) * (e * e); r.lp = e; }
        else { r.l = p * (ae - T(0.5) * p); r.lp = p * jl_sign(e); }
    } else if constexpr (KIND == DE_LOSS_LOGCOSH) {
        r.l = lk_logcosh(e);
        r.lp = M<T>::tanh(e);
    } else if constexpr (KIND == DE_LOSS_L1_EPS) { // p = eps >= 0
        if (ae > p) { r.l = ae - p; r.lp = jl_sign(e); }
        else { r.l = ae != ae ? ae : T(0); r.lp = T(0); } // (a NaN residual stays NaN)
    } else if constexpr (KIND == DE_LOSS_L2_EPS) {
        const T d = ae - p;
        if (ae > p) { r.l = d * d; r.lp = T(2) * jl_sign(e) * d; }
        else { r.l = ae != ae ? ae : T(0); r.lp = T(0); }
    } else if constexpr (KIND == DE_LOSS_QUANTILE) { // p = tau in [0, 1]
        const T c = (e > T(0) ? T(1) : T(0)) - p;
        r.l = e * c;
        r.lp = c;
    } else if constexpr (KIND == DE_LOSS_LP) { // p >= 1
        r.l = lk_pow(ae, p);
        r.lp = p * jl_sign(e) * lk_pow(ae, p - T(1));
    } else if constexpr (KIND == DE_LOSS_LOGIT_DIST) {
        const T h = T(0.5) * e;
        r.l = T(2) * lk_logcosh(h);
        r.lp = M<T>::tanh(h);
    } else if constexpr (KIND == DE_LOSS_LOGIT_MARGIN) { // log(1 + exp(-a)) = max(-a, 0) + log1p(exp(-|a|))
        const T a = y * x;
        r.l = (a < T(0) ? -a : T(0)) + M<T>::log1p(lk_exp(-M<T>::abs(a)));
        r.lp = -y / (T(1) + lk_exp(a));
    } else {
        static_assert(KIND == DE_LOSS_L1_HINGE, "a kind of de_loss_kind_t behind DE_LOSS_PULLBACK");
        const T a = y * x;
        if (a < T(1)) { r.l = T(1) - a; r.lp = -y; }
        else { r.l = a != a ? a : T(0); r.lp = T(0); }
    }
    return r;
}
// The curvature weight c >= 0 of ONE sample under kind KIND: the Gauss-Newton tree ends sum w c d_i d_k, so that
// (M + lam diag M) delta = -g / 2 is the damped generalised Gauss-Newton / IRLS step of the kind; c == 1 for L2.  2c = l'(e) / e, the IRLS
// weight, for the distance kinds and the true l'' for the logistic margin.  f = the residual floor of the kinds whose weight is unbounded
// at e = 0 (L1, L1_EPS, QUANTILE, LP with p < 2; already converted to T on the host, as p is); the others ignore it.  tanh(t) / t is 1 to
// half an ulp below tau = 2^-12 (Float32) / 2^-27 (Float64): 1 - t^2 / 3 + ...
template <typename T> __device__ __forceinline__ T lk_curv_tau() { return sizeof(T) == 4 ? T(0x1p-12) : T(0x1p-27); }
template <int KIND, typename T> __device__ __forceinline__ T loss_kind_curv(T x, T y, T p, T f) {
    const T e = x - y, ae = M<T>::abs(e);
    if constexpr (KIND == DE_LOSS_L2) return T(1);
    else if constexpr (KIND == DE_LOSS_L1) return T(1) / (T(2) * (ae > f ? ae : f));
    else if constexpr (KIND == DE_LOSS_HUBER) return ae <= p ? T(0.5) : p / (T(2) * ae);
    else if constexpr (KIND == DE_LOSS_LOGCOSH) return ae < lk_curv_tau<T>() ? T(0.5) : M<T>::tanh(e) / (T(2) * e);
    else if constexpr (KIND == DE_LOSS_L1_EPS) return ae > p ? T(1) / (T(2) * (ae > f ? ae : f)) : T(0);
    else if constexpr (KIND == DE_LOSS_L2_EPS) return ae > p ? (ae - p) / ae : T(0);
    else if constexpr (KIND == DE_LOSS_QUANTILE) return M<T>::abs((e > T(0) ? T(1) : T(0)) - p) / (T(2) * (ae > f ? ae : f));
    else if constexpr (KIND == DE_LOSS_LP) {
        if (p == T(2)) return T(1);
        return (p * lk_pow(p < T(2) && !(ae > f) ? f : ae, p - T(2))) * T(0.5);
    } else if constexpr (KIND == DE_LOSS_LOGIT_DIST) {
        const T h = T(0.5) * e;
        return M<T>::abs(h) < lk_curv_tau<T>() ? T(0.25) : M<T>::tanh(h) / (T(4) * h);
    } else {
        static_assert(KIND == DE_LOSS_LOGIT_MARGIN, "a kind without a curvature: the host refuses it (de_gn_spec_check)");
        const T a = y * x; // each sigmoid on its own: 1 - s(a) would cancel
        const T s1 = T(1) / (T(1) + lk_exp(a)), s2 = T(1) / (T(1) + lk_exp(-a));
        return (((y * y) * s1) * s2) * T(0.5);
    }
}
// (the run-time kind is one the host admitted: neither DE_LOSS_PULLBACK nor DE_LOSS_L1_HINGE gets here)
template <typename T> __device__ __forceinline__ T loss_kind_curv_term(int kind, T x, T y, T p, T f) {
    switch (kind) {
    case DE_LOSS_L1: return loss_kind_curv<DE_LOSS_L1, T>(x, y, p, f);
    case DE_LOSS_HUBER: return loss_kind_curv<DE_LOSS_HUBER, T>(x, y, p, f);
    case DE_LOSS_LOGCOSH: return loss_kind_curv<DE_LOSS_LOGCOSH, T>(x, y, p, f);
    case DE_LOSS_L1_EPS: return loss_kind_curv<DE_LOSS_L1_EPS, T>(x, y, p, f);
    case DE_LOSS_L2_EPS: return loss_kind_curv<DE_LOSS_L2_EPS, T>(x, y, p, f);
    case DE_LOSS_QUANTILE: return loss_kind_curv<DE_LOSS_QUANTILE, T>(x, y, p, f);
    case DE_LOSS_LP: return loss_kind_curv<DE_LOSS_LP, T>(x, y, p, f);
    case DE_LOSS_LOGIT_DIST: return loss_kind_curv<DE_LOSS_LOGIT_DIST, T>(x, y, p, f);
    case DE_LOSS_LOGIT_MARGIN: return loss_kind_curv<DE_LOSS_LOGIT_MARGIN, T>(x, y, p, f);
    default: return loss_kind_curv<DE_LOSS_L2, T>(x, y, p, f);
    }
}
// STMT with `KIND` = the compile-time constant of the run-time kind (the host admits no other: de_loss_spec_check)
#define DE_LOSS_KIND_SWITCH(kind, STMT)                                        \
    switch (kind) {                                                            \
    case DE_LOSS_HUBER: { constexpr int KIND = DE_LOSS_HUBER; STMT; } break;   \
    case DE_LOSS_LOGCOSH: { constexpr int KIND = DE_LOSS_LOGCOSH; STMT; } break; \
    case DE_LOSS_L1_EPS: { constexpr int KIND = DE_LOSS_L1_EPS; STMT; } break; \
    case DE_LOSS_L2_EPS: { constexpr int KIND = DE_LOSS_L2_EPS; STMT; } break; \
    case DE_LOSS_QUANTILE: { constexpr int KIND = DE_LOSS_QUANTILE; STMT; } break; \
    case DE_LOSS_LP: { constexpr int KIND = DE_LOSS_LP; STMT; } break;         \
    case DE_LOSS_LOGIT_DIST: { constexpr int KIND = DE_LOSS_LOGIT_DIST; STMT; } break; \
    case DE_LOSS_LOGIT_MARGIN: { constexpr int KIND = DE_LOSS_LOGIT_MARGIN; STMT; } break; \
    default: { constexpr int KIND = DE_LOSS_L1_HINGE; STMT; } break;           \
    }
template <typename T> __device__ __forceinline__ LossKindTerm<T> loss_kind_term(int kind, T x, T y, T p) {
    LossKindTerm<T> r;
    DE_LOSS_KIND_SWITCH(kind, (r = loss_kind_one<KIND, T>(x, y, p)))
    return r;
}

} // namespace de
