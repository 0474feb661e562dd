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
