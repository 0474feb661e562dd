// de_real_vec.h — the per-lane value of the real (Float32 / Float64) eval kernels and the operator code they share: the threaded kernel's
// handlers and de_fold_kernel (de_kernels.hip) and the flat-switch interpreter's real policy (de_flat_real.hip) call the SAME cold_op /
// cold_op3 / vec_trig / vec_exp, so a value is the same bits whichever kernel computed it.
#pragma once
#include <hip/hip_runtime.h>

#include "de_device_ops.h"
#include "de_program.h"

namespace de {

// A thread owns G groups of VW consecutive samples (VW*sizeof(T) = 16 bytes, one
// ds_read_b128 / global_store_dwordx4 per group): samples base + g*(BLOCK*VW) + tid*VW + i.
template <typename T> struct VecOf;
template <> struct VecOf<float> { typedef float type __attribute__((ext_vector_type(4))); static constexpr int W = 4; };
template <> struct VecOf<double> { typedef double type __attribute__((ext_vector_type(2))); static constexpr int W = 2; };

template <typename T> __device__ __forceinline__ T imm_of(uint32_t w2, uint32_t w3);
template <> __device__ __forceinline__ float imm_of<float>(uint32_t w2, uint32_t) { return __uint_as_float(w2); }
template <> __device__ __forceinline__ double imm_of<double>(uint32_t w2, uint32_t w3) {
    return __longlong_as_double((long long)(((unsigned long long)w3 << 32) | w2));
}

#define DE_UNROLL _Pragma("unroll")
#define FOR_G DE_UNROLL for (int g = 0; g < G; g++)
#define FOR_I DE_UNROLL for (int i = 0; i < VW; i++)

// acc = f(b) for every sample
#define U_CASE(OPC, EXPR)                                    \
    case OPC:                                                \
        FOR_G FOR_I {                                        \
            const T x = b[g][i];                             \
            acc[g][i] = (EXPR);                              \
        }                                                    \
        break;
// acc = f(acc, b)
#define B_CASE(OPC, EXPR)                                    \
    case OPC:                                                \
        FOR_G FOR_I {                                        \
            const T x = acc[g][i], y = b[g][i];              \
            acc[g][i] = (EXPR);                              \
        }                                                    \
        break;

// The interpreter's inner loop must contain ONLY wave-uniform control flow: one divergent
// branch anywhere inside it makes LLVM structurize the whole loop and bury the scalar
// dispatch under "Flow" blocks (the kernel is scalar-issue bound).  Anything
// with lane-divergent branches (OCML pow/fmod/tgamma/Payne-Hanek ...) therefore lives in
// __noinline__ functions that take and return register-resident values.
template <typename T, int G> struct VG { typename VecOf<T>::type v[G]; };

// Everything that is not on the fast path of the interpreter loop.
template <typename T, int G>
__device__ __noinline__ VG<T, G> cold_op(uint32_t op, VG<T, G> accv, VG<T, G> bv) {
    using m = M<T>;
    typedef typename VecOf<T>::type V;
    constexpr int VW = VecOf<T>::W;
    V (&acc)[G] = accv.v;
    const V (&b)[G] = bv.v;
    switch (op) {
        U_CASE(DE_U_NEG, -x)
        U_CASE(DE_U_ABS, m::abs(x))
        U_CASE(DE_U_SQUARE, x * x)
        U_CASE(DE_U_CUBE, (x * x) * x)
        U_CASE(DE_U_RELU, x < T(0) ? T(0) : x)
        U_CASE(DE_U_SIGN, jl_sign(x))
        U_CASE(DE_U_ROUND, m::rint(x))
        U_CASE(DE_U_FLOOR, m::floor(x))
        U_CASE(DE_U_CEIL, m::ceil(x))
        U_CASE(DE_U_INV, T(1) / x)
        U_CASE(DE_U_SQRT, m::sqrt(x))
        U_CASE(DE_U_CBRT, m::cbrt(x))
        U_CASE(DE_U_EXP, m::exp(x))
        U_CASE(DE_U_COS, m::cos(x))
        U_CASE(DE_U_EXP2, m::exp2(x))
        U_CASE(DE_U_LOG, m::log(x))
        U_CASE(DE_U_LOG2, m::log2(x))
        U_CASE(DE_U_LOG10, m::log10(x))
        U_CASE(DE_U_LOG1P, m::log1p(x))
        U_CASE(DE_U_SIN, m::sin(x))
        U_CASE(DE_U_TAN, m::tan(x))
        U_CASE(DE_U_SINH, m::sinh(x))
        U_CASE(DE_U_COSH, m::cosh(x))
        U_CASE(DE_U_TANH, m::tanh(x))
        U_CASE(DE_U_ASIN, m::asin(x))
        U_CASE(DE_U_ACOS, m::acos(x))
        U_CASE(DE_U_ATAN, m::atan(x))
        U_CASE(DE_U_ASINH, m::asinh(x))
        U_CASE(DE_U_ACOSH, m::acosh(x))
        U_CASE(DE_U_ATANH, m::atanh(x))
        U_CASE(DE_U_SAFE_LOG, x <= T(0) ? m::nan() : m::log(x))
        U_CASE(DE_U_SAFE_LOG2, x <= T(0) ? m::nan() : m::log2(x))
        U_CASE(DE_U_SAFE_LOG10, x <= T(0) ? m::nan() : m::log10(x))
        U_CASE(DE_U_SAFE_LOG1P, x <= T(-1) ? m::nan() : m::log1p(x))
        U_CASE(DE_U_SAFE_SQRT, x < T(0) ? m::nan() : m::sqrt(x))
        U_CASE(DE_U_SAFE_ACOSH, x < T(1) ? m::nan() : m::acosh(x))
    case DE_U_COS2:
        FOR_G FOR_I {
            const T c = m::cos(b[g][i]);
            acc[g][i] = c * c;
        }
        break;
        U_CASE(DE_U_GAMMA, m::tgamma(x))
        B_CASE(DE_B_ADD, x + y)
        B_CASE(DE_B_SUB, x - y)
        B_CASE(DOP_RSUB, y - x)
        B_CASE(DE_B_MUL, x * y)
        B_CASE(DE_B_DIV, x / y)
        B_CASE(DOP_RDIV, y / x)
        B_CASE(DE_B_POW, m::pow(x, y))
        B_CASE(DOP_RPOW, m::pow(y, x))
        B_CASE(DE_B_MAX, jl_max(x, y))
        B_CASE(DE_B_MIN, jl_min(x, y))
        B_CASE(DE_B_MOD, jl_mod(x, y))
        B_CASE(DOP_RMOD, jl_mod(y, x))
        B_CASE(DE_B_REM, m::fmod(x, y))
        B_CASE(DOP_RREM, m::fmod(y, x))
        B_CASE(DE_B_GREATER, x > y ? T(1) : T(0))
        B_CASE(DOP_RGREATER, y > x ? T(1) : T(0))
        B_CASE(DE_B_POW_ABS2, jl_pow_abs2(x, y))
        B_CASE(DOP_RPOW_ABS2, jl_pow_abs2(y, x))
    default: break;
    }
    return accv;
}

// acc = op3(b, c, acc): b, c from spill slots, acc = third argument
template <typename T, int G>
__device__ __noinline__ VG<T, G> cold_op3(uint32_t op, VG<T, G> accv, VG<T, G> bv, VG<T, G> cv) {
    using m = M<T>;
    typedef typename VecOf<T>::type V;
    constexpr int VW = VecOf<T>::W;
    V (&acc)[G] = accv.v;
    const V (&b)[G] = bv.v;
    const V (&c)[G] = cv.v;
    FOR_G FOR_I {
        const T x = b[g][i], y = c[g][i], z = acc[g][i];
        T r;
        switch (op) {
        case DE_T_FMA: r = m::fma(x, y, z); break;
        case DE_T_CLAMP: r = x > z ? z : (x < y ? y : x); break;
        case DE_T_ADD3: r = (x + y) + z; break;
        default: r = jl_max(jl_max(x, y), z); break;
        }
        acc[g][i] = r;
    }
    return accv;
}

// Validity accumulation without touching the scalar unit: poison = fma(v, 0, poison) stays
// +0 while every tested value is finite and turns (and stays) NaN at the first Inf/NaN.
template <typename T, int G, typename V>
__device__ __forceinline__ void poison_with(T &poison, const V (&v)[G]) {
    constexpr int VW = VecOf<T>::W;
    FOR_G FOR_I poison = M<T>::fma(v[g][i], T(0), poison);
}
// ... and, in the CERT variant of the flat-switch kernel, the running maximum of |tested value| (NaN is dropped by fmax: the poison has it)
template <typename T, int G, typename V, bool CERT>
__device__ __forceinline__ void test_with(T &poison, T &vmax, const V (&v)[G]) {
    constexpr int VW = VecOf<T>::W;
    poison_with<T, G, V>(poison, v);
    if constexpr (CERT) { FOR_G FOR_I vmax = M<T>::abs(v[g][i]) > vmax ? M<T>::abs(v[g][i]) : vmax; }
}

// cos/sin/exp over the G*VW samples of a thread.  Float32 uses the fast versions of
// de_device_ops.h with ONE divergent fix-up region for out-of-range arguments.
template <int G, bool SIN>
__device__ __noinline__ VG<float, G> trig_fixup(VG<float, G> r, VG<float, G> x) {
    DE_UNROLL for (int g = 0; g < G; g++) DE_UNROLL for (int i = 0; i < 4; i++)
        if (fabsf(x.v[g][i]) > DE_TRIG_FAST_BOUND) r.v[g][i] = SIN ? sinf(x.v[g][i]) : cosf(x.v[g][i]);
    return r;
}
template <int G, bool SIN>
__device__ __noinline__ VG<double, G> trig_f64(VG<double, G> x) {
    DE_UNROLL for (int g = 0; g < G; g++) DE_UNROLL for (int i = 0; i < 2; i++)
        x.v[g][i] = SIN ? ::sin(x.v[g][i]) : ::cos(x.v[g][i]);
    return x;
}
template <typename T, int G, typename V, bool SIN>
__device__ __forceinline__ void vec_trig(V (&out)[G], const V (&x)[G]) {
    constexpr int VW = VecOf<T>::W;
    if constexpr (sizeof(T) == 4) {
        bool big = false;
        VG<float, G> r, xv;
        FOR_G FOR_I {
            r.v[g][i] = fast_trig_f32<SIN>(x[g][i]);
            big |= M<T>::abs(x[g][i]) > DE_TRIG_FAST_BOUND;
        }
        if (__ballot(big) != 0ull) { // wave-uniform: keeps the interpreter loop free of divergent branches
            FOR_G xv.v[g] = x[g];
            r = trig_fixup<G, SIN>(r, xv);
        }
        FOR_G out[g] = r.v[g];
    } else {
        VG<double, G> xv;
        FOR_G xv.v[g] = x[g];
        xv = trig_f64<G, SIN>(xv);
        FOR_G out[g] = xv.v[g];
    }
}
template <typename T, int G, typename V>
__device__ __forceinline__ void vec_exp(V (&out)[G], const V (&x)[G]) {
    constexpr int VW = VecOf<T>::W;
    V r[G];
    if constexpr (sizeof(T) == 4) { FOR_G FOR_I r[g][i] = fast_exp_f32(x[g][i]); }
    else { FOR_G FOR_I r[g][i] = M<T>::exp(x[g][i]); } // OCML exp (f64) is branch-free
    FOR_G out[g] = r[g];
}

#define COLD_CALL(BV)                                          \
    {                                                          \
        VG<T, G> av_, bv_;                                     \
        FOR_G { av_.v[g] = acc[g]; bv_.v[g] = BV[g]; }         \
        av_ = cold_op<T, G>(op, av_, bv_);                     \
        FOR_G acc[g] = av_.v[g];                               \
    }

} // namespace de
