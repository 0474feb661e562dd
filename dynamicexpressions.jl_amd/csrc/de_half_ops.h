// de_half_ops.h — the binary16 (DE_F16) operator table of de_half.hip and de_half_grad.hip, and the staging of their X tile
// (h16_stage_x): Julia's Float16 arithmetic as STEPS in Float32 registers.
//
// Every operand is a binary16 value held exactly in a float; every step computes in Float32 with the Float32 operator code of
// de_device_ops.h and rounds its result to binary16 (r16: v_cvt_f16_f32, round to nearest even, then back), so an F16 cos is exactly
// round16(the Float32 library's cos).  + - * / rounded once are the correctly rounded binary16 results (24 >= 2 * 11 + 2); Julia's
// Float16 methods of the transcendentals compute in Float32 and round once.  A composite rounds at every Julia-level step of its
// definition (test/test_params.jl:7-28, test/test_derivatives.jl:12): cube = (x*x)*x two roundings, custom_cos = cos(x)^2 two,
// pow_abs2 = exp(y*log(abs(x))) three, +(x, y, z) two.  The table of all 53 opcodes is DESIGN.md §13.1.
#pragma once
#include "de_device_ops.h"

namespace de {

__device__ __forceinline__ float r16(float x) { return (float)(_Float16)x; }
// The Float32 value of a step in a register of its own, before r16 reads it.  Where two roundings follow each other the compiler otherwise
// contracts the operation and the conversion into v_fma_mixlo_f16, which rounds the EXACT result to binary16 once: for fma that is not
// Julia's Float16(muladd(Float32...)) (exact -> Float32 -> binary16: the two differ where the Float32 value lands on a binary16 tie), and a
// product becomes fma(x, y, +0), whose zero is +0 where the product is -0 (cube of a negative x whose square underflows to +0).  Both
// found by tests/test_gpu_f16_accuracy.py.
__device__ __forceinline__ float f32_step(float v) { asm("" : "+v"(v)); return v; }

// cos / sin / exp: the functions of the Float32 kernels' hot handlers.  Every finite binary16 lies inside the fast trigonometric range
// (|x| <= 65504 < DE_TRIG_FAST_BOUND), so no Payne-Hanek fix-up path; Inf and NaN give NaN there as in OCML.
__device__ __forceinline__ float h_cos(float x) { return fast_trig_f32<false>(x); }
__device__ __forceinline__ float h_sin(float x) { return fast_trig_f32<true>(x); }
__device__ __forceinline__ float h_exp(float x) { return fast_exp_f32(x); }

// acc = op(x) (degree 1) or op(x, y) (degree 2, reversed forms DOP_R* already resolved by the caller's operand order), binary16 steps
__device__ __forceinline__ float h16_op(uint32_t op, float x, float y) {
    using m = M<float>;
    switch (op) {
    case DE_U_NEG: return -x;
    case DE_U_ABS: return m::abs(x);
    case DE_U_SQUARE: return r16(x * x);
    case DE_U_CUBE: return r16(f32_step(r16(x * x) * x));
    case DE_U_RELU: return x < 0.0f ? 0.0f : x;
    case DE_U_SIGN: return jl_sign(x);
    case DE_U_ROUND: return m::rint(x);
    case DE_U_FLOOR: return m::floor(x);
    case DE_U_CEIL: return m::ceil(x);
    case DE_U_INV: return r16(1.0f / x);
    case DE_U_SQRT: return r16(m::sqrt(x));
    case DE_U_CBRT: return r16(m::cbrt(x));
    case DE_U_EXP: return r16(h_exp(x));
    case DE_U_EXP2: return r16(m::exp2(x));
    case DE_U_LOG: return r16(m::log(x));
    case DE_U_LOG2: return r16(m::log2(x));
    case DE_U_LOG10: return r16(m::log10(x));
    case DE_U_LOG1P: return r16(m::log1p(x));
    case DE_U_SIN: return r16(h_sin(x));
    case DE_U_COS: return r16(h_cos(x));
    case DE_U_TAN: return r16(m::tan(x));
    case DE_U_SINH: return r16(m::sinh(x));
    case DE_U_COSH: return r16(m::cosh(x));
    case DE_U_TANH: return r16(m::tanh(x));
    case DE_U_ASIN: return r16(m::asin(x));
    case DE_U_ACOS: return r16(m::acos(x));
    case DE_U_ATAN: return r16(m::atan(x));
    case DE_U_ASINH: return r16(m::asinh(x));
    case DE_U_ACOSH: return r16(m::acosh(x));
    case DE_U_ATANH: return r16(m::atanh(x));
    case DE_U_SAFE_LOG: return x <= 0.0f ? m::nan() : r16(m::log(x));
    case DE_U_SAFE_LOG2: return x <= 0.0f ? m::nan() : r16(m::log2(x));
    case DE_U_SAFE_LOG10: return x <= 0.0f ? m::nan() : r16(m::log10(x));
    case DE_U_SAFE_LOG1P: return x <= -1.0f ? m::nan() : r16(m::log1p(x));
    case DE_U_SAFE_SQRT: return x < 0.0f ? m::nan() : r16(m::sqrt(x));
    case DE_U_SAFE_ACOSH: return x < 1.0f ? m::nan() : r16(m::acosh(x));
    case DE_U_COS2: { const float c = r16(h_cos(x)); return r16(c * c); }
    case DE_U_GAMMA: return r16(m::tgamma(x));
    case DE_B_ADD: return r16(x + y);
    case DE_B_SUB: return r16(x - y);
    case DOP_RSUB: return r16(y - x);
    case DE_B_MUL: return r16(x * y);
    case DE_B_DIV: return r16(x / y);
    case DOP_RDIV: return r16(y / x);
    case DE_B_POW: return r16(m::pow(x, y));
    case DOP_RPOW: return r16(m::pow(y, x));
    case DE_B_MAX: return jl_max(x, y);
    case DE_B_MIN: return jl_min(x, y);
    case DE_B_MOD: return r16(jl_mod(x, y)); // rem is exact; the one step is r + y
    case DOP_RMOD: return r16(jl_mod(y, x));
    case DE_B_REM: return m::fmod(x, y);     // exact
    case DOP_RREM: return m::fmod(y, x);
    case DE_B_GREATER: return x > y ? 1.0f : 0.0f;
    case DOP_RGREATER: return y > x ? 1.0f : 0.0f;
    case DE_B_POW_ABS2: return r16(h_exp(r16(y * r16(m::log(m::abs(x))))));
    case DOP_RPOW_ABS2: return r16(h_exp(r16(x * r16(m::log(m::abs(y))))));
    default: return m::nan(); // (never reached: the lowering admits de_opcodes.h only)
    }
}

// acc = op3(x, y, z): fma is Julia's Float16 fma, Float16(muladd(Float32...)): the exact x y + z rounded to Float32, and that value rounded
// to binary16 (two roundings: f32_step); +(x, y, z) two additions, clamp and max exact
__device__ __forceinline__ float h16_op3(uint32_t op, float x, float y, float z) {
    switch (op) {
    case DE_T_FMA: return r16(f32_step(M<float>::fma(x, y, z)));
    case DE_T_CLAMP: return x > z ? z : (x < y ? y : x);
    case DE_T_ADD3: return r16(r16(x + y) + z);
    default: return jl_max(jl_max(x, y), z);
    }
}

// A workgroup's binary16 X tile — `samples` samples from sample `base`, F features each — read once with coalesced loads by `threads`
// threads and written TRANSPOSED into LDS as Float32 rows (binary16 -> Float32 is exact): sample j of feature f at rows[f * stride + j].
// Aligned pairs where the tile is contiguous and its first element 4-byte aligned, single elements where the pointer is 2 mod 4, and the
// clamped path for a ragged or strided tile.  (de_half.hip: the eval tile; de_half_grad.hip: the gradient tile.)
__device__ __forceinline__ void h16_stage_x(float *__restrict__ rows, const _Float16 *__restrict__ X, int64_t ldX, uint32_t F, int64_t base, int64_t N,
                                            int tid, uint32_t samples, uint32_t stride, uint32_t threads) {
    const uint32_t total = samples * F;
    if (ldX == (int64_t)F && base + samples <= N) {
        const _Float16 *__restrict__ src = X + base * (int64_t)F; // contiguous samples * F elements (an even count)
        if ((reinterpret_cast<uintptr_t>(src) & 3u) == 0) {
            const uint32_t *__restrict__ s2 = reinterpret_cast<const uint32_t *>(src);
            for (uint32_t e2 = tid; e2 < total / 2; e2 += threads) {
                const uint32_t w = s2[e2];
                _Float16 h[2];
                __builtin_memcpy(h, &w, 4);
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const uint32_t e = 2 * e2 + k, j = e / F, f = e - j * F;
                    rows[f * stride + j] = (float)h[k];
                }
            }
        } else {
            for (uint32_t e = tid; e < total; e += threads) {
                const uint32_t j = e / F, f = e - j * F;
                rows[f * stride + j] = (float)src[e];
            }
        }
    } else { // ragged tail / strided X: samples past N repeat the last one
        const int64_t last = N - 1;
        for (uint32_t e = tid; e < total; e += threads) {
            const uint32_t j = e / F, f = e - j * F;
            int64_t jj = base + j;
            jj = jj < last ? jj : last;
            rows[f * stride + j] = (float)X[f + ldX * jj];
        }
    }
}

} // namespace de
