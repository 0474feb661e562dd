// de_half_grad_ops.h — value and partials of every operator in binary16 (DE_F16) steps, for de_half_grad.hip: Julia's Float16 arithmetic
// through grad_degn_eval (src/EvaluateDerivative.jl:340-365).  The executable statement is the CPU oracle instantiated for _Float16
// (tests/oracle_f16: oracle/de_oracle_ops.h o_unary_grad / o_binary_grad / o_ternary_grad); DESIGN.md §13.6.
//
// VALUES are de_half_ops.h's steps (h16_op / h16_op3), so a tree's value row carries the bits of de_eval's.  PARTIALS are the table of
// de_grad_common.h (unary_vg / binary_vg / ternary_vg) with EVERY operation rounded to binary16; constants such as ln 2 are binary16
// values.  Where a partial is a library function it is the value table's own step at the same point — the partial of sin is the cos
// opcode's value, of cos the negated sin value, tan / tanh / cbrt / ^ / pow_abs2 / custom_cos are built from their own value steps — so
// the device's partials can be composed from the device's values.  One exception, as in the oracle: the partial of gamma is the Float32
// product tgamma(x) digamma(x) (unary_vg<float>'s partial) rounded once.
//
// A product is rounded through hmul: the Float32 product in a register of its own (f32_step), then r16.  Without it the compiler may
// contract product and conversion into v_fma_mixlo_f16 with a +0 addend, whose zero is +0 where the product is -0 (de_half_ops.h).
// Sums and quotients have no such form.  Binary16 subnormals are kept (1 / 65504 is a subnormal partial).
#pragma once
#include "de_half_ops.h"

namespace de {

__device__ __forceinline__ float hmul(float x, float y) { return r16(f32_step(x * y)); }
__device__ __forceinline__ float hadd(float x, float y) { return r16(x + y); }
__device__ __forceinline__ float hsub(float x, float y) { return r16(x - y); }
__device__ __forceinline__ float hdiv(float x, float y) { return r16(x / y); }

// the chain rule of grad_degn_eval, every operation a binary16 step: d = g1 d1 + g2 d2 and (g0 a + g1 b) + g2 c
__device__ __forceinline__ float hchain2(float g1, float d1, float g2, float d2) { return hadd(hmul(g1, d1), hmul(g2, d2)); }
__device__ __forceinline__ float hchain3(float g0, float a, float g1, float b, float g2, float c) { return hadd(hadd(hmul(g0, a), hmul(g1, b)), hmul(g2, c)); }

struct HUG { float y, g; };
struct HBG { float v, gx, gy; };
struct HTG { float v, g0, g1, g2; };

__device__ __forceinline__ HUG h16_unary_vg(uint32_t op, float x) {
    using m = M<float>;
    const float LN2 = r16(0.693147180559945309417232121458176568f), LN10 = r16(2.302585092994045684017991454684364208f);
    HUG r;
    r.y = h16_op(op, x, 0.0f);
    const float o = r.y;
    switch (op) {
    case DE_U_NEG: r.g = -1.0f; break;
    case DE_U_ABS: r.g = jl_sign(x); break;
    case DE_U_SQUARE: r.g = hadd(x, x); break;
    case DE_U_CUBE: r.g = hmul(hmul(3.0f, x), x); break;
    case DE_U_RELU: r.g = x < 0.0f ? 0.0f : 1.0f; break;
    case DE_U_SIGN: case DE_U_ROUND: case DE_U_FLOOR: case DE_U_CEIL: r.g = 0.0f; break;
    case DE_U_INV: r.g = -hmul(o, o); break;
    case DE_U_SQRT: r.g = hdiv(1.0f, hmul(2.0f, o)); break;
    case DE_U_CBRT: r.g = hdiv(1.0f, hmul(3.0f, hmul(o, o))); break;
    case DE_U_EXP: r.g = o; break;
    case DE_U_EXP2: r.g = hmul(o, LN2); break;
    case DE_U_LOG: r.g = hdiv(1.0f, x); break;
    case DE_U_LOG2: r.g = hdiv(hdiv(1.0f, x), LN2); break;
    case DE_U_LOG10: r.g = hdiv(hdiv(1.0f, x), LN10); break;
    case DE_U_LOG1P: r.g = hdiv(1.0f, hadd(x, 1.0f)); break;
    case DE_U_SIN: r.g = r16(h_cos(x)); break;
    case DE_U_COS: r.g = -r16(h_sin(x)); break;
    case DE_U_TAN: r.g = hadd(1.0f, hmul(o, o)); break;
    case DE_U_SINH: r.g = r16(m::cosh(x)); break;
    case DE_U_COSH: r.g = r16(m::sinh(x)); break;
    case DE_U_TANH: r.g = hsub(1.0f, hmul(o, o)); break;
    case DE_U_ASIN: r.g = hdiv(1.0f, r16(m::sqrt(hsub(1.0f, hmul(x, x))))); break;
    case DE_U_ACOS: r.g = -hdiv(1.0f, r16(m::sqrt(hsub(1.0f, hmul(x, x))))); break;
    case DE_U_ATAN: r.g = hdiv(1.0f, hadd(1.0f, hmul(x, x))); break;
    case DE_U_ASINH: r.g = hdiv(1.0f, r16(m::sqrt(hadd(hmul(x, x), 1.0f)))); break;
    case DE_U_ACOSH: r.g = hdiv(1.0f, hmul(r16(m::sqrt(hsub(x, 1.0f))), r16(m::sqrt(hadd(x, 1.0f))))); break;
    case DE_U_ATANH: r.g = hdiv(1.0f, hsub(1.0f, hmul(x, x))); break;
    case DE_U_SAFE_LOG: r.g = x <= 0.0f ? 0.0f : hdiv(1.0f, x); break;
    case DE_U_SAFE_LOG2: r.g = x <= 0.0f ? 0.0f : hdiv(hdiv(1.0f, x), LN2); break;
    case DE_U_SAFE_LOG10: r.g = x <= 0.0f ? 0.0f : hdiv(hdiv(1.0f, x), LN10); break;
    case DE_U_SAFE_LOG1P: r.g = x <= -1.0f ? 0.0f : hdiv(1.0f, hadd(x, 1.0f)); break;
    case DE_U_SAFE_SQRT: r.g = x < 0.0f ? 0.0f : hdiv(1.0f, hmul(2.0f, o)); break;
    case DE_U_SAFE_ACOSH: r.g = x < 1.0f ? 0.0f : hdiv(1.0f, hmul(r16(m::sqrt(hsub(x, 1.0f))), r16(m::sqrt(hadd(x, 1.0f))))); break;
    case DE_U_COS2: { const float c = r16(h_cos(x)), s = r16(h_sin(x)); r.g = hmul(hmul(2.0f, c), -s); } break;
    case DE_U_GAMMA: r.g = r16(f32_step(m::tgamma(x) * dev_digamma(x))); break;
    default: r.g = m::nan(); break;
    }
    return r;
}

// op(x, y), x the first (left) argument; the reversed forms DOP_R* are resolved by the caller's operand order
__device__ __forceinline__ HBG h16_binary_vg(uint32_t op, float x, float y) {
    using m = M<float>;
    HBG r;
    r.v = h16_op(op, x, y);
    const float o = r.v;
    switch (op) {
    case DE_B_ADD: r.gx = 1.0f; r.gy = 1.0f; break;
    case DE_B_SUB: r.gx = 1.0f; r.gy = -1.0f; break;
    case DE_B_MUL: r.gx = y; r.gy = x; break;
    case DE_B_DIV: r.gx = hdiv(1.0f, y); r.gy = -hdiv(o, y); break;
    case DE_B_POW: { // ChainRules _pow_grad_x / _pow_grad_p (real case)
        if (x != 0.0f || y < 0.0f) r.gx = (!m::isfinite(x) && x == x && y == 1.0f) ? 1.0f : hdiv(hmul(o, y), x);
        else if (y == 1.0f) r.gx = 1.0f;
        else if (y == 0.0f || y > 1.0f) r.gx = 0.0f;
        else r.gx = m::inf();
        if (x != 0.0f) r.gy = hmul(o, r16(m::log(m::abs(x))));
        else if (y > 0.0f) r.gy = 0.0f;
        else r.gy = m::nan();
    } break;
    case DE_B_MAX: { const bool gt = x > y; r.gx = gt ? 1.0f : 0.0f; r.gy = gt ? 0.0f : 1.0f; } break;
    case DE_B_MIN: { const bool gt = x > y; r.gx = gt ? 0.0f : 1.0f; r.gy = gt ? 1.0f : 0.0f; } break;
    case DE_B_MOD: {
        const float u = hdiv(x, y);
        const bool isint = (u == m::floor(u)) && m::isfinite(u);
        r.gx = isint ? m::nan() : 1.0f;
        r.gy = isint ? m::nan() : -m::floor(u);
    } break;
    case DE_B_REM: {
        const float u = hdiv(x, y);
        const bool isint = (u == m::floor(u)) && m::isfinite(u);
        r.gx = isint ? m::nan() : 1.0f;
        r.gy = isint ? m::nan() : -m::trunc(u);
    } break;
    case DE_B_GREATER: r.gx = 0.0f; r.gy = 0.0f; break;
    case DE_B_POW_ABS2: {
        const float a = m::abs(x), l = r16(m::log(a));
        r.gx = hmul(hmul(hmul(o, y), hdiv(1.0f, a)), jl_sign(x));
        r.gy = hmul(o, l);
    } break;
    default: r.gx = r.gy = m::nan(); break;
    }
    return r;
}

__device__ __forceinline__ HTG h16_ternary_vg(uint32_t op, float x, float y, float z) {
    HTG r;
    r.v = h16_op3(op, x, y, z);
    switch (op) {
    case DE_T_FMA: r.g0 = y; r.g1 = x; r.g2 = 1.0f; break;
    case DE_T_CLAMP:
        r.g0 = (x > z || x < y) ? 0.0f : 1.0f;
        r.g1 = (x > z) ? 0.0f : (x < y ? 1.0f : 0.0f);
        r.g2 = (x > z) ? 1.0f : 0.0f;
        break;
    case DE_T_ADD3: r.g0 = r.g1 = r.g2 = 1.0f; break;
    default: {
        const float mx = jl_max(x, y);
        const bool gt1 = x > y, gt2 = mx > z;
        r.g0 = (gt2 && gt1) ? 1.0f : 0.0f;
        r.g1 = (gt2 && !gt1) ? 1.0f : 0.0f;
        r.g2 = gt2 ? 0.0f : 1.0f;
    } break;
    }
    return r;
}

} // namespace de
