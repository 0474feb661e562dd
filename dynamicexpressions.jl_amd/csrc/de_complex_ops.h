// de_complex_ops.h — the complex (DE_CF32 / DE_CF64) operator table of de_complex.hip: Julia's Complex{Float32} / Complex{Float64}
// methods of the 19 supported opcodes, restated (DESIGN.md §14.1 has the table with every special case).
//
// A value is a pair (re, im) of the component type T.  The real functions inside the formulas (sin cos exp log log1p sinh cosh tan
// sqrt asinh atan2) are the project's exact real operator code, M<T> of de_device_ops.h (never the turbo forms).  Every TU builds with
// -ffp-contract=off: a*b - c*d is two roundings of products and one of the difference, as Julia computes it.
#pragma once
#include "de_device_ops.h"

namespace de {

template <typename T> struct Cx { T re, im; };

// the real helpers M<T> lacks
template <typename T> struct CR;
template <> struct CR<float> {
    static __device__ __forceinline__ float atan2(float y, float x) { return atan2f(y, x); }
    static __device__ __forceinline__ float ldexp(float x, int k) { return ldexpf(x, k); }
    static __device__ __forceinline__ int exponent(float x) { return ilogbf(x); } // (finite, non-zero x)
    static __device__ __forceinline__ float tan(float x) { return tanf(x); }
    static __device__ __forceinline__ float asinh_omega() { return 89.415985f; } // asinh(prevfloat(floatmax(Float32)))
    static __device__ __forceinline__ float ssqs_tiny() { return 0x1p-104f; }      // nextfloat(0f0) / (2 eps(Float32)^2)
};
template <> struct CR<double> {
    static __device__ __forceinline__ double atan2(double y, double x) { return ::atan2(y, x); }
    static __device__ __forceinline__ double ldexp(double x, int k) { return ::ldexp(x, k); }
    static __device__ __forceinline__ int exponent(double x) { return ::ilogb(x); }
    static __device__ __forceinline__ double tan(double x) { return ::tan(x); }
    static __device__ __forceinline__ double asinh_omega() { return 710.4758600739439; } // asinh(prevfloat(floatmax(Float64)))
    static __device__ __forceinline__ double ssqs_tiny() { return 0x1p-971; }            // nextfloat(0.0) / (2 eps(Float64)^2)
};

template <typename T> __device__ __forceinline__ bool c_valid(Cx<T> z) { return __builtin_isfinite(z.re) && __builtin_isfinite(z.im); }
template <typename T> __device__ __forceinline__ Cx<T> c_add(Cx<T> a, Cx<T> b) { return {a.re + b.re, a.im + b.im}; }
template <typename T> __device__ __forceinline__ Cx<T> c_sub(Cx<T> a, Cx<T> b) { return {a.re - b.re, a.im - b.im}; }
// (ac - bd, ad + bc): four products and two sums, each rounded once — no fused multiply-add
template <typename T> __device__ __forceinline__ Cx<T> c_mul(Cx<T> a, Cx<T> b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }

// Julia max on floats: NaN-propagating
__device__ __forceinline__ double c_jmax(double a, double b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }

// inv(w::ComplexF64): Smith's algorithm with power-of-two scaling against over- and underflow
__device__ __forceinline__ Cx<double> c_inv64(double c, double d) {
    if (__builtin_isinf(c) || __builtin_isinf(d)) return {::copysign(0.0, c), __builtin_signbit(d) ? 0.0 : -0.0};
    const double cd = c_jmax(::fabs(c), ::fabs(d));
    const double eps = 0x1p-52, bs = 2.0 / (eps * eps);
    double s = 1.0;
    if (cd >= 0.5 * 1.7976931348623157e308) { c = 0.5 * c; d = 0.5 * d; s = s * 0.5; }
    if (cd <= 2.2250738585072014e-308 * 2.0 / eps) { c = c * bs; d = d * bs; s = s * bs; }
    double p, q;
    if (::fabs(d) <= ::fabs(c)) {
        const double r = d / c, t = 1.0 / (c + d * r);
        p = t;
        q = -r * t;
    } else {
        const double c2 = d, d2 = c;
        const double r = d2 / c2, t = 1.0 / (c2 + d2 * r);
        p = r * t;
        q = -t;
    }
    return {p * s, q * s};
}
__device__ __forceinline__ double c_rdiv2(double a, double b, double c, double d, double r, double t) {
    if (r != 0.0) {
        const double br = b * r;
        return br != 0.0 ? (a + br) * t : a * t + (b * t) * r;
    }
    return (a + d * (b / c)) * t;
}
__device__ __forceinline__ void c_rdiv1(double a, double b, double c, double d, double *p, double *q) {
    const double r = d / c, t = 1.0 / (c + d * r);
    *p = c_rdiv2(a, b, c, d, r, t);
    *q = c_rdiv2(b, -a, c, d, r, t);
}
__device__ __forceinline__ void c_cdiv(double a, double b, double c, double d, double *p, double *q) {
    if (::fabs(d) <= ::fabs(c)) c_rdiv1(a, b, c, d, p, q);
    else {
        c_rdiv1(b, a, d, c, p, q);
        *q = -*q;
    }
}
// /(z::ComplexF64, w::ComplexF64): Baudin & Smith's robust division, scaled when an operand is near over- or underflow
__device__ __forceinline__ Cx<double> c_div64(double a, double b, double c, double d) {
    const double absa = ::fabs(a), absb = ::fabs(b), ab = absa >= absb ? absa : absb;
    const double absc = ::fabs(c), absd = ::fabs(d), cd = absc >= absd ? absc : absd;
    const double halfov = 0.5 * 1.7976931348623157e308, twoun = 2.2250738585072014e-308 * 2.0 / 0x1p-52;
    double p, q;
    if (ab >= halfov || ab <= twoun || cd >= halfov || cd <= twoun) {
        const double bs = 2.0 / (0x1p-52 * 0x1p-52);
        double s = 1.0;
        if (ab >= halfov) { a *= 0.5; b *= 0.5; s *= 2.0; }
        else if (ab <= twoun) { a *= bs; b *= bs; s /= bs; }
        if (cd >= halfov) { c *= 0.5; d *= 0.5; s *= 0.5; }
        else if (cd <= twoun) { c *= bs; d *= bs; s *= bs; }
        c_cdiv(a, b, c, d, &p, &q);
        p *= s;
        q *= s;
    } else c_cdiv(a, b, c, d, &p, &q);
    return {p, q};
}

template <typename T> __device__ __forceinline__ Cx<T> c_div(Cx<T> z, Cx<T> w);
template <> __device__ __forceinline__ Cx<double> c_div(Cx<double> z, Cx<double> w) { return c_div64(z.re, z.im, w.re, w.im); }
// ComplexF32: widen(z) * inv(widen(w)) in Float64, each component rounded to Float32 once
template <> __device__ __forceinline__ Cx<float> c_div(Cx<float> z, Cx<float> w) {
    const Cx<double> iw = c_inv64((double)w.re, (double)w.im), r = c_mul(Cx<double>{(double)z.re, (double)z.im}, iw);
    return {(float)r.re, (float)r.im};
}
template <typename T> __device__ __forceinline__ Cx<T> c_inv(Cx<T> w);
template <> __device__ __forceinline__ Cx<double> c_inv(Cx<double> w) { return c_inv64(w.re, w.im); }
// ComplexF32: conj(widen(w)) / abs2(widen(w)) in Float64, rounded once
template <> __device__ __forceinline__ Cx<float> c_inv(Cx<float> w) {
    const double re = w.re, im = w.im, a2 = re * re + im * im;
    return {(float)(re / a2), (float)(-im / a2)};
}

// ssqs: x^2 + y^2 scaled by 2^-2k away from over- and underflow
template <typename T> __device__ __forceinline__ T c_ssqs(T x, T y, int *k) {
    *k = 0;
    T rho = x * x + y * y;
    if (!__builtin_isfinite(rho) && (__builtin_isinf(x) || __builtin_isinf(y))) rho = M<T>::inf();
    else if (__builtin_isinf(rho) || (rho == T(0) && (x != T(0) || y != T(0))) || rho < CR<T>::ssqs_tiny()) {
        const T ax = M<T>::abs(x), ay = M<T>::abs(y);
        const T m = (ax != ax || ay != ay) ? ax + ay : (ax > ay ? ax : ay);
        *k = m == T(0) ? 0 : CR<T>::exponent(m);
        const T xk = CR<T>::ldexp(x, -*k), yk = CR<T>::ldexp(y, -*k);
        rho = xk * xk + yk * yk;
    }
    return rho;
}
template <typename T> __device__ __forceinline__ Cx<T> c_sqrt(Cx<T> z) {
    const T x = z.re, y = z.im;
    if (x == T(0) && y == T(0)) return {T(0), y};
    int k;
    T rho = c_ssqs(x, y, &k);
    if (__builtin_isfinite(x)) rho = CR<T>::ldexp(M<T>::abs(x), -k) + M<T>::sqrt(rho);
    if (k & 1) k = (k - 1) / 2; // (k odd: div(k - 1, 2) is exact)
    else {
        k = k / 2 - 1;
        rho += rho;
    }
    rho = CR<T>::ldexp(M<T>::sqrt(rho), k);
    T xi = rho, eta = y;
    if (rho != T(0)) {
        if (__builtin_isfinite(eta)) eta = (eta / rho) / T(2);
        if (x < T(0)) {
            xi = M<T>::abs(eta);
            eta = M<T>::copysign(rho, y);
        }
    }
    return {xi, eta};
}
template <typename T> __device__ __forceinline__ Cx<T> c_log(Cx<T> z) {
    const T x = z.re, y = z.im;
    int k;
    const T rho = c_ssqs(x, y, &k);
    const T ax = M<T>::abs(x), ay = M<T>::abs(y);
    const T theta = ax < ay ? ax : ay, beta = ax < ay ? ay : ax;
    T rr;
    if (k == 0 && T(0.5) < beta * beta && (beta <= T(1.25) || rho < T(3))) rr = M<T>::log1p((beta - T(1)) * (beta + T(1)) + theta * theta) / T(2);
    else rr = M<T>::log(rho) / T(2) + T(k) * T(0.6931471805599453);
    return {rr, CR<T>::atan2(y, x)};
}
template <typename T> __device__ __forceinline__ Cx<T> c_exp(Cx<T> z) {
    const T zr = z.re, zi = z.im;
    if (zr != zr) return {zr, zi == T(0) ? zi : zr};
    if (!__builtin_isfinite(zi)) {
        if (zr == M<T>::inf()) return {-zr, M<T>::nan()};
        if (zr == -M<T>::inf()) return {-T(0), M<T>::copysign(T(0), zi)};
        return {M<T>::nan(), M<T>::nan()};
    }
    const T er = M<T>::exp(zr);
    if (zi == T(0)) return {er, zi};
    return {er * M<T>::cos(zi), er * M<T>::sin(zi)};
}
__device__ __forceinline__ float c_flipsign(float x, float y) { return __builtin_signbit(y) ? -x : x; }
__device__ __forceinline__ double c_flipsign(double x, double y) { return __builtin_signbit(y) ? -x : x; }
template <typename T> __device__ __forceinline__ Cx<T> c_sin(Cx<T> z) {
    const T zr = z.re, zi = z.im;
    if (zr == T(0)) return {zr, M<T>::sinh(zi)};
    if (!__builtin_isfinite(zr)) {
        if (zi == T(0) || __builtin_isinf(zi)) return {M<T>::nan(), zi};
        return {M<T>::nan(), M<T>::nan()};
    }
    return {M<T>::sin(zr) * M<T>::cosh(zi), M<T>::cos(zr) * M<T>::sinh(zi)};
}
template <typename T> __device__ __forceinline__ Cx<T> c_cos(Cx<T> z) {
    const T zr = z.re, zi = z.im;
    if (zr == T(0)) return {M<T>::cosh(zi), zi != zi ? zr : -c_flipsign(zr, zi)};
    if (!__builtin_isfinite(zr)) {
        if (zi == T(0)) return {M<T>::nan(), zr != zr ? T(0) : -c_flipsign(zi, zr)};
        if (__builtin_isinf(zi)) return {M<T>::inf(), M<T>::nan()};
        return {M<T>::nan(), M<T>::nan()};
    }
    return {M<T>::cos(zr) * M<T>::cosh(zi), -M<T>::sin(zr) * M<T>::sinh(zi)};
}
// tanh in Kahan's form: the overflow branch for 4|re| > asinh(prevfloat(floatmax)), tan / sinh / sqrt otherwise
template <typename T> __device__ __forceinline__ Cx<T> c_tanh(Cx<T> z) {
    const T xi = z.re, eta = z.im;
    if (xi != xi && eta == T(0)) return {xi, eta};
    if (T(4) * M<T>::abs(xi) > CR<T>::asinh_omega()) {
        // the sign of the zero is that of eta sin(2|eta|); where 2|eta| overflows (Julia's sin(Inf) throws) sin(2a) = 2 sin a cos a gives it
        T sg = T(1);
        if (__builtin_isfinite(eta)) {
            const T a = M<T>::abs(eta), a2 = T(2) * a;
            sg = __builtin_isfinite(a2) ? M<T>::sin(a2) : M<T>::sin(a) * M<T>::cos(a);
        }
        return {M<T>::copysign(T(1), xi), M<T>::copysign(T(0), eta * sg)};
    }
    const T t = CR<T>::tan(eta), beta = T(1) + t * t, s = M<T>::sinh(xi), rho = M<T>::sqrt(T(1) + s * s);
    if (__builtin_isinf(t)) return {rho / s, T(1) / t};
    const T den = T(1) + beta * s * s;
    return {beta * rho * s / den, t / den};
}
template <typename T> __device__ __forceinline__ Cx<T> c_sinh(Cx<T> z) { const Cx<T> w = c_sin(Cx<T>{z.im, z.re}); return {w.im, w.re}; }
template <typename T> __device__ __forceinline__ Cx<T> c_cosh(Cx<T> z) { return c_cos(Cx<T>{z.im, -z.re}); }
template <typename T> __device__ __forceinline__ Cx<T> c_tan(Cx<T> z) { const Cx<T> w = c_tanh(Cx<T>{-z.im, z.re}); return {w.im, -w.re}; }

// acc = op(x) (degree 1) or op(x, y) (degree 2; DOP_RSUB / DOP_RDIV: op(y, x)); only the opcodes complex_opcode_ok admits reach here
template <typename T> __device__ __forceinline__ Cx<T> c_op(uint32_t op, Cx<T> x, Cx<T> y) {
    switch (op) {
    case DE_U_NEG: return {-x.re, -x.im};
    case DE_U_SQUARE: return c_mul(x, x);
    case DE_U_CUBE: return c_mul(c_mul(x, x), x);
    case DE_U_INV: return c_inv(x);
    case DE_U_SQRT: return c_sqrt(x);
    case DE_U_EXP: return c_exp(x);
    case DE_U_LOG: return c_log(x);
    case DE_U_SIN: return c_sin(x);
    case DE_U_COS: return c_cos(x);
    case DE_U_TAN: return c_tan(x);
    case DE_U_SINH: return c_sinh(x);
    case DE_U_COSH: return c_cosh(x);
    case DE_U_TANH: return c_tanh(x);
    case DE_U_COS2: { const Cx<T> c = c_cos(x); return c_mul(c, c); }
    case DE_B_ADD: return c_add(x, y);
    case DE_B_SUB: return c_sub(x, y);
    case DOP_RSUB: return c_sub(y, x);
    case DE_B_MUL: return c_mul(x, y);
    case DE_B_DIV: return c_div(x, y);
    case DOP_RDIV: return c_div(y, x);
    default: return {M<T>::nan(), M<T>::nan()};
    }
}

} // namespace de
