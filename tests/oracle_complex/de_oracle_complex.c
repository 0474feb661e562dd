/*
 * de_oracle_complex.c — the CPU oracle's tree walk and flag logic (oracle/de_oracle_impl.h) instantiated for Julia's ComplexF32 and
 * ComplexF64: OT = float _Complex / double _Complex.  TEST INFRASTRUCTURE of tests/test_complex_host.py and tests/test_gpu_complex.py,
 * built by their module-scoped fixtures (tests/complex_oracle.py):
 *
 *     clang -O2 -fPIC -shared -ffp-contract=off
 *
 * Its own is_valid and operators, written from Julia's Complex methods on the host libm — nothing here is shared with
 * the library's device code.  The shared walker evaluates + - * / and square inline with T's own operators; C's complex * and / are not
 * Julia's (Annex G recovery of infinities, other division algorithms), so those opcodes are renamed away while the walker is compiled
 * and every one of them reaches o_binary / o_unary below.
 */
#define _GNU_SOURCE
#include <complex.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/de_hip.h"

typedef struct onode {
    uint8_t degree, op;
    uint16_t arg;
    int child[3];
    int is_const; /* no feature / parameter leaf below */
} onode;

/* Post-order tape -> indexed tree; root index or -2 malformed, -3 unknown opcode, -6 index out of range */
static int o_parse(const de_tape_node_t *tape, int64_t n, int64_t n_consts, int F, int P, onode **out) {
    if (n <= 0) return -2;
    onode *nodes = (onode *)calloc((size_t)n, sizeof(onode));
    int *stack = (int *)malloc((size_t)n * sizeof(int));
    int sp = 0, err = 0;
    for (int64_t i = 0; i < n && !err; i++) {
        onode *nd = &nodes[i];
        nd->degree = tape[i].degree;
        nd->op = tape[i].op;
        nd->arg = tape[i].arg;
        if (nd->degree == 0) {
            if (nd->op == DE_LEAF_CONST) { nd->is_const = 1; if (nd->arg >= n_consts) err = -6; }
            else if (nd->op == DE_LEAF_FEATURE) { if (nd->arg >= F) err = -6; }
            else if (nd->op == DE_LEAF_PARAM) { if (nd->arg >= P) err = -6; }
            else err = -2;
        } else if (nd->degree <= 3) {
            int lo = nd->degree == 1 ? DE_U_NEG : (nd->degree == 2 ? DE_B_ADD : DE_T_FMA);
            int hi = nd->degree == 1 ? DE_U_LAST_ : (nd->degree == 2 ? DE_B_LAST_ : DE_T_LAST_);
            if (nd->op < lo || nd->op >= hi) { err = -3; break; }
            if (sp < nd->degree) { err = -2; break; }
            nd->is_const = 1;
            for (int k = nd->degree - 1; k >= 0; k--) {
                nd->child[k] = stack[--sp];
                nd->is_const &= nodes[nd->child[k]].is_const;
            }
        } else err = -2;
        stack[sp++] = (int)i;
    }
    if (!err && sp != 1) err = -2;
    int root = err ? err : stack[0];
    free(stack);
    if (err) { free(nodes); return err; }
    *out = nodes;
    return root;
}

/* ---- Julia's Complex methods on (re, im) pairs, generic over the component type R (float / double) ---------------------------- */
#define JL_COMPLEX_OPS(R, S, CT, FS, FMAXV, TINY, OMEGA)                                                                          \
    static inline CT mk##S(R re, R im) { CT z; __real__ z = re; __imag__ z = im; return z; }                                  \
    static inline CT mul##S(CT a, CT b) {                                                                                       \
        R ar = crealf_##S(a), ai = cimagf_##S(a), br = crealf_##S(b), bi = cimagf_##S(b);                                       \
        R re = ar * br - ai * bi, im = ar * bi + ai * br;                                                                        \
        return mk##S(re, im);                                                                                                    \
    }                                                                                                                            \
    static inline R ssqs##S(R x, R y, int *k) {                                                                                  \
        *k = 0;                                                                                                                  \
        R rho = x * x + y * y;                                                                                                   \
        if (!isfinite(rho) && (isinf(x) || isinf(y))) rho = (R)INFINITY;                                                       \
        else if (isinf(rho) || (rho == 0 && (x != 0 || y != 0)) || rho < (R)(TINY)) {                                          \
            R ax = fabs##FS(x), ay = fabs##FS(y);                                                                               \
            R m = (isnan(ax) || isnan(ay)) ? ax + ay : (ax > ay ? ax : ay);                                                      \
            *k = m == 0 ? 0 : ilogb##FS(m);                                                                                       \
            R xk = ldexp##FS(x, -*k), yk = ldexp##FS(y, -*k);                                                                    \
            rho = xk * xk + yk * yk;                                                                                             \
        }                                                                                                                        \
        return rho;                                                                                                              \
    }                                                                                                                            \
    static CT csqrt_jl##S(CT z) {                                                                                              \
        R x = crealf_##S(z), y = cimagf_##S(z);                                                                                 \
        if (x == 0 && y == 0) return mk##S(0, y);                                                                               \
        int k;                                                                                                                   \
        R rho = ssqs##S(x, y, &k);                                                                                               \
        if (isfinite(x)) rho = ldexp##FS(fabs##FS(x), -k) + sqrt##FS(rho);                                                      \
        if (k % 2 != 0) k = (k - 1) / 2;                                                                                         \
        else { k = k / 2 - 1; rho += rho; }                                                                                      \
        rho = ldexp##FS(sqrt##FS(rho), k);                                                                                       \
        R xi = rho, eta = y;                                                                                                     \
        if (rho != 0) {                                                                                                          \
            if (isfinite(eta)) eta = (eta / rho) / 2;                                                                            \
            if (x < 0) { xi = fabs##FS(eta); eta = copysign##FS(rho, y); }                                                     \
        }                                                                                                                        \
        return mk##S(xi, eta);                                                                                                   \
    }                                                                                                                            \
    static CT clog_jl##S(CT z) {                                                                                               \
        R x = crealf_##S(z), y = cimagf_##S(z);                                                                                 \
        int k;                                                                                                                   \
        R rho = ssqs##S(x, y, &k), ax = fabs##FS(x), ay = fabs##FS(y);                                                         \
        R th = ax < ay ? ax : ay, be = ax < ay ? ay : ax, rr;                                                                   \
        if (k == 0 && (R)0.5 < be * be && (be <= (R)1.25 || rho < (R)3)) rr = log1p##FS((be - 1) * (be + 1) + th * th) / 2;   \
        else rr = log##FS(rho) / 2 + (R)k * (R)0.6931471805599453;                                                              \
        return mk##S(rr, atan2##FS(y, x));                                                                                       \
    }                                                                                                                            \
    static CT cexp_jl##S(CT z) {                                                                                               \
        R zr = crealf_##S(z), zi = cimagf_##S(z);                                                                               \
        if (isnan(zr)) return mk##S(zr, zi == 0 ? zi : zr);                                                                     \
        if (!isfinite(zi)) {                                                                                                     \
            if (zr == (R)INFINITY) return mk##S(-zr, (R)NAN);                                                                   \
            if (zr == -(R)INFINITY) return mk##S(-(R)0, copysign##FS(0, zi));                                                  \
            return mk##S((R)NAN, (R)NAN);                                                                                        \
        }                                                                                                                        \
        R er = exp##FS(zr);                                                                                                      \
        if (zi == 0) return mk##S(er, zi);                                                                                      \
        return mk##S(er * cos##FS(zi), er * sin##FS(zi));                                                                        \
    }                                                                                                                            \
    static CT csin_jl##S(CT z) {                                                                                               \
        R zr = crealf_##S(z), zi = cimagf_##S(z);                                                                               \
        if (zr == 0) return mk##S(zr, sinh##FS(zi));                                                                            \
        if (!isfinite(zr)) return (zi == 0 || isinf(zi)) ? mk##S((R)NAN, zi) : mk##S((R)NAN, (R)NAN);                         \
        return mk##S(sin##FS(zr) * cosh##FS(zi), cos##FS(zr) * sinh##FS(zi));                                                   \
    }                                                                                                                            \
    static inline R flip##S(R x, R y) { return signbit(y) ? -x : x; }                                                          \
    static CT ccos_jl##S(CT z) {                                                                                               \
        R zr = crealf_##S(z), zi = cimagf_##S(z);                                                                               \
        if (zr == 0) return mk##S(cosh##FS(zi), isnan(zi) ? zr : -flip##S(zr, zi));                                             \
        if (!isfinite(zr)) {                                                                                                     \
            if (zi == 0) return mk##S((R)NAN, isnan(zr) ? (R)0 : -flip##S(zi, zr));                                             \
            if (isinf(zi)) return mk##S((R)INFINITY, (R)NAN);                                                                   \
            return mk##S((R)NAN, (R)NAN);                                                                                        \
        }                                                                                                                        \
        return mk##S(cos##FS(zr) * cosh##FS(zi), -sin##FS(zr) * sinh##FS(zi));                                                  \
    }                                                                                                                            \
    static CT ctanh_jl##S(CT z) {                                                                                              \
        R xi = crealf_##S(z), eta = cimagf_##S(z);                                                                              \
        if (isnan(xi) && eta == 0) return z;                                                                                     \
        if (4 * fabs##FS(xi) > (R)(OMEGA)) { /* 2|eta| overflowing: the sign of sin(2a) from sin a cos a */      \
            R sg = 1, a = fabs##FS(eta);                                                                                         \
            if (isfinite(eta)) sg = isfinite(2 * a) ? sin##FS(2 * a) : sin##FS(a) * cos##FS(a);                                  \
            return mk##S(copysign##FS(1, xi), copysign##FS(0, eta * sg));                                                        \
        }                                                                                                                        \
        R t = tan##FS(eta), be = 1 + t * t, s = sinh##FS(xi), rho = sqrt##FS(1 + s * s);                                        \
        if (isinf(t)) return mk##S(rho / s, 1 / t);                                                                             \
        R den = 1 + be * s * s;                                                                                                  \
        return mk##S(be * rho * s / den, t / den);                                                                               \
    }                                                                                                                            \
    static CT csinh_jl##S(CT z) { CT w = csin_jl##S(mk##S(cimagf_##S(z), crealf_##S(z))); return mk##S(cimagf_##S(w), crealf_##S(w)); } \
    static CT ccosh_jl##S(CT z) { return ccos_jl##S(mk##S(cimagf_##S(z), -crealf_##S(z))); }                                   \
    static CT ctan_jl##S(CT z) { CT w = ctanh_jl##S(mk##S(-cimagf_##S(z), crealf_##S(z))); return mk##S(cimagf_##S(w), -crealf_##S(w)); }

static inline float crealf_f(float _Complex z) { return __real__ z; }
static inline float cimagf_f(float _Complex z) { return __imag__ z; }
static inline double crealf_d(double _Complex z) { return __real__ z; }
static inline double cimagf_d(double _Complex z) { return __imag__ z; }
#define fabsd fabs
#define ilogbd ilogb
#define ldexpd ldexp
#define sqrtd sqrt
#define copysignd copysign
#define log1pd log1p
#define logd log
#define atan2d atan2
#define expd exp
#define cosd cos
#define sind sin
#define sinhd sinh
#define coshd cosh
#define tand tan
JL_COMPLEX_OPS(float, f, float _Complex, f, FLT_MAX, 0x1p-104, 89.415985f)
JL_COMPLEX_OPS(double, d, double _Complex, d, DBL_MAX, 0x1p-971, 710.4758600739439)

/* Division and inv.  ComplexF64: inv is Smith's algorithm scaled by powers of two; / is Baudin & Smith's robust division, scaled
 * when an operand is near over- or underflow.  ComplexF32: both widen to ComplexF64 — inv = conj(w) / abs2(w), z / w = z * inv(w) —
 * and round each component once. */
static double _Complex inv64(double c, double d) {
    if (isinf(c) || isinf(d)) return mkd(copysign(0.0, c), signbit(d) ? 0.0 : -0.0);
    double cd = (isnan(c) || isnan(d)) ? fabs(c) + fabs(d) : fmax(fabs(c), fabs(d));
    const double eps = DBL_EPSILON, bs = 2.0 / (eps * eps);
    double s = 1.0, p, q;
    if (cd >= 0.5 * DBL_MAX) { c *= 0.5; d *= 0.5; s *= 0.5; }
    if (cd <= DBL_MIN * 2.0 / eps) { c *= bs; d *= bs; s *= bs; }
    if (fabs(d) <= fabs(c)) {
        double r = d / c, t = 1.0 / (c + d * r);
        p = t;
        q = -r * t;
    } else {
        double r = c / d, t = 1.0 / (d + c * r);
        p = r * t;
        q = -t;
    }
    return mkd(p * s, q * s);
}
static double rdiv2(double a, double b, double c, double d, double r, double t) {
    if (r != 0) {
        double br = b * r;
        return br != 0 ? (a + br) * t : a * t + (b * t) * r;
    }
    return (a + d * (b / c)) * t;
}
static void rdiv1(double a, double b, double c, double d, double *p, double *q) {
    double r = d / c, t = 1.0 / (c + d * r);
    *p = rdiv2(a, b, c, d, r, t);
    *q = rdiv2(b, -a, c, d, r, t);
}
static void cdiv(double a, double b, double c, double d, double *p, double *q) {
    if (fabs(d) <= fabs(c)) rdiv1(a, b, c, d, p, q);
    else { rdiv1(b, a, d, c, p, q); *q = -*q; }
}
static double _Complex div64(double a, double b, double c, double d) {
    double ab = fabs(a) >= fabs(b) ? fabs(a) : fabs(b), cd = fabs(c) >= fabs(d) ? fabs(c) : fabs(d);
    const double halfov = 0.5 * DBL_MAX, twoun = DBL_MIN * 2.0 / DBL_EPSILON, bs = 2.0 / (DBL_EPSILON * DBL_EPSILON);
    double p, q, s = 1.0;
    if (ab >= halfov || ab <= twoun || cd >= halfov || cd <= twoun) {
        if (ab >= halfov) { a *= 0.5; b *= 0.5; s *= 2.0; }
        else if (ab <= twoun) { a *= bs; b *= bs; s /= bs; }
        if (cd >= halfov) { c *= 0.5; d *= 0.5; s *= 0.5; }
        else if (cd <= twoun) { c *= bs; d *= bs; s *= bs; }
        cdiv(a, b, c, d, &p, &q);
        return mkd(p * s, q * s);
    }
    cdiv(a, b, c, d, &p, &q);
    return mkd(p, q);
}
static inline double _Complex divd(double _Complex z, double _Complex w) { return div64(crealf_d(z), cimagf_d(z), crealf_d(w), cimagf_d(w)); }
static inline double _Complex invd(double _Complex w) { return inv64(crealf_d(w), cimagf_d(w)); }
static inline float _Complex divf(float _Complex z, float _Complex w) {
    double _Complex r = muld(mkd(crealf_f(z), cimagf_f(z)), inv64(crealf_f(w), cimagf_f(w)));
    return mkf((float)crealf_d(r), (float)cimagf_d(r));
}
static inline float _Complex invf(float _Complex w) {
    double re = crealf_f(w), im = cimagf_f(w), a2 = re * re + im * im;
    return mkf((float)(re / a2), (float)(-im / a2));
}

/* the opcode dispatch: the 19 opcodes DESIGN.md §14.1 admits, NaN + NaN im for anything else (the library refuses those) */
#define JL_COMPLEX_DISPATCH(S, CT, R)                                                                                             \
    static CT o_unary_c##S(int op, CT x) {                                                                                       \
        switch (op) {                                                                                                            \
        case DE_U_NEG: return mk##S(-crealf_##S(x), -cimagf_##S(x));                                                             \
        case DE_U_SQUARE: return mul##S(x, x);                                                                                   \
        case DE_U_CUBE: return mul##S(mul##S(x, x), x);                                                                          \
        case DE_U_INV: return inv##S(x);                                                                                         \
        case DE_U_SQRT: return csqrt_jl##S(x);                                                                                   \
        case DE_U_EXP: return cexp_jl##S(x);                                                                                     \
        case DE_U_LOG: return clog_jl##S(x);                                                                                     \
        case DE_U_SIN: return csin_jl##S(x);                                                                                     \
        case DE_U_COS: return ccos_jl##S(x);                                                                                     \
        case DE_U_TAN: return ctan_jl##S(x);                                                                                     \
        case DE_U_SINH: return csinh_jl##S(x);                                                                                   \
        case DE_U_COSH: return ccosh_jl##S(x);                                                                                   \
        case DE_U_TANH: return ctanh_jl##S(x);                                                                                   \
        case DE_U_COS2: { CT c = ccos_jl##S(x); return mul##S(c, c); }                                                          \
        default: return mk##S((R)NAN, (R)NAN);                                                                                   \
        }                                                                                                                        \
    }                                                                                                                            \
    static CT o_binary_c##S(int op, CT x, CT y) {                                                                                \
        switch (op) {                                                                                                            \
        case DE_B_ADD: return mk##S(crealf_##S(x) + crealf_##S(y), cimagf_##S(x) + cimagf_##S(y));                               \
        case DE_B_SUB: return mk##S(crealf_##S(x) - crealf_##S(y), cimagf_##S(x) - cimagf_##S(y));                               \
        case DE_B_MUL: return mul##S(x, y);                                                                                      \
        case DE_B_DIV: return div##S(x, y);                                                                                      \
        default: return mk##S((R)NAN, (R)NAN);                                                                                   \
        }                                                                                                                        \
    }                                                                                                                            \
    static CT o_ternary_c##S(int op, CT x, CT y, CT z) {                                                                         \
        if (op != DE_T_ADD3) return mk##S((R)NAN, (R)NAN);                                                                       \
        return mk##S((crealf_##S(x) + crealf_##S(y)) + crealf_##S(z), (cimagf_##S(x) + cimagf_##S(y)) + cimagf_##S(z));         \
    }                                                                                                                            \
    /* (the walker's gradient code is compiled, never called: no complex gradients) */                                          \
    static void o_unary_grad_c##S(int op, CT x, CT *g) { (void)op; (void)x; g[0] = mk##S((R)NAN, (R)NAN); }                    \
    static void o_binary_grad_c##S(int op, CT x, CT y, CT *g) { (void)op; (void)x; (void)y; g[0] = g[1] = mk##S((R)NAN, (R)NAN); } \
    static void o_ternary_grad_c##S(int op, CT x, CT y, CT z, CT *g) {                                                          \
        (void)op; (void)x; (void)y; (void)z;                                                                                     \
        g[0] = g[1] = g[2] = mk##S((R)NAN, (R)NAN);                                                                              \
    }
JL_COMPLEX_DISPATCH(f, float _Complex, float)
JL_COMPLEX_DISPATCH(d, double _Complex, double)

/* ---- the walker, twice.  is_valid(z) = isfinite(re) && isfinite(im) (src/ValueInterface.jl:6); the walker's sum of an array adds
 * complex values, i.e. each component separately (:9).  + - * / and square leave the walker's inline paths (renamed opcodes). */
#undef isfinite
#define isfinite(z) (__builtin_isfinite(__real__(z)) && __builtin_isfinite(__imag__(z)))
#define DE_B_MUL (-1001)
#define DE_B_DIV (-1002)
#define DE_U_SQUARE (-1003)
#define DE_B_ADD (-1004)
#define DE_B_SUB (-1005)

#define OT float _Complex
#define ONAME _cf32
#define o_unary_cf32 o_unary_cf
#define o_binary_cf32 o_binary_cf
#define o_ternary_cf32 o_ternary_cf
#define o_unary_grad_cf32 o_unary_grad_cf
#define o_binary_grad_cf32 o_binary_grad_cf
#define o_ternary_grad_cf32 o_ternary_grad_cf
#include "../../oracle/de_oracle_impl.h"
#undef OT
#undef ONAME

#define OT double _Complex
#define ONAME _cf64
#define o_unary_cf64 o_unary_cd
#define o_binary_cf64 o_binary_cd
#define o_ternary_cf64 o_ternary_cd
#define o_unary_grad_cf64 o_unary_grad_cd
#define o_binary_grad_cf64 o_binary_grad_cd
#define o_ternary_grad_cf64 o_ternary_grad_cd
#include "../../oracle/de_oracle_impl.h"
#undef OT
#undef ONAME
#undef DE_B_MUL
#undef DE_B_DIV
#undef DE_U_SQUARE
#undef DE_B_ADD
#undef DE_B_SUB

/* Scalar probes: (re, im) in, (re, im) out — in double for both instantiations (ComplexF32 values are exact in double) */
void de_oracle_op_cf64(int degree, int op, const double *x, const double *y, const double *z, double *out) {
    double _Complex a = mkd(x[0], x[1]), b = y ? mkd(y[0], y[1]) : a, c = z ? mkd(z[0], z[1]) : a, r;
    r = degree == 1 ? o_unary_cd(op, a) : degree == 2 ? o_binary_cd(op, a, b) : o_ternary_cd(op, a, b, c);
    out[0] = crealf_d(r);
    out[1] = cimagf_d(r);
}
void de_oracle_op_cf32(int degree, int op, const double *x, const double *y, const double *z, double *out) {
    float _Complex a = mkf((float)x[0], (float)x[1]), b = y ? mkf((float)y[0], (float)y[1]) : a, c = z ? mkf((float)z[0], (float)z[1]) : a, r;
    r = degree == 1 ? o_unary_cf(op, a) : degree == 2 ? o_binary_cf(op, a, b) : o_ternary_cf(op, a, b, c);
    out[0] = crealf_f(r);
    out[1] = cimagf_f(r);
}
int de_oracle_complex_abi(void) { return DE_HIP_ABI_VERSION; }
