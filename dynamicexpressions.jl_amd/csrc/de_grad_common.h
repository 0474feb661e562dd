// de_grad_common.h — device code shared by the three gradient kernels (de_grad_tape.h: flat switch,
// eval_diff and wide gradients; de_grad_threaded.hip: threaded code; de_rev_threaded.hip: reverse accumulation):
// kernel arguments, value+partial functions of every operator (ChainRules scalar rules, same table as
// oracle/de_oracle_ops.h), tile map, tile prologue (X rows, parameter rows), loss term.  What a module of the two
// threaded kernels exports (GradModule).  The launch itself is host code in de_grad_tape.h and de_grad_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "de_device_ops.h"
#include "de_kernels.h"
#include "de_loss_kinds.h"
#include "de_plan.h"

namespace de {

#define DE_UNROLL _Pragma("unroll")

template <typename T> struct GArgs {
    const BoundInstr *code;  // BOUND form of the UNFOLDED program (de_bind.h, ee binding), +1 pad
    const int32_t *code_off; // n_trees + 1
    const T *X;
    T *out;                  // may be null
    T *grad;
    const int64_t *grad_off; // n_trees element offsets
    const int32_t *n_grad;   // n_trees
    uint8_t *ok;
    const T *params;
    const void *classes;
    int64_t N, ldX, ld_out, ld_params, n_tiles, n_classes;
    int32_t F, P, n_trees, trees_per_chunk, n_chunks, n_slots;
    int32_t mode; // mode, uses_params and check are read by the flat kernel only (the threaded kernels: template parameter PARAMS, always checked)
    int32_t FX; // threaded kernels: rows of X; F - FX further leaf rows hold the parameters gathered by class (0 elsewhere)
    int32_t classes_is_i64, class_base, uses_params, check;
    int32_t skip_flagged; // early exit at tree granularity: the trees of a chunk whose flag is already 0 are not evaluated (de_kernels.hip)
    int32_t diff_g0; // >= 0: eval_diff mode — single component diff_g0, dense [n_trees, ld_out] output
    // fused loss + pullback (de_eval_loss_grad): instead of storing x and d[k] the kernel reduces
    //   sum_j w_j l(x_j - y_j)   and   sum_j w_j l'(x_j - y_j) d_k[j]   per wavefront
    int32_t loss_mode;       // 0 = off, 1 + de_loss_kind otherwise
    const T *y;
    const T *w;              // may be null
    T *partial;              // [n_tiles][n_cols][4 waves]; tree t owns columns col_off[t] .. col_off[t] + n_grad[t] (loss first)
    const int64_t *col_off;  // n_trees + 1
    const int32_t *tree_ids; // threaded kernel: the n_trees trees this launch evaluates (null = 0..n_trees-1)
    int32_t n_all_trees;     // trees of the program (col_off has n_all_trees + 1 entries)
    const int64_t *tile_range; // de_rev_threaded.hip, by-class reduction: (first sample, last sample) of every tile, or null
    const int32_t *rev_mid;  // de_rev_threaded.hip: first backward instruction of every tree
    int32_t rev_rows;        // ... and LDS rows per wave (X + slots + partial rows + staging)
    int32_t rev_stage_cols, rev_stage_rows; // per-wave staging of the column sums (elements / rows)
    // priority tiles (de_kernels.hip de_tile_extremes_kernel): the first n_prio_blocks workgroups (of every window) run the tiles
    // (prio[k] & 0xFFFFFFFF) >> prio_shift first; null / 0: none
    const unsigned long long *prio;
    uint32_t n_prio, n_prio_blocks, prio_shift;
    // de_grad_threaded.hip, SHARED LEAF ROWS (de_kernels.h GradArgs::gt_share): a workgroup = four waves on the same 64 x VS samples, wave w
    // runs every fourth tree of the chunk through stream variant w (var_stride records apart); tiles are 64 x VS samples
    int32_t share;
    int64_t var_stride;
    T loss_param; // the parameter of a parameterised loss kind (de_loss_kinds.h), in T; 0 for the kinds that have none
    T loss_floor; // Gauss-Newton tree ends: the residual floor of the kind's curvature weight (de_loss_kinds.h loss_kind_curv), in T
};

// Early exit at tree granularity (src/Evaluate.jl:26-32, src/EvaluateDerivative.jl:230-243: the reference returns at the first
// non-finite array): bit i = the i-th tree of this workgroup's chunk was already flagged incomplete when the workgroup started —
// by a workgroup that ran earlier or by the host (non-finite constant).  Its values / Jacobian rows are unspecified then (SURVEY
// §8a), fused reductions of it are NaN (the finish kernels look at the flag), so the chunk loop steps over it.  Chunks have <= 64
// trees (else: no skipping).  Agent-scope load: past this CU's vector cache.
template <typename IDS> __device__ __forceinline__ uint64_t gskip_mask(uint8_t *ok, IDS tree_ids, int t0, int t1, int enabled, int64_t tile) {
    if (!enabled || t1 - t0 > 64) return 0ull;
    const int i = t0 + (int)(threadIdx.x & 63);
    uint8_t f = 1;
    if (i < t1) f = skip_flag_load(ok + (tree_ids ? tree_ids[i] : i), enabled, tile);
    return __ballot(f == 0);
}
template <typename T> __device__ __forceinline__ T gimm(uint32_t w2, uint32_t w3);
template <> __device__ __forceinline__ float gimm<float>(uint32_t w2, uint32_t) { return __uint_as_float(w2); }
template <> __device__ __forceinline__ double gimm<double>(uint32_t w2, uint32_t w3) {
    return __longlong_as_double((long long)(((unsigned long long)w3 << 32) | w2));
}

// value + partial of a unary operator; Zygote `nothing` -> 0 (ext/DynamicExpressionsZygoteExt.jl:12-15)
template <typename T> struct UG { T y, g; };
template <typename T> __device__ __noinline__ UG<T> unary_vg(uint32_t op, T x) {
    using m = M<T>;
    UG<T> r;
    const T LN2 = T(0.693147180559945309417232121458176568), LN10 = T(2.302585092994045684017991454684364208);
    switch (op) {
    case DE_U_NEG: r.y = -x; r.g = T(-1); break;
    case DE_U_ABS: r.y = m::abs(x); r.g = jl_sign(x); break;
    case DE_U_SQUARE: r.y = x * x; r.g = x + x; break;
    case DE_U_CUBE: r.y = (x * x) * x; r.g = (T(3) * x) * x; break;
    case DE_U_RELU: r.y = x < T(0) ? T(0) : x; r.g = x < T(0) ? T(0) : T(1); break;
    case DE_U_SIGN: r.y = jl_sign(x); r.g = T(0); break;
    case DE_U_ROUND: r.y = m::rint(x); r.g = T(0); break;
    case DE_U_FLOOR: r.y = m::floor(x); r.g = T(0); break;
    case DE_U_CEIL: r.y = m::ceil(x); r.g = T(0); break;
    case DE_U_INV: r.y = T(1) / x; r.g = -(r.y * r.y); break;
    case DE_U_SQRT: r.y = m::sqrt(x); r.g = T(1) / (T(2) * r.y); break;
    case DE_U_CBRT: r.y = m::cbrt(x); r.g = T(1) / (T(3) * (r.y * r.y)); break;
    case DE_U_EXP: r.y = m::exp(x); r.g = r.y; break;
    case DE_U_EXP2: r.y = m::exp2(x); r.g = r.y * LN2; break;
    case DE_U_LOG: r.y = m::log(x); r.g = T(1) / x; break;
    case DE_U_LOG2: r.y = m::log2(x); r.g = (T(1) / x) / LN2; break;
    case DE_U_LOG10: r.y = m::log10(x); r.g = (T(1) / x) / LN10; break;
    case DE_U_LOG1P: r.y = m::log1p(x); r.g = T(1) / (x + T(1)); break;
    case DE_U_SIN: r.y = m::sin(x); r.g = m::cos(x); break;
    case DE_U_COS: r.y = m::cos(x); r.g = -m::sin(x); break;
    case DE_U_TAN: r.y = m::tan(x); r.g = T(1) + r.y * r.y; break;
    case DE_U_SINH: r.y = m::sinh(x); r.g = m::cosh(x); break;
    case DE_U_COSH: r.y = m::cosh(x); r.g = m::sinh(x); break;
    case DE_U_TANH: r.y = m::tanh(x); r.g = T(1) - r.y * r.y; break;
    case DE_U_ASIN: r.y = m::asin(x); r.g = T(1) / m::sqrt(T(1) - x * x); break;
    case DE_U_ACOS: r.y = m::acos(x); r.g = -(T(1) / m::sqrt(T(1) - x * x)); break;
    case DE_U_ATAN: r.y = m::atan(x); r.g = T(1) / (T(1) + x * x); break;
    case DE_U_ASINH: r.y = m::asinh(x); r.g = T(1) / m::sqrt(x * x + T(1)); break;
    case DE_U_ACOSH: r.y = m::acosh(x); r.g = T(1) / (m::sqrt(x - T(1)) * m::sqrt(x + T(1))); break;
    case DE_U_ATANH: r.y = m::atanh(x); r.g = T(1) / (T(1) - x * x); break;
    case DE_U_SAFE_LOG: r.y = x <= T(0) ? m::nan() : m::log(x); r.g = x <= T(0) ? T(0) : T(1) / x; break;
    case DE_U_SAFE_LOG2: r.y = x <= T(0) ? m::nan() : m::log2(x); r.g = x <= T(0) ? T(0) : (T(1) / x) / LN2; break;
    case DE_U_SAFE_LOG10: r.y = x <= T(0) ? m::nan() : m::log10(x); r.g = x <= T(0) ? T(0) : (T(1) / x) / LN10; break;
    case DE_U_SAFE_LOG1P: r.y = x <= T(-1) ? m::nan() : m::log1p(x); r.g = x <= T(-1) ? T(0) : T(1) / (x + T(1)); break;
    case DE_U_SAFE_SQRT:
        if (x < T(0)) { r.y = m::nan(); r.g = T(0); } else { r.y = m::sqrt(x); r.g = T(1) / (T(2) * r.y); }
        break;
    case DE_U_SAFE_ACOSH:
        r.y = x < T(1) ? m::nan() : m::acosh(x);
        r.g = x < T(1) ? T(0) : T(1) / (m::sqrt(x - T(1)) * m::sqrt(x + T(1)));
        break;
    case DE_U_COS2: { const T c = m::cos(x), s = m::sin(x); r.y = c * c; r.g = (T(2) * c) * (-s); } break;
    case DE_U_GAMMA: r.y = m::tgamma(x); r.g = r.y * dev_digamma(x); break;
    default: r.y = m::nan(); r.g = m::nan(); break;
    }
    return r;
}

// Value and derivative of the cheap unary operators, inline: the same expressions as unary_vg (de_grad_common.h), so a tree
// gives the same bits whichever handler serves it.  K: 3 neg 4 square 5 cube 6 abs 7 log 8 safe_log 9 sqrt 10 safe_sqrt 11 tanh 12 relu
template <typename T, int K> __device__ __forceinline__ UG<T> gun_inline(T x) {
    using m = M<T>;
    UG<T> r;
    if constexpr (K == 3) { r.y = -x; r.g = T(-1); }
    else if constexpr (K == 4) { r.y = x * x; r.g = x + x; }
    else if constexpr (K == 5) { r.y = (x * x) * x; r.g = (T(3) * x) * x; }
    else if constexpr (K == 6) { r.y = m::abs(x); r.g = jl_sign(x); }
    else if constexpr (K == 7) { r.y = m::log(x); r.g = T(1) / x; }
    else if constexpr (K == 8) { r.y = x <= T(0) ? m::nan() : m::log(x); r.g = x <= T(0) ? T(0) : T(1) / x; }
    else if constexpr (K == 9) { r.y = m::sqrt(x); r.g = T(1) / (T(2) * r.y); }
    else if constexpr (K == 10) {
        if (x < T(0)) { r.y = m::nan(); r.g = T(0); } else { r.y = m::sqrt(x); r.g = T(1) / (T(2) * r.y); }
    } else if constexpr (K == 11) { r.y = m::tanh(x); r.g = T(1) - r.y * r.y; }
    else { r.y = x < T(0) ? T(0) : x; r.g = x < T(0) ? T(0) : T(1); }
    return r;
}
// value + both partials of op(x, y) (x = first/left argument)
template <typename T> struct BG { T v, gx, gy; };
template <typename T> __device__ __noinline__ BG<T> binary_vg(uint32_t op, T x, T y) {
    using m = M<T>;
    BG<T> r;
    switch (op) {
    case DE_B_ADD: r.v = x + y; r.gx = T(1); r.gy = T(1); break;
    case DE_B_SUB: r.v = x - y; r.gx = T(1); r.gy = T(-1); break;
    case DE_B_MUL: r.v = x * y; r.gx = y; r.gy = x; break;
    case DE_B_DIV: r.v = x / y; r.gx = T(1) / y; r.gy = -(r.v / y); break;
    case DE_B_POW: { // ChainRules _pow_grad_x / _pow_grad_p (real case)
        r.v = m::pow(x, y);
        if (x != T(0) || y < T(0)) r.gx = (!m::isfinite(x) && x == x && y == T(1)) ? T(1) : (r.v * y) / x;
        else if (y == T(1)) r.gx = T(1);
        else if (y == T(0) || y > T(1)) r.gx = T(0);
        else r.gx = m::inf();
        if (x != T(0)) r.gy = r.v * m::log(m::abs(x));
        else if (y > T(0)) r.gy = T(0);
        else r.gy = m::nan();
    } break;
    case DE_B_MAX: { const bool gt = x > y; r.v = jl_max(x, y); r.gx = gt ? T(1) : T(0); r.gy = gt ? T(0) : T(1); } break;
    case DE_B_MIN: { const bool gt = x > y; r.v = jl_min(x, y); r.gx = gt ? T(0) : T(1); r.gy = gt ? T(1) : T(0); } break;
    case DE_B_MOD: {
        r.v = jl_mod(x, y);
        const T u = x / y;
        const bool isint = (u == m::floor(u)) && m::isfinite(u);
        r.gx = isint ? m::nan() : T(1);
        r.gy = isint ? m::nan() : -m::floor(u);
    } break;
    case DE_B_REM: {
        r.v = m::fmod(x, y);
        const T u = x / y;
        const bool isint = (u == m::floor(u)) && m::isfinite(u);
        r.gx = isint ? m::nan() : T(1);
        r.gy = isint ? m::nan() : -m::trunc(u);
    } break;
    case DE_B_GREATER: r.v = x > y ? T(1) : T(0); r.gx = T(0); r.gy = T(0); break;
    case DE_B_POW_ABS2: {
        const T a = m::abs(x), l = m::log(a), mm = y * l;
        r.v = m::exp(mm);
        r.gx = ((r.v * y) * (T(1) / a)) * jl_sign(x);
        r.gy = r.v * l;
    } break;
    default: r.v = r.gx = r.gy = m::nan(); break;
    }
    return r;
}

template <typename T> struct TG { T v, g0, g1, g2; };
template <typename T> __device__ __noinline__ TG<T> ternary_vg(uint32_t op, T x, T y, T z) {
    using m = M<T>;
    TG<T> r;
    switch (op) {
    case DE_T_FMA: r.v = m::fma(x, y, z); r.g0 = y; r.g1 = x; r.g2 = T(1); break;
    case DE_T_CLAMP:
        r.v = x > z ? z : (x < y ? y : x);
        r.g0 = (x > z || x < y) ? T(0) : T(1);
        r.g1 = (x > z) ? T(0) : (x < y ? T(1) : T(0));
        r.g2 = (x > z) ? T(1) : T(0);
        break;
    case DE_T_ADD3: r.v = (x + y) + z; r.g0 = r.g1 = r.g2 = T(1); break;
    default: {
        const T mx = jl_max(x, y);
        const bool gt1 = x > y, gt2 = mx > z;
        r.v = jl_max(mx, z);
        r.g0 = (gt2 && gt1) ? T(1) : T(0);
        r.g1 = (gt2 && !gt1) ? T(1) : T(0);
        r.g2 = gt2 ? T(0) : T(1);
    } break;
    }
    return r;
}

// map_block (de_plan.h) with the launch's priority tiles in front (their flags travel at agent scope whatever the launch's protocol is)
struct GTileMap : TileMap { bool prio; };
template <typename T> __device__ __forceinline__ GTileMap gmap_block_prio(const GArgs<T> &a, uint32_t bid) {
    if (bid >= a.n_prio_blocks) return GTileMap{map_block(bid - a.n_prio_blocks, a.n_chunks, a.n_tiles), false};
    GTileMap m;
    const uint32_t k = bid / (uint32_t)a.n_chunks;
    m.chunk = (int32_t)(bid % (uint32_t)a.n_chunks);
    m.tile = k < a.n_prio ? (int64_t)((uint32_t)a.prio[k] >> a.prio_shift) : 0;
    m.valid = k < a.n_prio && m.tile < a.n_tiles;
    m.prio = true;
    return m;
}
__device__ __noinline__ void gflag_incomplete(uint8_t *ok, int agent) { // agent scope (written through): workgroups that start later skip the tree
    if ((threadIdx.x & 63) == 0) {
        if (agent) __hip_atomic_store(ok, (uint8_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else *ok = 0;
    }
}

constexpr int GBLK = 256;

// ---- tile prologue -----------------------------------------------------------------------------------------------------------------
// Stage leaf rows of a tile of `samples` samples that starts at sample `base` (samples behind `last` are copies of `last`); at(j, f) = the
// LDS element of (sample j of the tile, leaf row f), which is all the kernels' layouts differ in.  Plain values, not the kernel-argument
// struct (g_epilogue_loss, de_grad_threaded.hip: handing that around by address makes its loads look divergent).
// ... rows [0, n_rows): X
template <typename T, typename AT>
__device__ __forceinline__ void stage_x_rows(T *rows, const T *X, int64_t ldX, uint32_t n_rows, uint32_t samples, int64_t base, int64_t last, AT at) {
    const uint32_t total = samples * n_rows;
    for (uint32_t e = threadIdx.x; e < total; e += GBLK) {
        const uint32_t j = e / n_rows, f = e - j * n_rows;
        int64_t jj = base + j;
        jj = jj < last ? jj : last;
        rows[at(j, f)] = X[f + ldX * jj];
    }
}
// ... rows [row0, row0 + n_rows): params[:, class of the sample] (src/ParametricExpression.jl:381-389), read through the caches
template <typename T, typename AT>
__device__ __forceinline__ void stage_param_rows(T *rows, const T *params, int64_t ld_params, const void *classes, int32_t classes_is_i64, int32_t class_base,
                                                 int64_t n_classes, uint32_t row0, uint32_t n_rows, uint32_t samples, int64_t base, int64_t last, AT at) {
    const uint32_t total = samples * n_rows;
    for (uint32_t e = threadIdx.x; e < total; e += GBLK) {
        const uint32_t j = e / n_rows, q = e - j * n_rows;
        int64_t jj = base + j;
        jj = jj < last ? jj : last;
        const int64_t cl = clamp_class((classes_is_i64 ? reinterpret_cast<const int64_t *>(classes)[jj] : (int64_t) reinterpret_cast<const int32_t *>(classes)[jj]) - class_base, n_classes);
        rows[at(j, row0 + q)] = params[q + ld_params * cl];
    }
}

// Loss term of one sample — value x, target yv, weight wv —: l = w * l(x - y) and lp = w * l'(x - y), the factor of the pullback.
// loss_mode = 1 + de_loss_kind; weight 0 (and samples past N) really excludes the sample.  p = GArgs::loss_param: the parameter of the
// kinds of de_loss_kinds.h (wave-uniform dispatch on loss_mode, the three first kinds first).
template <typename T> struct LossTerm { T l, lp; };
// (out of line: the table's transcendental arms stay out of the kernels' and epilogues' own code, which L2 / L1 / PULLBACK run as before)
template <typename T> __device__ __noinline__ LossKindTerm<T> loss_kind_term_ool(int kind, T x, T yv, T p) { return loss_kind_term<T>(kind, x, yv, p); }
template <typename T> __device__ __forceinline__ LossTerm<T> loss_term(int loss_mode, T x, T yv, T wv, T p) {
    const T e = x - yv;
    LossTerm<T> r;
    if (loss_mode == 1 + DE_LOSS_L2) { r.l = wv * (e * e); r.lp = wv * (T(2) * e); }
    else if (loss_mode == 1 + DE_LOSS_L1) { r.l = wv * M<T>::abs(e); r.lp = wv * jl_sign(e); }
    else if (loss_mode <= 1 + DE_LOSS_PULLBACK) { r.l = wv * (x * yv); r.lp = wv * yv; } // DE_LOSS_PULLBACK: y holds the cotangent dY
    else { const LossKindTerm<T> k = loss_kind_term_ool<T>(loss_mode - 1, x, yv, p); r.l = wv * k.l; r.lp = wv * k.lp; }
    if (wv == T(0)) { r.l = T(0); r.lp = T(0); }
    return r;
}
// A wave-uniform value that reached an out-of-line function in a vector register (the calling convention passes every argument in one):
// back into scalar registers, so that it costs no vector register across the function's own calls and branches on it are scalar.
__device__ __forceinline__ int guni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t guni(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
template <typename P> __device__ __forceinline__ const P *guni(const P *p) { return reinterpret_cast<const P *>((uintptr_t)guni((int64_t)(uintptr_t)p)); }
__device__ __forceinline__ float guni(float v) { return __int_as_float(guni(__float_as_int(v))); }
__device__ __forceinline__ double guni(double v) { return __longlong_as_double((long long)guni((int64_t)__double_as_longlong(v))); }
// The curvature weight of one sample for the Gauss-Newton tree ends (de_loss_kinds.h loss_kind_curv; loss_mode != 1 + DE_LOSS_L2, whose
// weight is 1 and whose tree ends keep the code they had): out of line like the loss table, f = GArgs::loss_floor.
template <typename T> __device__ __noinline__ T loss_kind_curv_ool(int kind, T x, T yv, T p, T f) { return loss_kind_curv_term<T>(guni(kind), x, yv, guni(p), guni(f)); }

// What a module of the threaded kernels (de_grad_threaded.hip: 18, de_rev_threaded.hip: 2) hands to the one launch path
// (de_grad_kernels.hip): the host stubs of its handler-table fill kernel and of its kernel, kernel[PARAMS][SHARE] (the reverse kernel
// has no SHARE form); kernel_gn: the same kernels with the Gauss-Newton tree end (de_eval_loss_gn; forward modules only).  Every kernel
// takes (GArgs<T>, handler base, parameter handler offset).  kernel_fit: the same kernels with the fit-statistics tree end
// (de_eval_fit_stats_grad, g_epilogue_fit; forward modules only).
struct GradModule { const void *fill; const void *kernel[2][2]; const void *kernel_gn[2][2]; const void *kernel_fit[2][2]; };

// Fit-statistics launches (de_eval_fit_stats_grad; GArgs::loss_mode = FIT_MODE_PLAIN / FIT_MODE_JTJ, GArgs::loss_param =
// T(mean_y)).  Columns of a tree in `partial`, per (tile of 256 x VS samples, wave):
//   0 m   1 S1   2 B   3 Cc   4 W_wave   5 R_wave   6 + k: D_k   6 + G + k: P'_k   6 + 2 G + k: Q'_k   6 + 3 G + k (k + 1) / 2 + i: the triangle
// (the triangle where the tree has at most DE_GN_MAX_ROWS rows and the caller wants the matrix; FIT_COLS, FIT_MODE_*: de_kernels.h).
// the value wave_sum_to_lane63 left in lane 63, in every lane
__device__ __forceinline__ float gwave_lane63(float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63)); }
__device__ __forceinline__ double gwave_lane63(double v) {
    const long long b = __double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)b >> 32), 63);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

} // namespace de
