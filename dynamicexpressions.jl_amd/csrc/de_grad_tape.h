// de_grad_tape.h — the forward-dual tape interpreter over the generic bound stream, once, and the one launch path of the gradient kernels.
// Replaces the reference's src/EvaluateDerivative.jl: eval_grad_tree_array (:193-243), grad_degn_eval (:340-365), grad_deg0_eval
// (:367-404) and eval_diff_tree_array (:40-168).
//
// Every sample carries a dual number (x, d[0..GC)) through the same accumulator program the eval kernel runs (de_program.h, generic
// form): one sample per lane, a 256-sample tile per workgroup.  GC = the window of gradient components a launch handles; wider gradients
// (constant mode with many constants, :both mode) are covered by several windows (blockIdx.y), each recomputing x — the alternative,
// (1+n_grad) live values per spill slot, would wreck occupancy.  Semantics follow the reference exactly:
//   * d[k] = g1*d1[k] + g2*d2[k] with dense arithmetic, leaf gradients materialised as 0/1 (so an infinite partial times a zero seed is
//     NaN, as in grad_degn_eval);
//   * after EVERY node (leaves included) x and all d[k] are validity-tested (:239-242);
//   * eval_diff (single direction) performs NO validity test (:99-119).
//
// The skeleton, de_grad_tape_kernel<A, GC, GN, FIT>, owns the control flow: tile map, class lookup, seeds, skip mask, windows, the loop
// over records and its switch, spill slots, the root's validity test, the stores and the flag.  The ARITHMETIC POLICY A says what a value
// is and never sees a record (RealGrad<T> in de_grad_kernels.hip: Float32 / Float64; HalfGrad in de_half_grad.hip: binary16 steps):
//   Elem, V                   the element in memory; the value in a register and in an LDS row (float for binary16)
//   TREE_ENDS                 do the fused tree ends (loss, GN, FIT) exist for the policy?
//   NAMES                     the kernel names reported through kernel_name: plain and, where the tree ends exist, GN, FIT
//   stage_x                   the workgroup's X tile into LDS rows 0 .. F-1 (row stride GRAD_TAPE_ROW elements of V)
//   imm                       the immediate of a constant operand
//   bin<K>, bin_dual<K>       a hot binary form (K: 0 add, 1 sub, 2 rsub, 3 mul, 4 div, 5 rdiv) of (left, right): value and partials; its
//                             dual update from (partial, dual) of left and of right
//   un<K>                     a hot unary form (K: 0 cos, 1 exp, 2 sin): value and partial
//   scale, chain2, chain3     the chain rule: g d,  g1 d1 + g2 d2,  (g0 a + g1 b) + g2 c
//   unary, binary, ternary    the cold tables: value and partials of every other operator, out of line
// The host side — make_gargs, launch_grad_kernel (shared with the threaded and reverse kernels), launch_grad_t and the window ladder
// launch_grad_dt — is templated on the same policy; window and LDS footprint are grad_window / grad_tape_lds_bytes (de_kernels.h).
#pragma once
#include "de_grad_common.h"

namespace de {

static_assert(GBLK + 4 == GRAD_TAPE_ROW, "de_kernels.h GRAD_TAPE_ROW");

// a binary opcode of the generic stream -> (forward opcode, reversed): a reversed form DOP_R* takes the operand as its LEFT argument
__device__ __forceinline__ uint32_t gtape_forward_op(uint32_t gop, bool *rev) {
    uint32_t fop = gop;
    *rev = false;
    switch (gop) {
    case DOP_RSUB: fop = DE_B_SUB; *rev = true; break;
    case DOP_RDIV: fop = DE_B_DIV; *rev = true; break;
    case DOP_RPOW: fop = DE_B_POW; *rev = true; break;
    case DOP_RMOD: fop = DE_B_MOD; *rev = true; break;
    case DOP_RREM: fop = DE_B_REM; *rev = true; break;
    case DOP_RGREATER: fop = DE_B_GREATER; *rev = true; break;
    case DOP_RPOW_ABS2: fop = DE_B_POW_ABS2; *rev = true; break;
    case DOP_RMAX: fop = DE_B_MAX; *rev = true; break;
    case DOP_RMIN: fop = DE_B_MIN; *rev = true; break;
    default: break;
    }
    return fop;
}

// LDS rows of GRAD_TAPE_ROW elements of V: rows [0,F) = X tile, then each spill slot s owns 1+GC rows (x, d[0..GC)).
// GN: the launch of de_eval_loss_gn — behind the loss and its gradient the tree end also reduces the products
// sum_j w_j c_j d_i(j) d_k(j), i <= k < G (c = the loss kind's curvature weight, 1 for L2), of a tree whose rows lie in this one window
// (de_grad_threaded.hip g_epilogue_gn: same columns, same association order).  A template parameter: the other instantiations keep the
// code they had.
// FIT: the launch of de_eval_fit_stats_grad — the tree end of de_grad_threaded.hip g_epilogue_fit, one sample per lane.
template <typename A, int GC, bool GN = false, bool FIT = false>
__global__ void __launch_bounds__(GBLK) de_grad_tape_kernel(const GArgs<typename A::Elem> a) {
    using V = typename A::V;
    using Elem = typename A::Elem;
    constexpr int RS = GRAD_TAPE_ROW; // row stride (elements)
    extern __shared__ __align__(16) unsigned char gsmem[];
    V *__restrict__ rows = reinterpret_cast<V *>(gsmem);

    const TileMap tm = map_block(blockIdx.x, a.n_chunks, a.n_tiles);
    if (!tm.valid) return;
    const int tid = threadIdx.x;
    const int64_t base = tm.tile * GBLK;
    const int64_t last = a.N - 1;
    const int g0 = a.diff_g0 >= 0 ? a.diff_g0 : (int)blockIdx.y * GC; // first gradient component of this window
    const int F = a.F, P = a.P;
    int loss_mode = 0; // (a policy without tree ends: the stores, always)
    if constexpr (A::TREE_ENDS) loss_mode = a.loss_mode;

    A::stage_x(rows, a.X, a.ldX, (uint32_t)F, base, a.N, tid);
    int64_t jj0 = base + tid;
    const bool live = jj0 < a.N;
    jj0 = jj0 < last ? jj0 : last;
    int64_t cls = 0;
    if (a.uses_params)
        cls = clamp_class((a.classes_is_i64 ? reinterpret_cast<const int64_t *>(a.classes)[jj0]
                                            : (int64_t) reinterpret_cast<const int32_t *>(a.classes)[jj0]) - a.class_base, a.n_classes);
    V yv = V(0), wv = V(0);
    if (loss_mode) {
        yv = a.y[jj0];
        wv = live ? (a.w ? (V)a.w[jj0] : V(1)) : V(0);
    }
    __syncthreads();

    const ConstU4Ptr code = (ConstU4Ptr)(uintptr_t)a.code;
    const ConstI32Ptr code_off = (ConstI32Ptr)(uintptr_t)a.code_off;
    const ConstI64Ptr col_off = (ConstI64Ptr)(uintptr_t)a.col_off;
    const ConstI32Ptr n_grad = (ConstI32Ptr)(uintptr_t)a.n_grad;
    const ConstI64Ptr grad_off = (ConstI64Ptr)(uintptr_t)a.grad_off;
    const int t0 = tm.chunk * a.trees_per_chunk;
    const int t1 = (t0 + a.trees_per_chunk < a.n_trees) ? t0 + a.trees_per_chunk : a.n_trees;
    V *__restrict__ stk = rows + (size_t)F * RS;

    // window-local seed of a leaf = its gradient row - g0 (or < 0: no gradient in this mode/window)
    const int feat_seed0 = a.mode != DE_GRAD_CONSTANT ? P - g0 : -0x40000000;
    const int param_seed0 = a.mode != DE_GRAD_CONSTANT ? -g0 : -0x40000000;
    const int const_seed0 = a.mode == DE_GRAD_CONSTANT ? -g0 : (a.mode == DE_GRAD_BOTH ? P + F - g0 : -0x40000000);

    const uint64_t skip = gskip_mask(a.ok, (const int32_t *)nullptr, t0, t1, a.check ? a.skip_flagged : 0, (int64_t)tm.tile);
    for (int tree = t0; tree < t1; ++tree) {
        if ((skip >> (tree - t0)) & 1ull) continue; // already incomplete (early exit)
        const int G = a.diff_g0 >= 0 ? 1 : n_grad[tree];
        if (a.diff_g0 < 0 && g0 >= G && g0 > 0) continue; // window without a component of this tree (window 0 always runs: x, flag)
        int pc = code_off[tree];
        const int pe = code_off[tree + 1];
        V x = V(0), d[GC];
        DE_UNROLL for (int k = 0; k < GC; k++) d[k] = V(0);
        V poison = V(0);
        U32x4 nxt = code[pc];
        for (; pc < pe; ++pc) {
            const U32x4 w = nxt;
            nxt = code[pc + 1];
            // One flat wave-uniform switch over the bound handler id (de_bind.h); the operand is a LEAF row (< F: one-hot seed), a spill
            // ROW (>= F: a popped dual number) or a constant (seed).  Seeds are materialised 0 / 1: Inf * 0 = NaN as in the reference.
#define G_SLOT(r) (stk + ((r) - (uint32_t)F) * (1 + GC) * RS + tid)
#define G_LEAF_ROW(r) { xb = rows[(r) * RS + tid]; seed = (int)(r) + feat_seed0; if (a.check) poison = M<V>::fma(xb, V(0), poison); }
#define G_ROW_OPERAND(r)                                                                           \
    V xb, db[GC];                                                                                  \
    if ((r) < (uint32_t)F) {                                                                       \
        int seed;                                                                                  \
        G_LEAF_ROW(r)                                                                              \
        DE_UNROLL for (int k = 0; k < GC; k++) db[k] = (k == seed) ? V(1) : V(0);                  \
    } else {                                                                                       \
        const V *__restrict__ s_ = G_SLOT(r);                                                      \
        xb = s_[0];                                                                                \
        DE_UNROLL for (int k = 0; k < GC; k++) db[k] = s_[(1 + k) * RS];                           \
    }
#define G_CONST_OPERAND()                                                                          \
    const V xb = A::imm(w);                                                                        \
    V db[GC];                                                                                      \
    { const int seed = (int)(w.y & 0xFFFFu) + const_seed0;                                         \
      DE_UNROLL for (int k = 0; k < GC; k++) db[k] = (k == seed) ? V(1) : V(0); }
#define G_CHK() if (a.check) poison = M<V>::fma(x, V(0), poison);
            // binary hot ops (K: 0 add, 1 sub, 2 rsub, 3 mul, 4 div, 5 rdiv): value and partials w.r.t. (left, right); REV: left = operand
#define G_BIN_APPLY(K)                                                                             \
    {                                                                                              \
        constexpr bool REV = (K == 2 || K == 5);                                                   \
        const V lx = REV ? xb : x, ly = REV ? x : xb;                                              \
        const auto r = A::template bin<K>(lx, ly);                                                 \
        x = r.v;                                                                                   \
        if (REV) { DE_UNROLL for (int k = 0; k < GC; k++) d[k] = A::template bin_dual<K>(r.gx, db[k], r.gy, d[k]); } \
        else { DE_UNROLL for (int k = 0; k < GC; k++) d[k] = A::template bin_dual<K>(r.gx, d[k], r.gy, db[k]); } \
    }
#define G_BIN4(K)                                                                                  \
    case BOP_BIN_BASE + 4 * K + 0: { G_ROW_OPERAND(w.y) G_BIN_APPLY(K) } break;                    \
    case BOP_BIN_BASE + 4 * K + 1: { G_ROW_OPERAND(w.y) G_BIN_APPLY(K) G_CHK() } break;            \
    case BOP_BIN_BASE + 4 * K + 2: { G_CONST_OPERAND() G_BIN_APPLY(K) } break;                     \
    case BOP_BIN_BASE + 4 * K + 3: { G_CONST_OPERAND() G_BIN_APPLY(K) G_CHK() } break;
            // unary hot ops (K: 0 cos, 1 exp, 2 sin) on xin with incoming gradient din[]
#define G_UN_APPLY(K, XIN, DIN)                                                                    \
    {                                                                                              \
        const auto r = A::template un<K>(XIN);                                                     \
        x = r.y;                                                                                   \
        DE_UNROLL for (int k = 0; k < GC; k++) d[k] = A::scale(r.g, DIN[k]);                       \
    }
#define G_UN4(K)                                                                                   \
    case BOP_UN_BASE + 4 * K + 0: G_UN_APPLY(K, x, d) break;                                       \
    case BOP_UN_BASE + 4 * K + 1: G_UN_APPLY(K, x, d) G_CHK() break;                               \
    case BOP_UN_BASE + 4 * K + 2: { G_ROW_OPERAND(w.y) G_UN_APPLY(K, xb, db) } break;              \
    case BOP_UN_BASE + 4 * K + 3: { G_ROW_OPERAND(w.y) G_UN_APPLY(K, xb, db) G_CHK() } break;
            // generic (cold) operators through the policy's out-of-line value+partials functions
#define G_GEN_APPLY(OP, SRC_IS_ACC)                                                                \
    {                                                                                              \
        const uint32_t gop_ = (OP);                                                                \
        if (gop_ < DE_B_ADD) {                                                                     \
            const auto r = A::unary(gop_, SRC_IS_ACC ? x : xb);                                    \
            x = r.y;                                                                               \
            if (SRC_IS_ACC) { DE_UNROLL for (int k = 0; k < GC; k++) d[k] = A::scale(r.g, d[k]); } \
            else { DE_UNROLL for (int k = 0; k < GC; k++) d[k] = A::scale(r.g, db[k]); }           \
        } else {                                                                                   \
            bool rev;                                                                              \
            const uint32_t fop = gtape_forward_op(gop_, &rev);                                     \
            const auto r = rev ? A::binary(fop, xb, x) : A::binary(fop, x, xb);                    \
            x = r.v;                                                                               \
            if (rev) { DE_UNROLL for (int k = 0; k < GC; k++) d[k] = A::chain2(r.gx, db[k], r.gy, d[k]); } \
            else { DE_UNROLL for (int k = 0; k < GC; k++) d[k] = A::chain2(r.gx, d[k], r.gy, db[k]); } \
        }                                                                                          \
    }
            switch (w.x) {
            case BOP_LOAD_ROW: { G_ROW_OPERAND(w.y) x = xb; DE_UNROLL for (int k = 0; k < GC; k++) d[k] = db[k]; } break;
            case BOP_LOAD_CONST: { G_CONST_OPERAND() x = xb; DE_UNROLL for (int k = 0; k < GC; k++) d[k] = db[k]; } break;
            case BOP_PUSH: {
                V *__restrict__ s_ = G_SLOT(w.y);
                s_[0] = x;
                DE_UNROLL for (int k = 0; k < GC; k++) s_[(1 + k) * RS] = d[k];
            } break;
            case BOP_CHECK_ROW: break; // every leaf operand is tested where it is read (G_LEAF_ROW)
            case BOP_CHECK_ACC: G_CHK() break;
            G_BIN4(0) G_BIN4(1) G_BIN4(2) G_BIN4(3) G_BIN4(4) G_BIN4(5)
            G_UN4(0) G_UN4(1) G_UN4(2)
            case BOP_GEN_ROW: { G_ROW_OPERAND(w.y & 0xFFFFFFu) G_GEN_APPLY(w.y >> 24, false) } break;
            case BOP_GEN_CONST: { G_CONST_OPERAND() G_GEN_APPLY(w.y >> 24, false) } break;
            case BOP_GEN_ACC: { const V xb = x; V db[GC]; DE_UNROLL for (int k = 0; k < GC; k++) db[k] = d[k]; G_GEN_APPLY(w.y >> 24, true) } break;
            case BOP_GEN_PARAM: {
                const uint32_t prow = w.y & 0xFFFFu, op_ = w.y >> 24;
                const V xb = (V)a.params[prow + a.ld_params * cls];
                if (a.check) poison = M<V>::fma(xb, V(0), poison);
                V db[GC];
                { const int seed = (int)prow + param_seed0; DE_UNROLL for (int k = 0; k < GC; k++) db[k] = (k == seed) ? V(1) : V(0); }
                if (op_ == DOP_LOAD) { x = xb; DE_UNROLL for (int k = 0; k < GC; k++) d[k] = db[k]; }
                else G_GEN_APPLY(op_, false)
            } break;
            case BOP_TERN: { // acc = op3(row B, row C, acc)
                const V *__restrict__ sb = G_SLOT(w.y & 0xFFFFFFu);
                const V *__restrict__ sc = G_SLOT(w.z);
                const auto r = A::ternary(w.y >> 24, sb[0], sc[0], x);
                x = r.v;
                DE_UNROLL for (int k = 0; k < GC; k++) d[k] = A::chain3(r.g0, sb[(1 + k) * RS], r.g1, sc[(1 + k) * RS], r.g2, d[k]);
            } break;
            default: break;
            }
        }
        // a non-finite d[k] always survives to the root (every update is linear in it), so the gradient
        // is validity-tested once, here; x was tested where the lowering kept a test (H_CHECK_OUT)
        if (a.check) {
            poison = M<V>::fma(x, V(0), poison);
            DE_UNROLL for (int k = 0; k < GC; k++) poison = M<V>::fma(g0 + k < G ? d[k] : V(0), V(0), poison); // real rows only
        }
        if constexpr (A::TREE_ENDS && FIT) {
            const int64_t n_cols = col_off[a.n_trees];
            V *__restrict__ pp = a.partial + ((int64_t)tm.tile * n_cols + col_off[tree]) * 4 + (tid >> 6);
            const bool in = wv != V(0), l63 = (tid & 63) == 63;
            const V yc = yv - a.loss_param; // the centred target: loss_param = T(mean_y)
            const V sw = gwave_lane63(wave_sum_to_lane63(wv)), sy = gwave_lane63(wave_sum_to_lane63(in ? wv * x : V(0)));
            const V m = sw != V(0) ? sy / sw : V(0);
            const V dx = x - m;
            if (g0 == 0) {
                const V wd = wv * dx;
                const V s1 = wave_sum_to_lane63(in ? wd : V(0)), b = wave_sum_to_lane63(in ? M<V>::fma(wd, dx, V(0)) : V(0));
                const V cc = wave_sum_to_lane63(in ? M<V>::fma(wd, yc, V(0)) : V(0)), r = wave_sum_to_lane63(in ? wv * yc : V(0));
                if (l63) { pp[0] = m; pp[4] = s1; pp[8] = b; pp[12] = cc; pp[16] = sw; pp[20] = r; }
            }
            V *__restrict__ pd = pp + FIT_COLS * 4;
            DE_UNROLL for (int k = 0; k < GC; k++) {
                if (g0 + k < G) { // wave-uniform
                    const V wdk = wv * d[k];
                    const V cd = wave_sum_to_lane63(in ? wdk : V(0)), cp = wave_sum_to_lane63(in ? M<V>::fma(wdk, dx, V(0)) : V(0));
                    const V cq = wave_sum_to_lane63(in ? M<V>::fma(wdk, yc, V(0)) : V(0));
                    if (l63) {
                        pd[(int64_t)(g0 + k) * 4] = cd;
                        pd[(int64_t)(G + g0 + k) * 4] = cp;
                        pd[(int64_t)(2 * G + g0 + k) * 4] = cq;
                    }
                }
            }
            if (a.loss_mode == FIT_MODE_JTJ && g0 == 0 && G <= GC) {
                V *__restrict__ pj = pd + (int64_t)(3 * G) * 4;
                DE_UNROLL for (int k = 0; k < GC; k++) {
                    if (k < G) { // wave-uniform
                        DE_UNROLL for (int i = 0; i <= k; i++) {
                            const V s = wave_sum_to_lane63(wv == V(0) ? V(0) : (wv * d[i]) * d[k]);
                            if (l63) pj[(k * (k + 1) / 2 + i) * 4] = s;
                        }
                    }
                }
            }
        } else
        if (loss_mode) {
            if constexpr (A::TREE_ENDS) {
                const LossTerm<V> lt = loss_term<V>(a.loss_mode, x, yv, wv, a.loss_param);
                const int64_t n_cols = col_off[a.n_trees];
                V *__restrict__ pp = a.partial + ((int64_t)tm.tile * n_cols + col_off[tree]) * 4 + (tid >> 6);
                if (g0 == 0) {
                    const V s = wave_sum_to_lane63(lt.l);
                    if ((tid & 63) == 63) pp[0] = s;
                }
                DE_UNROLL for (int k = 0; k < GC; k++) {
                    if (g0 + k < G) { // wave-uniform
                        const V s = wave_sum_to_lane63(wv == V(0) ? V(0) : lt.lp * d[k]);
                        if ((tid & 63) == 63) pp[(int64_t)(1 + g0 + k) * 4] = s;
                    }
                }
                if constexpr (GN) {
                    if (g0 == 0 && G <= GC) {
                        V *__restrict__ pj = pp + (int64_t)(1 + G) * 4;
                        // w c: the kind's curvature weight (de_loss_kinds.h loss_kind_curv); L2 keeps the plain weight it had
                        V wc = wv;
                        if (a.loss_mode != 1 + DE_LOSS_L2) wc = wv * loss_kind_curv_ool<V>(a.loss_mode - 1, x, yv, a.loss_param, a.loss_floor);
                        DE_UNROLL for (int k = 0; k < GC; k++) {
                            if (k < G) { // wave-uniform
                                DE_UNROLL for (int i = 0; i <= k; i++) {
                                    const V s = wave_sum_to_lane63(wv == V(0) ? V(0) : (wc * d[i]) * d[k]);
                                    if ((tid & 63) == 63) pj[(k * (k + 1) / 2 + i) * 4] = s;
                                }
                            }
                        }
                    }
                }
            }
        } else if (live) { // (Elem(v): exact — a policy whose V is wider than Elem keeps every value representable in Elem)
            if (a.diff_g0 >= 0) {
                if (a.out) a.out[(int64_t)tree * a.ld_out + base + tid] = (Elem)x;
                a.grad[(int64_t)tree * a.ld_out + base + tid] = (Elem)d[0];
            } else {
                if (a.out && g0 == 0) a.out[(int64_t)tree * a.ld_out + base + tid] = (Elem)x;
                Elem *__restrict__ gp = a.grad + grad_off[tree] + (int64_t)G * (base + tid) + g0;
                DE_UNROLL for (int k = 0; k < GC; k++)
                    if (g0 + k < G) gp[k] = (Elem)d[k];
            }
        }
        if (a.check && __ballot(poison != poison) != 0ull) gflag_incomplete(a.ok + tree, a.skip_flagged == 1);
    }
}

#undef G_SLOT
#undef G_LEAF_ROW
#undef G_ROW_OPERAND
#undef G_CONST_OPERAND
#undef G_CHK
#undef G_BIN_APPLY
#undef G_BIN4
#undef G_UN_APPLY
#undef G_UN4
#undef G_GEN_APPLY

// ---- one launch path for the gradient kernels ----------------------------------------------------------------------------------------
// The kernel arguments every gradient kernel shares, from the caller's GradArgs; every other field is 0.  What is particular to a
// kernel — its code pointers, the trees of the launch (tree_ids / n_trees), n_slots, n_tiles, the parameter rows behind F, share /
// var_stride, rev_*, tile_range, diff_g0 / check — is set by that kernel's own lines.
template <typename T> static GArgs<T> make_gargs(const GradArgs &ga) {
    const EvalArgs &e = ga.e;
    GArgs<T> a = {};
    a.X = static_cast<const T *>(e.X);
    a.out = static_cast<T *>(e.out);
    a.grad = static_cast<T *>(ga.grad);
    a.grad_off = ga.grad_off;
    a.n_grad = ga.n_grad;
    a.ok = e.ok;
    a.params = static_cast<const T *>(e.params);
    a.classes = e.classes;
    a.N = e.N;
    a.ldX = e.ldX;
    a.ld_out = e.ld_out;
    a.ld_params = e.ld_params;
    a.F = a.FX = e.F;
    a.P = ga.P;
    a.n_all_trees = e.n_trees;
    a.mode = ga.mode;
    a.classes_is_i64 = e.classes_is_i64;
    a.class_base = e.class_base;
    a.n_classes = e.n_classes > 0 ? e.n_classes : 1;
    a.uses_params = e.uses_params ? 1 : 0;
    a.check = 1;
    a.skip_flagged = e.skip_flagged ? 1 : 0;
    a.diff_g0 = -1;
    if (ga.loss) {
        a.loss_mode = 1 + ga.loss->kind;
        a.loss_param = (T)ga.loss->param;
        a.loss_floor = (T)ga.loss->e_floor;
        a.y = static_cast<const T *>(ga.loss->y);
        a.w = static_cast<const T *>(ga.loss->w);
        a.partial = static_cast<T *>(ga.loss->partial);
        a.col_off = ga.col_off;
    }
    return a;
}

// Plans and starts one gradient launch: a.n_trees trees x a.n_tiles sample tiles x `windows` gradient windows (grid.y) of `kern`, the
// host stub of a kernel that takes (GArgs<T>, handler base, parameter handler offset) — the tape kernel: the first of them —, with
// `lds` bytes of dynamic LDS.  prio_keys != null: the launch has priority tiles (de_kernels.hip de_tile_extremes_kernel) of
// prio_tile_samples samples each; prio_cached: grad_flag_protocol (de_plan.h).
template <typename T>
static hipError_t launch_grad_kernel(const void *kern, GArgs<T> a, int windows, size_t lds, const void *prio_keys, int prio_tile_samples,
                                     bool prio_cached, uint64_t handler_base, uint32_t param_off, hipStream_t stream) {
    grad_chunk_plan(a.n_trees, a.n_tiles, windows, cu_count(), &a.trees_per_chunk, &a.n_chunks);
    if (a.skip_flagged) a.skip_flagged = grad_flag_protocol(a.trees_per_chunk, prio_cached, env_int("DE_SKIP_PROTOCOL", 0));
    const int64_t blocks = ((a.n_tiles + 7) / 8) * 8 * a.n_chunks;
    if (blocks <= 0 || blocks > 0x7fffffffLL || windows > 65535) return hipErrorInvalidValue;
    if (lds > 64 * 1024) {
        if (lds > 160 * 1024) return hipErrorInvalidValue;
        const hipError_t st = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (st != hipSuccess) return st;
    }
    if (a.skip_flagged && prio_keys) { // the priority tiles as a launch of their own in front, in short chunks (de_kernels.hip launch_threaded_t: no blind first wave)
        GArgs<T> pa = a;
        pa.prio = static_cast<const unsigned long long *>(prio_keys);
        pa.n_prio = (uint32_t)(3 * a.FX);
        while ((64 << pa.prio_shift) < prio_tile_samples) ++pa.prio_shift;
        pa.trees_per_chunk = 4;
        pa.n_chunks = (int32_t)((a.n_trees + 3) / 4);
        pa.n_prio_blocks = (uint32_t)(((int64_t)pa.n_prio * pa.n_chunks + 7) / 8 * 8);
        void *pargs[] = {&pa, &handler_base, &param_off};
        const hipError_t ps = hipLaunchKernel(kern, dim3(pa.n_prio_blocks, (unsigned)windows), dim3(GBLK), pargs, lds, stream);
        if (ps != hipSuccess) return ps;
    }
    void *args[] = {&a, &handler_base, &param_off};
    return hipLaunchKernel(kern, dim3((unsigned)blocks, (unsigned)windows), dim3(GBLK), args, lds, stream);
}

// the tape kernel of policy A with window GC over every tree of the program; behind a fused launch, the reduction passes
template <typename A, int GC, bool GN = false, bool FIT = false>
static hipError_t launch_grad_t(const GradArgs &ga, int windows, hipStream_t stream) {
    using Elem = typename A::Elem;
    const EvalArgs &e = ga.e;
    GArgs<Elem> a = make_gargs<Elem>(ga);
    a.code = ga.generic_code;
    a.code_off = e.code_off;
    a.n_trees = e.n_trees;
    a.n_slots = e.n_slots;
    a.n_tiles = (e.N + GBLK - 1) / GBLK;
    a.check = ga.diff_direction >= 0 ? 0 : 1;
    a.diff_g0 = ga.diff_direction >= 0 ? ga.P + ga.diff_direction : -1;
    const size_t lds = grad_tape_lds_bytes(a.F, a.n_slots, GC, sizeof(typename A::V));
    const hipError_t st = launch_grad_kernel(reinterpret_cast<const void *>(&de_grad_tape_kernel<A, GC, GN, FIT>), a, windows, lds, nullptr, 0, false, 0, 0, stream);
    if constexpr (A::TREE_ENDS) {
        if (st == hipSuccess && ga.loss) return launch_loss_grad_finish(sizeof(Elem) == 4 ? DE_F32 : DE_F64, ga, a.n_tiles, stream);
    }
    return st;
}

// the window ladder: the smallest window that covers the widest gradient in one pass, else windows of 8 (grad_window, de_kernels.h);
// eval_diff: one component
template <typename A, bool GN = false, bool FIT = false> static hipError_t launch_grad_dt(const GradArgs &ga, hipStream_t stream) {
    const int maxg = ga.diff_direction >= 0 || ga.max_grad < 1 ? 1 : ga.max_grad;
    switch (grad_window(maxg)) {
    case 1: return launch_grad_t<A, 1, GN, FIT>(ga, 1, stream);
    case 2: return launch_grad_t<A, 2, GN, FIT>(ga, 1, stream);
    case 3: return launch_grad_t<A, 3, GN, FIT>(ga, 1, stream);
    case 4: return launch_grad_t<A, 4, GN, FIT>(ga, 1, stream);
    case 5: return launch_grad_t<A, 5, GN, FIT>(ga, 1, stream);
    case 6: return launch_grad_t<A, 6, GN, FIT>(ga, 1, stream);
    default: return launch_grad_t<A, 8, GN, FIT>(ga, (maxg + 7) / 8, stream);
    }
}

} // namespace de
