// de_half_grad.hip — forward-mode gradients of DE_F16 (IEEE binary16) programs created with DE_OPT_F16_GRAD: de_eval_grad in its three
// modes and de_eval_diff.  Julia's Float16 arithmetic through eval_grad_tree_array / grad_degn_eval / eval_diff_tree_array
// (src/EvaluateDerivative.jl), as the reference's test/test_derivatives.jl runs it for Float16.
//
// The same forward-dual interpreter over the generic bound stream as de_grad_kernels.hip's de_grad_tape_kernel: one sample per lane, a
// 256-sample tile per workgroup, windows of at most 8 gradient components (blockIdx.y), the same seeds, row order and eval_diff path.
// What differs is the arithmetic: every value and every partial is a binary16 value held in a Float32 register, and every operation of
// the value table (de_half_ops.h), of the partials and of the chain rule (de_half_grad_ops.h) is rounded to binary16 before the next one
// reads it.  X, the constants, the parameters, out and grad are binary16 in global memory; the X tile is staged once per workgroup into
// LDS as Float32 rows (binary16 -> Float32 is exact), as de_half.hip does, and spill rows are Float32 like them.  A value or partial that
// rounds to Inf (from 65520 up) is non-finite.
#include "de_grad_common.h"
#include "de_half_grad_ops.h"

namespace de {

// Everything but the hot operators: noinline functions (the interpreter loop keeps only wave-uniform control flow)
__device__ __noinline__ HUG hg_unary(uint32_t op, float x) { return h16_unary_vg(op, x); }
__device__ __noinline__ HBG hg_binary(uint32_t op, float x, float y) { return h16_binary_vg(op, x, y); }
__device__ __noinline__ HTG hg_ternary(uint32_t op, float x, float y, float z) { return h16_ternary_vg(op, x, y, z); }

constexpr int HG_RS = GBLK + 4; // LDS row stride (Float32 elements)

// The binary16 X tile, read once per workgroup with coalesced loads: aligned pairs where the tile is contiguous and its first element
// 4-byte aligned, single elements where the pointer is 2 mod 4, and the clamped path for a ragged or strided tile (de_half.hip stage_x)
__device__ __forceinline__ void hg_stage_x(float *__restrict__ rows, const _Float16 *__restrict__ X, int64_t ldX, uint32_t F, int64_t base, int64_t N, int tid) {
    const uint32_t total = (uint32_t)GBLK * F;
    if (ldX == (int64_t)F && base + GBLK <= N) {
        const _Float16 *__restrict__ src = X + base * (int64_t)F; // contiguous GBLK * F elements (an even count)
        if ((reinterpret_cast<uintptr_t>(src) & 3u) == 0) {
            const uint32_t *__restrict__ s2 = reinterpret_cast<const uint32_t *>(src);
            for (uint32_t e2 = tid; e2 < total / 2; e2 += GBLK) {
                const uint32_t w = s2[e2];
                _Float16 h[2];
                __builtin_memcpy(h, &w, 4);
                DE_UNROLL for (int k = 0; k < 2; k++) {
                    const uint32_t e = 2 * e2 + k, j = e / F, f = e - j * F;
                    rows[f * HG_RS + j] = (float)h[k];
                }
            }
        } else {
            for (uint32_t e = tid; e < total; e += GBLK) {
                const uint32_t j = e / F, f = e - j * F;
                rows[f * HG_RS + j] = (float)src[e];
            }
        }
    } else { // ragged tail / strided X: samples past N repeat the last one
        const int64_t last = N - 1;
        for (uint32_t e = tid; e < total; e += GBLK) {
            const uint32_t j = e / F, f = e - j * F;
            int64_t jj = base + j;
            jj = jj < last ? jj : last;
            rows[f * HG_RS + j] = (float)X[f + ldX * jj];
        }
    }
}

template <int GC>
__global__ void __launch_bounds__(GBLK) de_grad_half_kernel(const GArgs<_Float16> a) {
    constexpr int RS = HG_RS;
    extern __shared__ __align__(16) unsigned char hgsmem[];
    float *__restrict__ rows = reinterpret_cast<float *>(hgsmem);

    const TileMap tm = map_block(blockIdx.x, a.n_chunks, a.n_tiles);
    if (!tm.valid) return;
    const int tid = threadIdx.x;
    const int64_t base = tm.tile * GBLK;
    const int64_t last = a.N - 1;
    const int g0 = a.diff_g0 >= 0 ? a.diff_g0 : (int)blockIdx.y * GC; // first gradient component of this window
    const int F = a.F, P = a.P;

    hg_stage_x(rows, a.X, a.ldX, (uint32_t)F, base, a.N, tid);
    int64_t jj0 = base + tid;
    const bool live = jj0 < a.N;
    jj0 = jj0 < last ? jj0 : last;
    int64_t cls = 0;
    if (a.uses_params)
        cls = clamp_class((a.classes_is_i64 ? reinterpret_cast<const int64_t *>(a.classes)[jj0]
                                            : (int64_t) reinterpret_cast<const int32_t *>(a.classes)[jj0]) - a.class_base, a.n_classes);
    __syncthreads();

    const ConstU4Ptr code = (ConstU4Ptr)(uintptr_t)a.code;
    const ConstI32Ptr code_off = (ConstI32Ptr)(uintptr_t)a.code_off;
    const ConstI32Ptr n_grad = (ConstI32Ptr)(uintptr_t)a.n_grad;
    const ConstI64Ptr grad_off = (ConstI64Ptr)(uintptr_t)a.grad_off;
    const int t0 = tm.chunk * a.trees_per_chunk;
    const int t1 = (t0 + a.trees_per_chunk < a.n_trees) ? t0 + a.trees_per_chunk : a.n_trees;
    float *__restrict__ stk = rows + (size_t)F * RS;

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
        float x = 0.0f, d[GC];
        DE_UNROLL for (int k = 0; k < GC; k++) d[k] = 0.0f;
        float poison = 0.0f;
        U32x4 nxt = code[pc];
        for (; pc < pe; ++pc) {
            const U32x4 w = nxt;
            nxt = code[pc + 1];
            // One flat wave-uniform switch over the bound handler id (de_bind.h); the operand is a LEAF row (< F: one-hot seed), a spill
            // ROW (>= F: a popped dual number) or a constant (seed).  Seeds are materialised 0 / 1: Inf * 0 = NaN as in the reference.
#define HG_SLOT(r) (stk + ((r) - (uint32_t)F) * (1 + GC) * RS + tid)
#define HG_ROW_OPERAND(r)                                                                          \
    float xb, db[GC];                                                                              \
    if ((r) < (uint32_t)F) {                                                                       \
        xb = rows[(r) * RS + tid];                                                                 \
        const int seed = (int)(r) + feat_seed0;                                                    \
        if (a.check) poison = __builtin_fmaf(xb, 0.0f, poison);                                    \
        DE_UNROLL for (int k = 0; k < GC; k++) db[k] = (k == seed) ? 1.0f : 0.0f;                  \
    } else {                                                                                       \
        const float *__restrict__ s_ = HG_SLOT(r);                                                 \
        xb = s_[0];                                                                                \
        DE_UNROLL for (int k = 0; k < GC; k++) db[k] = s_[(1 + k) * RS];                           \
    }
#define HG_CONST_OPERAND()                                                                         \
    const float xb = __uint_as_float(w.z); /* a binary16 value, held exactly in the Float32 immediate */ \
    float db[GC];                                                                                  \
    { const int seed = (int)(w.y & 0xFFFFu) + const_seed0;                                         \
      DE_UNROLL for (int k = 0; k < GC; k++) db[k] = (k == seed) ? 1.0f : 0.0f; }
#define HG_CHK() if (a.check) poison = __builtin_fmaf(x, 0.0f, poison);
            // binary hot ops: value v and partials (gl, gr) w.r.t. (left, right); REV: left = operand.  1 * d and -1 * d are exact.
#define HG_BIN_APPLY(K)                                                                            \
    {                                                                                              \
        constexpr bool REV = (K == 2 || K == 5);                                                   \
        const float lx = REV ? xb : x, ly = REV ? x : xb;                                          \
        if (K == 0) { x = hadd(lx, ly); DE_UNROLL for (int k = 0; k < GC; k++) d[k] = hadd(d[k], db[k]); } \
        else if (K == 1) { x = hsub(lx, ly); DE_UNROLL for (int k = 0; k < GC; k++) d[k] = hadd(d[k], -db[k]); } \
        else if (K == 2) { x = hsub(lx, ly); DE_UNROLL for (int k = 0; k < GC; k++) d[k] = hadd(db[k], -d[k]); } \
        else {                                                                                     \
            float gl, gr;                                                                          \
            if (K == 3) { x = hmul(lx, ly); gl = ly; gr = lx; }                                    \
            else { x = hdiv(lx, ly); gl = hdiv(1.0f, ly); gr = -hdiv(x, ly); }                     \
            if (REV) { DE_UNROLL for (int k = 0; k < GC; k++) d[k] = hchain2(gl, db[k], gr, d[k]); } \
            else { DE_UNROLL for (int k = 0; k < GC; k++) d[k] = hchain2(gl, d[k], gr, db[k]); }   \
        }                                                                                          \
    }
#define HG_BIN4(K)                                                                                 \
    case BOP_BIN_BASE + 4 * K + 0: { HG_ROW_OPERAND(w.y) HG_BIN_APPLY(K) } break;                  \
    case BOP_BIN_BASE + 4 * K + 1: { HG_ROW_OPERAND(w.y) HG_BIN_APPLY(K) HG_CHK() } break;         \
    case BOP_BIN_BASE + 4 * K + 2: { HG_CONST_OPERAND() HG_BIN_APPLY(K) } break;                   \
    case BOP_BIN_BASE + 4 * K + 3: { HG_CONST_OPERAND() HG_BIN_APPLY(K) HG_CHK() } break;
            // unary hot ops (K: 0 cos, 1 exp, 2 sin) on xin with incoming gradient din[]: the partial is the value table's own step
#define HG_UN_APPLY(K, XIN, DIN)                                                                   \
    {                                                                                              \
        const float xin_ = (XIN);                                                                  \
        float y_, g_;                                                                              \
        if (K == 1) { y_ = r16(h_exp(xin_)); g_ = y_; }                                            \
        else if (K == 0) { y_ = r16(h_cos(xin_)); g_ = -r16(h_sin(xin_)); }                        \
        else { y_ = r16(h_sin(xin_)); g_ = r16(h_cos(xin_)); }                                     \
        x = y_;                                                                                    \
        DE_UNROLL for (int k = 0; k < GC; k++) d[k] = hmul(g_, DIN[k]);                            \
    }
#define HG_UN4(K)                                                                                  \
    case BOP_UN_BASE + 4 * K + 0: HG_UN_APPLY(K, x, d) break;                                      \
    case BOP_UN_BASE + 4 * K + 1: HG_UN_APPLY(K, x, d) HG_CHK() break;                             \
    case BOP_UN_BASE + 4 * K + 2: { HG_ROW_OPERAND(w.y) HG_UN_APPLY(K, xb, db) } break;            \
    case BOP_UN_BASE + 4 * K + 3: { HG_ROW_OPERAND(w.y) HG_UN_APPLY(K, xb, db) HG_CHK() } break;
            // generic (cold) operators through the noinline value+partials functions
#define HG_GEN_APPLY(OP, SRC_IS_ACC)                                                               \
    {                                                                                              \
        const uint32_t gop_ = (OP);                                                                \
        if (gop_ < DE_B_ADD) {                                                                     \
            const HUG r = hg_unary(gop_, SRC_IS_ACC ? x : xb);                                     \
            x = r.y;                                                                               \
            if (SRC_IS_ACC) { DE_UNROLL for (int k = 0; k < GC; k++) d[k] = hmul(r.g, d[k]); }     \
            else { DE_UNROLL for (int k = 0; k < GC; k++) d[k] = hmul(r.g, db[k]); }               \
        } else {                                                                                   \
            uint32_t fop = gop_;                                                                   \
            bool rev = false;                                                                      \
            switch (gop_) {                                                                        \
            case DOP_RSUB: fop = DE_B_SUB; rev = true; break;                                      \
            case DOP_RDIV: fop = DE_B_DIV; rev = true; break;                                      \
            case DOP_RPOW: fop = DE_B_POW; rev = true; break;                                      \
            case DOP_RMOD: fop = DE_B_MOD; rev = true; break;                                      \
            case DOP_RREM: fop = DE_B_REM; rev = true; break;                                      \
            case DOP_RGREATER: fop = DE_B_GREATER; rev = true; break;                              \
            case DOP_RPOW_ABS2: fop = DE_B_POW_ABS2; rev = true; break;                            \
            case DOP_RMAX: fop = DE_B_MAX; rev = true; break;                                      \
            case DOP_RMIN: fop = DE_B_MIN; rev = true; break;                                      \
            default: break;                                                                        \
            }                                                                                      \
            const HBG r = rev ? hg_binary(fop, xb, x) : hg_binary(fop, x, xb);                     \
            x = r.v;                                                                               \
            if (rev) { DE_UNROLL for (int k = 0; k < GC; k++) d[k] = hchain2(r.gx, db[k], r.gy, d[k]); } \
            else { DE_UNROLL for (int k = 0; k < GC; k++) d[k] = hchain2(r.gx, d[k], r.gy, db[k]); } \
        }                                                                                          \
    }
            switch (w.x) {
            case BOP_LOAD_ROW: { HG_ROW_OPERAND(w.y) x = xb; DE_UNROLL for (int k = 0; k < GC; k++) d[k] = db[k]; } break;
            case BOP_LOAD_CONST: { HG_CONST_OPERAND() x = xb; DE_UNROLL for (int k = 0; k < GC; k++) d[k] = db[k]; } break;
            case BOP_PUSH: {
                float *__restrict__ s_ = HG_SLOT(w.y);
                s_[0] = x;
                DE_UNROLL for (int k = 0; k < GC; k++) s_[(1 + k) * RS] = d[k];
            } break;
            case BOP_CHECK_ROW: break; // every leaf operand is tested where it is read (HG_ROW_OPERAND)
            case BOP_CHECK_ACC: HG_CHK() break;
            HG_BIN4(0) HG_BIN4(1) HG_BIN4(2) HG_BIN4(3) HG_BIN4(4) HG_BIN4(5)
            HG_UN4(0) HG_UN4(1) HG_UN4(2)
            case BOP_GEN_ROW: { HG_ROW_OPERAND(w.y & 0xFFFFFFu) HG_GEN_APPLY(w.y >> 24, false) } break;
            case BOP_GEN_CONST: { HG_CONST_OPERAND() HG_GEN_APPLY(w.y >> 24, false) } break;
            case BOP_GEN_ACC: { const float xb = x; float db[GC]; DE_UNROLL for (int k = 0; k < GC; k++) db[k] = d[k]; HG_GEN_APPLY(w.y >> 24, true) } break;
            case BOP_GEN_PARAM: {
                const uint32_t prow = w.y & 0xFFFFu, op_ = w.y >> 24;
                const float xb = (float)a.params[prow + a.ld_params * cls];
                if (a.check) poison = __builtin_fmaf(xb, 0.0f, poison);
                float db[GC];
                { const int seed = (int)prow + param_seed0; DE_UNROLL for (int k = 0; k < GC; k++) db[k] = (k == seed) ? 1.0f : 0.0f; }
                if (op_ == DOP_LOAD) { x = xb; DE_UNROLL for (int k = 0; k < GC; k++) d[k] = db[k]; }
                else HG_GEN_APPLY(op_, false)
            } break;
            case BOP_TERN: { // acc = op3(row B, row C, acc)
                const float *__restrict__ sb = HG_SLOT(w.y & 0xFFFFFFu);
                const float *__restrict__ sc = HG_SLOT(w.z);
                const HTG r = hg_ternary(w.y >> 24, sb[0], sc[0], x);
                x = r.v;
                DE_UNROLL for (int k = 0; k < GC; k++) d[k] = hchain3(r.g0, sb[(1 + k) * RS], r.g1, sc[(1 + k) * RS], r.g2, d[k]);
            } break;
            default: break;
            }
        }
        // a non-finite d[k] always survives to the root (every update is linear in it), so the gradient is validity-tested once,
        // here; x was tested where the lowering kept a test
        if (a.check) {
            poison = __builtin_fmaf(x, 0.0f, poison);
            DE_UNROLL for (int k = 0; k < GC; k++) poison = __builtin_fmaf(g0 + k < G ? d[k] : 0.0f, 0.0f, poison); // real rows only
        }
        if (live) { // (exact conversions: every value is a binary16 already)
            if (a.diff_g0 >= 0) {
                if (a.out) a.out[(int64_t)tree * a.ld_out + base + tid] = (_Float16)x;
                a.grad[(int64_t)tree * a.ld_out + base + tid] = (_Float16)d[0];
            } else {
                if (a.out && g0 == 0) a.out[(int64_t)tree * a.ld_out + base + tid] = (_Float16)x;
                _Float16 *__restrict__ gp = a.grad + grad_off[tree] + (int64_t)G * (base + tid) + g0;
                DE_UNROLL for (int k = 0; k < GC; k++)
                    if (g0 + k < G) gp[k] = (_Float16)d[k];
            }
        }
        if (a.check && __ballot(poison != poison) != 0ull) gflag_incomplete(a.ok + tree, a.skip_flagged == 1);
    }
}

template <int GC> static hipError_t launch_grad_half_t(const GradArgs &ga, int windows, hipStream_t stream) {
    const EvalArgs &e = ga.e;
    GArgs<_Float16> a = {};
    a.code = ga.generic_code;
    a.code_off = e.code_off;
    a.X = static_cast<const _Float16 *>(e.X);
    a.out = static_cast<_Float16 *>(e.out);
    a.grad = static_cast<_Float16 *>(ga.grad);
    a.grad_off = ga.grad_off;
    a.n_grad = ga.n_grad;
    a.ok = e.ok;
    a.params = static_cast<const _Float16 *>(e.params);
    a.classes = e.classes;
    a.N = e.N;
    a.ldX = e.ldX;
    a.ld_out = e.ld_out;
    a.ld_params = e.ld_params;
    a.F = a.FX = e.F;
    a.P = ga.P;
    a.n_trees = a.n_all_trees = e.n_trees;
    a.n_slots = e.n_slots;
    a.n_tiles = (e.N + GBLK - 1) / GBLK;
    a.mode = ga.mode;
    a.classes_is_i64 = e.classes_is_i64;
    a.class_base = e.class_base;
    a.n_classes = e.n_classes > 0 ? e.n_classes : 1;
    a.uses_params = e.uses_params ? 1 : 0;
    a.check = ga.diff_direction >= 0 ? 0 : 1;
    a.skip_flagged = e.skip_flagged ? 1 : 0;
    a.diff_g0 = ga.diff_direction >= 0 ? ga.P + ga.diff_direction : -1;
    grad_chunk_plan(a.n_trees, a.n_tiles, windows, cu_count(), &a.trees_per_chunk, &a.n_chunks);
    if (a.skip_flagged) a.skip_flagged = grad_flag_protocol(a.trees_per_chunk, false, env_int("DE_SKIP_PROTOCOL", 0));
    const int64_t blocks = ((a.n_tiles + 7) / 8) * 8 * a.n_chunks;
    if (blocks <= 0 || blocks > 0x7fffffffLL || windows > 65535) return hipErrorInvalidValue;
    const size_t lds = grad_f16_lds_bytes(a.F, a.n_slots, GC);
    const void *kern = reinterpret_cast<const void *>(&de_grad_half_kernel<GC>);
    if (lds > 64 * 1024) {
        if (lds > 160 * 1024) return hipErrorInvalidValue;
        const hipError_t st = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (st != hipSuccess) return st;
    }
    void *args[] = {&a};
    return hipLaunchKernel(kern, dim3((unsigned)blocks, (unsigned)windows), dim3(GBLK), args, lds, stream);
}
static_assert(HG_RS * sizeof(float) == GRAD_F16_ROW_BYTES, "de_kernels.h GRAD_F16_ROW_BYTES");

hipError_t launch_grad_f16(const GradArgs &a, hipStream_t stream, const char **kernel_name) {
    if (kernel_name) *kernel_name = "de_grad_half_kernel";
    if (a.loss || a.gn || a.fit) return hipErrorInvalidValue; // (binary16 programs have no fused losses)
    if (a.diff_direction >= 0) return launch_grad_half_t<1>(a, 1, stream);
    const int maxg = a.max_grad < 1 ? 1 : a.max_grad;
    // smallest window that covers the widest gradient in one pass, else windows of 8 (de_grad_kernels.hip launch_grad_dt)
    if (maxg <= 1) return launch_grad_half_t<1>(a, 1, stream);
    if (maxg <= 2) return launch_grad_half_t<2>(a, 1, stream);
    if (maxg <= 3) return launch_grad_half_t<3>(a, 1, stream);
    if (maxg <= 4) return launch_grad_half_t<4>(a, 1, stream);
    if (maxg <= 5) return launch_grad_half_t<5>(a, 1, stream);
    if (maxg <= 6) return launch_grad_half_t<6>(a, 1, stream);
    return launch_grad_half_t<8>(a, (maxg + 7) / 8, stream);
}

} // namespace de
