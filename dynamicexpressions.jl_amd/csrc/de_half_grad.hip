// de_half_grad.hip — forward-mode gradients of DE_F16 (IEEE binary16) programs created with DE_OPT_F16_GRAD: de_eval_grad in its three
// modes and de_eval_diff.  Julia's Float16 arithmetic through eval_grad_tree_array / grad_degn_eval / eval_diff_tree_array
// (src/EvaluateDerivative.jl), as the reference's test/test_derivatives.jl runs it for Float16.
//
// The binary16 arithmetic policy of the forward-dual tape interpreter (de_grad_tape.h: tile, windows, seeds, row order, eval_diff path and
// launch are the Float32 / Float64 kernel's, de_grad_kernels.hip).  Every value and every partial is a binary16 value held in a Float32
// register, and every operation of the value table (de_half_ops.h), of the partials and of the chain rule (de_half_grad_ops.h) is rounded
// to binary16 before the next one reads it.  X, the constants, the parameters, out and grad are binary16 in global memory; the X tile is
// staged once per workgroup into LDS as Float32 rows (binary16 -> Float32 is exact), as de_half.hip does, and spill rows are Float32 like
// them.  A value or partial that rounds to Inf (from 65520 up) is non-finite.  Binary16 programs have no fused losses: no tree ends.
#include "de_grad_tape.h"
#include "de_half_grad_ops.h"

namespace de {

// Everything but the hot operators: noinline functions (the interpreter loop keeps only wave-uniform control flow)
__device__ __noinline__ HUG hg_unary(uint32_t op, float x) { return h16_unary_vg(op, x); }
__device__ __noinline__ HBG hg_binary(uint32_t op, float x, float y) { return h16_binary_vg(op, x, y); }
__device__ __noinline__ HTG hg_ternary(uint32_t op, float x, float y, float z) { return h16_ternary_vg(op, x, y, z); }

struct HalfGrad {
    typedef _Float16 Elem;
    typedef float V;
    static constexpr bool TREE_ENDS = false;
    static constexpr const char *NAMES[1] = {"de_grad_half_kernel"};

    static __device__ __forceinline__ void stage_x(float *rows, const _Float16 *X, int64_t ldX, uint32_t F, int64_t base, int64_t N, int tid) {
        h16_stage_x(rows, X, ldX, F, base, N, tid, GBLK, GRAD_TAPE_ROW, GBLK);
    }
    static __device__ __forceinline__ float imm(U32x4 w) { return __uint_as_float(w.z); } // a binary16 value, held exactly in the Float32 immediate

    template <int K> static __device__ __forceinline__ HBG bin(float lx, float ly) {
        HBG r;
        if (K == 0) { r.v = hadd(lx, ly); r.gx = 1.0f; r.gy = 1.0f; }
        else if (K == 1 || K == 2) { r.v = hsub(lx, ly); r.gx = 1.0f; r.gy = -1.0f; }
        else if (K == 3) { r.v = hmul(lx, ly); r.gx = ly; r.gy = lx; }
        else { r.v = hdiv(lx, ly); r.gx = hdiv(1.0f, ly); r.gy = -hdiv(r.v, ly); }
        return r;
    }
    // 1 * d and -1 * d are exact: sums and differences take no product step
    template <int K> static __device__ __forceinline__ float bin_dual(float gl, float dl, float gr, float dr) {
        return K == 0 ? hadd(dl, dr) : (K <= 2 ? hadd(dl, -dr) : hchain2(gl, dl, gr, dr));
    }
    // the partial is the value table's own step
    template <int K> static __device__ __forceinline__ HUG un(float xin) {
        HUG r;
        if (K == 1) { r.y = r16(h_exp(xin)); r.g = r.y; }
        else if (K == 0) { r.y = r16(h_cos(xin)); r.g = -r16(h_sin(xin)); }
        else { r.y = r16(h_sin(xin)); r.g = r16(h_cos(xin)); }
        return r;
    }
    static __device__ __forceinline__ float scale(float g, float d) { return hmul(g, d); }
    static __device__ __forceinline__ float chain2(float g1, float d1, float g2, float d2) { return hchain2(g1, d1, g2, d2); }
    static __device__ __forceinline__ float chain3(float g0, float a, float g1, float b, float g2, float c) { return hchain3(g0, a, g1, b, g2, c); }
    static __device__ __forceinline__ HUG unary(uint32_t op, float x) { return hg_unary(op, x); }
    static __device__ __forceinline__ HBG binary(uint32_t op, float x, float y) { return hg_binary(op, x, y); }
    static __device__ __forceinline__ HTG ternary(uint32_t op, float x, float y, float z) { return hg_ternary(op, x, y, z); }
};

hipError_t launch_grad_f16(const GradArgs &a, hipStream_t stream, const char **kernel_name) {
    if (kernel_name) *kernel_name = HalfGrad::NAMES[0];
    if (a.loss || a.gn || a.fit) return hipErrorInvalidValue; // (binary16 programs have no fused losses)
    return launch_grad_dt<HalfGrad>(a, stream);
}

} // namespace de
