// de_half.hip — the DE_F16 (IEEE binary16) value policy of the flat-switch interpreter (de_flat.h): X, constants, parameters and outputs
// are binary16, every operator step computes in Float32 registers and is rounded to binary16 before the next step reads it
// (de_half_ops.h).
//
// A lane owns 4 consecutive samples, a workgroup a 1024-sample tile.  The binary16 X tile is read once per workgroup with coalesced loads
// and written TRANSPOSED into LDS as Float32 rows (binary16 -> Float32 is exact), so a leaf read is one ds_read_b128 per lane and spill
// slots are Float32 rows like X.  Results go out as four packed binary16 values per lane (one 8-byte store).  A tested value that rounds
// to Inf (from 65520 up) is non-finite.
#include "de_flat.h"
#include "de_half_ops.h"

namespace de {

typedef float HV __attribute__((ext_vector_type(4)));
typedef _Float16 HH4 __attribute__((ext_vector_type(4)));
constexpr int HVW = 4;

// Everything but the hot operators: one noinline function (the interpreter loop keeps only wave-uniform control flow)
__device__ __noinline__ HV h16_cold(uint32_t op, HV x, HV y) {
    HV r;
#pragma unroll
    for (int i = 0; i < HVW; i++) r[i] = h16_op(op, x[i], y[i]);
    return r;
}
__device__ __noinline__ HV h16_cold3(uint32_t op, HV x, HV y, HV z) {
    HV r;
#pragma unroll
    for (int i = 0; i < HVW; i++) r[i] = h16_op3(op, x[i], y[i], z[i]);
    return r;
}
__device__ __noinline__ void h_store_ragged(_Float16 *o, HV v, int64_t remaining) {
#pragma unroll
    for (int i = 0; i < HVW; i++) if (i < remaining) o[i] = (_Float16)v[i];
}
__device__ __forceinline__ HV h_round(HV v) {
    HV r;
#pragma unroll
    for (int i = 0; i < HVW; i++) r[i] = r16(v[i]);
    return r;
}

struct HalfPolicy {
    typedef _Float16 Elem;
    typedef float Scalar;
    typedef HV V;
    static constexpr int VW = HVW, TILE = FLAT_BLK * VW, EPS = 1;
    static constexpr int ROWV = FLAT_BLK + 1; // (LDS row: 256 vectors + one of padding: bank spread)
    static constexpr size_t ROW_BYTES = FLAT_ROW_BYTES, STORE_BYTES = 8;
    static_assert(ROWV * 16 == FLAT_ROW_BYTES, "de_kernels.h FLAT_ROW_BYTES");
    static constexpr bool HAS_PARAMS = true;
    static constexpr const char *NAMES[5] = {"de_eval_half_kernel", "de_eval_half_kernel<direct>", "de_eval_half_kernel<cert>",
                                             "de_eval_half_kernel<loss>", "de_eval_half_kernel<direct,loss>"};
    typedef HV LY, LW; // (binary16 targets and weights, widened exactly)
    static constexpr bool LOSS_ALL_KINDS = false;

    // coalesced read of binary16 pairs, transposed Float32 write (sample j of row f at rows[f * ROWV * 4 + j]): de_half_ops.h
    static __device__ __forceinline__ void stage_x(const FlatArgs<_Float16> &a, unsigned char *smem, int64_t base, int tid) {
        h16_stage_x(reinterpret_cast<float *>(smem), a.X, a.ldX, (uint32_t)a.F, base, a.N, tid, TILE, ROWV * VW, FLAT_BLK);
    }
    static __device__ __forceinline__ V load_row(const unsigned char *smem, uint32_t r, int tid) { return reinterpret_cast<const V *>(smem)[(size_t)r * ROWV + tid]; }
    static __device__ __forceinline__ void store_row(unsigned char *smem, uint32_t r, int tid, V v) { reinterpret_cast<V *>(smem)[(size_t)r * ROWV + tid] = v; }
    // (binary16 from global memory; the L1 / L2 absorb the re-reads)
    static __device__ __forceinline__ V gather(const FlatArgs<_Float16> &a, uint32_t f, int64_t j0) {
        V v;
#pragma unroll
        for (int i = 0; i < VW; i++) {
            const int64_t jj = j0 + i < a.N - 1 ? j0 + i : a.N - 1;
            v[i] = (float)a.X[f + a.ldX * jj];
        }
        return v;
    }
    static __device__ __forceinline__ V zero() { return V{0.0f, 0.0f, 0.0f, 0.0f}; }
    static __device__ __forceinline__ V constant(const FlatArgs<_Float16> &, U32x4 w) { // (a binary16 value, held exactly in the Float32 immediate)
        const float c = __uint_as_float(w.z);
        return V{c, c, c, c};
    }
    static __device__ __forceinline__ V param(const FlatArgs<_Float16> &a, uint32_t idx, const int64_t (&cls)[VW]) {
        V v;
#pragma unroll
        for (int i = 0; i < VW; i++) v[i] = (float)a.params[idx + a.ld_params * cls[i]];
        return v;
    }

    static __device__ __forceinline__ V add(V x, V y) { return h_round(x + y); }
    static __device__ __forceinline__ V sub(V x, V y) { return h_round(x - y); }
    static __device__ __forceinline__ V rsub(V x, V y) { return h_round(y - x); }
    static __device__ __forceinline__ V mul(V x, V y) { return h_round(x * y); }
    static __device__ __forceinline__ V div(V x, V y) { return h_round(x / y); }
    static __device__ __forceinline__ V rdiv(V x, V y) { return h_round(y / x); }
    static __device__ __forceinline__ V cos(V x) { return h_round(V{h_cos(x[0]), h_cos(x[1]), h_cos(x[2]), h_cos(x[3])}); }
    static __device__ __forceinline__ V exp(V x) { return h_round(V{h_exp(x[0]), h_exp(x[1]), h_exp(x[2]), h_exp(x[3])}); }
    static __device__ __forceinline__ V sin(V x) { return h_round(V{h_sin(x[0]), h_sin(x[1]), h_sin(x[2]), h_sin(x[3])}); }
    static __device__ __forceinline__ V cold(uint32_t op, V x, V y) { return h16_cold(op, x, y); }
    static __device__ __forceinline__ V cold_inj(uint32_t op, V x, V y) { return cold(op, x, y); }
    static __device__ __forceinline__ V cold3(uint32_t op, V x, V y, V z) { return h16_cold3(op, x, y, z); }

    template <bool CERT> static __device__ __forceinline__ void test(float &poison, float &vmax, V v) {
#pragma unroll
        for (int i = 0; i < VW; i++) {
            poison = __builtin_fmaf(v[i], 0.0f, poison); // stays +0 while every tested value is finite, NaN from the first Inf / NaN on
            if constexpr (CERT) vmax = __builtin_fabsf(v[i]) > vmax ? __builtin_fabsf(v[i]) : vmax;
        }
    }
    static __device__ __forceinline__ V inject(V x, V r) {
#pragma unroll
        for (int i = 0; i < VW; i++) r[i] = __builtin_isfinite(x[i]) ? r[i] : __builtin_inff();
        return r;
    }
    static __device__ __forceinline__ void store_vec(_Float16 *o, V v) {
        HH4 h;
#pragma unroll
        for (int i = 0; i < VW; i++) h[i] = (_Float16)v[i]; // (exact: every value is a binary16 already)
        *reinterpret_cast<HH4 *>(o) = h;                    // four samples, one 8-byte store per lane
    }
    static __device__ __forceinline__ void store_ragged(_Float16 *o, V v, int64_t remaining) { h_store_ragged(o, v, remaining); }

    // ---- LOSS: Julia's Float16 steps per term — e = r16(yhat - y); L2 l = r16(e * e), L1 l = |e|; weighted r16(w * l).  The term is the
    // reference's, the sum is the library's: the binary16 terms are summed in Float32 (a binary16 sum of N terms overflows at 65504)
    static __device__ __forceinline__ V widen4(const _Float16 *q) {
        const HH4 h = *reinterpret_cast<const HH4 *>(q); // four samples, one 8-byte load per lane
        return V{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
    }
    static __device__ __forceinline__ V load_y(const FlatArgs<_Float16> &a, int64_t j0, bool vec) {
        if (vec) return widen4(a.y + j0);
        V v;
#pragma unroll
        for (int i = 0; i < VW; i++) v[i] = (float)a.y[j0 + i < a.N - 1 ? j0 + i : a.N - 1];
        return v;
    }
    static __device__ __forceinline__ V load_w(const FlatArgs<_Float16> &a, int64_t j0, bool vec) {
        if (a.w && vec) return widen4(a.w + j0);
        V v;
#pragma unroll
        for (int i = 0; i < VW; i++) v[i] = j0 + i < a.N ? (a.w ? (float)a.w[j0 + i < a.N - 1 ? j0 + i : a.N - 1] : 1.0f) : 0.0f;
        return v;
    }
    static __device__ __forceinline__ float loss_sum(int kind, float, V acc, V y, V w) { // (DE_LOSS_L2 / DE_LOSS_L1: launch_flat admits no other)
        const V e = h_round(acc - y);
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < VW; i++) {
            const float l = kind == (int)DE_LOSS_L1 ? __builtin_fabsf(e[i]) : r16(e[i] * e[i]);
            s += w[i] != 0.0f ? r16(w[i] * l) : 0.0f;
        }
        return s;
    }
};
static_assert(HalfPolicy::TILE == flat_tile_samples(DE_F16), "de_kernels.h flat_tile_samples");

hipError_t launch_eval_f16(const EvalArgs &e, hipStream_t stream, const char **kname) { return launch_flat<HalfPolicy>(e, nullptr, stream, kname); }

} // namespace de
