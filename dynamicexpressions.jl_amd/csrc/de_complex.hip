// de_complex.hip — the complex (DE_CF32 / DE_CF64) value policy of the flat-switch interpreter (de_flat.h): X, constants and outputs are
// (re, im) pairs, every operator is Julia's Complex method (de_complex_ops.h).
//
// A lane owns VW samples (2 for ComplexF32, 1 for ComplexF64): its value is VW re and VW im components in separate VGPRs.  The interleaved
// X tile is read once per workgroup with coalesced loads and written TRANSPOSED into LDS as separate re and im rows, so one LDS row (a
// feature of X or a spill slot) is 256 * VW * 2 components = 4096 bytes for both dtypes (CROW_BYTES) and a leaf read is two 8-byte LDS
// reads per lane.  Constant operands are (re, im) pairs of the program's constant table, read with wave-uniform scalar loads (the
// immediate is the pair's index).  Results go out interleaved, 16 bytes per lane.  A value is valid when both components are finite; the
// certificate keeps the largest max(|re|, |im|).  Complex programs have no parameters.
#include "de_flat.h"
#include "de_complex_ops.h"

namespace de {

constexpr int CROW_BYTES = 4096;
template <typename T> struct CGeom {
    static constexpr int VW = sizeof(T) == 4 ? 2 : 1; // samples per lane
    static constexpr int TILE = FLAT_BLK * VW;        // samples per workgroup
    static constexpr int ROW = 2 * TILE;              // components per LDS row: TILE re, then TILE im
    static_assert(ROW * (int)sizeof(T) == CROW_BYTES, "one LDS row is 4096 bytes");
};

// VW samples of one lane
template <typename T> struct CV {
    T re[CGeom<T>::VW], im[CGeom<T>::VW];
};

// Everything but + - * : one noinline function (the interpreter loop keeps only wave-uniform control flow)
template <typename T> __device__ __noinline__ CV<T> c_cold(uint32_t op, CV<T> x, CV<T> y) {
    CV<T> r;
#pragma unroll
    for (int i = 0; i < CGeom<T>::VW; i++) {
        const Cx<T> v = c_op<T>(op, Cx<T>{x.re[i], x.im[i]}, Cx<T>{y.re[i], y.im[i]});
        r.re[i] = v.re;
        r.im[i] = v.im;
    }
    return r;
}
template <typename T> __device__ __noinline__ void c_store_ragged(T *o, CV<T> v, int64_t remaining) {
#pragma unroll
    for (int i = 0; i < CGeom<T>::VW; i++)
        if (i < remaining) {
            o[2 * i] = v.re[i];
            o[2 * i + 1] = v.im[i];
        }
}
__device__ __forceinline__ float c_fma0(float v, float p) { return __builtin_fmaf(v, 0.0f, p); }
__device__ __forceinline__ double c_fma0(double v, double p) { return __builtin_fma(v, 0.0, p); }
// |e| of a loss term (LOSS launches): OCML's hypot — de_complex_ops.h forms no modulus of its own (its sqrt and log go through c_ssqs);
// a loss term claims no bit parity with a CPU library
__device__ __forceinline__ float c_hypot(float x, float y) { return ::hypotf(x, y); }
__device__ __forceinline__ double c_hypot(double x, double y) { return ::hypot(x, y); }

template <typename T> struct ComplexPolicy {
    using G = CGeom<T>;
    typedef T Elem;   // a component: a sample is EPS = 2 of them, interleaved
    typedef T Scalar;
    typedef CV<T> V;
    static constexpr int VW = G::VW, TILE = G::TILE, EPS = 2;
    static constexpr size_t ROW_BYTES = CROW_BYTES, STORE_BYTES = 16;
    static constexpr bool HAS_PARAMS = false;
    static constexpr const char *NAMES[5] = {"de_eval_complex_kernel", "de_eval_complex_kernel<direct>", "de_eval_complex_kernel<cert>",
                                             "de_eval_complex_kernel<loss>", "de_eval_complex_kernel<direct,loss>"};
    typedef CV<T> LY;                 // complex targets, interleaved in memory
    struct LW { T v[G::VW]; };        // REAL weights
    static constexpr bool LOSS_ALL_KINDS = false;

    // coalesced reads of the interleaved pairs, transposed writes (sample j of feature f: re at rows[f * ROW + j], im at rows[f * ROW + TILE + j])
    static __device__ __forceinline__ void stage_x(const FlatArgs<T> &a, unsigned char *smem, int64_t base, int tid) {
        T *__restrict__ rows = reinterpret_cast<T *>(smem);
        const uint32_t F = (uint32_t)a.F;
        const uint32_t total = (uint32_t)TILE * F;
        if (a.ldX == (int64_t)F && base + TILE <= a.N) {
            const T *__restrict__ src = a.X + 2 * base * (int64_t)F; // contiguous TILE * F pairs
            for (uint32_t e = tid; e < total; e += FLAT_BLK) {
                const uint32_t j = e / F, f = e - j * F;
                rows[f * G::ROW + j] = src[2 * e];
                rows[f * G::ROW + TILE + j] = src[2 * e + 1];
            }
        } else { // ragged tail / strided X: samples past N repeat the last one
            const int64_t last = a.N - 1;
            for (uint32_t e = tid; e < total; e += FLAT_BLK) {
                const uint32_t j = e / F, f = e - j * F;
                int64_t jj = base + j;
                jj = jj < last ? jj : last;
                const T *q = a.X + 2 * ((int64_t)f + a.ldX * jj);
                rows[f * G::ROW + j] = q[0];
                rows[f * G::ROW + TILE + j] = q[1];
            }
        }
    }
    static __device__ __forceinline__ V load_row(const unsigned char *smem, uint32_t r, int tid) {
        V v;
        const T *q = reinterpret_cast<const T *>(smem) + (size_t)r * G::ROW + tid * VW;
#pragma unroll
        for (int i = 0; i < VW; i++) {
            v.re[i] = q[i];
            v.im[i] = q[TILE + i];
        }
        return v;
    }
    static __device__ __forceinline__ void store_row(unsigned char *smem, uint32_t r, int tid, const V &v) {
        T *q = reinterpret_cast<T *>(smem) + (size_t)r * G::ROW + tid * VW;
#pragma unroll
        for (int i = 0; i < VW; i++) {
            q[i] = v.re[i];
            q[TILE + i] = v.im[i];
        }
    }
    static __device__ __forceinline__ V gather(const FlatArgs<T> &a, uint32_t f, int64_t j0) {
        V v;
#pragma unroll
        for (int i = 0; i < VW; i++) {
            const int64_t jj = j0 + i < a.N - 1 ? j0 + i : a.N - 1;
            const T *q = a.X + 2 * ((int64_t)f + a.ldX * jj);
            v.re[i] = q[0];
            v.im[i] = q[1];
        }
        return v;
    }
    static __device__ __forceinline__ V splat(T re, T im) {
        V v;
#pragma unroll
        for (int i = 0; i < VW; i++) {
            v.re[i] = re;
            v.im[i] = im;
        }
        return v;
    }
    static __device__ __forceinline__ V zero() { return splat(T(0), T(0)); }
    static __device__ __forceinline__ V constant(const FlatArgs<T> &a, U32x4 w) { // the pair w.z of the constant table (wave-uniform index: scalar loads)
        const DE_CONSTANT T *ctab = (const DE_CONSTANT T *)(uintptr_t)a.ctab;
        return splat(ctab[2 * (size_t)w.z], ctab[2 * (size_t)w.z + 1]);
    }

    static __device__ __forceinline__ V add(V x, const V &y) {
#pragma unroll
        for (int i = 0; i < VW; i++) { x.re[i] = x.re[i] + y.re[i]; x.im[i] = x.im[i] + y.im[i]; }
        return x;
    }
    static __device__ __forceinline__ V sub(V x, const V &y) {
#pragma unroll
        for (int i = 0; i < VW; i++) { x.re[i] = x.re[i] - y.re[i]; x.im[i] = x.im[i] - y.im[i]; }
        return x;
    }
    static __device__ __forceinline__ V rsub(V x, const V &y) {
#pragma unroll
        for (int i = 0; i < VW; i++) { x.re[i] = y.re[i] - x.re[i]; x.im[i] = y.im[i] - x.im[i]; }
        return x;
    }
    static __device__ __forceinline__ V mul(V x, const V &y) {
#pragma unroll
        for (int i = 0; i < VW; i++) {
            const Cx<T> r = c_mul(Cx<T>{x.re[i], x.im[i]}, Cx<T>{y.re[i], y.im[i]});
            x.re[i] = r.re;
            x.im[i] = r.im;
        }
        return x;
    }
    static __device__ __forceinline__ V div(const V &x, const V &y) { return c_cold<T>(DE_B_DIV, x, y); }
    static __device__ __forceinline__ V rdiv(const V &x, const V &y) { return c_cold<T>(DOP_RDIV, x, y); }
    static __device__ __forceinline__ V cos(const V &x) { return c_cold<T>(DE_U_COS, x, x); }
    static __device__ __forceinline__ V exp(const V &x) { return c_cold<T>(DE_U_EXP, x, x); }
    static __device__ __forceinline__ V sin(const V &x) { return c_cold<T>(DE_U_SIN, x, x); }
    static __device__ __forceinline__ V cold(uint32_t op, const V &x, const V &y) { return c_cold<T>(op, x, y); }
    static __device__ __forceinline__ V cold_inj(uint32_t op, const V &x, const V &y) { return cold(op, x, y); }
    static __device__ __forceinline__ V cold3(uint32_t, V x, const V &y, const V &z) { // +(x, y, z) = (x + y) + z: DE_T_ADD3, the lowering admits no other
#pragma unroll
        for (int i = 0; i < VW; i++) {
            x.re[i] = (x.re[i] + y.re[i]) + z.re[i];
            x.im[i] = (x.im[i] + y.im[i]) + z.im[i];
        }
        return x;
    }

    // is_valid(z) = isfinite(re) && isfinite(im): the poison stays +0 while every tested component is finite, NaN from the first Inf / NaN on
    template <bool CERT> static __device__ __forceinline__ void test(T &poison, T &vmax, const V &v) {
#pragma unroll
        for (int i = 0; i < VW; i++) {
            poison = c_fma0(v.re[i], poison);
            poison = c_fma0(v.im[i], poison);
            if constexpr (CERT) {
                const T a = M<T>::abs(v.re[i]), b = M<T>::abs(v.im[i]);
                vmax = a > vmax ? a : vmax;
                vmax = b > vmax ? b : vmax;
            }
        }
    }
    static __device__ __forceinline__ V inject(const V &x, V r) { // is_valid(x) ? r : Inf + 0im
#pragma unroll
        for (int i = 0; i < VW; i++) {
            const bool v = __builtin_isfinite(x.re[i]) && __builtin_isfinite(x.im[i]);
            r.re[i] = v ? r.re[i] : M<T>::inf();
            r.im[i] = v ? r.im[i] : T(0);
        }
        return r;
    }
    static __device__ __forceinline__ void store_vec(T *o, const V &v) { // this lane's samples, interleaved: one 16-byte store
        typedef T Q __attribute__((ext_vector_type(16 / sizeof(T))));
        Q q;
#pragma unroll
        for (int i = 0; i < VW; i++) {
            q[2 * i] = v.re[i];
            q[2 * i + 1] = v.im[i];
        }
        *reinterpret_cast<Q *>(o) = q;
    }
    static __device__ __forceinline__ void store_ragged(T *o, const V &v, int64_t remaining) { c_store_ragged<T>(o, v, remaining); }

    // ---- LOSS: e = yhat - y per component in T; L2 l = abs2(e) = re * re + im * im (two products, one sum; the build never contracts),
    // L1 l = abs(e) = hypot(re, im); real weights, a real sum
    static __device__ __forceinline__ LY load_y(const FlatArgs<T> &a, int64_t j0, bool vec) {
        LY v;
        if (vec) { // this lane's samples, interleaved: one 16-byte load
            typedef T Q __attribute__((ext_vector_type(16 / sizeof(T))));
            const Q q = *reinterpret_cast<const Q *>(a.y + 2 * j0);
#pragma unroll
            for (int i = 0; i < VW; i++) {
                v.re[i] = q[2 * i];
                v.im[i] = q[2 * i + 1];
            }
            return v;
        }
#pragma unroll
        for (int i = 0; i < VW; i++) {
            const T *q = a.y + 2 * (j0 + i < a.N - 1 ? j0 + i : a.N - 1);
            v.re[i] = q[0];
            v.im[i] = q[1];
        }
        return v;
    }
    static __device__ __forceinline__ LW load_w(const FlatArgs<T> &a, int64_t j0, bool vec) {
        LW v;
        if (a.w && vec) { // 8 bytes per lane
            typedef T Q __attribute__((ext_vector_type(VW)));
            const Q q = *reinterpret_cast<const Q *>(a.w + j0);
#pragma unroll
            for (int i = 0; i < VW; i++) v.v[i] = q[i];
            return v;
        }
#pragma unroll
        for (int i = 0; i < VW; i++) v.v[i] = j0 + i < a.N ? (a.w ? a.w[j0 + i < a.N - 1 ? j0 + i : a.N - 1] : T(1)) : T(0);
        return v;
    }
    static __device__ __forceinline__ T loss_sum(int kind, T, const V &acc, const LY &y, const LW &w) { // (DE_LOSS_L2 / DE_LOSS_L1: launch_flat admits no other)
        T s = T(0);
#pragma unroll
        for (int i = 0; i < VW; i++) {
            const T er = acc.re[i] - y.re[i], ei = acc.im[i] - y.im[i];
            const T l = kind == (int)DE_LOSS_L1 ? c_hypot(er, ei) : er * er + ei * ei;
            s += w.v[i] != T(0) ? w.v[i] * l : T(0);
        }
        return s;
    }
};
static_assert(ComplexPolicy<float>::TILE == flat_tile_samples(DE_CF32) && ComplexPolicy<double>::TILE == flat_tile_samples(DE_CF64), "de_kernels.h flat_tile_samples");

size_t complex_row_bytes(int) { return CROW_BYTES; }

bool complex_opcode_ok(int degree, int op) {
    if (degree == 1)
        switch (op) {
        case DE_U_NEG: case DE_U_SQUARE: case DE_U_CUBE: case DE_U_INV: case DE_U_SQRT: case DE_U_EXP: case DE_U_LOG: case DE_U_SIN:
        case DE_U_COS: case DE_U_TAN: case DE_U_SINH: case DE_U_COSH: case DE_U_TANH: case DE_U_COS2: return true;
        default: return false;
        }
    if (degree == 2) return op == DE_B_ADD || op == DE_B_SUB || op == DE_B_MUL || op == DE_B_DIV;
    return degree == 3 && op == DE_T_ADD3;
}

hipError_t launch_eval_complex(int io, const EvalArgs &e, const void *ctab, hipStream_t stream, const char **kname) {
    if (!ctab) return hipErrorInvalidValue;
    if (io == DE_CF32) return launch_flat<ComplexPolicy<float>>(e, ctab, stream, kname);
    if (io == DE_CF64) return launch_flat<ComplexPolicy<double>>(e, ctab, stream, kname);
    return hipErrorInvalidValue;
}

} // namespace de
