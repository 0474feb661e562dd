// de_complex.hip — gfx950 kernel of complex (DE_CF32 / DE_CF64) evaluation: X, constants and outputs are (re, im) pairs, every operator
// is Julia's Complex method (de_complex_ops.h).
//
// One flat, wave-uniform switch over the BOUND program (de_bind.h), as de_half.hip: 256 threads, a chunk of <= 63 trees per workgroup, an
// XCD-aware block map.  A lane owns CVW samples (2 for ComplexF32, 1 for ComplexF64): its value is CVW re and CVW im components in separate
// VGPRs.  The interleaved X tile is read once per workgroup with coalesced loads and written TRANSPOSED into LDS as separate re and im
// rows, so one LDS row (a feature of X or a spill slot) is 256 * CVW * 2 components = 4096 bytes for both dtypes (CROW_BYTES) and a leaf
// read is two 8-byte LDS reads per lane.  Constant operands are (re, im) pairs of the program's constant table, read with wave-uniform
// scalar loads (the immediate is the pair's index).  Results go out interleaved, 16 bytes per lane.  Flags: the per-lane NaN poison over
// both components of every tested value, one ballot per tree, the early-exit skip of trees already flagged (protocol 2).  The CERT variant
// (de_eval_sum_certificate) stores nothing and keeps the largest max(|re|, |im|) of every tree's tested values.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "de_bind.h"
#include "de_complex_ops.h"
#include "de_kernels.h"

namespace de {

typedef uint32_t CU4 __attribute__((ext_vector_type(4)));
#define DE_CCONSTANT __attribute__((address_space(4)))
typedef const DE_CCONSTANT CU4 *CCodePtr;
typedef const DE_CCONSTANT int32_t *COffPtr;

constexpr int CBLK = 256;
constexpr int CROW_BYTES = 4096;
template <typename T> struct CGeom {
    static constexpr int VW = sizeof(T) == 4 ? 2 : 1; // samples per lane
    static constexpr int TILE = CBLK * VW;            // samples per workgroup
    static constexpr int ROW = 2 * TILE;              // components per LDS row: TILE re, then TILE im
    static_assert(ROW * (int)sizeof(T) == CROW_BYTES, "one LDS row is 4096 bytes");
};

// VW samples of one lane
template <typename T> struct CV {
    T re[CGeom<T>::VW], im[CGeom<T>::VW];
};

template <typename T> struct CArgs {
    const BoundInstr *code;
    const int32_t *code_off;
    const T *X; // interleaved (re, im), [F, N] column-major in elements, ld = ldX elements
    T *out;     // interleaved, [n_trees, ld_out] in elements
    uint8_t *ok;
    const T *ctab; // (re, im) pairs: the constant table
    void *cert_max; // CERT: per tree the bits of the largest |component| of a tested value (non-negative)
    int64_t N, ldX, ld_out, n_tiles;
    int32_t F, n_trees, trees_per_chunk, n_chunks;
    int32_t vec_store, skip_flagged;
};

// blockIdx -> (sample tile, tree chunk), XCD-aware as de_kernels.hip map_block: block b runs on XCD b % 8, all chunks of one tile on one XCD
__device__ __forceinline__ bool c_map_block(uint32_t bid, int32_t n_chunks, int64_t n_tiles, int64_t *tile, int32_t *chunk) {
    if (n_tiles < 64) {
        *tile = (int64_t)(bid % (uint32_t)n_tiles);
        *chunk = (int32_t)(bid / (uint32_t)n_tiles);
        return *chunk < n_chunks;
    }
    const uint32_t xcd = bid & 7u, idx = bid >> 3;
    *chunk = (int32_t)(idx % (uint32_t)n_chunks);
    *tile = (int64_t)(idx / (uint32_t)n_chunks) * 8 + xcd;
    return *tile < n_tiles;
}

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
template <typename T> __device__ __forceinline__ CV<T> c_add3(CV<T> x, CV<T> y, CV<T> z) { // +(x, y, z) = (x + y) + z, the one ternary opcode
    CV<T> r;
#pragma unroll
    for (int i = 0; i < CGeom<T>::VW; i++) {
        r.re[i] = (x.re[i] + y.re[i]) + z.re[i];
        r.im[i] = (x.im[i] + y.im[i]) + z.im[i];
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
__device__ __noinline__ void c_flag_incomplete(uint8_t *ok, int agent) { // agent scope under protocol 1: later workgroups skip the tree
    if ((threadIdx.x & 63) == 0) {
        if (agent) __hip_atomic_store(ok, (uint8_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else *ok = 0;
    }
}

__device__ __forceinline__ float c_fma0(float v, float p) { return __builtin_fmaf(v, 0.0f, p); }
__device__ __forceinline__ double c_fma0(double v, double p) { return __builtin_fma(v, 0.0, p); }
// is_valid(z) = isfinite(re) && isfinite(im): the poison stays +0 while every tested component is finite, NaN from the first Inf / NaN on
template <typename T, bool CERT> __device__ __forceinline__ void c_test(T &poison, T &vmax, const CV<T> &v) {
#pragma unroll
    for (int i = 0; i < CGeom<T>::VW; i++) {
        poison = c_fma0(v.re[i], poison);
        poison = c_fma0(v.im[i], poison);
        if constexpr (CERT) {
            const T a = M<T>::abs(v.re[i]), b = M<T>::abs(v.im[i]);
            vmax = a > vmax ? a : vmax;
            vmax = b > vmax ? b : vmax;
        }
    }
}
// DIRECT kernels: feature f of this lane's samples from global memory (samples past N repeat the last one)
template <typename T> __device__ __forceinline__ CV<T> c_gather(const CArgs<T> &a, uint32_t f, int64_t j0) {
    CV<T> v;
#pragma unroll
    for (int i = 0; i < CGeom<T>::VW; i++) {
        const int64_t jj = j0 + i < a.N - 1 ? j0 + i : a.N - 1;
        const T *q = a.X + 2 * ((int64_t)f + a.ldX * jj);
        v.re[i] = q[0];
        v.im[i] = q[1];
    }
    return v;
}
template <typename T> __device__ __forceinline__ CV<T> c_row(const T *rows, uint32_t r, int tid) {
    using G = CGeom<T>;
    CV<T> v;
    const T *q = rows + (size_t)r * G::ROW + tid * G::VW;
#pragma unroll
    for (int i = 0; i < G::VW; i++) {
        v.re[i] = q[i];
        v.im[i] = q[G::TILE + i];
    }
    return v;
}
template <typename T> __device__ __forceinline__ void c_put_row(T *rows, uint32_t r, int tid, const CV<T> &v) {
    using G = CGeom<T>;
    T *q = rows + (size_t)r * G::ROW + tid * G::VW;
#pragma unroll
    for (int i = 0; i < G::VW; i++) {
        q[i] = v.re[i];
        q[G::TILE + i] = v.im[i];
    }
}
template <typename T> __device__ __forceinline__ CV<T> c_splat(T re, T im) {
    CV<T> v;
#pragma unroll
    for (int i = 0; i < CGeom<T>::VW; i++) {
        v.re[i] = re;
        v.im[i] = im;
    }
    return v;
}

// DIRECT: a feature matrix too wide for the LDS tile (de_api_program.cpp make_threaded) — feature operands are gathered from global
// memory and LDS holds the spill-slot rows only
template <typename T, bool EE, bool CERT, bool DIRECT>
__global__ void __launch_bounds__(CBLK) de_eval_complex_kernel(const CArgs<T> a) {
    using G = CGeom<T>;
    extern __shared__ __align__(16) unsigned char smem_cplx[];
    T *__restrict__ rows = reinterpret_cast<T *>(smem_cplx); // rows 0..F-1: the X tile; F + s: spill slot s (DIRECT: slot s at row s)
    int64_t tile;
    int32_t chunk;
    if (!c_map_block(blockIdx.x, a.n_chunks, a.n_tiles, &tile, &chunk)) return;
    const int tid = threadIdx.x;
    const int64_t base = tile * G::TILE;
    const int64_t last = a.N - 1;

    // ---- stage the X tile: coalesced reads of the interleaved pairs, transposed writes (sample j of feature f: re at rows[f * ROW + j],
    // im at rows[f * ROW + TILE + j])
    if (!DIRECT) {
        const uint32_t F = (uint32_t)a.F;
        const uint32_t total = (uint32_t)G::TILE * F;
        if (a.ldX == (int64_t)F && base + G::TILE <= a.N) {
            const T *__restrict__ src = a.X + 2 * base * (int64_t)F; // contiguous TILE * F pairs
            for (uint32_t e = tid; e < total; e += CBLK) {
                const uint32_t j = e / F, f = e - j * F;
                rows[f * G::ROW + j] = src[2 * e];
                rows[f * G::ROW + G::TILE + j] = src[2 * e + 1];
            }
        } else { // ragged tail / strided X: samples past N repeat the last one
            for (uint32_t e = tid; e < total; e += CBLK) {
                const uint32_t j = e / F, f = e - j * F;
                int64_t jj = base + j;
                jj = jj < last ? jj : last;
                const T *q = a.X + 2 * ((int64_t)f + a.ldX * jj);
                rows[f * G::ROW + j] = q[0];
                rows[f * G::ROW + G::TILE + j] = q[1];
            }
        }
    }
    __syncthreads();

    const CCodePtr code = (CCodePtr)(uintptr_t)a.code;
    const COffPtr code_off = (COffPtr)(uintptr_t)a.code_off;
    const DE_CCONSTANT T *ctab = (const DE_CCONSTANT T *)(uintptr_t)a.ctab; // (wave-uniform index: scalar loads)
    const int t0 = chunk * a.trees_per_chunk;
    const int t1 = (t0 + a.trees_per_chunk < a.n_trees) ? t0 + a.trees_per_chunk : a.n_trees;
    const bool full = base + G::TILE <= a.N;
    uint64_t skip = 0ull; // trees of the chunk already known to be incomplete: not evaluated (early exit at tree granularity)
    if (EE && a.skip_flagged && t1 - t0 <= 64) {
        const int i = t0 + (tid & 63);
        const uint8_t f = i >= t1 ? (uint8_t)1 : skip_flag_load(a.ok + i, a.skip_flagged, tile);
        skip = __ballot(f == 0);
    }

    int pe = code_off[t0];
    for (int tree = t0; tree < t1; ++tree) {
        int pc = pe;
        pe = code_off[tree + 1];
        if ((skip >> (tree - t0)) & 1ull) continue;
        CV<T> acc = c_splat<T>(T(0), T(0));
        T poison = T(0), vmax = T(0);
        CU4 nxt = code[pc];
        for (; pc < pe; ++pc) {
            const CU4 w = nxt;
            nxt = code[pc + 1]; // (the code buffer carries one trailing pad instruction)
// CSLOT(r): a slot row; CROW(r): a feature row of the X tile or a slot row; CCONST: the operand's pair of the constant table
#define CSLOT_IDX(r) ((r) - (DIRECT ? (uint32_t)a.F : 0u))
#define CROW(r) (DIRECT && (r) < (uint32_t)a.F ? c_gather<T>(a, (r), base + tid * G::VW) : c_row<T>(rows, CSLOT_IDX(r), tid))
#define CCONST (c_splat<T>(ctab[2 * (size_t)w.z], ctab[2 * (size_t)w.z + 1]))
#define CBIN_HOT(K, EXPR)                                                                                                        \
    case BOP_BIN_BASE + 4 * K + 0: { const CV<T> y = CROW(w.y); EXPR; } break;                                                   \
    case BOP_BIN_BASE + 4 * K + 1: { const CV<T> y = CROW(w.y); EXPR; c_test<T, CERT>(poison, vmax, acc); } break;              \
    case BOP_BIN_BASE + 4 * K + 2: { const CV<T> y = CCONST; EXPR; } break;                                                      \
    case BOP_BIN_BASE + 4 * K + 3: { const CV<T> y = CCONST; EXPR; c_test<T, CERT>(poison, vmax, acc); } break;
#define CADD for (int i = 0; i < G::VW; i++) { acc.re[i] = acc.re[i] + y.re[i]; acc.im[i] = acc.im[i] + y.im[i]; }
#define CSUB for (int i = 0; i < G::VW; i++) { acc.re[i] = acc.re[i] - y.re[i]; acc.im[i] = acc.im[i] - y.im[i]; }
#define CRSUB for (int i = 0; i < G::VW; i++) { acc.re[i] = y.re[i] - acc.re[i]; acc.im[i] = y.im[i] - acc.im[i]; }
#define CMUL for (int i = 0; i < G::VW; i++) { const Cx<T> r = c_mul(Cx<T>{acc.re[i], acc.im[i]}, Cx<T>{y.re[i], y.im[i]}); acc.re[i] = r.re; acc.im[i] = r.im; }
#define CUN(K, OP)                                                                                                               \
    case BOP_UN_BASE + 4 * K + 0: acc = c_cold<T>(OP, acc, acc); break;                                                          \
    case BOP_UN_BASE + 4 * K + 1: acc = c_cold<T>(OP, acc, acc); c_test<T, CERT>(poison, vmax, acc); break;                     \
    case BOP_UN_BASE + 4 * K + 2: { const CV<T> x = CROW(w.y); acc = c_cold<T>(OP, x, x); } break;                              \
    case BOP_UN_BASE + 4 * K + 3: { const CV<T> x = CROW(w.y); acc = c_cold<T>(OP, x, x); c_test<T, CERT>(poison, vmax, acc); } break;
            switch (w.x) {
            case BOP_LOAD_ROW: acc = CROW(w.y); break;
            case BOP_LOAD_CONST: acc = CCONST; break;
            case BOP_PUSH: c_put_row<T>(rows, CSLOT_IDX(w.y), tid, acc); break;
            case BOP_CHECK_ROW: c_test<T, CERT>(poison, vmax, CROW(w.y)); break;
            case BOP_CHECK_ACC: c_test<T, CERT>(poison, vmax, acc); break;
            CBIN_HOT(0, CADD)
            CBIN_HOT(1, CSUB)
            CBIN_HOT(2, CRSUB)
            CBIN_HOT(3, CMUL)
            CBIN_HOT(4, acc = c_cold<T>(DE_B_DIV, acc, y))
            CBIN_HOT(5, acc = c_cold<T>(DOP_RDIV, acc, y))
            CUN(0, DE_U_COS)
            CUN(1, DE_U_EXP)
            CUN(2, DE_U_SIN)
            case BOP_GEN_ROW: { const uint32_t op = w.y >> 24; const CV<T> b = CROW(w.y & 0xFFFFFFu); acc = c_cold<T>(op, op < 64u ? b : acc, b); } break;
            case BOP_GEN_CONST: { const uint32_t op = w.y >> 24; const CV<T> b = CCONST; acc = c_cold<T>(op, op < 64u ? b : acc, b); } break;
            case BOP_GEN_ACC: acc = c_cold<T>(w.y >> 24, acc, acc); break;
            case BOP_TERN: acc = c_add3<T>(CROW(w.y & 0xFFFFFFu), CROW(w.z), acc); break; // (DE_T_ADD3: the lowering admits no other)
            // is_valid(x_l) ? op(x_l) : Inf + 0im   (src/Evaluate.jl:722,787): the fused kernels, early_exit = false
            case BOP_INJ_ACC: {
                const CV<T> x = acc, r = c_cold<T>(w.y >> 24, acc, x);
                for (int i = 0; i < G::VW; i++) {
                    const bool v = __builtin_isfinite(x.re[i]) && __builtin_isfinite(x.im[i]);
                    acc.re[i] = v ? r.re[i] : M<T>::inf();
                    acc.im[i] = v ? r.im[i] : T(0);
                }
            } break;
            case BOP_INJ_ROW: {
                const uint32_t op = w.y >> 24;
                const CV<T> x = CROW(w.y & 0xFFFFFFu), r = c_cold<T>(op, op < 64u ? x : acc, x);
                for (int i = 0; i < G::VW; i++) {
                    const bool v = __builtin_isfinite(x.re[i]) && __builtin_isfinite(x.im[i]);
                    acc.re[i] = v ? r.re[i] : M<T>::inf();
                    acc.im[i] = v ? r.im[i] : T(0);
                }
            } break;
            default: break; // (BOP_GEN_PARAM: complex programs have no parameters)
            }
#undef CSLOT_IDX
#undef CROW
#undef CCONST
#undef CBIN_HOT
#undef CADD
#undef CSUB
#undef CRSUB
#undef CMUL
#undef CUN
        }
        if constexpr (CERT) {
            // the tree's largest |component|: wave maximum, one atomicMax per wave on the bits (non-negative floats order as unsigned)
            for (int m = 32; m >= 1; m >>= 1) {
                const T o2 = __shfl_xor(vmax, m, 64);
                vmax = o2 > vmax ? o2 : vmax;
            }
            if ((tid & 63) == 0 && vmax > T(0)) {
                if constexpr (sizeof(T) == 4) atomicMax(reinterpret_cast<unsigned int *>(a.cert_max) + tree, __float_as_uint((float)vmax));
                else atomicMax(reinterpret_cast<unsigned long long *>(a.cert_max) + tree, (unsigned long long)__double_as_longlong((double)vmax));
            }
        } else {
            T *__restrict__ o = a.out + 2 * ((int64_t)tree * a.ld_out + base + tid * G::VW);
            if (full && a.vec_store) {
                // this lane's samples, interleaved: one 16-byte store
                if constexpr (sizeof(T) == 4) {
                    typedef float F4 __attribute__((ext_vector_type(4)));
                    *reinterpret_cast<F4 *>(o) = F4{(float)acc.re[0], (float)acc.im[0], (float)acc.re[G::VW - 1], (float)acc.im[G::VW - 1]};
                } else {
                    typedef double D2 __attribute__((ext_vector_type(2)));
                    *reinterpret_cast<D2 *>(o) = D2{(double)acc.re[0], (double)acc.im[0]};
                }
            } else {
                c_store_ragged<T>(o, acc, a.N - (base + tid * G::VW));
            }
        }
        if (__ballot(poison != poison) != 0ull) c_flag_incomplete(a.ok + tree, a.skip_flagged == 1);
    }
}

static int c_cu_count() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) cus = n;
        else cus = 256; // MI355X
    }
    return cus;
}

// Chunks of <= 63 trees (the skip mask is one 64-bit ballot), more of them while the grid would not cover the chip 32 workgroups per CU,
// never fewer than 8 trees per chunk (de_half.hip h_plan, the same rule)
static void c_plan(int64_t n, int64_t n_tiles, int32_t *n_chunks_out, int32_t *tpc_out) {
    const int64_t want = (int64_t)c_cu_count() * 4 * 8;
    int64_t n_chunks = (n + 62) / 63;
    if (n_tiles > 0 && n_tiles * n_chunks < want) n_chunks = (want + n_tiles - 1) / n_tiles;
    const int64_t max_chunks = (n + 7) / 8;
    if (n_chunks > max_chunks) n_chunks = max_chunks;
    if (n_chunks < 1) n_chunks = 1;
    const int64_t tpc = n > 0 ? (n + n_chunks - 1) / n_chunks : 1;
    *tpc_out = (int32_t)tpc;
    *n_chunks_out = (int32_t)(n > 0 ? (n + tpc - 1) / tpc : 1);
}

static int c_tile(int io) { return io == DE_CF32 ? CGeom<float>::TILE : CGeom<double>::TILE; }

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

void eval_plan_complex(int io, int64_t n_trees, int64_t N, int32_t *tile, int32_t *n_chunks, int32_t *trees_per_chunk) {
    *tile = c_tile(io);
    c_plan(n_trees, (N + *tile - 1) / *tile, n_chunks, trees_per_chunk);
}

template <typename T> static hipError_t launch_t(const EvalArgs &e, const void *ctab, hipStream_t stream, const char **kname) {
    using G = CGeom<T>;
    CArgs<T> a;
    a.code = e.code;
    a.code_off = e.code_off;
    a.X = static_cast<const T *>(e.X);
    a.out = static_cast<T *>(e.out);
    a.ok = e.ok;
    a.ctab = static_cast<const T *>(ctab);
    a.cert_max = e.cert_max;
    a.N = e.N;
    a.ldX = e.ldX;
    a.ld_out = e.ld_out;
    a.n_tiles = (e.N + G::TILE - 1) / G::TILE;
    a.F = e.F;
    a.n_trees = e.n_trees;
    a.vec_store = (reinterpret_cast<uintptr_t>(e.out) % 16 == 0 && (e.ld_out * 2 * (int64_t)sizeof(T)) % 16 == 0) ? 1 : 0;
    c_plan(e.n_trees, a.n_tiles, &a.n_chunks, &a.trees_per_chunk);
    a.skip_flagged = (e.early_exit && e.skip_flagged && a.trees_per_chunk <= 64) ? 2 : 0; // (protocol 2: de_device_ops.h skip_flag_load)
    const int64_t blocks = (a.n_tiles < 64 ? a.n_tiles : (a.n_tiles + 7) / 8 * 8) * a.n_chunks;
    if (blocks <= 0 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    void (*kern)(const CArgs<T>);
    size_t lds;
    if (e.cert_max) {
        if (!e.early_exit || e.direct) return hipErrorInvalidValue;
        kern = de_eval_complex_kernel<T, true, true, false>;
    } else if (e.direct) kern = e.early_exit ? de_eval_complex_kernel<T, true, false, true> : de_eval_complex_kernel<T, false, false, true>;
    else kern = e.early_exit ? de_eval_complex_kernel<T, true, false, false> : de_eval_complex_kernel<T, false, false, false>;
    if (e.direct) lds = (size_t)(e.n_slots > 0 ? e.n_slots : 1) * CROW_BYTES;
    else lds = (size_t)(e.F + e.n_slots) * CROW_BYTES;
    if (kname) *kname = e.cert_max ? "de_eval_complex_kernel<cert>" : e.direct ? "de_eval_complex_kernel<direct>" : "de_eval_complex_kernel";
    if (lds > 64 * 1024) {
        const hipError_t st = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (st != hipSuccess) return st;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(CBLK), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_eval_complex(int io, const EvalArgs &e, const void *ctab, hipStream_t stream, const char **kname) {
    if (e.threaded || e.loss || e.uses_params || !ctab) return hipErrorInvalidValue; // (the host refuses these first)
    if (e.ok_init) { // the constant part of the flags, then the launch only clears bytes
        const hipError_t cs = hipMemcpyAsync(e.ok, e.ok_init, (size_t)e.n_trees, hipMemcpyDeviceToDevice, stream);
        if (cs != hipSuccess) return cs;
    }
    if (io == DE_CF32) return launch_t<float>(e, ctab, stream, kname);
    if (io == DE_CF64) return launch_t<double>(e, ctab, stream, kname);
    return hipErrorInvalidValue;
}

} // namespace de
