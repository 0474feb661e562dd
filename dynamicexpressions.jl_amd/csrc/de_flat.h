// de_flat.h — the flat-switch interpreter: ONE kernel template over a value policy, and its launch.
//
// Serves everything the direct-threaded kernel (de_kernels.hip) does not: Float32 / Float64 with a feature matrix too wide for its
// LDS tile, the certificate pass and DE_EVAL_THREADED=0 (de_flat_real.hip), DE_F16 (de_half.hip), DE_CF32 / DE_CF64 (de_complex.hip).
//
// The skeleton below owns the interpreting: 256 threads, P::VW consecutive samples per lane, a chunk of <= 63 trees per workgroup, the
// XCD-aware block map, one wave-uniform switch over the BOUND program (de_bind.h) whose records come through the scalar cache (the next
// one requested before the current case runs), which operand a case reads and when a value is validity-tested, the per-lane NaN poison
// with one ballot per tree, the protocol-2 skip of trees already flagged, the DIRECT variant (feature operands gathered from global
// memory, LDS holds the spill rows only) and the CERT variant (de_eval_sum_certificate: nothing stored, the largest |tested value| of
// every tree).  It never asks which policy it serves.
//
// A value policy P says what a value is and how to compute with it — and holds no control flow of the interpreter:
//   Elem, Scalar, V        element of X / out / params in memory; type of the poison and of the CERT maximum; a lane's value (by value
//                          through the __noinline__ cold functions)
//   VW, TILE, EPS          samples per lane, per workgroup (256 * VW), memory elements per sample
//   ROW_BYTES, STORE_BYTES one LDS row (a feature of the X tile, a spill slot, a staged parameter row); the lane's vector store
//   HAS_PARAMS, NAMES      whether PARAMS = true is ever instantiated; the kernel names reported {plain, <direct>, <cert>}
//   stage_x                the workgroup's X tile into LDS rows 0 .. F-1
//   load_row / store_row   this lane's value of an LDS row;  gather: of feature f from global memory (DIRECT)
//   zero, constant, param  the initial accumulator; a record's constant operand; parameter `idx` of this lane's classes
//   add sub rsub mul div rdiv (acc, y) / cos exp sin (x)      the hot operators
//   cold (op, x, y), cold3 (op, x, y, z)                      every other opcode: x = the operand of a unary operator, (x, y) of a binary
//   test<CERT>, inject     poison (and the running maximum) over a tested value; is_valid(x) ? r : Inf
//   store_vec / store_ragged                                  a full tile's aligned store; the ragged tail's
#pragma once
#include <hip/hip_runtime.h>

#include "de_bind.h"
#include "de_device_ops.h"
#include "de_kernels.h"
#include "de_plan.h"

namespace de {

constexpr int FLAT_BLK = 256;

template <typename E> struct FlatArgs {
    const BoundInstr *code;  // bound program, padded with one trailing instruction (the prefetch reads pc + 1)
    const int32_t *code_off; // n_trees + 1
    const E *X;
    E *out;
    uint8_t *ok;
    const E *params;
    const void *classes;
    const void *ctab;     // policies whose constant operands are table indices (complex)
    void *cert_max;       // CERT: per tree the bits of the largest |tested value| (a non-negative Scalar in an unsigned word)
    int64_t N, ldX, ld_out, ld_params, n_tiles, n_classes;
    int32_t F, n_trees, trees_per_chunk, n_chunks;
    int32_t prow_base, n_prows; // parameters staged as LDS rows (EvalArgs)
    int32_t classes_is_i64, class_base, vec_store, skip_flagged;
};

__device__ __noinline__ void flag_incomplete(uint8_t *ok, int agent) { // agent scope under protocol 1: workgroups that start later skip the tree
    if ((threadIdx.x & 63) == 0) {
        if (agent) __hip_atomic_store(ok, (uint8_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else *ok = 0;
    }
}
// (non-negative floats order like unsigned integers)
__device__ __forceinline__ void cert_atomic_max(void *words, int tree, float v) { atomicMax(static_cast<unsigned int *>(words) + tree, __float_as_uint(v)); }
__device__ __forceinline__ void cert_atomic_max(void *words, int tree, double v) {
    atomicMax(static_cast<unsigned long long *>(words) + tree, (unsigned long long)__double_as_longlong(v));
}

template <class P, bool EE, bool PARAMS, bool DIRECT, bool CERT>
__global__ void __launch_bounds__(FLAT_BLK) de_eval_flat_kernel(const FlatArgs<typename P::Elem> a) {
    typedef typename P::V V;
    typedef typename P::Scalar S;
    typedef typename P::Elem E;
    constexpr int VW = P::VW;
    static_assert(P::TILE == FLAT_BLK * VW, "a lane owns VW consecutive samples of the tile");
    extern __shared__ __align__(16) unsigned char smem[]; // rows 0..F-1: the X tile; F + s: row s behind it (DIRECT: row s alone)

    const TileMap tm = map_block(blockIdx.x, a.n_chunks, a.n_tiles);
    if (!tm.valid) return;
    const int tid = threadIdx.x;
    const int64_t base = tm.tile * P::TILE;
    const int64_t j0 = base + tid * VW; // this lane's first sample
    const int64_t last = a.N - 1;

    if (!DIRECT) P::stage_x(a, smem, base, tid);
    int64_t cls[VW]; // (PARAMS) the classes of this lane's samples; samples past N repeat the last one
    if constexpr (PARAMS) {
#pragma unroll
        for (int i = 0; i < VW; i++) {
            const int64_t jj = j0 + i < last ? j0 + i : last;
            cls[i] = clamp_class((a.classes_is_i64 ? reinterpret_cast<const int64_t *>(a.classes)[jj]
                                                   : (int64_t) reinterpret_cast<const int32_t *>(a.classes)[jj]) - a.class_base, a.n_classes);
        }
        // parameters as rows: row prow_base + p holds params[p, class of the sample] (src/ParametricExpression.jl:381-389), every lane its own samples
        if (!DIRECT)
            for (int p = 0; p < a.n_prows; p++) P::store_row(smem, (uint32_t)(a.prow_base + p), tid, P::param(a, (uint32_t)p, cls));
    }
    __syncthreads();

    const ConstU4Ptr code = (ConstU4Ptr)(uintptr_t)a.code;
    const ConstI32Ptr code_off = (ConstI32Ptr)(uintptr_t)a.code_off;
    const int t0 = tm.chunk * a.trees_per_chunk;
    const int t1 = (t0 + a.trees_per_chunk < a.n_trees) ? t0 + a.trees_per_chunk : a.n_trees;
    const bool full = base + P::TILE <= a.N;
    uint64_t skip = 0ull; // trees of the chunk already known to be incomplete: not evaluated (early exit at tree granularity)
    if (EE && a.skip_flagged && t1 - t0 <= 64) {
        const int i = t0 + (tid & 63);
        const uint8_t f = i >= t1 ? (uint8_t)1 : skip_flag_load(a.ok + i, a.skip_flagged, tm.tile);
        skip = __ballot(f == 0);
    }

    int pe = code_off[t0];
    for (int tree = t0; tree < t1; ++tree) {
        int pc = pe;
        pe = code_off[tree + 1];
        if ((skip >> (tree - t0)) & 1ull) continue;
        V acc = P::zero();
        S poison = S(0);
        S vmax = S(0); // (CERT) largest |tested value| of this lane's samples
        U32x4 nxt = code[pc]; // scalar load; a tree has at least one instruction
        for (; pc < pe; ++pc) {
            const U32x4 w = nxt;
            nxt = code[pc + 1]; // prefetch (the code buffer carries one trailing pad instruction)
            // One flat, wave-uniform switch over the bound handler id (de_bind.h): every case is straight-line code.
            // SLOT(r): the LDS index of row r >= F;  ROW(r): this lane's value of row r (a feature of X, a spill slot, a staged parameter row)
#define SLOT(r) ((r) - (DIRECT ? (uint32_t)a.F : 0u))
#define ROW(r) (DIRECT && (r) < (uint32_t)a.F ? P::gather(a, (r), j0) : P::load_row(smem, SLOT(r), tid))
#define TEST(v) P::template test<CERT>(poison, vmax, (v))
#define BIN4(K, OP)                                                                                  \
    case BOP_BIN_BASE + 4 * K + 0: acc = P::OP(acc, ROW(w.y)); break;                                \
    case BOP_BIN_BASE + 4 * K + 1: acc = P::OP(acc, ROW(w.y)); TEST(acc); break;                     \
    case BOP_BIN_BASE + 4 * K + 2: acc = P::OP(acc, P::constant(a, w)); break;                       \
    case BOP_BIN_BASE + 4 * K + 3: acc = P::OP(acc, P::constant(a, w)); TEST(acc); break;
#define UN4(K, OP)                                                                                   \
    case BOP_UN_BASE + 4 * K + 0: acc = P::OP(acc); break;                                           \
    case BOP_UN_BASE + 4 * K + 1: acc = P::OP(acc); TEST(acc); break;                                \
    case BOP_UN_BASE + 4 * K + 2: acc = P::OP(ROW(w.y)); break;                                      \
    case BOP_UN_BASE + 4 * K + 3: acc = P::OP(ROW(w.y)); TEST(acc); break;
// a generic operator with operand b: a unary one (opcodes below 64) maps b, a binary one combines the accumulator with it
#define GEN(op, b) P::cold((op), (op) < 64u ? (b) : acc, (b))
            switch (w.x) {
            case BOP_LOAD_ROW: acc = ROW(w.y); break;
            case BOP_LOAD_CONST: acc = P::constant(a, w); break;
            case BOP_PUSH: P::store_row(smem, SLOT(w.y), tid, acc); break;
            case BOP_CHECK_ROW: TEST(ROW(w.y)); break;
            case BOP_CHECK_ACC: TEST(acc); break;
            BIN4(0, add)
            BIN4(1, sub)
            BIN4(2, rsub)
            BIN4(3, mul)
            BIN4(4, div)
            BIN4(5, rdiv)
            UN4(0, cos)
            UN4(1, exp)
            UN4(2, sin)
            case BOP_GEN_ROW: { const uint32_t op = w.y >> 24; const V b = ROW(w.y & 0xFFFFFFu); acc = GEN(op, b); } break;
            case BOP_GEN_CONST: { const uint32_t op = w.y >> 24; const V b = P::constant(a, w); acc = GEN(op, b); } break;
            case BOP_GEN_ACC: acc = P::cold(w.y >> 24, acc, acc); break;
            case BOP_TERN: acc = P::cold3(w.y >> 24, ROW(w.y & 0xFFFFFFu), ROW(w.z), acc); break; // op3(slot, slot, acc)
            // is_valid(x_l) ? op(x_l) : Inf   (src/Evaluate.jl:722,787): the fused kernels, early_exit = false — x_l is the operand (the
            // accumulator or a row); a binary operator combines the accumulator with it, as the generic cases do
            // (P::cold_inj: cold, but cos / sin of a real Float32 program are the functions of BOP_UN — the bits of the threaded kernel's b_gen<INJ>)
            case BOP_INJ_ACC: { const V x = acc; acc = P::inject(x, P::cold_inj(w.y >> 24, acc, x)); } break;
            case BOP_INJ_ROW: { const uint32_t op = w.y >> 24; const V x = ROW(w.y & 0xFFFFFFu); acc = P::inject(x, P::cold_inj(op, op < 64u ? x : acc, x)); } break;
            case BOP_GEN_PARAM:
                if constexpr (PARAMS) {
                    const uint32_t op = w.y >> 24;
                    const V b = P::param(a, w.y & 0xFFFFu, cls);
                    if (EE && (w.y & (1u << 23))) TEST(b);
                    if (op == DOP_LOAD) acc = b;
                    else acc = GEN(op, b);
                }
                break;
            default: break;
            }
#undef SLOT
#undef ROW
#undef TEST
#undef BIN4
#undef UN4
#undef GEN
        }
        if constexpr (CERT) {
            // the tree's largest |tested value|: wave maximum, one atomicMax per wave on the value's bits; samples past N repeat the
            // last real one, so they add nothing
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const S o2 = __shfl_xor(vmax, m, 64);
                vmax = o2 > vmax ? o2 : vmax;
            }
            if ((tid & 63) == 0 && vmax > S(0)) cert_atomic_max(a.cert_max, tree, vmax);
        } else {
            E *__restrict__ o = a.out + P::EPS * ((int64_t)tree * a.ld_out + j0);
            if (full && a.vec_store) P::store_vec(o, acc);
            else P::store_ragged(o, acc, a.N - j0);
        }
        // ---- completion flag: one ballot per wave, one byte store per failing wave
        if (__ballot(poison != poison) != 0ull) flag_incomplete(a.ok + tree, a.skip_flagged == 1);
    }
}

// ---- launch -----------------------------------------------------------------------------------------------------------------------
// The kernels that exist: (EE, PARAMS, DIRECT) and, for the certificate pass, (EE = true, PARAMS, CERT) without the gather
template <class P, bool PARAMS> static auto flat_kernel(bool ee, bool direct, bool cert) -> void (*)(const FlatArgs<typename P::Elem>) {
    if (cert) return de_eval_flat_kernel<P, true, PARAMS, false, true>;
    if (direct) return ee ? de_eval_flat_kernel<P, true, PARAMS, true, false> : de_eval_flat_kernel<P, false, PARAMS, true, false>;
    return ee ? de_eval_flat_kernel<P, true, PARAMS, false, false> : de_eval_flat_kernel<P, false, PARAMS, false, false>;
}

// ctab: the program's device constant table, for the policies that read one
template <class P> static hipError_t launch_flat(const EvalArgs &e, const void *ctab, hipStream_t stream, const char **kname) {
    typedef typename P::Elem E;
    if (e.loss || (e.uses_params && !P::HAS_PARAMS)) return hipErrorInvalidValue; // (the host refuses these first)
    if (e.cert_max && (!e.early_exit || e.direct)) return hipErrorInvalidValue;   // (the certificate pass: early-exit flag semantics, no gather)
    if (e.ok_init) { // the constant part of the flags, then the launch only clears bytes
        const hipError_t cs = hipMemcpyAsync(e.ok, e.ok_init, (size_t)e.n_trees, hipMemcpyDeviceToDevice, stream);
        if (cs != hipSuccess) return cs;
    }
    FlatArgs<E> a;
    a.code = e.code;
    a.code_off = e.code_off;
    a.X = static_cast<const E *>(e.X);
    a.out = static_cast<E *>(e.out);
    a.ok = e.ok;
    a.params = static_cast<const E *>(e.params);
    a.classes = e.classes;
    a.ctab = ctab;
    a.cert_max = e.cert_max;
    a.N = e.N;
    a.ldX = e.ldX;
    a.ld_out = e.ld_out;
    a.ld_params = e.ld_params;
    a.n_tiles = (e.N + P::TILE - 1) / P::TILE;
    a.n_classes = e.n_classes > 0 ? e.n_classes : 1;
    a.F = e.F;
    a.n_trees = e.n_trees;
    a.prow_base = e.prow_base;
    a.n_prows = e.n_prows;
    a.classes_is_i64 = e.classes_is_i64;
    a.class_base = e.class_base;
    a.vec_store = (reinterpret_cast<uintptr_t>(e.out) % P::STORE_BYTES == 0 && (e.ld_out * P::EPS * (int64_t)sizeof(E)) % P::STORE_BYTES == 0) ? 1 : 0;
    plan_chunks(e.n_trees, a.n_tiles, &a.n_chunks, &a.trees_per_chunk);
    a.skip_flagged = (e.early_exit && e.skip_flagged && a.trees_per_chunk <= 64) ? 2 : 0; // (protocol 2: de_device_ops.h skip_flag_load)
    // (map_block: from 64 tiles on a block's XCD picks its tile, and the workgroups past the last tile return)
    const int64_t blocks = (a.n_tiles < 64 ? a.n_tiles : (a.n_tiles + 7) / 8 * 8) * a.n_chunks;
    if (blocks <= 0 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    void (*kern)(const FlatArgs<E>) = flat_kernel<P, false>(e.early_exit, e.direct, e.cert_max != nullptr);
    if constexpr (P::HAS_PARAMS) {
        if (e.uses_params) kern = flat_kernel<P, true>(e.early_exit, e.direct, e.cert_max != nullptr);
    }
    // (DIRECT: no staged parameter rows either — a program gathers its features only when the rows would not fit)
    const size_t lds = (size_t)(e.direct ? (e.n_slots > 0 ? e.n_slots : 1) : e.F + e.n_slots) * P::ROW_BYTES;
    if (kname) *kname = P::NAMES[e.cert_max ? 2 : e.direct ? 1 : 0];
    if (lds > 64 * 1024) {
        const hipError_t st = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (st != hipSuccess) return st;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(FLAT_BLK), lds, stream, a);
    return hipGetLastError();
}

} // namespace de
