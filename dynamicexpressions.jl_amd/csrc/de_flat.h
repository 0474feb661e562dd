// de_flat.h — the flat-switch interpreter: ONE kernel template over a value policy, and its launch.
//
// Serves everything the direct-threaded kernel (de_kernels.hip) does not: Float32 / Float64 with a feature matrix too wide for its
// LDS tile, the certificate pass and DE_EVAL_THREADED=0 (de_flat_real.hip), DE_F16 (de_half.hip), DE_CF32 / DE_CF64 (de_complex.hip).
//
// The skeleton below owns the interpreting: 256 threads, P::VW consecutive samples per lane, a chunk of <= 63 trees per workgroup, the
// XCD-aware block map, one wave-uniform switch over the BOUND program (de_bind.h) whose records come through the scalar cache (the next
// one requested before the current case runs), which operand a case reads and when a value is validity-tested, the per-lane NaN poison
// with one ballot per tree, the protocol-2 skip of trees already flagged, the DIRECT variant (feature operands gathered from global
// memory, LDS holds the spill rows only), the CERT variant (de_eval_sum_certificate: nothing stored, the largest |tested value| of
// every tree) and the LOSS variant (de_eval_loss: nothing stored, one partial sum of loss terms per (tile, tree, wave); DESIGN.md
// §4.4.17).  It never asks which policy it serves.
//
// A value policy P says what a value is and how to compute with it — and holds no control flow of the interpreter:
//   Elem, Scalar, V        element of X / out / params in memory; type of the poison and of the CERT maximum; a lane's value (by value
//                          through the __noinline__ cold functions)
//   VW, TILE, EPS          samples per lane, per workgroup (256 * VW), memory elements per sample
//   ROW_BYTES, STORE_BYTES one LDS row (a feature of the X tile, a spill slot, a staged parameter row); the lane's vector store
//   HAS_PARAMS, NAMES      whether PARAMS = true is ever instantiated; the kernel names reported {plain, <direct>, <cert>, <loss>,
//                          <direct,loss>}
//   stage_x                the workgroup's X tile into LDS rows 0 .. F-1
//   load_row / store_row   this lane's value of an LDS row;  gather: of feature f from global memory (DIRECT)
//   zero, constant, param  the initial accumulator; a record's constant operand; parameter `idx` of this lane's classes
//   add sub rsub mul div rdiv (acc, y) / cos exp sin (x)      the hot operators
//   cold (op, x, y), cold3 (op, x, y, z)                      every other opcode: x = the operand of a unary operator, (x, y) of a binary
//   test<CERT>, inject     poison (and the running maximum) over a tested value; is_valid(x) ? r : Inf
//   store_vec / store_ragged                                  a full tile's aligned store; the ragged tail's
// and, for the LOSS variant, what a loss term is:
//   LY, LW                 a lane's VW targets / weights (by value)
//   load_y, load_w (a, j0, vec)   vec: the lane's aligned vector load (a full tile, aligned arrays); else loads clamped to N - 1 — no
//                          read past element N - 1 of either array.  load_w: 1 without weights, 0 for a sample past N
//   LOSS_ALL_KINDS         whether the parameterised kinds (de_loss_kinds.h) are served, or DE_LOSS_L2 / DE_LOSS_L1 alone
//   loss_sum (kind, p, acc, y, w)   sum over the lane's samples, in sample order and in Scalar, of  w != 0 ? w * l : 0  — a weight equal
//                          to 0 (a sample past N) excludes a sample by the select, never by the product.  The parameterised kinds sit
//                          behind one __noinline__ function per policy: the switch over the kind stays out of the interpreter's own
//                          switch.  The sum is the library's, in Scalar (Float32 for binary16 terms: a binary16 sum overflows at 65504)
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
    // LOSS: targets and weights (N samples; w null = 1), one Scalar per (tile, tree, wave), the kind and its parameter
    const E *y, *w;
    void *partial;
    double loss_param;
    int32_t loss_kind, yw_vec; // yw_vec: y and w are 16-byte aligned (a full tile's lanes use their vector loads)
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

template <class P, bool EE, bool PARAMS, bool DIRECT, bool CERT, bool LOSS = false>
__global__ void __launch_bounds__(FLAT_BLK) de_eval_flat_kernel(const FlatArgs<typename P::Elem> a) {
    typedef typename P::V V;
    typedef typename P::Scalar S;
    typedef typename P::Elem E;
    constexpr int VW = P::VW;
    static_assert(P::TILE == FLAT_BLK * VW, "a lane owns VW consecutive samples of the tile");
    static_assert(!(LOSS && CERT), "the certificate pass has no loss");
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
    // (LOSS) this lane's targets and weights, read once per workgroup; a sample past N has weight 0
    [[maybe_unused]] typename P::LY ly;
    [[maybe_unused]] typename P::LW lw;
    [[maybe_unused]] S lparam = S(0);
    if constexpr (LOSS) {
        ly = P::load_y(a, j0, full && a.yw_vec);
        lw = P::load_w(a, j0, full && a.yw_vec);
        lparam = (S)a.loss_param;
    }
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
        } else if constexpr (LOSS) {
            // the lane's terms in sample order, the wave's 64 lane sums in the fixed order of wave_sum_to_lane63: partial[tile, tree, wave]
            // (a skipped tree writes none: the finish pass selects NaN by ok[t])
            const S s = wave_sum_to_lane63(P::loss_sum(a.loss_kind, lparam, acc, ly, lw));
            if ((tid & 63) == 63) static_cast<S *>(a.partial)[(tm.tile * a.n_trees + tree) * (FLAT_BLK / 64) + (tid >> 6)] = s;
        } else {
            E *__restrict__ o = a.out + P::EPS * ((int64_t)tree * a.ld_out + j0);
            if (full && a.vec_store) P::store_vec(o, acc);
            else P::store_ragged(o, acc, a.N - j0);
        }
        // ---- completion flag: one ballot per wave, one byte store per failing wave
        if (__ballot(poison != poison) != 0ull) flag_incomplete(a.ok + tree, a.skip_flagged == 1);
    }
}

// Pass 3 of a loss launch (pass 2 is launch_loss_reduce_tiles, de_kernels.h): thread = one tree, its segments and waves in a fixed
// order, in double; NaN where the evaluation was incomplete, whatever the partials of a skipped tree hold
template <class P>
__global__ void __launch_bounds__(256) de_flat_loss_finish_kernel(const double *__restrict__ seg_sum, int64_t n_trees, int32_t n_segs,
                                                                 const uint8_t *__restrict__ ok, typename P::Scalar *__restrict__ loss) {
    typedef typename P::Scalar S;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_trees) return;
    double s = 0.0;
    for (int32_t g = 0; g < n_segs; ++g)
        for (int w = 0; w < FLAT_BLK / 64; ++w) s += seg_sum[((int64_t)g * n_trees + t) * (FLAT_BLK / 64) + w];
    loss[t] = ok[t] ? (S)s : M<S>::nan();
}

// ---- launch -----------------------------------------------------------------------------------------------------------------------
// The kernels that exist: (EE, PARAMS, DIRECT), each with and without LOSS, and, for the certificate pass, (EE = true, PARAMS, CERT)
// without the gather
template <class P, bool PARAMS> static auto flat_kernel(bool ee, bool direct, bool cert, bool loss) -> void (*)(const FlatArgs<typename P::Elem>) {
    if (cert) return de_eval_flat_kernel<P, true, PARAMS, false, true>;
    if (loss) {
        if (direct) return ee ? de_eval_flat_kernel<P, true, PARAMS, true, false, true> : de_eval_flat_kernel<P, false, PARAMS, true, false, true>;
        return ee ? de_eval_flat_kernel<P, true, PARAMS, false, false, true> : de_eval_flat_kernel<P, false, PARAMS, false, false, true>;
    }
    if (direct) return ee ? de_eval_flat_kernel<P, true, PARAMS, true, false> : de_eval_flat_kernel<P, false, PARAMS, true, false>;
    return ee ? de_eval_flat_kernel<P, true, PARAMS, false, false> : de_eval_flat_kernel<P, false, PARAMS, false, false>;
}

// ctab: the program's device constant table, for the policies that read one
template <class P> static hipError_t launch_flat(const EvalArgs &e, const void *ctab, hipStream_t stream, const char **kname) {
    typedef typename P::Elem E;
    if (e.uses_params && !P::HAS_PARAMS) return hipErrorInvalidValue; // (the host refuses these first)
    if (e.loss) { // no fit statistics, no certificate with a loss, and only the kinds the policy serves
        const int32_t k = e.loss->kind;
        if (e.cert_max || e.loss->stats || !e.loss->y || !e.loss->partial || !e.loss->seg_sum || !e.loss->loss) return hipErrorInvalidValue;
        if (k != DE_LOSS_L2 && k != DE_LOSS_L1 && !(P::LOSS_ALL_KINDS && k >= DE_LOSS_HUBER && k <= DE_LOSS_L1_HINGE)) return hipErrorInvalidValue;
    }
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
    a.y = e.loss ? static_cast<const E *>(e.loss->y) : nullptr;
    a.w = e.loss ? static_cast<const E *>(e.loss->w) : nullptr;
    a.partial = e.loss ? e.loss->partial : nullptr;
    a.loss_param = e.loss ? e.loss->param : 0.0;
    a.loss_kind = e.loss ? e.loss->kind : 0;
    a.yw_vec = ((reinterpret_cast<uintptr_t>(a.y) | reinterpret_cast<uintptr_t>(a.w)) % 16 == 0) ? 1 : 0;
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
    void (*kern)(const FlatArgs<E>) = flat_kernel<P, false>(e.early_exit, e.direct, e.cert_max != nullptr, e.loss != nullptr);
    if constexpr (P::HAS_PARAMS) {
        if (e.uses_params) kern = flat_kernel<P, true>(e.early_exit, e.direct, e.cert_max != nullptr, e.loss != nullptr);
    }
    // (DIRECT: no staged parameter rows either — a program gathers its features only when the rows would not fit)
    const size_t lds = (size_t)(e.direct ? (e.n_slots > 0 ? e.n_slots : 1) : e.F + e.n_slots) * P::ROW_BYTES;
    if (kname) *kname = P::NAMES[e.cert_max ? 2 : e.loss ? (e.direct ? 4 : 3) : e.direct ? 1 : 0];
    if (lds > 64 * 1024) {
        const hipError_t st = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (st != hipSuccess) return st;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(FLAT_BLK), lds, stream, a);
    hipError_t st = hipGetLastError();
    if (st != hipSuccess || !e.loss) return st;
    // the two fixed-order passes in double, on the same stream: tiles -> segments, segments and waves -> loss[t]
    typedef typename P::Scalar S;
    static_assert(sizeof(S) == 4 || sizeof(S) == 8, "Float32 or Float64 partials");
    int32_t n_segs = 1;
    st = launch_loss_reduce_tiles(sizeof(S) == 4 ? DE_F32 : DE_F64, a.partial, (int64_t)e.n_trees * (FLAT_BLK / 64), a.n_tiles, e.loss->seg_sum, &n_segs, stream);
    if (st != hipSuccess) return st;
    hipLaunchKernelGGL(de_flat_loss_finish_kernel<P>, dim3((unsigned)((e.n_trees + 255) / 256)), dim3(256), 0, stream,
                       static_cast<const double *>(e.loss->seg_sum), (int64_t)e.n_trees, n_segs, e.ok, static_cast<S *>(e.loss->loss));
    return hipGetLastError();
}

} // namespace de
