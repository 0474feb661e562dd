// de_half.hip — gfx950 kernel of DE_F16 (IEEE binary16) evaluation: X, constants, parameters and outputs are binary16, every operator
// step computes in Float32 registers and is rounded to binary16 before the next step reads it (de_half_ops.h).
//
// One flat, wave-uniform switch over the BOUND program (de_bind.h), as de_kernels.hip's de_eval_tape_kernel: 256 threads, 4 consecutive
// samples per lane, a 1024-sample tile per workgroup, a chunk of <= 63 trees per workgroup.  The binary16 X tile is read once per
// workgroup with coalesced loads and written TRANSPOSED into LDS as Float32 rows (binary16 -> Float32 is exact), so a leaf read is one
// ds_read_b128 per lane and spill slots are Float32 rows like X.  Results go out as four packed binary16 values per lane (one 8-byte
// store).  Flags: the per-lane NaN poison over every tested value (after rounding: a value that rounds to Inf, i.e. from 65520 up, is
// non-finite), one ballot per tree, the early-exit skip of trees already flagged (de_device_ops.h skip_flag_load, protocol 2).
// The CERT variant (de_eval_sum_certificate) stores nothing and keeps the largest |tested value| of every tree.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "de_bind.h"
#include "de_half_ops.h"
#include "de_kernels.h"

namespace de {

typedef float HV __attribute__((ext_vector_type(4)));
typedef _Float16 HH4 __attribute__((ext_vector_type(4)));
typedef uint32_t HU4 __attribute__((ext_vector_type(4)));
#define DE_HCONSTANT __attribute__((address_space(4)))
typedef const DE_HCONSTANT HU4 *HCodePtr;
typedef const DE_HCONSTANT int32_t *HOffPtr;

constexpr int HBLK = 256, HVW = 4, HTILE = HBLK * HVW, HROWV = HBLK + 1; // (LDS row: 256 vectors + one of padding: bank spread)

struct HArgs {
    const BoundInstr *code;
    const int32_t *code_off;
    const _Float16 *X;
    _Float16 *out;
    uint8_t *ok;
    const _Float16 *params;
    const void *classes;
    void *cert_max; // CERT: per tree the bits of the largest |tested value| (a non-negative float)
    int64_t N, ldX, ld_out, ld_params, n_tiles, n_classes;
    int32_t F, n_trees, trees_per_chunk, n_chunks, prow_base, n_prows;
    int32_t classes_is_i64, class_base, vec_store, skip_flagged;
};

// blockIdx -> (sample tile, tree chunk), XCD-aware as de_kernels.hip map_block: block b runs on XCD b % 8, all chunks of one tile on one XCD
__device__ __forceinline__ bool h_map_block(uint32_t bid, int32_t n_chunks, int64_t n_tiles, int64_t *tile, int32_t *chunk) {
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

// Everything but the hot operators: one noinline function (the interpreter loop keeps only wave-uniform control flow; de_kernels.hip)
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
__device__ __noinline__ void h_flag_incomplete(uint8_t *ok, int agent) { // agent scope under protocol 1: later workgroups skip the tree
    if ((threadIdx.x & 63) == 0) {
        if (agent) __hip_atomic_store(ok, (uint8_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else *ok = 0;
    }
}

template <bool CERT> __device__ __forceinline__ void h_test(float &poison, float &vmax, HV v) {
#pragma unroll
    for (int i = 0; i < HVW; i++) {
        poison = __builtin_fmaf(v[i], 0.0f, poison); // stays +0 while every tested value is finite, NaN from the first Inf / NaN on
        if constexpr (CERT) vmax = __builtin_fabsf(v[i]) > vmax ? __builtin_fabsf(v[i]) : vmax;
    }
}
// DIRECT kernels: feature row f of this lane's four samples from global memory (samples past N repeat the last one)
__device__ __forceinline__ HV h_gather(const HArgs &a, uint32_t f, int64_t j0) {
    HV v;
#pragma unroll
    for (int i = 0; i < HVW; i++) {
        const int64_t jj = j0 + i < a.N - 1 ? j0 + i : a.N - 1;
        v[i] = (float)a.X[f + a.ldX * jj];
    }
    return v;
}
__device__ __forceinline__ HV h_round(HV v) {
    HV r;
#pragma unroll
    for (int i = 0; i < HVW; i++) r[i] = r16(v[i]);
    return r;
}

// DIRECT: a feature matrix too wide for the LDS tile (de_api_program.cpp `direct`) — feature operands are gathered from global memory
// (binary16, the L1 / L2 absorb the re-reads) and LDS holds the spill-slot rows only, as de_eval_tape_kernel<DIRECT> does
template <bool EE, bool PARAMS, bool CERT, bool DIRECT = false>
__global__ void __launch_bounds__(HBLK) de_eval_half_kernel(const HArgs a) {
    extern __shared__ __align__(16) unsigned char smem_half[];
    float *__restrict__ rows = reinterpret_cast<float *>(smem_half); // rows 0..F-1: the X tile; F + s: spill slot s; then parameter rows
    HV *__restrict__ rowsv = reinterpret_cast<HV *>(smem_half);
    int64_t tile;
    int32_t chunk;
    if (!h_map_block(blockIdx.x, a.n_chunks, a.n_tiles, &tile, &chunk)) return;
    const int tid = threadIdx.x;
    const int64_t base = tile * HTILE;
    const int64_t last = a.N - 1;

    // ---- stage the X tile: coalesced read of binary16 pairs, transposed Float32 write (sample j of row f at rows[f * HROWV * 4 + j])
    if (!DIRECT) {
        const uint32_t F = (uint32_t)a.F;
        const uint32_t total = (uint32_t)HTILE * F;
        if (a.ldX == (int64_t)F && base + HTILE <= a.N) {
            const _Float16 *__restrict__ src = a.X + base * (int64_t)F; // contiguous HTILE * F elements (an even count)
            if ((reinterpret_cast<uintptr_t>(src) & 3u) == 0) {
                const uint32_t *__restrict__ s2 = reinterpret_cast<const uint32_t *>(src);
                for (uint32_t e2 = tid; e2 < total / 2; e2 += HBLK) {
                    const uint32_t w = s2[e2];
                    _Float16 h[2];
                    __builtin_memcpy(h, &w, 4);
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        const uint32_t e = 2 * e2 + k, j = e / F, f = e - j * F;
                        rows[f * (HROWV * HVW) + j] = (float)h[k];
                    }
                }
            } else {
                for (uint32_t e = tid; e < total; e += HBLK) {
                    const uint32_t j = e / F, f = e - j * F;
                    rows[f * (HROWV * HVW) + j] = (float)src[e];
                }
            }
        } else { // ragged tail / strided X: samples past N repeat the last one
            for (uint32_t e = tid; e < total; e += HBLK) {
                const uint32_t j = e / F, f = e - j * F;
                int64_t jj = base + j;
                jj = jj < last ? jj : last;
                rows[f * (HROWV * HVW) + j] = (float)a.X[f + a.ldX * jj];
            }
        }
    }
    int64_t cls[HVW];
    if constexpr (PARAMS) {
#pragma unroll
        for (int i = 0; i < HVW; i++) {
            int64_t jj = base + tid * HVW + i;
            jj = jj < last ? jj : last;
            cls[i] = clamp_class((a.classes_is_i64 ? reinterpret_cast<const int64_t *>(a.classes)[jj]
                                                   : (int64_t) reinterpret_cast<const int32_t *>(a.classes)[jj]) - a.class_base, a.n_classes);
        }
        if (!DIRECT && a.n_prows > 0) { // parameters as staged rows prow_base + p (de_api_program.cpp `prows`): this lane's own four samples
#pragma unroll
            for (int i = 0; i < HVW; i++)
                for (int p = 0; p < a.n_prows; p++) rows[(size_t)(a.prow_base + p) * (HROWV * HVW) + tid * HVW + i] = (float)a.params[p + a.ld_params * cls[i]];
        }
    }
    __syncthreads();

    const HCodePtr code = (HCodePtr)(uintptr_t)a.code;
    const HOffPtr code_off = (HOffPtr)(uintptr_t)a.code_off;
    const int t0 = chunk * a.trees_per_chunk;
    const int t1 = (t0 + a.trees_per_chunk < a.n_trees) ? t0 + a.trees_per_chunk : a.n_trees;
    const bool full = base + HTILE <= a.N;
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
        HV acc = {0.0f, 0.0f, 0.0f, 0.0f};
        float poison = 0.0f, vmax = 0.0f;
        HU4 nxt = code[pc];
        for (; pc < pe; ++pc) {
            const HU4 w = nxt;
            nxt = code[pc + 1]; // (the code buffer carries one trailing pad instruction)
// HROW(r): this lane's four values of row r (a feature row of the X tile, a spill slot, a staged parameter row); HSLOT(r): a slot row
#define HSLOT(r) (rowsv[(size_t)((r) - (DIRECT ? (uint32_t)a.F : 0u)) * HROWV + tid])
#define HROW(r) (DIRECT && (r) < (uint32_t)a.F ? h_gather(a, (r), base + tid * HVW) : HSLOT(r))
#define HBIN4(K, EXPR)                                                                                                       \
    case BOP_BIN_BASE + 4 * K + 0: { const HV y = HROW(w.y); const HV x = acc; acc = h_round(EXPR); } break;                     \
    case BOP_BIN_BASE + 4 * K + 1: { const HV y = HROW(w.y); const HV x = acc; acc = h_round(EXPR); h_test<CERT>(poison, vmax, acc); } break; \
    case BOP_BIN_BASE + 4 * K + 2: { const HV y = __uint_as_float(w.z); const HV x = acc; acc = h_round(EXPR); } break;        \
    case BOP_BIN_BASE + 4 * K + 3: { const HV y = __uint_as_float(w.z); const HV x = acc; acc = h_round(EXPR); h_test<CERT>(poison, vmax, acc); } break;
#define HUN4(K, OP)                                                                                                          \
    case BOP_UN_BASE + 4 * K + 0: { HV r; for (int i = 0; i < HVW; i++) r[i] = r16(OP(acc[i])); acc = r; } break;             \
    case BOP_UN_BASE + 4 * K + 1: { HV r; for (int i = 0; i < HVW; i++) r[i] = r16(OP(acc[i])); acc = r; h_test<CERT>(poison, vmax, acc); } break; \
    case BOP_UN_BASE + 4 * K + 2: { const HV x = HROW(w.y); HV r; for (int i = 0; i < HVW; i++) r[i] = r16(OP(x[i])); acc = r; } break; \
    case BOP_UN_BASE + 4 * K + 3: { const HV x = HROW(w.y); HV r; for (int i = 0; i < HVW; i++) r[i] = r16(OP(x[i])); acc = r; h_test<CERT>(poison, vmax, acc); } break;
            switch (w.x) {
            case BOP_LOAD_ROW: acc = HROW(w.y); break;
            case BOP_LOAD_CONST: { const float c = __uint_as_float(w.z); acc = HV{c, c, c, c}; } break;
            case BOP_PUSH: HSLOT(w.y) = acc; break;
            case BOP_CHECK_ROW: h_test<CERT>(poison, vmax, HROW(w.y)); break;
            case BOP_CHECK_ACC: h_test<CERT>(poison, vmax, acc); break;
            HBIN4(0, x + y)
            HBIN4(1, x - y)
            HBIN4(2, y - x)
            HBIN4(3, x * y)
            HBIN4(4, x / y)
            HBIN4(5, y / x)
            HUN4(0, h_cos)
            HUN4(1, h_exp)
            HUN4(2, h_sin)
            case BOP_GEN_ROW: acc = h16_cold(w.y >> 24, ((w.y >> 24) < 64u) ? HROW(w.y & 0xFFFFFFu) : acc, HROW(w.y & 0xFFFFFFu)); break;
            case BOP_GEN_CONST: { const float c = __uint_as_float(w.z); const HV b = {c, c, c, c}; acc = h16_cold(w.y >> 24, ((w.y >> 24) < 64u) ? b : acc, b); } break;
            case BOP_GEN_ACC: acc = h16_cold(w.y >> 24, acc, acc); break;
            case BOP_TERN: acc = h16_cold3(w.y >> 24, HROW(w.y & 0xFFFFFFu), HROW(w.z), acc); break;
            // is_valid(x_l) ? op(x_l) : Inf   (src/Evaluate.jl:722,787): the fused kernels, early_exit = false — x_l is the operand B (the
            // accumulator or a row); a binary operator combines the accumulator with it, as the generic handlers do
            case BOP_INJ_ACC: {
                const HV x = acc, r = h16_cold(w.y >> 24, acc, x);
                for (int i = 0; i < HVW; i++) acc[i] = __builtin_isfinite(x[i]) ? r[i] : __builtin_inff();
            } break;
            case BOP_INJ_ROW: {
                const uint32_t op = w.y >> 24;
                const HV x = HROW(w.y & 0xFFFFFFu), r = h16_cold(op, op < 64u ? x : acc, x);
                for (int i = 0; i < HVW; i++) acc[i] = __builtin_isfinite(x[i]) ? r[i] : __builtin_inff();
            } break;
            case BOP_GEN_PARAM:
                if constexpr (PARAMS) {
                    const uint32_t op = w.y >> 24;
                    HV b;
                    for (int i = 0; i < HVW; i++) b[i] = (float)a.params[(w.y & 0xFFFFu) + a.ld_params * cls[i]];
                    if (EE && (w.y & (1u << 23))) h_test<CERT>(poison, vmax, b);
                    if (op == DOP_LOAD) acc = b;
                    else acc = h16_cold(op, op < 64u ? b : acc, b);
                }
                break;
            default: break;
            }
#undef HROW
#undef HSLOT
#undef HBIN4
#undef HUN4
        }
        if constexpr (CERT) {
            // the tree's largest |tested value|: wave maximum, one atomicMax per wave on the bits (non-negative floats order as unsigned)
            for (int m = 32; m >= 1; m >>= 1) {
                const float o2 = __shfl_xor(vmax, m, 64);
                vmax = o2 > vmax ? o2 : vmax;
            }
            if ((tid & 63) == 0 && vmax > 0.0f) atomicMax(reinterpret_cast<unsigned int *>(a.cert_max) + tree, __float_as_uint(vmax));
        } else {
            _Float16 *__restrict__ o = a.out + (int64_t)tree * a.ld_out + base + tid * HVW;
            if (full && a.vec_store) {
                HH4 h;
                for (int i = 0; i < HVW; i++) h[i] = (_Float16)acc[i]; // (exact: every value is a binary16 already)
                *reinterpret_cast<HH4 *>(o) = h;                        // four samples, one 8-byte store per lane
            } else {
                h_store_ragged(o, acc, a.N - (base + tid * HVW));
            }
        }
        if (__ballot(poison != poison) != 0ull) h_flag_incomplete(a.ok + tree, a.skip_flagged == 1);
    }
}

static int h_cu_count() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) cus = n;
        else cus = 256; // MI355X
    }
    return cus;
}

// Chunks of <= 63 trees (the skip mask is one 64-bit ballot), more of them while the grid would not cover the chip 32 workgroups per CU,
// never fewer than 8 trees per chunk (de_kernels.hip chunk_plan, the same rule)
static void h_plan(int64_t n, int64_t n_tiles, int32_t *n_chunks_out, int32_t *tpc_out) {
    const int64_t want = (int64_t)h_cu_count() * 4 * 8;
    int64_t n_chunks = (n + 62) / 63;
    if (n_tiles > 0 && n_tiles * n_chunks < want) n_chunks = (want + n_tiles - 1) / n_tiles;
    const int64_t max_chunks = (n + 7) / 8;
    if (n_chunks > max_chunks) n_chunks = max_chunks;
    if (n_chunks < 1) n_chunks = 1;
    const int64_t tpc = n > 0 ? (n + n_chunks - 1) / n_chunks : 1;
    *tpc_out = (int32_t)tpc;
    *n_chunks_out = (int32_t)(n > 0 ? (n + tpc - 1) / tpc : 1);
}

void eval_plan_f16(int64_t n_trees, int64_t N, int32_t *tile, int32_t *n_chunks, int32_t *trees_per_chunk) {
    *tile = HTILE;
    h_plan(n_trees, (N + HTILE - 1) / HTILE, n_chunks, trees_per_chunk);
}

hipError_t launch_eval_f16(const EvalArgs &e, hipStream_t stream, const char **kname) {
    if (e.threaded || e.loss || (e.direct && e.cert_max)) return hipErrorInvalidValue; // (the host refuses these first)
    if (e.ok_init) { // the constant part of the flags, then the launch only clears bytes
        const hipError_t cs = hipMemcpyAsync(e.ok, e.ok_init, (size_t)e.n_trees, hipMemcpyDeviceToDevice, stream);
        if (cs != hipSuccess) return cs;
    }
    HArgs a;
    a.code = e.code;
    a.code_off = e.code_off;
    a.X = static_cast<const _Float16 *>(e.X);
    a.out = static_cast<_Float16 *>(e.out);
    a.ok = e.ok;
    a.params = static_cast<const _Float16 *>(e.params);
    a.classes = e.classes;
    a.cert_max = e.cert_max;
    a.N = e.N;
    a.ldX = e.ldX;
    a.ld_out = e.ld_out;
    a.ld_params = e.ld_params;
    a.n_tiles = (e.N + HTILE - 1) / HTILE;
    a.n_classes = e.n_classes > 0 ? e.n_classes : 1;
    a.F = e.F;
    a.n_trees = e.n_trees;
    a.prow_base = e.prow_base;
    a.n_prows = e.n_prows;
    a.classes_is_i64 = e.classes_is_i64;
    a.class_base = e.class_base;
    a.vec_store = (reinterpret_cast<uintptr_t>(e.out) % 8 == 0 && (e.ld_out * 2) % 8 == 0) ? 1 : 0;
    h_plan(e.n_trees, a.n_tiles, &a.n_chunks, &a.trees_per_chunk);
    a.skip_flagged = (e.early_exit && e.skip_flagged && a.trees_per_chunk <= 64) ? 2 : 0; // (protocol 2: de_device_ops.h skip_flag_load)
    const int64_t blocks = (a.n_tiles < 64 ? a.n_tiles : (a.n_tiles + 7) / 8 * 8) * a.n_chunks;
    if (blocks <= 0 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    void (*kern)(const HArgs);
    if (e.cert_max) {
        if (!e.early_exit) return hipErrorInvalidValue;
        kern = e.uses_params ? de_eval_half_kernel<true, true, true> : de_eval_half_kernel<true, false, true>;
    } else if (e.early_exit) kern = e.uses_params ? de_eval_half_kernel<true, true, false> : de_eval_half_kernel<true, false, false>;
    else kern = e.uses_params ? de_eval_half_kernel<false, true, false> : de_eval_half_kernel<false, false, false>;
    size_t lds = (size_t)(e.F + e.n_slots) * HROWV * 16;
    if (e.direct) { // (no staged parameter rows either: a program gathers its features only when the rows would not fit, de_api_program.cpp rebind)
        if (e.early_exit) kern = e.uses_params ? de_eval_half_kernel<true, true, false, true> : de_eval_half_kernel<true, false, false, true>;
        else kern = e.uses_params ? de_eval_half_kernel<false, true, false, true> : de_eval_half_kernel<false, false, false, true>;
        lds = (size_t)(e.n_slots > 0 ? e.n_slots : 1) * HROWV * 16;
    }
    if (kname) *kname = e.cert_max ? "de_eval_half_kernel<cert>" : e.direct ? "de_eval_half_kernel<direct>" : "de_eval_half_kernel";
    if (lds > 64 * 1024) {
        const hipError_t st = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (st != hipSuccess) return st;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(HBLK), lds, stream, a);
    return hipGetLastError();
}

} // namespace de
