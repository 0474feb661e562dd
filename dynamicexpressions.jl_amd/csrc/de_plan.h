// de_plan.h — what every kernel's launch shares: the scalar-load pointer types, the chunk plans (eval: chunk_plan / plan_chunks; gradient:
// grad_chunk_plan, grad_flag_protocol), the blockIdx -> (tile, chunk) map and the host's CU count.  Included by the threaded kernel's module
// (de_kernels.hip), by the flat-switch interpreter (de_flat.h) and by the gradient kernels (de_grad_common.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

namespace de {

// Wave-uniform read-only data is addressed through the constant address space so
// the compiler emits scalar loads (s_load_*) for it.
#define DE_CONSTANT __attribute__((address_space(4)))
typedef uint32_t U32x4 __attribute__((ext_vector_type(4)));
typedef const DE_CONSTANT U32x4 *ConstU4Ptr;
typedef const DE_CONSTANT int32_t *ConstI32Ptr;
typedef const DE_CONSTANT int64_t *ConstI64Ptr;

// Chunk plan of a launch over n trees and n_tiles sample tiles (host: plan_chunks; device: de_compact_live_kernel for the live trees):
// chunks of <= tpc_max trees, more of them while the grid would not cover the chip `want_blocks` times, never fewer than 8 trees per chunk.
// nc0 = the chunk count before trees are spread evenly: an upper bound of the final count that is monotone in n.
__host__ __device__ inline void chunk_plan(int64_t n, int64_t n_tiles, int64_t tpc_max, int64_t want_blocks, int32_t *n_chunks_out, int32_t *tpc_out, int32_t *nc0_out) {
    if (tpc_max < 1) tpc_max = 63;
    int64_t n_chunks = (n + tpc_max - 1) / tpc_max;
    if (n_tiles > 0 && n_tiles * n_chunks < want_blocks) n_chunks = (want_blocks + n_tiles - 1) / n_tiles;
    const int64_t max_chunks = (n + 7) / 8; // >= 8 trees per chunk
    if (n_chunks > max_chunks) n_chunks = max_chunks;
    if (n_chunks < 1) n_chunks = 1;
    if (nc0_out) *nc0_out = (int32_t)n_chunks;
    const int64_t tpc = n > 0 ? (n + n_chunks - 1) / n_chunks : 1;
    *tpc_out = (int32_t)tpc;
    *n_chunks_out = (int32_t)(n > 0 ? (n + tpc - 1) / tpc : 0);
}

// XCD-aware block mapping: hardware dispatches block b to XCD b % 8 (observed, used
// for L2 affinity only — correctness never depends on it).  All chunks of a sample
// tile get block ids with the same residue, i.e. run on one XCD back to back.
struct TileMap {
    int64_t tile;
    int32_t chunk;
    bool valid;
};
__device__ __forceinline__ TileMap map_block(uint32_t bid, int32_t n_chunks, int64_t n_tiles) {
    TileMap m;
    if (n_tiles < 64) {
        // few sample tiles (the many-trees x few-rows shape): X fits in every L2 anyway, and the XCD-aware
        // order below would put all work of tile t on XCD t mod 8 (one eighth of the chip for a single tile)
        m.tile = (int64_t)(bid % (uint32_t)n_tiles);
        m.chunk = (int32_t)(bid / (uint32_t)n_tiles);
        m.valid = m.chunk < n_chunks;
        return m;
    }
    const uint32_t xcd = bid & 7u, idx = bid >> 3;
    m.chunk = (int32_t)(idx % (uint32_t)n_chunks);
    m.tile = (int64_t)(idx / (uint32_t)n_chunks) * 8 + xcd;
    m.valid = m.tile < n_tiles;
    return m;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
inline int env_int(const char *name, int dflt) {
    const char *v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

inline int cu_count() {
    static int cus = 0;
    if (cus == 0) {
        const int forced = env_int("DE_CU_COUNT", 0); // experiments: < 0 disables the small-grid re-split
        if (forced != 0) { cus = forced; return forced < 0 ? 0 : forced; }
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
        if (cus <= 0) cus = 256; // MI355X
    }
    return cus < 0 ? 0 : cus;
}

// Tree chunking: chunks of ~64 trees keep workgroups short (fine-grained tail) while the
// X-tile staging (one L2 read of the tile per chunk) stays a few percent of the work; with few
// sample tiles, split further so the grid still covers the chip several times.
// (`waves` > 1: the chunks of a wave group — one per wave, 1 / waves of the trees each: a workgroup keeps the trees, and the record
// footprint, of a one-wave workgroup)
inline int32_t plan_tpc_max(int waves) {
    const int64_t tpc_env = env_int("DE_EVAL_TPC", 63); // trees per chunk (experiments: X staging per tree against the tail of a short launch)
    const int64_t t = (tpc_env < 1 ? 63 : (tpc_env > 63 && waves > 1 ? 63 : tpc_env)) / (waves > 1 ? waves : 1);
    return (int32_t)(t < 1 ? 1 : t);
}
inline void plan_chunks(int64_t n_trees, int64_t n_tiles, int32_t *n_chunks_out, int32_t *tpc_out, int32_t *nc0_out = nullptr, int waves = 1) {
    chunk_plan(n_trees, n_tiles, plan_tpc_max(waves), (int64_t)cu_count() * 4 * 8, n_chunks_out, tpc_out, nc0_out);
    if (*n_chunks_out < 1) *n_chunks_out = 1;
}

// ---- the gradient kernels (launch_grad_kernel, de_grad_kernels.hip) -----------------------------------------------------------------
// Chunk plan of a gradient launch over n trees, n_tiles sample tiles and `windows` gradient windows (grid.y): chunks of <= 32 trees, more of
// them while the grid is below cus * 4 * 8 workgroups, never fewer than 4 trees per chunk; then the trees are spread evenly.  (Not
// chunk_plan: other constants, no nc0.)  Plain arithmetic, the CU count is passed in.
inline void grad_chunk_plan(int64_t n, int64_t n_tiles, int64_t windows, int64_t cus, int32_t *tpc_out, int32_t *n_chunks_out) {
    *tpc_out = *n_chunks_out = 0;
    if (n < 1 || n_tiles < 1 || windows < 1) return; // (an empty grid: the launch refuses it)
    int64_t n_chunks = (n + 31) / 32;
    const int64_t want_blocks = cus * 4 * 8;
    if (n_tiles * n_chunks * windows < want_blocks) n_chunks = (want_blocks + n_tiles * windows - 1) / (n_tiles * windows);
    const int64_t max_chunks = (n + 3) / 4;
    if (n_chunks > max_chunks) n_chunks = max_chunks;
    if (n_chunks < 1) n_chunks = 1;
    const int64_t tpc = (n + n_chunks - 1) / n_chunks;
    *tpc_out = (int32_t)tpc;
    *n_chunks_out = (int32_t)((n + tpc - 1) / tpc);
}
// Flag protocol of a gradient launch that skips flagged trees (skip_flag_load, de_device_ops.h): these kernels write little, their L1 lines
// go stale under 2 (reverse kernel 17.0 / 16.0 ms), so 1 (agent scope); 2 only for tiny chunks (many tiles on one flag line).
// prio_cached — the one difference between the kernels: the FORWARD threaded kernel takes 2 when its launch has priority tiles (the flags
// are then down before most workgroups first look, a stale line is rare and the cached protocol wins: fused loss gradient 6.65 -> 5.98 ms);
// the reverse kernel keeps 1 (15.9 against 16.9 ms) and so does the flat one.  forced: DE_SKIP_PROTOCOL = 1 .. 3 (experiments), else 0.
inline int32_t grad_flag_protocol(int32_t trees_per_chunk, bool prio_cached, int forced) {
    if (forced >= 1 && forced <= 3) return forced;
    return trees_per_chunk >= 8 && !prio_cached ? 1 : 2;
}

} // namespace de
