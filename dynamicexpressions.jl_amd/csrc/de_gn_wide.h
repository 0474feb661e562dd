// de_gn_wide.h — launchers of de_gn_wide.hip: Gauss-Newton matrices and Levenberg-Marquardt steps of trees of 9 .. 32 gradient rows
// (de_eval_loss_gn_wide / de_gn_lm_step_wide / de_fit_consts_lm_wide).
//
// The forward-dual kernels hold at most DE_GN_MAX_ROWS dual rows in one window, so a wider tree's cross-window products exist nowhere in
// them.  The wide route forms them from the Jacobian instead, chunk by chunk: de_eval_grad's kernels write the rows of the wide trees
// alone for `chunk` samples ([G, chunk] column-major per tree, G contiguous values per sample) and the tree's values, the Gram kernel
// below reduces ((w c) d_i) d_k over the chunk, and nothing of size N outlives a chunk.
//
// SCRATCH.  With R = sum of G_t and n_w = the number of wide trees, a chunk of n samples needs (R + n_w) n elements for the rows and the
// values.  The default chunk is the largest multiple of 256 with
//     (R + n_w) * chunk * sizeof(T) <= 256 MiB,    at least 256 and at most N rounded up to 256,
// and DE_GN_WIDE_CHUNK=<samples> (rounded up to a multiple of 64) overrides it.  The partial sums take
// ceil(chunk / GNW_SLICE) * sum_t G_t (G_t + 1) / 2 doubles, the running totals sum_t G_t (G_t + 1) / 2 doubles.
//
// ACCURACY.  Every product ((w c) d_i) d_k is formed in the element type — three roundings, two when c == 1 — and converted to double at
// once; every sum is a double sum in a fixed order, in four levels: the GNW_TILE = 64 samples of a tile, the 16 tiles of a slice, the
// slices of a chunk, the chunks.  Float32: no accumulator chain runs in the element type at all, |H - H_ref| <= 3 u A + O(2^-53) A.
// Float64: the longest chain is a tile's 64 terms (the narrow kernels' wave sums run over up to 128), and the levels above it add one
// rounding per partial sum like the narrow kernels' sums across waves and tiles.  Both lie inside the 256 u A of
// tests/test_gpu_gauss_newton.py, and the result is reproducible run to run.
#ifndef DE_GN_WIDE_H
#define DE_GN_WIDE_H
#include <hip/hip_runtime.h>
#include <cstdint>

#include "de_lm.h"

namespace de {

constexpr int DE_GN_WIDE_MAX_ROWS = 32; // de_gn_wide_max_rows()
constexpr int GNW_SLICE = 1024;         // samples one workgroup of the Gram kernel reduces
constexpr int GNW_TILE = 64;            // samples staged in LDS at a time

// One entry per wide tree, in the order of the hidden sub-program (device table)
struct GnWideTree {
    int32_t tree;    // index in the population
    int32_t G;       // gradient rows, 9 .. 32
    int64_t row0;    // rows of the wide trees before this one: its chunk Jacobian starts at row0 * n elements
    int64_t tri0;    // lower-triangle entries of the wide trees before this one
    int64_t joff;    // element offset of its G x G block in jtj
};

// sub[k] = full[idx[k]]: the wide trees' constants out of the population's (element type of `dtype`)
hipError_t launch_gnw_gather(int dtype, const void *full, const int64_t *idx, int64_t n, void *sub, hipStream_t stream);

struct GnWideGramArgs {
    const GnWideTree *trees;
    int32_t n_wide;
    const void *jac;   // the chunk's rows: tree s at jac + row0 * n, element (k, j) at k + G j
    const void *vals;  // the chunk's values: tree s at vals + s * n
    const void *y, *w; // the chunk's targets and weights (w may be null)
    int64_t n;         // samples of the chunk
    int32_t kind;      // de_loss_kind_t
    double param, e_floor;
    double *partial;   // [ceil(n / GNW_SLICE)][tri_total]
    int64_t tri_total;
};
hipError_t launch_gnw_gram(int dtype, const GnWideGramArgs &a, hipStream_t stream);

// total[e] = (first ? 0 : total[e]) + sum over the chunk's slices, in order; last: jtj block of every wide tree = total (both triangles), or
// NaN where ok[tree] == 0
hipError_t launch_gnw_fold(int dtype, const GnWideTree *trees, int32_t n_wide, const double *partial, int64_t n_slices, int64_t tri_total,
                           double *total, bool first, bool last, void *jtj, const uint8_t *ok, hipStream_t stream);

// One wave per tree with 8 < n_grad <= 32: LmStepArgs' contract with lm_solve_wide's arithmetic (de_lm_solve_wide.h); every other tree is
// left alone (launch_lm_step has served it).
hipError_t launch_lm_step_wide(int dtype, const LmStepArgs &a, hipStream_t stream);

} // namespace de
#endif
