// de_batch.hip — the device side of the minibatch entry points (arithmetic and launchers: de_batch.h).
//   de_batch_sample_kernel   one lane per row of the batch, no state: the counter-based sampler
//   de_batch_gather_kernel   one launch copies the rows of X and of the present columns y / w / classes into a dense batch
// The gather is a copy of bytes: a buffer is an array of words of the real component type's size (a complex element is two words), so
// three instantiations serve the five dtypes.  A workgroup takes a tile of `tile_rows` batch rows: lane t < tile_rows reads the row index
// of row t ONCE, tests it, parks it in LDS and copies that row's y / w / class; then all 256 lanes walk the tile's X words, consecutive
// lanes on consecutive words of the destination (one contiguous run of the whole tile when dst.ldX == n_features).  A lane finds its
// (row, word) without a division: the first pair from a host-computed reciprocal, every next one by adding 256 in mixed radix.
// Every address is computed in 64 bits.  A row index outside [0, N) reads nothing: its X, y and w words become quiet NaNs, its class that
// of source row 0, and it is counted in *n_bad.
#include "de_batch.h"

#include "../../include/de_hip.h"

namespace de {

__global__ void __launch_bounds__(256) de_batch_sample_kernel(int mode, uint64_t N, uint64_t k, int h, uint64_t offset, int64_t n_rows,
                                                              int64_t *__restrict__ rows) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n_rows; j += stride)
        rows[j] = mode == DE_BATCH_PERMUTE ? batch_row_permute(k, N, h, offset + (uint64_t)j) : batch_row_replace(k, N, offset + (uint64_t)j);
}

template <typename W> __device__ __forceinline__ W batch_quiet_nan();
template <> __device__ __forceinline__ uint16_t batch_quiet_nan<uint16_t>() { return 0x7E00u; }
template <> __device__ __forceinline__ uint32_t batch_quiet_nan<uint32_t>() { return 0x7FC00000u; }
template <> __device__ __forceinline__ uint64_t batch_quiet_nan<uint64_t>() { return 0x7FF8000000000000ull; }

template <typename W>
__global__ void __launch_bounds__(256) de_batch_gather_kernel(const BatchGatherArgs a) {
    __shared__ int64_t srow[256];
    const uint32_t tid = threadIdx.x;
    const W *__restrict__ sX = static_cast<const W *>(a.sX);
    const W *__restrict__ sy = static_cast<const W *>(a.sy);
    const W *__restrict__ sw = static_cast<const W *>(a.sw);
    W *__restrict__ dX = static_cast<W *>(a.dX);
    W *__restrict__ dy = static_cast<W *>(a.dy);
    W *__restrict__ dw = static_cast<W *>(a.dw);
    const W nan = batch_quiet_nan<W>();
    const uint32_t xw = (uint32_t)a.xw;
    const int64_t n_tiles = (a.n_rows + a.tile_rows - 1) / a.tile_rows; // (uniform: scalar arithmetic)
    // the lane's first word of a tile: tid = r0 * xw + f0
    const uint32_t r0 = (uint32_t)(((uint64_t)tid * a.recip) >> 32);
    const uint32_t f0 = tid - r0 * xw;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t j0 = tile * a.tile_rows;
        const int64_t left = a.n_rows - j0;
        const uint32_t nr = (uint32_t)(left < a.tile_rows ? left : (int64_t)a.tile_rows);
        if (tid < nr) {
            const int64_t j = j0 + tid;
            int64_t row = a.rows[j];
            const bool bad = row < 0 || row >= a.N;
            if (bad) {
                row = -1;
                if (a.n_bad) atomicAdd(a.n_bad, 1);
            }
            srow[tid] = row;
            if (dy)
                for (int32_t p = 0; p < a.yw; p++) dy[j * a.yw + p] = bad ? nan : sy[row * a.yw + p];
            if (dw) dw[j] = bad ? nan : sw[row];
            if (a.dcls) {
                const int64_t from = bad ? 0 : row;
                if (a.cls_bytes == 8) static_cast<int64_t *>(a.dcls)[j] = static_cast<const int64_t *>(a.scls)[from];
                else static_cast<int32_t *>(a.dcls)[j] = static_cast<const int32_t *>(a.scls)[from];
            }
        }
        __syncthreads();
        if (xw) {
            uint32_t r = r0, f = f0;
            while (r < nr) {
                const int64_t row = srow[r];
                dX[(j0 + r) * a.d_ld + f] = row < 0 ? nan : sX[row * a.s_ld + f];
                f += (uint32_t)a.step_r;
                r += (uint32_t)a.step_q;
                if (f >= xw) {
                    f -= xw;
                    r++;
                }
            }
        }
        __syncthreads(); // (the next tile rewrites srow)
    }
}

hipError_t launch_batch_sample(int mode, int64_t N, uint64_t seed, uint64_t step, int64_t offset, int64_t n_rows, int64_t *rows, hipStream_t stream) {
    if (n_rows <= 0) return hipSuccess;
    const int64_t blocks = (n_rows + 255) / 256;
    hipLaunchKernelGGL(de_batch_sample_kernel, dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(256), 0, stream, mode, (uint64_t)N,
                       batch_key(seed, step), batch_half_bits((uint64_t)N), (uint64_t)offset, n_rows, rows);
    return hipGetLastError();
}

hipError_t launch_batch_gather(int word, const BatchGatherArgs &a, hipStream_t stream) {
    if (a.n_rows <= 0) return hipSuccess;
    const int64_t n_tiles = (a.n_rows + a.tile_rows - 1) / a.tile_rows;
    const dim3 grid((unsigned)(n_tiles < (1 << 20) ? n_tiles : (1 << 20)));
    if (word == 2) hipLaunchKernelGGL(de_batch_gather_kernel<uint16_t>, grid, dim3(256), 0, stream, a);
    else if (word == 4) hipLaunchKernelGGL(de_batch_gather_kernel<uint32_t>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(de_batch_gather_kernel<uint64_t>, grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

} // namespace de
