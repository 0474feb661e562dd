// de_batch.h — minibatches: the arithmetic of the counter-based row sampler, shared by the kernel of de_batch.hip and
// the host function de_batch_rows_host (the same integer operations, so the same bits), and the launchers of de_batch.hip.
//
// THE SAMPLER.  Row j of a batch is a pure function of (mode, N, seed, step, offset + j); all arithmetic is modulo 2^64.
//   G      = 0x9E3779B97F4A7C15
//   fin(z) : z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31      (SplitMix64's output function:
//            fin(G), fin(2G), fin(3G) = e220a8397b1dcdaf 6e789e6aa1b965f4 06c45d188009454f, the published stream of seed 0)
//   key    : k = fin(seed ^ fin(step + G))                       (`seed` names the run, `step` the batch)
//   REPLACE (with replacement):  i = offset + j;  r = fin(k + G * (i + 1));  row = mulhi64(r, N)             (bias at most N / 2^64)
//   PERMUTE (the slice [offset, offset + n_rows) of a keyed permutation of [0, N)):
//            b = max(2, bit_length(N - 1)) rounded up to even, h = b / 2, mask = 2^h - 1;  x = offset + j;
//            repeat { L = x >> h; R = x & mask; for r = 0 .. 5: (L, R) = (R, L ^ (fin(k ^ (R + G * (r + 1))) & mask)); x = (L << h) | R }
//            until x < N                                          (a 6-round Feistel network over [0, 2^b), cycle-walked into [0, N))
#ifndef DE_BATCH_H
#define DE_BATCH_H
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define DE_BATCH_HD __host__ __device__ __forceinline__
#else
#define DE_BATCH_HD inline
#endif

namespace de {

constexpr uint64_t BATCH_G = 0x9E3779B97F4A7C15ull;

DE_BATCH_HD uint64_t batch_fin(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

DE_BATCH_HD uint64_t batch_key(uint64_t seed, uint64_t step) { return batch_fin(seed ^ batch_fin(step + BATCH_G)); }

DE_BATCH_HD uint64_t batch_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

// h of the definition above: half the (even) bit width of the Feistel domain of N rows
DE_BATCH_HD int batch_half_bits(uint64_t N) {
    int b = 0;
    for (uint64_t v = N - 1; v; v >>= 1) b++;
    if (b < 2) b = 2;
    return (b + 1) >> 1;
}

DE_BATCH_HD int64_t batch_row_replace(uint64_t k, uint64_t N, uint64_t i) { return (int64_t)batch_mulhi(batch_fin(k + BATCH_G * (i + 1)), N); }

DE_BATCH_HD int64_t batch_row_permute(uint64_t k, uint64_t N, int h, uint64_t i) {
    const uint64_t mask = ((uint64_t)1 << h) - 1;
    uint64_t x = i;
    // The domain [0, 2^(2h)) is smaller than 4 N and the network is a bijection of it: x lies on a cycle of that bijection, and the cycle
    // returns to its starting value i < N, so the walk ends (after fewer than 4 steps on average); no value below N is visited twice,
    // which is what makes the walked map a permutation of [0, N).
    do {
        uint64_t L = x >> h, R = x & mask;
        for (uint64_t r = 0; r < 6; r++) {
            const uint64_t t = L ^ (batch_fin(k ^ (R + BATCH_G * (r + 1))) & mask);
            L = R;
            R = t;
        }
        x = (L << h) | R;
    } while (x >= N);
    return (int64_t)x;
}

#if defined(__HIPCC__) || defined(__HIP__)
// rows[j] = row (offset + j) of the batch (mode, N, seed, step), one lane per row; the arguments were checked by the caller
hipError_t launch_batch_sample(int mode, int64_t N, uint64_t seed, uint64_t step, int64_t offset, int64_t n_rows, int64_t *rows, hipStream_t stream);

// One launch of the gather.  Buffers are seen as arrays of WORDS of `word` bytes (2, 4 or 8: the real component type), a complex element
// being two of them: xw words of X per row (n_features * parts) with leading dimensions in words, yw words of y per row (parts), one of w.
// A null source or destination column is not gathered.  n_bad may be null.
struct BatchGatherArgs {
    const void *sX, *sy, *sw, *scls;
    void *dX, *dy, *dw, *dcls;
    const int64_t *rows;
    int32_t *n_bad;
    int64_t N, n_rows, s_ld, d_ld; // leading dimensions in words
    int32_t xw, yw, cls_bytes;     // words of X and of y per row; 4 or 8
    int32_t tile_rows;             // rows of one workgroup's tile, 1 .. 256
    uint64_t recip;                // floor(2^32 / xw) + 1: lane / xw = (lane * recip) >> 32 for lane < 256
    int32_t step_q, step_r;        // 256 / xw and 256 % xw
};
hipError_t launch_batch_gather(int word, const BatchGatherArgs &a, hipStream_t stream);
#endif

} // namespace de
#endif
