// de_const_patch.h — launchers of de_const_patch.hip: the device side of de_program_set_consts_device.
#ifndef DE_CONST_PATCH_H
#define DE_CONST_PATCH_H
#include <hip/hip_runtime.h>
#include <cstdint>

namespace de {

// A site: the address of the immediate inside a 16-byte record of one of the program's device streams.  Bit 0 set: a 32-bit store (the
// `.arg` word of a Float32 chained record); clear: a 64-bit store to the record's `.lo/.hi` pair (Float32: the value's bits and a zero word).
constexpr uint64_t CONST_SITE_32 = 1;

// cvals image(s) of the fold kernel from the constants: dst0[k] = consts[idx[k]] for k < n0, dst1[k - n0] = consts[idx[k]] for the n1 behind them
hipError_t launch_const_gather(int dtype, const void *consts, const int64_t *idx, int64_t n0, void *dst0, int64_t n1, void *dst1, hipStream_t stream);
// one thread per site: the bits of vals[src[i]] to the site's address
hipError_t launch_const_scatter(int dtype, const void *vals, const uint64_t *addr, const uint32_t *src, int64_t n_sites, hipStream_t stream);
// one thread per tree: recompute_host_ok (de_api_program.cpp) on the device.  tfold: the folds of tree t are entries tfold_off[t] ..
// tfold_off[t + 1], each (index into fold_ok) << 1 | tested_always.  ok_grad may be null.
hipError_t launch_const_flags(int dtype, const void *vals, const int64_t *const_off, const uint8_t *const_checks, const int32_t *tfold_off,
                              const uint32_t *tfold, const uint8_t *fold_ok, int64_t n_trees, bool early_exit, uint8_t *ok_eval, uint8_t *ok_grad,
                              hipStream_t stream);

} // namespace de
#endif
