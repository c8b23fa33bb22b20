// kernels_dev.h — launchers of the tuning sweeps' kernels (kernels_dev.hip). Internal to
// libtips_hip_dev.so: runtime.cc includes it under TIPS_DEV for include/tips_hip_dev.h's sweep entries.
#pragma once

#include "kernels.h"

namespace tips {

// Tuning/sweep entry: explicit variant of the 2-input sum.
//   mode 0 = grid-stride over (blocks) workgroups, mode 1 = one tile per workgroup, mode 2 = the
//   same in XCD-contiguous tile order;
//   unroll = 16-B vectors per lane in flight, nt: 0 plain, 1 non-temporal loads+stores,
//   2 nt loads only, 3 nt stores only; threads = workgroup size. Non-default variants are f32 only.
//   mode 3 = buffer-op forms (nt = cache-policy pair index; blocks = bytes of unused LDS reserved
//   per workgroup), mode 4 = LDS-staged through gfx950's direct-to-LDS loads (unroll 1, 2 or 4;
//   256 threads), mode 5 = persistent streaming (unroll = workgroups per CU: 1, 2, 4 or 8),
//   mode 6 = other workgroup -> tile maps (unroll = stripe in KiB, 0: address order).
//   (3, 1, 7, 128) is what launch_sum2 launches; it and (3, 1, 1, 256) take every dtype.
hipError_t launch_sum2_variant(void* dst, const void* a, const void* b, int64_t n, int dtype, int mode, int unroll,
                               int nt, int blocks, int threads, hipStream_t s);

// Tuning/sweep entry for the multi-input sum (f32, nsrc 2/4/8); variants in kernels_dev.hip
// (run_multi_variant, run_multi_x). Variant 50 is launch_multi_sum.
hipError_t launch_multi_sum_variant(void* dst, const void* const* srcs, int nsrc, int64_t n, int dtype, int variant,
                                   hipStream_t s);

// Batched byte copy of a tile list: one workgroup per tile.
struct CopyTile {
  const char* src;
  char* dst;
  int64_t bytes;  // <= kCopyTileBytes
};
constexpr int64_t kCopyTileBytes = 64 * 1024;
hipError_t launch_copy_tiles(const CopyTile* tiles_dev, int ntiles, hipStream_t s);
// Tuning sweep (tools/copy_sweep.py): 0 = launch_copy_tiles; 1-8 = copy_tiles_g_kernel with G
// tiles per workgroup and load / store cache policies (copy_variant_u); tiles of at most
// max_tile_bytes (<= 16 KiB for variants 1-8).
hipError_t launch_copy_tiles_variant(const CopyTile* tiles_dev, int ntiles, int variant, int64_t max_tile_bytes,
                                     hipStream_t s);

}  // namespace tips
