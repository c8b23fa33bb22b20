// adasum.h — launchers of the Adasum kernels (adasum.hip).
// Internal to libtips_hip.so (not part of the C-ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tips {

// One segment (one tensor) of a buffer: `count` elements from element `off`, cut into chunks of
// adasum_chunk_elems; chunk0 is the index of its first chunk among the call's chunks (the running sum
// of the earlier segments' chunk counts). Segments ascend and do not overlap; an empty one has no chunk.
struct AdaSeg {
  int64_t off, count, chunk0;
};
// A call's segments: a device table of nseg records, or (table == nullptr, nseg == 1) the one by value.
struct AdaSegs {
  const AdaSeg* table;
  int nseg;
  AdaSeg one;
};

// A chunk is 32 KiB of each operand: 256 lanes x 8 vectors of 16 B, whatever the dtype.
constexpr int64_t kAdaChunkBytes = 32768;
int64_t adasum_chunk_elems(int dtype);  // 8192 f32, 4096 f64, 16384 f16 / bf16; 0 for the integers
inline int64_t adasum_chunks(int64_t count, int64_t chunk_elems) { return (count + chunk_elems - 1) / chunk_elems; }

// Workspace of one pair call: 3 doubles per chunk (the partial d, na, nb), then 2 per segment (ca,
// cb). The bound below holds for every float dtype (the smallest chunk is f64's 4096 elements) and
// every way of cutting `count` elements into nseg segments; a multiple of 256 B.
inline int64_t adasum_workspace_bytes(int64_t count, int nseg) {
  return (8 * (3 * (count / 4096 + nseg) + 2 * (int64_t)nseg) + 255) / 256 * 256;
}

// The three passes of out = ca a + cb b (the definition: adasum.hip's head comment), stream-ordered on
// s. a, b and dst are the buffers' bases (segment offsets are added to all three); dst may be a or b.
// nchunks = the sum of the segments' chunk counts (> 0). partials: 3 * nchunks doubles, coef: 2 * nseg
// doubles, 8-B aligned device memory. Float dtypes only (hipErrorInvalidValue otherwise).
hipError_t launch_adasum_dots(const void* a, const void* b, AdaSegs segs, int64_t nchunks, int dtype, double* partials,
                              hipStream_t s);
hipError_t launch_adasum_coef(AdaSegs segs, int dtype, const double* partials, double* coef, hipStream_t s);
hipError_t launch_adasum_combine(void* dst, const void* a, const void* b, AdaSegs segs, int64_t nchunks, int dtype,
                                 const double* coef, hipStream_t s);
// ... and the three in order, the workspace cut as adasum_workspace_bytes says
hipError_t launch_adasum_pair(void* dst, const void* a, const void* b, AdaSegs segs, int64_t nchunks, int dtype,
                              void* workspace, hipStream_t s);

}  // namespace tips
