// mxfp8.h — the MXFP8 wire format's sizes, the segment-cover step of a quantise and the launchers of
// mxfp8.hip's kernels: quantise and fold (each plain or, given a residual, with error feedback),
// dequantise and the reduce-scatter's fold-dequantise. Internal to
// libtips_hip.so (not part of the C-ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace tips {

// A block is 32 consecutive elements of the flat f32 layout (fused_layout: every tensor starts on a
// multiple of 64 elements, so no block straddles two tensors). The wire buffer of E flat elements:
// one payload byte per element from byte 0, one scale byte per block from byte round_up(E, 256).
constexpr int kMxBlock = 32;
inline int64_t mxfp8_blocks(int64_t elems) { return (elems + kMxBlock - 1) / kMxBlock; }
inline int64_t mxfp8_scales_offset(int64_t elems) { return (elems + 255) / 256 * 256; }
inline int64_t mxfp8_wire_bytes(int64_t elems) { return mxfp8_scales_offset(elems) + (mxfp8_blocks(elems) + 255) / 256 * 256; }

// One tensor of a quantise / dequantise launch: `count` f32 elements at `ptr` (4-B aligned), which
// lie at flat elements [off, off + count); the launch covers flat elements [off, off + span) (span a
// multiple of 32: for the quantise the tensor and the padding behind it, which encodes as zeros; for
// the dequantise the tensor's blocks). ptr == nullptr with count 0: padding only. Segments ascend.
struct MxSeg {
  const void* ptr;
  int64_t off, count, span;
};
// Up to this many segments travel with one launch, by value (no table upload: a training step
// brings new gradient pointers every time). Longer lists take several launches.
constexpr int kMxSegsPerLaunch = 48;
constexpr int64_t kMxTileElems = 4096;  // per workgroup: 256 lanes x 4 rounds x 4 elements

// Make sorted quantise segments cover every flat position of [0, end): each segment's span reaches
// the next one's off (the last one's reaches `end`), and where the first does not begin at 0 a
// padding-only segment is put in front of it. `segs` must not be empty.
inline void mxfp8_cover(std::vector<MxSeg>& segs, int64_t end) {
  for (size_t i = 0; i < segs.size(); i++) segs[i].span = (i + 1 < segs.size() ? segs[i + 1].off : end) - segs[i].off;
  if (segs[0].off > 0) segs.insert(segs.begin(), MxSeg{nullptr, 0, 0, segs[0].off});
}

// Quantise the segments into the wire buffer (payload, scales: 16-B aligned). The first launch also
// zeroes the scale bytes scales[tail_begin ... tail_end) (the alignment tail behind the last block;
// pass 0, 0 for none). `residual` null: the plain quantise. Otherwise the one with error feedback
// (DESIGN.md §17): the sender residual, one f32 per flat position from position 0 (16-B aligned,
// round_up(E, 256) floats); c = x + r is quantised and r' = c - dequantise(c) stored, +0 over a
// poisoned block; positions without a tensor element are not touched.
hipError_t launch_mxfp8_quantize(const MxSeg* segs, int nseg, unsigned char* payload, unsigned char* scales,
                                 float* residual, int64_t tail_begin, int64_t tail_end, hipStream_t s);
// dst = quantise(fold of the sources' blocks in order), over `nblocks` blocks: payload pointers at the
// range's first block (16-B aligned), scale pointers at its first scale byte. dst may be a source.
// `residual` null: the plain fold. Otherwise the one with error feedback: 32 f32 per block from the
// range's first block (16-B aligned); c = acc + o is quantised and o' = c - dequantise(c) stored, +0
// over a poisoned block.
constexpr int kMxMaxSrcs = 16;
struct MxSrcs {
  const unsigned char* payload[kMxMaxSrcs];
  const unsigned char* scales[kMxMaxSrcs];
};
hipError_t launch_mxfp8_fold(unsigned char* dst_payload, unsigned char* dst_scales, const MxSrcs& srcs, int nsrc,
                             int64_t nblocks, float* residual, hipStream_t s);
// Dequantise the segments' elements (segs[i].ptr: the f32 destination) from the wire buffer; factor
// as an f32 multiply behind the decode when it is not 1.
hipError_t launch_mxfp8_dequantize(const MxSeg* segs, int nseg, const unsigned char* payload, const unsigned char* scales,
                                   float factor, hipStream_t s);

// One output tensor of the MXFP8 reduce-scatter's fold: `count` f32 elements at `dst`
// (4-B aligned) folded from `own` (this rank's slice, 4-B aligned, not quantised) and, for every other
// source, from the flat elements [off, off + count) of its wire buffer (off a multiple of 64).
// Segments ascend by off and do not overlap.
struct MxFoldSeg {
  const void* own;
  void* dst;
  int64_t off, count;
};
// By value, like MxSeg lists; 80 records, their tile starts and the 32 source pointers keep the
// arguments under 4 KiB with room for the launch's hidden ones (config 5's 214 gradients: 3 launches).
constexpr int kMxFoldSegsPerLaunch = 80;
// For every segment and element k at flat position f = off + k: dst[k] = ((y_0 + y_1) + ...) + y_{nsrc-1},
// y_own_pos = own[k] and y_j = dequantise(wire j)[f] otherwise (wires.payload[j] / wires.scales[j]: a
// whole wire buffer's first payload and first scale byte; entry own_pos is not read), separate f32
// adds, then * factor when factor != 1; every NaN stored as 0x7FC00000. One source: reducescatter.hip's
// copy (factor 1, every bit kept) or scaled copy.
hipError_t launch_mxfp8_fold_segs(const MxFoldSeg* segs, int nseg, const MxSrcs& wires, int nsrc, int own_pos, float factor,
                                  hipStream_t s);

}  // namespace tips
