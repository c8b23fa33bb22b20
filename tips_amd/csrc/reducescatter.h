// reducescatter.h — the row split and region layout of the reduce-scatter and the
// launcher of its kernel (reducescatter.hip). Internal to libtips_hip.so (not part of the C-ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"

namespace tips {

// Rank q's rows of a [rows, ...] tensor split along dim 0 over p ranks: base + (q < rem) rows from row
// q * base + min(q, rem) (base = rows / p, rem = rows % p). A function of (rows, p, q) alone.
inline int64_t rs_rows(int64_t rows, int p, int q, int64_t* begin) {
  const int64_t base = rows / p, rem = rows % p;
  if (begin) *begin = q * base + std::min<int64_t>(q, rem);
  return base + (q < rem ? 1 : 0);
}

// Region q of a list: every tensor's slice q in list order, each non-empty slice at the next 256-B
// multiple (offsets[i], when given; an empty slice gets the offset the next one takes). Returns the
// region's bytes (up to the last slice's last byte).
inline int64_t rs_layout(const int64_t* rows, const int64_t* row_elems, int n, int es, int p, int q, int64_t* offsets) {
  int64_t next = 0, end = 0;
  for (int i = 0; i < n; i++) {
    const int64_t bytes = rs_rows(rows[i], p, q, nullptr) * row_elems[i] * es;
    if (offsets) offsets[i] = next;
    if (bytes > 0) {
      end = next + bytes;
      next = (end + 255) / 256 * 256;
    }
  }
  return end;
}

// One output tensor of a fold launch: `count` elements folded into `dst` from `own` (this rank's
// slice: any element-aligned address) and, for every other source j, from stages[j] + off (off: the
// slice's byte offset in the region, a 256-B multiple). Segments ascend by off and do not overlap.
struct FoldSeg {
  const void* own;
  void* dst;
  int64_t off;
  int64_t count;
};
// Up to this many segments travel with one launch, by value (as mxfp8.h's MxSeg lists: a training
// step brings new gradient pointers every time, so there is no table to upload). Longer lists take
// several launches. (112 records of 32 B and the 16 stage pointers keep the arguments under 4 KiB
// with room for the launch's hidden ones; config 5's 214 gradients are two launches.)
constexpr int kFoldSegsPerLaunch = 112;

// For every segment and element k: dst[k] = the fold, in ascending j < nsrc, of source own_pos = own[k]
// and source j != own_pos = (stages[j] + off)[k] (stages[own_pos] is not read). sc.op kOpSum: the sum
// in the working type, every source multiplied by sc.pre where it is read and the sum by sc.post
// (launch_multi_sum_scaled with every source raw; pre == post == 1: launch_multi_sum's plain fold);
// kOpMax / kOpMin: the exact compare, no factors. One source: the (scaled) copy.
hipError_t launch_fold_segs(const FoldSeg* segs, int nseg, const void* const* stages, int nsrc, int own_pos, int dtype,
                            const Scale& sc, hipStream_t s);

}  // namespace tips
