// kernels.h — launchers for the gfx950 kernels of the bucket-reduction path.
// Internal to libtips_hip.so (not part of the C-ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace tips {

int dtype_size(int dtype);  // 0 for unknown dtypes

// dst = a + b, elementwise (the per-chunk MPI_SUM step).
hipError_t launch_sum2(void* dst, const void* a, const void* b, int64_t n, int dtype, hipStream_t s);

// dst = rank-order fold of srcs[0..nsrc), nsrc <= kMaxSrcs.
constexpr int kMaxSrcs = 16;
hipError_t launch_multi_sum(void* dst, const void* const* srcs, int nsrc, int64_t n, int dtype, hipStream_t s);
// The same fold when most sources are peers' memory read over xGMI (the peer schedule's pull-fold,
// peer.cc): remote loads take microseconds, so every lane keeps 4 x 16 B per source in flight
// (256 lanes, 16 KiB per source per workgroup, no occupancy cap). Same bits as launch_multi_sum.
hipError_t launch_multi_sum_remote(void* dst, const void* const* srcs, int nsrc, int64_t n, int dtype, hipStream_t s);

// MAX / MIN (DESIGN.md §MAX and MIN): the same launches with the add replaced by an exact compare in
// the storage type - signed for the integers, IEEE 754-2019 maximum / minimum for the floats (a NaN
// operand gives a NaN, -0 < +0, subnormals kept). op: the C-ABI's tips_op values; kOpSum forwards to
// launch_sum2 / launch_multi_sum. One source is the copy, as in launch_multi_sum.
enum { kOpSum = 0, kOpMax = 1, kOpMin = 2 };
hipError_t launch_reduce2(void* dst, const void* a, const void* b, int64_t n, int dtype, int op, hipStream_t s);
hipError_t launch_multi_reduce(void* dst, const void* const* srcs, int nsrc, int64_t n, int dtype, int op, hipStream_t s);

// Scaled forms (float dtypes; DESIGN.md §Scaled allreduce): result = post * SUM (pre * x), in the
// working type (fp32 for f32 / f16 / bf16, f64 for f64), every multiply and add a separate IEEE
// operation, one rounding at the store. Bit j of `raw` marks source j as a rank's raw input, to be
// multiplied by pre where it is read; the other sources are partial sums that already carry it. The
// launch shapes are those of launch_sum2 / launch_multi_sum / launch_copy_buf; with nothing to scale
// (pre == 1 or no raw source, and post == 1) they are those launchers.
// The struct also carries the call's reduction op down the schedules (kOpSum unless the call is
// tips_allreduce_op's MAX / MIN, which never comes with factors).
struct Scale {
  double pre = 1.0, post = 1.0;
  int op = kOpSum;
  bool on() const { return pre != 1.0 || post != 1.0; }
  bool minmax() const { return op != kOpSum; }
  bool plain() const { return !on() && !minmax(); }  // the unscaled SUM: what a graph may capture
};
hipError_t launch_sum2_scaled(void* dst, const void* a, const void* b, int64_t n, int dtype, double pre, double post,
                              unsigned raw, hipStream_t s);
hipError_t launch_multi_sum_scaled(void* dst, const void* const* srcs, int nsrc, int64_t n, int dtype, double pre,
                                   double post, unsigned raw, hipStream_t s);
// dst = (src * pre) * post over n elements, in place allowed (tips_scale; the scaled allreduce at one rank).
hipError_t launch_scale_buf(void* dst, const void* src, int64_t n, int dtype, double pre, double post, hipStream_t s);

// Segment copy over a virtual byte space (fusion pack / unpack / identity copy, fusion.cc): tensor
// k occupies virtual bytes [begin, end) and byte v of it lives at src + v on the source side and
// dst + v on the destination side. Tiles of tile_bytes (4, 8 or 16 KiB) are cut from the virtual
// space; tiles[2t], tiles[2t + 1] (two per tile of the whole space) are the records of the one or
// two segments tile t meets (the second {0,0,0,0} when one), or {first segment, number of segments,
// -, -1} when it meets more (then read from segs[]).
// Segments begin 256-B aligned and in order. One launch copies tiles [tile0, tile0 + ntiles).
// pol = store cache policy: 0 plain, 1 nt, 2 sc1.
struct CopySeg {
  int64_t src, dst;  // addresses of virtual byte 0 (as integers: src + v = the byte's address)
  int64_t begin, end;
};
hipError_t launch_copy_segs(const CopySeg* tiles, const CopySeg* segs, int tile0, int ntiles, int64_t tile_bytes,
                            int pol, hipStream_t s);
// The pack launch's workgroup -> slot map: 1 MiB-style XCD stripes of this many 16-B vectors
// (TIPS_PACK_STRIPE_KIB; 0, the default, = one contiguous eighth of the slots per XCD), and the
// XCD / issue position of every slot under it (fusion.cc's tile_order places boundary tiles by it).
int64_t pack_stripe_vecs();
void stripe_slots(int64_t nslots, int64_t C, std::vector<int>* xcd, std::vector<int64_t>* pos);

// Several tile groups (a step's fusion buckets) in one launch: group k copies record slots
// [tile0[k], tile0[k] + ntiles[k]) with workgroups [blk0[k], blk0[k + 1]) (the launcher fills blk0).
// done[k] != null: when group k is complete its last workgroup stores sig_value[k] into *done[k]
// (signal memory: another stream waits for it with hipStreamWaitValue64); counters[k] (device
// memory, zero before the first launch) count the group's workgroups and are left at zero.
constexpr int kMaxPackGroups = 8;
struct PackGroups {
  int n;
  int tile0[kMaxPackGroups], ntiles[kMaxPackGroups];
  unsigned blk0[kMaxPackGroups + 1];
  unsigned* counters;
  unsigned long long* done[kMaxPackGroups];
  unsigned long long sig_value[kMaxPackGroups];
};
hipError_t launch_copy_segs_groups(const CopySeg* tiles, const CopySeg* segs, PackGroups g, int64_t tile_bytes, int pol,
                                   hipStream_t s);

// The segment copy with a cast (fused Compression.fp16): the byte space is the wire type's (wire =
// f16 or bf16 dtype code); the f32 side of a segment is at its record's address + 2 v. dir 0: pack
// (f32 -> wire, round to nearest even), dir 1: unpack (wire -> f32). And one contiguous range cast.
hipError_t launch_cast_segs(const CopySeg* tiles, const CopySeg* segs, int tile0, int ntiles, int64_t tile_bytes,
                            int dir, int wire, hipStream_t s);
hipError_t launch_cast_range(void* dst, const void* src, int64_t n, int dir, int wire, hipStream_t s);

// One contiguous device-to-device copy of `bytes` (tips_allreduce / tips_broadcast at one rank, out
// of place): copy_buf_kernel when both pointers are 16-B aligned, else hipMemcpyAsync.
hipError_t launch_copy_buf(void* dst, const void* src, int64_t bytes, hipStream_t s);

// Peer transfers of the xGMI peer schedule (peer.cc): up to kMaxXferSegs byte
// segments {src, dst, bytes} copied by one launch, segments interleaved over
// the workgroups so every xGMI link carries traffic at once. src/dst may be
// IPC-mapped peer memory. Passed by value (kernel argument), no descriptor upload.
struct XferSeg {
  const char* src;
  char* dst;
  int64_t bytes;
};
constexpr int kMaxXferSegs = 16;
constexpr int64_t kXferTileBytes = 16 * 1024;  // per workgroup: 256 lanes x 4 x 16 B
hipError_t launch_xfer(const XferSeg* segs, int nseg, hipStream_t s);

}  // namespace tips
