// reducescatter.hip — the reduce-scatter's kernel: the rank-order fold of nsrc
// sources into a list of output tensors, straight from the peers' staged regions and this rank's own
// input slices, so a grouped reduce-scatter needs neither a pack of the own slices nor an unpack.
//
// Work is cut over the region's byte space, as the segment copy of kernels.hip cuts a bucket: a
// workgroup takes one tile of blockDim x 16 bytes of the region, whatever segments it meets (they
// start 256-B aligned, so 16 lanes always share one), and only the padding between segments is idle.
// The segment records travel with the launch by value, kFoldSegsPerLaunch at a time. A workgroup finds
// the segment of its tile's first byte by a binary search and walks on over the segments that begin
// inside the tile; both loops are workgroup-uniform (scalar loads from the kernel arguments), every
// lane keeps the last record whose offset is not beyond its own vector.
//
// A lane whose 16 bytes lie wholly inside its segment, with `own` and `dst` 16-B aligned, takes the
// vector path: one 16-B non-temporal load per source, all issued before the fold, kernels_device.h's
// fold_first / fold_next / fold_store in between, one sc1 store (the fold's store policy). Every other
// lane - a segment whose own slice or output is not 16-B aligned, which is the usual case for a slice
// of a tensor with an odd row length, and the ragged last < 16 bytes of any segment - folds its up to
// 16 / es elements with fold_elem, the same arithmetic one element at a time. The staged side of a
// segment is 16-B aligned either way.
//
// The source count K is a template parameter for 1 ... 8 sources; 9 ... 16 sources share the K = 16
// instance, whose unrolled loads and fold steps sit behind a workgroup-uniform j < nsrc. One plain
// source is the exact copy (no trip through the working type, which would quiet a signalling NaN).
#include <type_traits>

#include "kernels_device.h"
#include "reducescatter.h"

namespace tips {

int64_t stripe_of(int64_t tile);  // kernels.hip: TIPS_STRIPE_KIB (1 MiB) in tiles of `tile` vectors

namespace {

// (addresses built from integers are cast to the global address space, as kernels.hip:52-57 explains)
typedef __attribute__((address_space(1))) u32x4 g_u32x4;

// the fold's store: sc1, the line leaves the XCD's L2 (kernels.hip's store16_pol<2>)
__device__ __forceinline__ void store16_sc1(int64_t d, u32x4 x) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(reinterpret_cast<g_u32x4*>(d)), "v"(x) : "memory");
}

constexpr int kFoldExact = 8;  // source counts with an instance of their own; beyond: the kMaxSrcs instance

struct FoldBatch {
  FoldSeg seg[kFoldSegsPerLaunch];
  const void* stage[kMaxSrcs];
  int64_t lo;      // the region byte the launch's first tile starts at (the first segment's offset)
  int64_t ntiles;  // tiles of blockDim x 16 bytes from there to the last segment's end
  int64_t stripe;  // stripe_tile's C
  int nseg, nsrc, own_pos;
};

template <class T>
struct is_minmax : std::false_type {};
template <int DT, bool IS_MAX>
struct is_minmax<MinMaxArgs<DT, IS_MAX>> : std::true_type {};

template <int DT, int K, class... SC>
__global__ __launch_bounds__(kBlock) void fold_segs_kernel(FoldBatch B, SC... sc) {
  using Elem = typename ScalarOf<DT>::T;
  constexpr int64_t es = sizeof(Elem);
  constexpr bool kExact = K <= kFoldExact;
  constexpr bool kCopy = K == 1 && sizeof...(SC) == 0;
  const int nsrc = kExact ? K : B.nsrc;
  const int64_t tile_bytes = (int64_t)blockDim.x * 16;
  const int64_t t = stripe_tile(blockIdx.x, gridDim.x, B.stripe);
  if (t >= B.ntiles) return;
  const int64_t t0 = B.lo + t * tile_bytes, t1 = t0 + tile_bytes;
  // the last segment that begins at or before the tile (B.seg[0].off == B.lo <= t0)
  int lo = 0, hi = B.nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (B.seg[mid].off <= t0) lo = mid;
    else hi = mid - 1;
  }
  const int64_t v = t0 + (int64_t)threadIdx.x * 16;  // this lane's 16 bytes of the region
  int64_t own = reinterpret_cast<int64_t>(B.seg[lo].own), dst = reinterpret_cast<int64_t>(B.seg[lo].dst);
  int64_t off = B.seg[lo].off, count = B.seg[lo].count;
  for (int i = lo + 1; i < B.nseg && B.seg[i].off < t1; i++) {
    const bool mine = B.seg[i].off <= v;
    own = mine ? reinterpret_cast<int64_t>(B.seg[i].own) : own;
    dst = mine ? reinterpret_cast<int64_t>(B.seg[i].dst) : dst;
    off = mine ? B.seg[i].off : off;
    count = mine ? B.seg[i].count : count;
  }
  const int64_t b = v - off, bytes = count * es;  // (b >= 0: off <= t0 <= v, or off <= v by the walk)
  if (b >= bytes) return;                         // padding behind the segment
  if (b + 16 <= bytes && ((own | dst) & 15) == 0) {
    u32x4 x[K];
#pragma unroll
    for (int j = 0; j < K; j++)
      if (kExact || j < nsrc) {
        const int64_t a = j == B.own_pos ? own + b : reinterpret_cast<int64_t>(B.stage[j]) + off + b;
        x[j] = __builtin_nontemporal_load(reinterpret_cast<const g_u32x4*>(a));
      }
    if constexpr (kCopy) {
      store16_sc1(dst + b, x[0]);
    } else {
      typename Wide<DT>::A acc = fold_first<DT>(x[0], sc...);
#pragma unroll
      for (int j = 1; j < K; j++)
        if (kExact || j < nsrc) acc = fold_next<DT>(acc, x[j], j, sc...);
      store16_sc1(dst + b, fold_store<DT>(acc, sc...));
    }
  } else {
    const void* src[K];
#pragma unroll
    for (int j = 0; j < K; j++)
      src[j] = j == B.own_pos ? reinterpret_cast<const void*>(own)
                              : reinterpret_cast<const void*>(reinterpret_cast<int64_t>(B.stage[j]) + off);
    const int64_t e0 = b / es;
#pragma unroll
    for (int k = 0; k < (int)(16 / es); k++)
      if (e0 + k < count) {
        if constexpr (kCopy) reinterpret_cast<Elem*>(dst)[e0 + k] = reinterpret_cast<const Elem*>(src[0])[e0 + k];
        else fold_elem<DT>(reinterpret_cast<void*>(dst), src, nsrc, e0 + k, sc...);
      }
  }
}

// The fold's occupancy cap for long regions (kernels.hip's run_multi, measured there): 128 lanes and
// unused LDS reserved per workgroup, 5 workgroups per CU from 6 sources, 8 for 4 and 5.
constexpr int kFoldLdsCap5 = 27648, kFoldLdsCap8 = 20480;
constexpr int64_t kFoldCapBytes = (int64_t)12 << 20;

template <int DT, int K, class... SC>
hipError_t run_batch(const FoldBatch& B, unsigned grid, int block, int lds, hipStream_t s, SC... sc) {
  hipLaunchKernelGGL((fold_segs_kernel<DT, K, SC...>), dim3(grid), dim3(block), lds, s, B, sc...);
  return hipGetLastError();
}

template <int DT, class... SC>
hipError_t run_count(const FoldBatch& B, unsigned grid, int block, int lds, hipStream_t s, SC... sc) {
  switch (B.nsrc) {
    case 1:  // (MAX / MIN of one source is the plain copy: launch_fold_segs never brings it here)
      if constexpr ((is_minmax<SC>::value || ...)) return hipErrorInvalidValue;
      else return run_batch<DT, 1>(B, grid, block, lds, s, sc...);
#define TIPS_FOLD_SEGS_CASE(K) \
  case K: return run_batch<DT, K>(B, grid, block, lds, s, sc...);
      TIPS_FOLD_SEGS_CASE(2) TIPS_FOLD_SEGS_CASE(3) TIPS_FOLD_SEGS_CASE(4) TIPS_FOLD_SEGS_CASE(5)
      TIPS_FOLD_SEGS_CASE(6) TIPS_FOLD_SEGS_CASE(7) TIPS_FOLD_SEGS_CASE(8)
#undef TIPS_FOLD_SEGS_CASE
    default: return run_batch<DT, kMaxSrcs>(B, grid, block, lds, s, sc...);
  }
}

template <int DT>
hipError_t run_op(const FoldBatch& B, unsigned grid, int block, int lds, const Scale& sc, hipStream_t s) {
  if (B.nsrc > 1 && sc.op == kOpMax) return run_count<DT>(B, grid, block, lds, s, MinMaxArgs<DT, true>{});
  if (B.nsrc > 1 && sc.op == kOpMin) return run_count<DT>(B, grid, block, lds, s, MinMaxArgs<DT, false>{});
  if (!sc.on()) return run_count<DT>(B, grid, block, lds, s);
  if constexpr (DT == kI32 || DT == kI64) {
    return hipErrorInvalidValue;
  } else {
    using T = typename WorkOf<DT>::T;  // (the factors' one conversion to the working type; every source is raw)
    return run_count<DT>(B, grid, block, lds, s, ScaleArgs<DT>{(T)sc.pre, (T)sc.post, (1u << B.nsrc) - 1u});
  }
}

}  // namespace

hipError_t launch_fold_segs(const FoldSeg* segs, int nseg, const void* const* stages, int nsrc, int own_pos, int dtype,
                            const Scale& sc, hipStream_t s) {
  const int es = dtype_size(dtype);
  if (nseg < 0 || (nseg > 0 && !segs) || nsrc < 1 || nsrc > kMaxSrcs || own_pos < 0 || own_pos >= nsrc || es == 0 ||
      (nsrc > 1 && !stages))
    return hipErrorInvalidValue;
  if (sc.op != kOpSum && sc.op != kOpMax && sc.op != kOpMin) return hipErrorInvalidValue;
  if (sc.minmax() && sc.on()) return hipErrorInvalidValue;
  FoldBatch B = {};
  for (int j = 0; j < nsrc; j++) B.stage[j] = j == own_pos ? nullptr : stages[j];
  B.nsrc = nsrc;
  B.own_pos = own_pos;
  int i = 0;
  while (i < nseg) {
    B.nseg = 0;
    for (; i < nseg && B.nseg < kFoldSegsPerLaunch; i++)
      if (segs[i].count > 0) B.seg[B.nseg++] = segs[i];
    if (!B.nseg) break;
    B.lo = B.seg[0].off;
    const int64_t span = B.seg[B.nseg - 1].off + B.seg[B.nseg - 1].count * es - B.lo;
    int block = kBlock, lds = 0;
    if (nsrc >= 4 && span > kFoldCapBytes) block = 128, lds = nsrc >= 6 ? kFoldLdsCap5 : kFoldLdsCap8;
    B.ntiles = (span + (int64_t)block * 16 - 1) / ((int64_t)block * 16);
    B.stripe = stripe_of(block);
    const int64_t grid = stripe_grid(B.ntiles, B.stripe);
    if (grid > 0x7fffffff) return hipErrorInvalidValue;
    hipError_t err;
    switch (dtype) {
      case kF32: err = run_op<kF32>(B, (unsigned)grid, block, lds, sc, s); break;
      case kF64: err = run_op<kF64>(B, (unsigned)grid, block, lds, sc, s); break;
      case kI32: err = run_op<kI32>(B, (unsigned)grid, block, lds, sc, s); break;
      case kI64: err = run_op<kI64>(B, (unsigned)grid, block, lds, sc, s); break;
      case kF16: err = run_op<kF16>(B, (unsigned)grid, block, lds, sc, s); break;
      case kBF16: err = run_op<kBF16>(B, (unsigned)grid, block, lds, sc, s); break;
      default: return hipErrorInvalidValue;
    }
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

}  // namespace tips
