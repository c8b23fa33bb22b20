// mxfp8.hip — the MXFP8 wire: block-scaled 8-bit quantise, fold-requantise and dequantise.
// The quantise and the fold each have one device body with two instances: the plain kernel and the
// one with error feedback (defined where the bodies are). Rules 1-3 below are written once.
//
// The operand is the flat f32 layout of a tensor list (fused_layout: tensors at 256-B aligned offsets).
// A block is 32 consecutive flat elements; it never straddles two tensors; positions that hold no
// tensor element count as +0. The wire buffer of E flat elements is E payload bytes (OCP e4m3fn, one
// per element) from byte 0 and one scale byte per block from byte round_up(E, 256).
//
// Quantise, per block x_0 ... x_31:
//   1. any NaN or +-Inf: the block is poisoned - scale byte 0xFF, all 32 payload bytes 0x7F.
//   2. else amax = max |x_j| with biased exponent be and fraction fr: e = max(be, 1) - 127,
//      s = e - 8 + (fr > 0x600000), clamped to [-127, 119], s = -127 for amax == 0; scale byte = s + 127.
//   3. v_j = x_j * 2^-s (one f32 multiply), |v_j| clamped to 448, rounded to nearest even onto the
//      e4m3fn grid, sign kept (-0 -> 0x80). amax * 2^-s <= 448 by the fr rule, so the clamp only binds
//      for amax > 448 * 2^119.
// Dequantise: y = decode(byte) * 2^(scale byte - 127), one IEEE f32 multiply for scale bytes 0 ... 254
// (subnormals honoured, overflow to +-Inf), NaN for scale byte 255 or payload 0x7F / 0xFF; with a
// factor other than 1 one more f32 multiply y * factor. Every NaN is stored as 0x7FC00000.
// Fold of sources 0 ... k-1: each dequantised (factor 1), acc = ((y0 + y1) + y2) + ... as separate f32
// adds, then quantised - a poisoned source block makes acc NaN, a sum that overflows makes it +-Inf,
// and rule 1 poisons the result block.
//
// Which conversions are the hardware's (each compared with the integer restatement over every f32
// input with |v| <= 448 resp. every code and scale byte on an MI355X: no difference):
//   f32 -> e4m3fn, after the multiply and the clamp: v_cvt_pk_fp8_f32;
//   e4m3fn -> f32 of the fold: v_cvt_pk_f32_fp8, then v_mul_f32 by the scale;
//   e4m3fn -> f32 * 2^(scale - 127) of the dequantise: v_cvt_scalef32_pk_f32_fp8.
// v_cvt_scalef32_pk_fp8_f32 is not used: it does not saturate (a quotient above 448 becomes 0x7F)
// and its result under the scale 2^-127 differs from the definition.
//
// The reduce-scatter's fold-dequantise (defined where its kernel is) reads the peers'
// wire bytes and this rank's own f32 slices and writes f32 straight into a list of output tensors.
//
// Launch shapes. Quantise and dequantise: one workgroup of 256 lanes per tile of 4096 flat elements
// of one segment (tensor), 4 rounds of 4 elements per lane - a 16-B load (store) per lane and round
// where the tensor's address is 16-B aligned and the 4 elements lie inside it, element by element
// otherwise, into the same lanes: the same bits. 8 lanes make a block; its maximum takes three
// cross-lane steps inside a row (DPP). Each lane stores its 4 payload bytes as one dword; the block's
// first lane stores the scale byte. Fold: 16 payload bytes per lane and source, two lanes per block.
#include <type_traits>
#include <vector>

#include "kernels_device.h"
#include "mxfp8.h"
#include "reducescatter.h"

namespace tips {

namespace {

constexpr int kMxRounds = 4;
static_assert(kMxTileElems == (int64_t)kBlock * kMxRounds * 4, "a tile is 256 lanes x 4 rounds x 4 elements");
constexpr unsigned kInfBits = 0x7f800000u, kQuietNaN = 0x7fc00000u, kMax448 = 0x43e00000u;

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct MxSegList {
  MxSeg seg[kMxSegsPerLaunch];
  int64_t tile0[kMxSegsPerLaunch + 1];  // the first tile of each segment among the launch's tiles
  int nseg;
};

// max over the 8 lanes of a block (lanes 8k ... 8k + 7 of a row): xor 1, xor 2 inside the quad, then
// the mirrored half row - after the first two steps every lane of a quad holds the quad's maximum
__device__ __forceinline__ unsigned max8(unsigned v) {
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));  // row_half_mirror
  return v;
}
__device__ __forceinline__ unsigned max2(unsigned v) {
  return max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));
}

// scale byte of a block whose largest |x| has the bits `am` (finite)
__device__ __forceinline__ unsigned scale_byte(unsigned am) {
  const int be = (int)(am >> 23);
  int s = max(be, 1) - 127 - 8 + ((am & 0x7fffffu) > 0x600000u ? 1 : 0);
  s = min(max(s, -127), 119);
  return am == 0 ? 0u : (unsigned)(s + 127);
}

// x * 2^-s with |.| clamped to 448, s = sb - 127: the multiplier's biased exponent is 254 - sb (8 ... 254)
__device__ __forceinline__ float scaled_clamped(float x, float mul) {
#pragma clang fp contract(off)
  const unsigned b = __builtin_bit_cast(unsigned, x * mul);
  return __builtin_bit_cast(float, min(b & 0x7fffffffu, kMax448) | (b & 0x80000000u));
}

// 4 elements -> 4 payload bytes (element j in byte j)
__device__ __forceinline__ unsigned encode4(f32x4 x, unsigned sb) {
  const float mul = __builtin_bit_cast(float, (254u - sb) << 23);
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(scaled_clamped(x[0], mul), scaled_clamped(x[1], mul), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(scaled_clamped(x[2], mul), scaled_clamped(x[3], mul), w, true);
  return (unsigned)w;
}

__device__ __forceinline__ unsigned abs_max4(f32x4 x) {
  const u32x4 b = __builtin_bit_cast(u32x4, x) & 0x7fffffffu;
  return max(max(b[0], b[1]), max(b[2], b[3]));
}

// 2^(sb - 127) for sb 0 ... 254 (sb 0: the subnormal 2^-127), NaN for 255
__device__ __forceinline__ float scale_value(unsigned sb) {
  return __builtin_bit_cast(float, sb == 255u ? kQuietNaN : (sb ? (sb << 23) : 0x00400000u));
}

// the segment that tile t of the launch belongs to (MxSegList, MxFoldList)
template <class List>
__device__ __forceinline__ int seg_of_tile(const List& L, int64_t t) {
  int lo = 0, hi = L.nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (L.tile0[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// two payload bytes of a word -> f32 (the hardware's decode), times the block's scale
template <bool HI>
__device__ __forceinline__ f32x2 decode2(unsigned w, float scale) {
#pragma clang fp contract(off)
  return __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI) * scale;
}

// the new residual of 4 elements c whose payload word is w under the scale byte sb (not poisoned)
__device__ __forceinline__ f32x4 residual4(f32x4 c, unsigned w, unsigned sb) {
#pragma clang fp contract(off)
  const float scale = scale_value(sb);
  const f32x2 lo = decode2<false>(w, scale), hi = decode2<true>(w, scale);
  return f32x4{c[0] - lo[0], c[1] - lo[1], c[2] - hi[0], c[3] - hi[1]};
}

// ---- the quantise and the fold: one body each, plain and with error feedback (§17) ----
//
// Error feedback (EF) carries a residual between steps: c = x + r (quantise) or acc + o (fold), one
// f32 add; c is quantised as the plain form quantises x or acc; y = decode(byte) * 2^(scale byte - 127)
// through decode2 (the fold's conversion and multiply); the new residual c - y, one f32 subtract,
// replaces the old one - +0 where the block is poisoned, so that a residual never carries a
// non-finite value. The residual is read once and written once per step and read again only a step
// later, behind every other byte the step moves: the quantise, whose residual accesses are whole
// coalesced lines, makes both sides nontemporal; the fold's are measured (below).

// One tile of the quantise. EF: `residual` is the sender residual, one f32 per flat position (16-B
// aligned; sg.off is a multiple of 64 and i0 of 4, so a lane's 4 residuals are 16-B aligned whatever
// the tensor's own address is); positions that hold no tensor element are neither read nor written.
template <bool EF>
__device__ __forceinline__ void quantize_tile(const MxSegList& L, unsigned char* __restrict__ payload,
                                              unsigned char* __restrict__ scales, float* __restrict__ residual,
                                              int64_t tail_begin, int64_t tail_end) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  if (blockIdx.x == 0)  // the scale bytes behind the last block, up to the buffer's end
    for (int64_t j = tail_begin + tid; j < tail_end; j += kBlock) scales[j] = 0;
  const int64_t t = blockIdx.x;
  const int si = seg_of_tile(L, t);
  const MxSeg sg = L.seg[si];
  const int64_t base = (t - L.tile0[si]) * kMxTileElems;
  const float* src = (const float*)sg.ptr;
  float* res = nullptr;
  if constexpr (EF) res = residual + sg.off;
  const bool vec = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
  f32x4 x[kMxRounds], r[kMxRounds];
  // The two load phases are kept apart on purpose: the feedback form's nesting compiles the plain
  // kernel into a different one (fewer registers, another instruction stream), which is a change
  // to measure on its own.
#pragma unroll
  for (int u = 0; u < kMxRounds; u++) {  // all of the lane's loads before the first use
    const int64_t i0 = base + ((int64_t)u * kBlock + tid) * 4;
    x[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (EF) {
      r[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i0 + 4 <= sg.count) {
        r[u] = __builtin_bit_cast(f32x4, ld16<true>((const u32x4*)(res + i0)));
        if (vec) {
          x[u] = __builtin_bit_cast(f32x4, ld16<true>((const u32x4*)(src + i0)));
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++) x[u][j] = src[i0 + j];
        }
      } else if (i0 < sg.count) {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (i0 + j < sg.count) x[u][j] = src[i0 + j], r[u][j] = res[i0 + j];
      }
    } else {
      if (vec && i0 + 4 <= sg.count) {
        x[u] = __builtin_bit_cast(f32x4, ld16<true>((const u32x4*)(src + i0)));
      } else if (i0 < sg.count) {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (i0 + j < sg.count) x[u][j] = src[i0 + j];
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kMxRounds; u++) {
    const int64_t i0 = base + ((int64_t)u * kBlock + tid) * 4;
    f32x4 c = x[u];
    if constexpr (EF) c = x[u] + r[u];       // (positions without a tensor element: +0 + +0)
    const unsigned am = max8(abs_max4(c));  // (every lane takes part: lanes past the span hold zeros)
    if (i0 >= sg.span) continue;
    const bool poisoned = am >= kInfBits;
    const unsigned sb = poisoned ? 255u : scale_byte(am);
    const unsigned w = poisoned ? 0x7f7f7f7fu : encode4(c, sb);
    *(unsigned*)(payload + sg.off + i0) = w;
    if ((tid & 7) == 0) scales[(sg.off + i0) >> 5] = (unsigned char)sb;
    if constexpr (EF) {
      if (i0 >= sg.count) continue;
      const f32x4 rn = poisoned ? f32x4{0.f, 0.f, 0.f, 0.f} : residual4(c, w, sb);
      if (i0 + 4 <= sg.count) {
        st16<true>((u32x4*)(res + i0), __builtin_bit_cast(u32x4, rn));
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (i0 + j < sg.count) res[i0 + j] = rn[j];
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void mxfp8_quantize_kernel(MxSegList L, unsigned char* __restrict__ payload,
                                                                unsigned char* __restrict__ scales, int64_t tail_begin,
                                                                int64_t tail_end) {
  quantize_tile<false>(L, payload, scales, nullptr, tail_begin, tail_end);
}

__global__ __launch_bounds__(kBlock) void mxfp8_quantize_ef_kernel(MxSegList L, unsigned char* __restrict__ payload,
                                                                   unsigned char* __restrict__ scales,
                                                                   float* __restrict__ residual, int64_t tail_begin,
                                                                   int64_t tail_end) {
  quantize_tile<true>(L, payload, scales, residual, tail_begin, tail_end);
}

// The fold of a lane's 16 elements. EF: `residual` is the owner residual of the range, 32 f32 per
// block from the range's first block (16-B aligned); every position of a block is read and written.
// A lane's 16 residuals are 64 contiguous bytes, so each of its four 16-B accesses touches a quarter
// of every 64 B the wave covers and the four together fill the lines: they are plain loads and
// stores, which lets the caches merge them - measured against the nontemporal forms
// (profiles/mxfp8_ef/README.md: 34 against 48 us over an eighth of 256 MiB, 16 against 22 us on
// config 5's list).
#ifndef TIPS_MXFP8_FOLD_EF_NT_LOAD
#define TIPS_MXFP8_FOLD_EF_NT_LOAD 0
#endif
#ifndef TIPS_MXFP8_FOLD_EF_NT_STORE
#define TIPS_MXFP8_FOLD_EF_NT_STORE 0
#endif
constexpr bool kFoldEfNtLoad = TIPS_MXFP8_FOLD_EF_NT_LOAD, kFoldEfNtStore = TIPS_MXFP8_FOLD_EF_NT_STORE;
template <bool EF>
__device__ __forceinline__ void fold_lane(unsigned char* dst_payload, unsigned char* dst_scales, const MxSrcs& srcs, int nsrc,
                                          int64_t nblocks, float* residual) {
#pragma clang fp contract(off)
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;  // 16 elements each: two lanes per block
  const int64_t blk = g >> 1;
  const bool active = blk < nblocks;
  float acc[16];
  f32x4 o[4];
#pragma unroll
  for (int j = 0; j < 16; j++) acc[j] = 0.f;
#pragma unroll
  for (int q = 0; q < 4; q++) o[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  u32x4* og = nullptr;
  if constexpr (EF) og = (u32x4*)residual + g * 4;
  if (active) {
    u32x4 v = ld16<true>((const u32x4*)srcs.payload[0] + g);
    unsigned sb = srcs.scales[0][blk];
    if constexpr (EF) {
#pragma unroll
      for (int q = 0; q < 4; q++) o[q] = __builtin_bit_cast(f32x4, ld16<kFoldEfNtLoad>(og + q));  // on their way beside source 0
    }
    for (int k = 0; k < nsrc; k++) {
      const u32x4 cur = v;
      const float scale = scale_value(sb);
      if (k + 1 < nsrc) {  // the next source's bytes are on their way while this one is decoded
        v = ld16<true>((const u32x4*)srcs.payload[k + 1] + g);
        sb = srcs.scales[k + 1][blk];
      }
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const f32x2 lo = decode2<false>(cur[q], scale), hi = decode2<true>(cur[q], scale);
        if (k == 0) {
          acc[4 * q] = lo[0], acc[4 * q + 1] = lo[1], acc[4 * q + 2] = hi[0], acc[4 * q + 3] = hi[1];
        } else {
          acc[4 * q] = acc[4 * q] + lo[0];
          acc[4 * q + 1] = acc[4 * q + 1] + lo[1];
          acc[4 * q + 2] = acc[4 * q + 2] + hi[0];
          acc[4 * q + 3] = acc[4 * q + 3] + hi[1];
        }
      }
    }
  }
  f32x4 c[4];
  unsigned am = 0;
  // The two instances write the block maximum differently on purpose (a max of four abs_max4; one
  // running max over the 16 values): either expression in the other instance reorders that kernel's
  // instructions, which is a change to measure on its own.
  if constexpr (EF) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      c[q] = f32x4{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]} + o[q];
      am = max(am, abs_max4(c[q]));
    }
  } else {
#pragma unroll
    for (int j = 0; j < 16; j++) am = max(am, __builtin_bit_cast(unsigned, acc[j]) & 0x7fffffffu);
#pragma unroll
    for (int q = 0; q < 4; q++) c[q] = f32x4{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
  }
  am = max2(am);
  if (!active) return;
  const bool poisoned = am >= kInfBits;
  const unsigned sb = poisoned ? 255u : scale_byte(am);
  u32x4 w;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    w[q] = poisoned ? 0x7f7f7f7fu : encode4(c[q], sb);
    if constexpr (EF) {
      const f32x4 on = poisoned ? f32x4{0.f, 0.f, 0.f, 0.f} : residual4(c[q], w[q], sb);
      st16<kFoldEfNtStore>(og + q, __builtin_bit_cast(u32x4, on));
    }
  }
  st16<false>((u32x4*)dst_payload + g, w);
  if ((g & 1) == 0) dst_scales[blk] = (unsigned char)sb;
}

__global__ __launch_bounds__(kBlock) void mxfp8_fold_kernel(unsigned char* dst_payload, unsigned char* dst_scales,
                                                            MxSrcs srcs, int nsrc, int64_t nblocks) {
  fold_lane<false>(dst_payload, dst_scales, srcs, nsrc, nblocks, nullptr);
}

__global__ __launch_bounds__(kBlock) void mxfp8_fold_ef_kernel(unsigned char* dst_payload, unsigned char* dst_scales,
                                                               MxSrcs srcs, int nsrc, int64_t nblocks,
                                                               float* __restrict__ residual) {
  fold_lane<true>(dst_payload, dst_scales, srcs, nsrc, nblocks, residual);
}

__device__ __forceinline__ float canonical(float y) {
  return y != y ? __builtin_bit_cast(float, kQuietNaN) : y;
}

__global__ __launch_bounds__(kBlock) void mxfp8_dequantize_kernel(MxSegList L, const unsigned char* __restrict__ payload,
                                                                  const unsigned char* __restrict__ scales, float factor,
                                                                  int has_factor) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.x;
  const int si = seg_of_tile(L, t);
  const MxSeg sg = L.seg[si];
  const int64_t base = (t - L.tile0[si]) * kMxTileElems;
  float* dst = (float*)const_cast<void*>(sg.ptr);
  const bool vec = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  unsigned w[kMxRounds], sb[kMxRounds];
#pragma unroll
  for (int u = 0; u < kMxRounds; u++) {
    const int64_t i0 = base + ((int64_t)u * kBlock + tid) * 4;
    w[u] = 0, sb[u] = 0;
    if (i0 < sg.count) {
      w[u] = *(const unsigned*)(payload + sg.off + i0);
      sb[u] = scales[(sg.off + i0) >> 5];
    }
  }
#pragma unroll
  for (int u = 0; u < kMxRounds; u++) {
    const int64_t i0 = base + ((int64_t)u * kBlock + tid) * 4;
    if (i0 >= sg.count) continue;
    const float scale = scale_value(sb[u]);
    const f32x2 lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8((int)w[u], scale, false);
    const f32x2 hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8((int)w[u], scale, true);
    f32x4 y = {lo[0], lo[1], hi[0], hi[1]};
    if (has_factor) y = y * factor;
#pragma unroll
    for (int j = 0; j < 4; j++) y[j] = canonical(y[j]);
    if (vec && i0 + 4 <= sg.count) {
      st16<false>((u32x4*)(dst + i0), __builtin_bit_cast(u32x4, y));
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (i0 + j < sg.count) dst[i0 + j] = y[j];
    }
  }
}

// ---- the reduce-scatter's fold-dequantise ----
//
// mxfp8_dequantize_kernel's launch shape over the output tensors of one region: a workgroup per tile
// of 4096 elements of one segment, 4 rounds of 4 elements per lane. Per round a lane loads its 4 own
// elements (one 16-B nontemporal load where `own` is 16-B aligned and the 4 elements lie inside the
// segment, element by element otherwise) and, per peer, one payload dword and the block's scale byte
// - all before the first add - then folds the sources in ascending order: the own slice raw, a peer
// through the dequantise's conversion (v_cvt_scalef32_pk_f32_fp8). A payload dword of a ragged tail
// reaches up to 3 bytes past the segment's last element: they lie inside the segment's last block,
// which the wire buffer holds whole. Source counts 2 ... 8 have an instance each; 9 ... 16 share the
// K = 16 instance behind a workgroup-uniform j < nsrc. One source never comes here (launch_fold_segs).
struct MxFoldList {
  MxFoldSeg seg[kMxFoldSegsPerLaunch];
  int64_t tile0[kMxFoldSegsPerLaunch + 1];
  MxSrcs srcs;
  int nseg, nsrc, own_pos;
};

constexpr int kMxFoldExact = 8;

template <int K>
__global__ __launch_bounds__(kBlock) void mxfp8_fold_segs_kernel(MxFoldList L, float factor, int has_factor) {
#pragma clang fp contract(off)
  constexpr bool kExact = K <= kMxFoldExact;
  constexpr int kUnroll = kExact ? kMxRounds : 1;
  const int nsrc = kExact ? K : L.nsrc;
  const int own_pos = L.own_pos;
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.x;
  const int si = seg_of_tile(L, t);
  const MxFoldSeg sg = L.seg[si];
  const int64_t base = (t - L.tile0[si]) * kMxTileElems;
  const float* own = (const float*)sg.own;
  float* dst = (float*)sg.dst;
  const bool vec_own = (reinterpret_cast<uintptr_t>(own) & 15) == 0, vec_dst = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  // (the K = 16 instance keeps its rounds apart: unrolled, their loads would take every register)
#pragma unroll kUnroll
  for (int u = 0; u < kMxRounds; u++) {
    const int64_t i0 = base + ((int64_t)u * kBlock + tid) * 4;
    if (i0 >= sg.count) continue;
    const bool full = i0 + 4 <= sg.count;
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (vec_own && full) {
      x = __builtin_bit_cast(f32x4, ld16<true>((const u32x4*)(own + i0)));
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (i0 + j < sg.count) x[j] = own[i0 + j];
    }
    unsigned w[K], sb[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
      w[j] = 0, sb[j] = 0;
      if ((kExact || j < nsrc) && j != own_pos) {
        w[j] = *(const unsigned*)(L.srcs.payload[j] + sg.off + i0);
        sb[j] = L.srcs.scales[j][(sg.off + i0) >> 5];
      }
    }
    f32x4 acc = x;  // (own_pos == 0; otherwise replaced by source 0 below)
#pragma unroll
    for (int j = 0; j < K; j++)
      if (kExact || j < nsrc) {
        f32x4 y = x;
        if (j != own_pos) {
          const float scale = scale_value(sb[j]);
          const f32x2 lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8((int)w[j], scale, false);
          const f32x2 hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8((int)w[j], scale, true);
          y = f32x4{lo[0], lo[1], hi[0], hi[1]};
        }
        acc = j == 0 ? y : acc + y;
      }
    if (has_factor) acc = acc * factor;
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = canonical(acc[j]);
    if (vec_dst && full) {
      st16<false>((u32x4*)(dst + i0), __builtin_bit_cast(u32x4, acc));
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (i0 + j < sg.count) dst[i0 + j] = acc[j];
    }
  }
}

template <int K>
hipError_t run_fold_segs(const MxFoldList& L, unsigned tiles, float factor, hipStream_t s) {
  hipLaunchKernelGGL(mxfp8_fold_segs_kernel<K>, dim3(tiles), dim3(kBlock), 0, s, L, factor, factor != 1.0f ? 1 : 0);
  return hipGetLastError();
}

// The launches of a segment list (L: an MxSegList or an MxFoldList, its other fields set by the
// caller): each launch's list is filled to its capacity with the next segments; cover(segment) is
// the elements a launch covers of it; launch(L, tiles) per part. A segment with nothing to cover
// would be skipped and take no place in a list; every caller passes only segments with something to
// cover, so a list of n segments takes ceil(n / capacity) launches.
template <class List, class Seg, class Cover, class F>
hipError_t for_each_part(List& L, const Seg* segs, int nseg, Cover cover, F launch) {
  constexpr int kCap = (int)std::extent<decltype(L.seg)>::value;
  for (int i = 0; i < nseg;) {
    L.nseg = 0;
    int64_t tiles = 0;
    for (; i < nseg && L.nseg < kCap; i++) {
      const int64_t elems = cover(segs[i]);
      if (elems <= 0) continue;
      L.seg[L.nseg] = segs[i];
      L.tile0[L.nseg++] = tiles;
      tiles += (elems + kMxTileElems - 1) / kMxTileElems;
    }
    if (!L.nseg) break;
    L.tile0[L.nseg] = tiles;
    if (tiles > 0x7fffffff) return hipErrorInvalidValue;
    const hipError_t err = launch(L, (unsigned)tiles);
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

}  // namespace

hipError_t launch_mxfp8_quantize(const MxSeg* segs, int nseg, unsigned char* payload, unsigned char* scales,
                                 float* residual, int64_t tail_begin, int64_t tail_end, hipStream_t s) {
  if (!segs || nseg < 1 || !payload || !scales) return hipErrorInvalidValue;
  MxSegList L;
  return for_each_part(L, segs, nseg, [](const MxSeg& sg) { return sg.span; }, [&](const MxSegList& part, unsigned tiles) {
    if (residual)
      hipLaunchKernelGGL(mxfp8_quantize_ef_kernel, dim3(tiles), dim3(kBlock), 0, s, part, payload, scales, residual,
                         tail_begin, tail_end);
    else
      hipLaunchKernelGGL(mxfp8_quantize_kernel, dim3(tiles), dim3(kBlock), 0, s, part, payload, scales, tail_begin, tail_end);
    tail_begin = tail_end = 0;  // (the first launch zeroes the tail)
    return hipGetLastError();
  });
}

hipError_t launch_mxfp8_fold(unsigned char* dst_payload, unsigned char* dst_scales, const MxSrcs& srcs, int nsrc,
                             int64_t nblocks, float* residual, hipStream_t s) {
  if (!dst_payload || !dst_scales || nsrc < 1 || nsrc > kMxMaxSrcs || nblocks < 0) return hipErrorInvalidValue;
  if (nblocks == 0) return hipSuccess;
  const int64_t grid = (2 * nblocks + kBlock - 1) / kBlock;
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  if (residual)
    hipLaunchKernelGGL(mxfp8_fold_ef_kernel, dim3((unsigned)grid), dim3(kBlock), 0, s, dst_payload, dst_scales, srcs, nsrc,
                       nblocks, residual);
  else
    hipLaunchKernelGGL(mxfp8_fold_kernel, dim3((unsigned)grid), dim3(kBlock), 0, s, dst_payload, dst_scales, srcs, nsrc,
                       nblocks);
  return hipGetLastError();
}

hipError_t launch_mxfp8_dequantize(const MxSeg* segs, int nseg, const unsigned char* payload, const unsigned char* scales,
                                   float factor, hipStream_t s) {
  if (!segs || nseg < 1 || !payload || !scales) return hipErrorInvalidValue;
  MxSegList L;
  return for_each_part(L, segs, nseg, [](const MxSeg& sg) { return sg.count; }, [&](const MxSegList& part, unsigned tiles) {
    hipLaunchKernelGGL(mxfp8_dequantize_kernel, dim3(tiles), dim3(kBlock), 0, s, part, payload, scales, factor,
                       factor != 1.0f ? 1 : 0);
    return hipGetLastError();
  });
}

hipError_t launch_mxfp8_fold_segs(const MxFoldSeg* segs, int nseg, const MxSrcs& wires, int nsrc, int own_pos, float factor,
                                  hipStream_t s) {
  if (nseg < 0 || (nseg > 0 && !segs) || nsrc < 1 || nsrc > kMxMaxSrcs || own_pos < 0 || own_pos >= nsrc)
    return hipErrorInvalidValue;
  if (nsrc == 1) {  // no peer, nothing quantised: the reduce-scatter's one-source fold, the (scaled) copy
    std::vector<FoldSeg> plain;
    for (int i = 0; i < nseg; i++)
      if (segs[i].count > 0) plain.push_back(FoldSeg{segs[i].own, segs[i].dst, segs[i].off * 4, segs[i].count});
    Scale sc;
    sc.post = factor;
    return launch_fold_segs(plain.data(), (int)plain.size(), nullptr, 1, 0, kF32, sc, s);
  }
  MxFoldList L;
  L.srcs = wires;
  L.nsrc = nsrc;
  L.own_pos = own_pos;
  return for_each_part(L, segs, nseg, [](const MxFoldSeg& sg) { return sg.count; }, [&](const MxFoldList& part, unsigned tiles) {
    switch (nsrc) {
#define TIPS_MX_FOLD_SEGS_CASE(K) \
  case K: return run_fold_segs<K>(part, tiles, factor, s);
      TIPS_MX_FOLD_SEGS_CASE(2) TIPS_MX_FOLD_SEGS_CASE(3) TIPS_MX_FOLD_SEGS_CASE(4) TIPS_MX_FOLD_SEGS_CASE(5)
      TIPS_MX_FOLD_SEGS_CASE(6) TIPS_MX_FOLD_SEGS_CASE(7) TIPS_MX_FOLD_SEGS_CASE(8)
#undef TIPS_MX_FOLD_SEGS_CASE
      default: return run_fold_segs<kMxMaxSrcs>(part, tiles, factor, s);
    }
  });
}

}  // namespace tips
