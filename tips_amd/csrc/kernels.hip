// kernels.hip — gfx950 (CDNA4) kernels of the gradient-bucket reduction path.
//
// What they replace: the local MPI_SUM reduction libmpi runs on every
// received chunk inside MPI_Allreduce, reached from AllreduceCpu<T>
// (reference tips/core/collective/utils.h:60-65, op from utils.cc:6-16).
//
// Design: the add is memory-bound — 1 flop per 12 B for
// f32 — so there is no MFMA and no LDS round trip; every lane moves 16 B per
// load/store (buffer_load_dwordx4 / buffer_store_dwordx4: one wave touches
// 1 KiB contiguous), every lane's loads are issued before its first add, and
// the grid covers the bucket one tile per workgroup, the tiles dealt to the 8
// XCDs in stripes. Elements that do
// not fill a 16-B vector (the "tail", < 8 elements) are done scalar by
// workgroup 0. Integer adds wrap (two's complement, as MPI_SUM on MPI_INT /
// MPI_LONG_LONG); f16 adds are v_pk_add_f16 (correctly rounded, = fp32 add
// rounded to half); bf16 adds in fp32 and rounds to nearest-even.
//
// This file is what libtips_hip.so launches; kernels_device.h has the sum, fold and copy kernel
// templates and the device helpers, kernels_dev.hip what only the tuning sweeps run.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "kernels_device.h"

namespace tips {

int dtype_size(int dtype) {
  switch (dtype) {
    case kF32: return 4;
    case kF64: return 8;
    case kI32: return 4;
    case kI64: return 8;
    case kF16: return 2;
    case kBF16: return 2;
    default: return 0;
  }
}

// ---------------------------------------------------------------------------
// Segment copy (fusion pack / unpack / identity copy since round 3; fusion.cc)
//
// Tiles are cut from a virtual byte space (a fusion bucket, or the flat layout of a whole tensor
// list), not per tensor: every workgroup moves T = 4 KiB x U bytes of the space, whatever tensors
// it meets; only the padding between tensors (< 256 B each) is skipped. The round-2 kernel cut
// tiles per tensor, so ~75 % of config 4's 1000 tensors ended in a partly empty workgroup, and
// moved a tile's last < 16 bytes one byte per lane. Tensors begin 256-B aligned in the space, so a
// tile meets at most T / 256 + 1 segments: the workgroup stages them in LDS (one load per lane,
// one barrier), each lane finds the segment of each of its 16-B vectors by binary search, issues
// all its nt loads, then its stores. A vector at a tensor's ragged end, or of a tensor that is not
// 16-B aligned, moves as dwords (shorts for 2-B element types) - one lane per tensor end.
// (The addresses are built from integers, so they are cast to the global address space: a generic
// pointer makes the compiler emit flat_load / flat_store, which also count against lgkmcnt.)
typedef __attribute__((address_space(1))) u32x4 g_u32x4;
typedef __attribute__((address_space(1))) unsigned g_u32;
typedef __attribute__((address_space(1))) unsigned short g_u16;
typedef __attribute__((address_space(1))) char g_u8;

template <int POL>
__device__ __forceinline__ void store16_pol(int64_t d, u32x4 x) {
  if constexpr (POL == 0) {
    *reinterpret_cast<g_u32x4*>(d) = x;
  } else if constexpr (POL == 1) {
    __builtin_nontemporal_store(x, reinterpret_cast<g_u32x4*>(d));
  } else {  // sc1: the line leaves the XCD's L2 (a vector store; the asm ends with the store's 2 wait states)
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(reinterpret_cast<g_u32x4*>(d)), "v"(x)
                 : "memory");
  }
}

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) u32x2 g_u32x2;

// the 8-B form (the wire side of the cast kernels: 4 half-width elements per lane)
__device__ __forceinline__ void store8_sc1(int64_t d, u32x2 x) {
  asm volatile("global_store_dwordx2 %0, %1, off sc1\n\ts_nop 1" ::"v"(reinterpret_cast<g_u32x2*>(d)), "v"(x)
               : "memory");
}

// The < 16 bytes of a vector at a tensor's ragged end, or a whole vector of a tensor that is not
// 16-B aligned: loaded as dwords (shorts when the tensor's offset or length is only 2-B aligned,
// 16-bit types) - phase 1 issues the loads, phase 2 the stores, so a lane waits for memory once.
struct Small {
  unsigned w[4];
  unsigned short h[8];
};

__device__ __forceinline__ void small_load(int64_t s, int64_t d, int len, Small& m) {
  if (((s | d | (int64_t)len) & 3) == 0) {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (4 * k < len) m.w[k] = *reinterpret_cast<const g_u32*>(s + 4 * k);
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (2 * k < len) m.h[k] = *reinterpret_cast<const g_u16*>(s + 2 * k);
  }
}

__device__ __forceinline__ void small_store(int64_t s, int64_t d, int len, const Small& m) {
  if (((s | d | (int64_t)len) & 3) == 0) {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (4 * k < len) *reinterpret_cast<g_u32*>(d + 4 * k) = m.w[k];
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (2 * k < len) *reinterpret_cast<g_u16*>(d + 2 * k) = m.h[k];
  }
}

// tiles[2t], tiles[2t + 1] (record slot t of the launch; fusion.cc puts a group's boundary tiles
// first): the tile's segment and {0, 0, tile byte, 0}; or its two segments (the tensor ending in
// it, the tensor starting in it); or {first segment, count, -, -1} and {0, 0, tile byte, 0} when
// it meets more than two (then staged from segs[] in LDS).
template <int U>
struct SegStage {  // a multi-segment tile's records, staged in LDS
  CopySeg L[(int)((int64_t)kBlock * 16 * U / 256) + 1];
};

// One tile of the segment copy: record slot t. Called by whole workgroups (the multi-segment
// branch has a barrier; every branch to it is workgroup-uniform).
template <int U, int POL>
__device__ __forceinline__ void copy_seg_tile(const CopySeg* __restrict__ tiles, const CopySeg* __restrict__ segs,
                                              int t, CopySeg* L) {
  constexpr int64_t kTileBytes = (int64_t)kBlock * 16 * U;
  constexpr int kMaxSeg = (int)(kTileBytes / 256) + 1;
  // One (scalar) load of both records before the first data load. (A tile -> segment index
  // followed by the segment's record puts two dependent loads there: 17.5 against 14.1 us per
  // config-4 bucket, measured.)
  // (field by field: a record selected as a whole per lane becomes a private-memory copy)
  const int64_t* tr = reinterpret_cast<const int64_t*>(tiles + 2 * (int64_t)t);
  const int64_t a_src = tr[0], a_dst = tr[1], a_beg = tr[2], a_end = tr[3];
  const int64_t b_src = tr[4], b_dst = tr[5], b_beg = tr[6], b_end = tr[7];
  const int tid = threadIdx.x;
  const bool multi = a_end < 0, two = b_end > 0;
  // the tile's first byte: the second record's begin, rounded down to the tile when that record is
  // the segment starting inside the tile
  const int64_t tb = two ? (b_beg & ~(kTileBytes - 1)) : b_beg;
  if (!multi && !two && a_beg <= tb && a_end >= tb + kTileBytes && ((a_src | a_dst) & 15) == 0) {
    // the tile lies inside one 16-B aligned tensor (most tiles): both sides are wave-uniform
    // contiguous ranges, moved as the round-2 kernel moved a whole tile - buffer loads nt, buffer
    // stores with the policy's cache bits, each store behind its own load
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(a_src + tb), (short)0, (int)kTileBytes,
                                                                  0x00020000);
    __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(a_dst + tb), (short)0, (int)kTileBytes,
                                                                  0x00020000);
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, (u * kBlock + tid) * 16, 0, 2);
#pragma unroll
    for (int u = 0; u < U; u++)
      __builtin_amdgcn_raw_buffer_store_b128(v[u], rd, (u * kBlock + tid) * 16, 0, POL == 0 ? 0 : POL == 1 ? 2 : 16);
    return;
  }
  int cnt = 1;
  if (multi) {  // workgroup-uniform branch
    const int s0 = (int)a_src;
    cnt = min((int)a_dst, kMaxSeg);
    if (cnt <= 0) return;  // (uniform: no segment meets this tile)
    if (tid < cnt) L[tid] = segs[s0 + tid];
    __syncthreads();
  }
  int64_t sp[U], dp[U];
  int len[U];
  bool full[U];
  u32x4 x[U];
  Small m[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int64_t v = tb + (int64_t)u * (kBlock * 16) + (int64_t)tid * 16;
    int64_t g_src, g_dst, g_beg, g_end;
    if (multi) {
      int lo = 0, hi = cnt - 1;  // the last segment beginning at or before v
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (L[mid].begin <= v) lo = mid;
        else hi = mid - 1;
      }
      g_src = L[lo].src;
      g_dst = L[lo].dst;
      g_beg = L[lo].begin;
      g_end = L[lo].end;
    } else {
      const bool b = two && v >= b_beg;
      g_src = b ? b_src : a_src;
      g_dst = b ? b_dst : a_dst;
      g_beg = b ? b_beg : a_beg;
      g_end = b ? b_end : a_end;
    }
    const int64_t left = g_end - v;
    len[u] = (v >= g_beg && left > 0) ? (int)(left < 16 ? left : 16) : 0;
    sp[u] = g_src + v;
    dp[u] = g_dst + v;
    full[u] = len[u] == 16 && ((sp[u] | dp[u]) & 15) == 0;
    if (full[u]) x[u] = __builtin_nontemporal_load(reinterpret_cast<const g_u32x4*>(sp[u]));
    else if (len[u] > 0) small_load(sp[u], dp[u], len[u], m[u]);
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    if (full[u]) store16_pol<POL>(dp[u], x[u]);
    else if (len[u] > 0) small_store(sp[u], dp[u], len[u], m[u]);
  }
}

template <int U, int POL>
__global__ __launch_bounds__(kBlock) void copy_segs_kernel(const CopySeg* __restrict__ tiles,
                                                          const CopySeg* __restrict__ segs, int tile0, int ntiles,
                                                          int64_t stripe) {
  __shared__ SegStage<U> st;
  const int64_t tt = stripe_tile(blockIdx.x, gridDim.x, stripe);
  if (tt >= ntiles) return;  // (whole workgroup: before any barrier)
  copy_seg_tile<U, POL>(tiles, segs, tile0 + (int)tt, st.L);  // (fusion.cc may order a group's tiles: slow ones first)
}

// ---------------------------------------------------------------------------
// Fusion pack / unpack with a cast (Compression.fp16 fused into the buckets):
// the layout's byte space is the WIRE type's (f16 or bf16, 2 B per element); the f32 side of a
// segment lives at base + 2 v for virtual byte v (fusion.cc's kSlotCast records). DIR 0 (pack):
// f32 source -> wire destination, RNE as oracle_float_to_half / oracle_float_to_bf16 (the
// reference's tf.cast, compression.py:49-66); DIR 1 (unpack): wire source -> f32 destination, exact.
// A lane moves quads: 4 elements = 16 B of f32 and 8 B of the wire type, so every access of a
// wave is one contiguous run (1 KiB of f32, 512 B of wire). (Round 6's first form moved 8 elements
// per lane as one 16-B wire vector and two 16-B f32 accesses 32 B apart: each f32 instruction then
// touched every other 16 B of a 2 KiB span, and config 5's round trip ran at 0.44 of HBM, the
// unpack at 0.37; profiles/r06/cast_probe_*.)

template <int WT>
__device__ __forceinline__ u32x2 narrow4(f32x4 a) {
  if constexpr (WT == kF16) {
    return __builtin_bit_cast(u32x2, __builtin_convertvector(a, f16x4));
  } else {  // bf16: word i = elements 2i (low half) and 2i + 1 (high half)
    const u32x4 x = __builtin_bit_cast(u32x4, a);
    return u32x2{bf16_round_bits(x[0]) | (bf16_round_bits(x[1]) << 16), bf16_round_bits(x[2]) | (bf16_round_bits(x[3]) << 16)};
  }
}

template <int WT>
__device__ __forceinline__ f32x4 widen4(u32x2 v) {
  if constexpr (WT == kF16) return __builtin_convertvector(__builtin_bit_cast(f16x4, v), f32x4);
  else return __builtin_bit_cast(f32x4, u32x4{v[0] << 16, v[0] & 0xffff0000u, v[1] << 16, v[1] & 0xffff0000u});
}

template <int WT>
__device__ __forceinline__ unsigned short narrow1(float f) {
  if constexpr (WT == kF16) return __builtin_bit_cast(unsigned short, (_Float16)f);
  else return (unsigned short)bf16_round_bits(__builtin_bit_cast(unsigned, f));
}

template <int WT>
__device__ __forceinline__ float widen1(unsigned short h) {
  if constexpr (WT == kF16) return (float)__builtin_bit_cast(_Float16, h);
  else return __builtin_bit_cast(float, (unsigned)h << 16);
}

typedef __attribute__((address_space(1))) f32x4 g_f32x4;
typedef __attribute__((address_space(1))) float g_f32;

// One whole tile of kBlock * 16 * U wire bytes, both sides 16-B aligned, moved 16 B per lane on
// both sides: the quads (16 B of f32 = 8 B of wire) are reordered through LDS, so the wire side is
// read or written as 16-B vectors too (8-B-per-lane wire accesses ran the round trip 10 % slower:
// profiles/r06/cast/). Called by whole workgroups; W holds 2 U quads per lane.
template <int U, int DIR, int WT>
__device__ __forceinline__ void cast_tile_staged(int64_t f32_base, int64_t wire_base, u32x2* W) {
  const int tid = threadIdx.x;
  if constexpr (DIR == 0) {
    f32x4 x[2 * U];
#pragma unroll
    for (int u = 0; u < 2 * U; u++)
      x[u] = __builtin_nontemporal_load(reinterpret_cast<const g_f32x4*>(f32_base + 16 * (int64_t)(u * kBlock + tid)));
#pragma unroll
    for (int u = 0; u < 2 * U; u++) W[u * kBlock + tid] = narrow4<WT>(x[u]);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; u++)
      store16_pol<2>(wire_base + 16 * (int64_t)(u * kBlock + tid), reinterpret_cast<const u32x4*>(W)[u * kBlock + tid]);
  } else {
    u32x4 x[U];
#pragma unroll
    for (int u = 0; u < U; u++)
      x[u] = __builtin_nontemporal_load(reinterpret_cast<const g_u32x4*>(wire_base + 16 * (int64_t)(u * kBlock + tid)));
#pragma unroll
    for (int u = 0; u < U; u++) reinterpret_cast<u32x4*>(W)[u * kBlock + tid] = x[u];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2 * U; u++)
      store16_pol<2>(f32_base + 16 * (int64_t)(u * kBlock + tid), __builtin_bit_cast(u32x4, widen4<WT>(W[u * kBlock + tid])));
  }
}

// VAR (sweeps, TIPS_CAST_VARIANT): bit 0 plain loads instead of nt; bits 1-2 the store policy
// (0 = sc1, the default; 1 = plain; 2 = nt); bit 3 (the default) one-segment tiles staged in LDS
// (cast_tile_staged); the other tiles move quads (staging the two-segment and ragged tiles
// as well was measured no faster on config 4's 1000 tensors: 49.41 vs 49.44 us per round trip)
template <int U, int DIR, int WT, int VAR = 8>
__global__ __launch_bounds__(kBlock) void cast_segs_kernel(const CopySeg* __restrict__ tiles,
                                                          const CopySeg* __restrict__ segs, int tile0, int ntiles) {
  constexpr int64_t kTileBytes = (int64_t)kBlock * 16 * U;  // wire bytes
  constexpr int kMaxSeg = (int)(kTileBytes / 256) + 1;
  constexpr int Q = 2 * U;  // quads per lane
  __shared__ CopySeg L[kMaxSeg];
  const int64_t tt = xcd_tile(blockIdx.x, gridDim.x);
  if (tt >= ntiles) return;  // (whole workgroup: before any barrier)
  const int64_t* tr = reinterpret_cast<const int64_t*>(tiles + 2 * (int64_t)(tile0 + tt));
  const int64_t a_src = tr[0], a_dst = tr[1], a_beg = tr[2], a_end = tr[3];
  const int64_t b_src = tr[4], b_dst = tr[5], b_beg = tr[6], b_end = tr[7];
  const int tid = threadIdx.x;
  const bool multi = a_end < 0, two = b_end > 0;
  const int64_t tb = two ? (b_beg & ~(kTileBytes - 1)) : b_beg;
  if constexpr ((VAR & 8) != 0) {
    // (bit 3, the default) a tile inside one segment with both sides 16-B aligned (workgroup-uniform)
    __shared__ u32x2 W[kBlock * Q];
    if (!multi && !two && a_beg <= tb && a_end >= tb + kTileBytes && ((a_src | a_dst) & 15) == 0) {
      if constexpr (DIR == 0) cast_tile_staged<U, 0, WT>(a_src + 2 * tb, a_dst + tb, W);
      else cast_tile_staged<U, 1, WT>(a_dst + 2 * tb, a_src + tb, W);
      return;
    }
  }
  int cnt = 1;
  if (multi) {  // workgroup-uniform branch
    cnt = min((int)a_dst, kMaxSeg);
    if (cnt <= 0) return;
    if (tid < cnt) L[tid] = segs[(int)a_src + tid];
    __syncthreads();
  }
  int64_t sp[Q], dp[Q];
  int len[Q];  // wire bytes of this quad inside its segment (8 = all four elements)
  bool full[Q];
  u32x2 nv[Q];  // unpack: the loaded wire quad
  f32x4 wa[Q];  // pack: the loaded f32 quad
#pragma unroll
  for (int u = 0; u < Q; u++) {
    const int64_t v = tb + (int64_t)u * (kBlock * 8) + (int64_t)tid * 8;
    int64_t g_src, g_dst, g_beg, g_end;
    if (multi) {
      int lo = 0, hi = cnt - 1;  // the last segment beginning at or before v
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (L[mid].begin <= v) lo = mid;
        else hi = mid - 1;
      }
      g_src = L[lo].src;
      g_dst = L[lo].dst;
      g_beg = L[lo].begin;
      g_end = L[lo].end;
    } else {
      const bool b = two && v >= b_beg;
      g_src = b ? b_src : a_src;
      g_dst = b ? b_dst : a_dst;
      g_beg = b ? b_beg : a_beg;
      g_end = b ? b_end : a_end;
    }
    const int64_t left = g_end - v;
    len[u] = (v >= g_beg && left > 0) ? (int)(left < 8 ? left : 8) : 0;
    sp[u] = g_src + (DIR == 0 ? 2 * v : v);  // the f32 side at base + 2 v
    dp[u] = g_dst + (DIR == 0 ? v : 2 * v);
    const int64_t f32_side = DIR == 0 ? sp[u] : dp[u], wire_side = DIR == 0 ? dp[u] : sp[u];
    full[u] = len[u] == 8 && (f32_side & 15) == 0 && (wire_side & 7) == 0;
    if (full[u]) {
      if constexpr (DIR == 0) wa[u] = (VAR & 1) ? *reinterpret_cast<const g_f32x4*>(sp[u])
                                                : __builtin_nontemporal_load(reinterpret_cast<const g_f32x4*>(sp[u]));
      else nv[u] = (VAR & 1) ? *reinterpret_cast<const g_u32x2*>(sp[u])
                             : __builtin_nontemporal_load(reinterpret_cast<const g_u32x2*>(sp[u]));
    }
  }
  constexpr int kStore = (VAR >> 1) & 3;
#pragma unroll
  for (int u = 0; u < Q; u++) {
    if (full[u]) {
      if constexpr (DIR == 0) {
        const u32x2 w = narrow4<WT>(wa[u]);
        if constexpr (kStore == 0) store8_sc1(dp[u], w);
        else if constexpr (kStore == 1) *reinterpret_cast<g_u32x2*>(dp[u]) = w;
        else __builtin_nontemporal_store(w, reinterpret_cast<g_u32x2*>(dp[u]));
      } else {
        store16_pol<kStore == 0 ? 2 : kStore == 1 ? 0 : 1>(dp[u], __builtin_bit_cast(u32x4, widen4<WT>(nv[u])));
      }
    } else {
      for (int e = 0; 2 * e < len[u]; e++) {  // a tensor's ragged end, or a side not aligned
        if constexpr (DIR == 0)
          *reinterpret_cast<g_u16*>(dp[u] + 2 * e) = narrow1<WT>(*reinterpret_cast<const g_f32*>(sp[u] + 4 * e));
        else
          *reinterpret_cast<g_f32*>(dp[u] + 4 * e) = widen1<WT>(*reinterpret_cast<const g_u16*>(sp[u] + 2 * e));
      }
    }
  }
}

// Cast of one contiguous range (a fused list's tensors of at least the threshold, which travel
// through a scratch buffer of the wire type): DIR 0 f32 -> wire, 1 wire -> f32. With both sides
// 16-B aligned, whole 8 KiB wire tiles go through cast_tile_staged (grid-stride over tiles), the
// rest in quads (16 B of f32, 8 B of wire per lane) and the last n % 4 elements one at a time; a
// misaligned range element by element.
template <int DIR, int WT>
__global__ __launch_bounds__(kBlock) void cast_range_kernel(void* __restrict__ dst, const void* __restrict__ src,
                                                           int64_t n) {
  constexpr int U = 2;
  constexpr int64_t kTileElems = (int64_t)kBlock * 8 * U;
  __shared__ u32x2 W[kBlock * 2 * U];
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t f32_side = (int64_t)(DIR == 0 ? src : dst), wire_side = (int64_t)(DIR == 0 ? dst : src);
  int64_t head = 0;
  if (((f32_side | wire_side) & 15) == 0) {
    const int64_t nt = n / kTileElems;
    for (int64_t t = blockIdx.x; t < nt; t += gridDim.x) {  // (workgroup-uniform trip count)
      cast_tile_staged<U, DIR, WT>(f32_side + 4 * t * kTileElems, wire_side + 2 * t * kTileElems, W);
      __syncthreads();  // (every lane's LDS reads before the next tile's writes)
    }
    head = nt * kTileElems;
  }
  if ((f32_side & 15) == 0 && (wire_side & 7) == 0) {
    const int64_t nq = n / 4;
    for (int64_t q = head / 4 + (int64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += stride) {
      if constexpr (DIR == 0)
        store8_sc1(wire_side + 8 * q, narrow4<WT>(__builtin_nontemporal_load(reinterpret_cast<const g_f32x4*>(f32_side + 16 * q))));
      else
        store16_pol<2>(f32_side + 16 * q, __builtin_bit_cast(u32x4, widen4<WT>(
                                              __builtin_nontemporal_load(reinterpret_cast<const g_u32x2*>(wire_side + 8 * q)))));
    }
    head = 4 * nq;
  }
  for (int64_t i = head + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    if constexpr (DIR == 0) static_cast<unsigned short*>(dst)[i] = narrow1<WT>(static_cast<const float*>(src)[i]);
    else static_cast<float*>(dst)[i] = widen1<WT>(static_cast<const unsigned short*>(src)[i]);
  }
}

// Several groups of tiles (a step's fusion buckets) in one launch, each group a contiguous range of
// workgroups in group order, XCD-contiguous inside it: the dispatcher hands out workgroups in
// order, so group 0 is done first and its allreduce can start while the later groups are still
// being packed. The launch pays one ramp and drain instead of one per bucket.
// With done[k] set, the last workgroup of group k (a device counter per group, reset by that
// workgroup for the next launch) stores sig_value[k] into *done[k] with a system-scope release, which
// the bucket stream waits on (hipStreamWaitValue64 on signal memory, fusion.cc).
template <int U, int POL>
__global__ __launch_bounds__(kBlock) void copy_segs_groups_kernel(const CopySeg* __restrict__ tiles,
                                                                 const CopySeg* __restrict__ segs, PackGroups g) {
  __shared__ SegStage<U> st;
  int k = 0;
  while (k + 1 < g.n && blockIdx.x >= g.blk0[k + 1]) k++;
  const unsigned local = blockIdx.x - g.blk0[k], gk = g.blk0[k + 1] - g.blk0[k];
  const int64_t tt = xcd_tile(local, gk);
  if (tt < g.ntiles[k]) copy_seg_tile<U, POL>(tiles, segs, g.tile0[k] + (int)tt, st.L);
  if (g.done[k]) {
    __syncthreads();  // (every wave's copies before the workgroup's count)
    if (threadIdx.x == 0 &&
        __hip_atomic_fetch_add(&g.counters[k], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gk - 1) {
      __hip_atomic_store(&g.counters[k], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(g.done[k], g.sig_value[k], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// ---------------------------------------------------------------------------
// Peer transfer (xGMI peer schedule, peer.cc)

struct XferList {
  XferSeg s[kMaxXferSegs];
};

// Workgroup b copies tile b / nseg of segment b % nseg: consecutive workgroups
// (and so every XCD) cover all segments, i.e. all peers' links, at once. Each
// lane issues its four 16-B loads before any store: a remote access over xGMI
// takes microseconds, so bytes in flight, not instructions, set the rate. The
// descriptors cover exactly the tile's 16-B-multiple prefix; the < 16 bytes
// past it (a ragged last chunk) go bytewise.
__global__ __launch_bounds__(kBlock) void xfer_kernel(XferList L, int nseg) {
  constexpr int U = (int)(kXferTileBytes / (kBlock * 16));
  const int seg = (int)(blockIdx.x % (unsigned)nseg);
  const int64_t off = (int64_t)(blockIdx.x / (unsigned)nseg) * kXferTileBytes;
  const XferSeg sg = L.s[seg];
  if (off >= sg.bytes) return;
  const int64_t len = sg.bytes - off < kXferTileBytes ? sg.bytes - off : kXferTileBytes;
  const char* src = sg.src + off;
  char* dst = sg.dst + off;
  const int tid = threadIdx.x;
  if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
    const int len16 = (int)(len & ~(int64_t)15);
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)src, (short)0, len16, 0x00020000);
    __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)dst, (short)0, len16, 0x00020000);
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, (u * kBlock + tid) * 16, 0, 0);
#pragma unroll
    for (int u = 0; u < U; u++) __builtin_amdgcn_raw_buffer_store_b128(v[u], rd, (u * kBlock + tid) * 16, 0, 0);
    if (len16 + tid < len) dst[len16 + tid] = src[len16 + tid];
  } else {
    for (int64_t i = tid; i < len; i += kBlock) dst[i] = src[i];
  }
}

// ---------------------------------------------------------------------------
// Launchers

// The stripe knobs (KiB of one operand, read once) in 16-B vectors; 0 = xcd_tile's contiguous eighths.
static int64_t env_kib_vecs(const char* name, long def) {
  const char* e = getenv(name);
  return (int64_t)std::max<long>(0, e && *e ? atol(e) : def) * 1024 / 16;
}

// Stripe size for stripe_tile (TIPS_STRIPE_KIB, default 1 MiB), in tiles of `tile` vectors.
int64_t stripe_of(int64_t tile) {
  static const int64_t v = env_kib_vecs("TIPS_STRIPE_KIB", 1024);
  return v / std::max<int64_t>(1, tile);
}

// The fusion pack's stripe (TIPS_PACK_STRIPE_KIB, default 0), in 16-B vectors; the layout's tile
// order (fusion.cc tile_order) places boundary tiles by the same map.
int64_t pack_stripe_vecs() {
  static const int64_t v = env_kib_vecs("TIPS_PACK_STRIPE_KIB", 0);
  return v;
}

// The 2-input sum's own stripe (TIPS_SUM_STRIPE_KIB, default 512 KiB): with its 128-lane launch,
// 512 KiB stripes ran config 2 0.6-0.8 % faster than 1 MiB, while the copy kept 1 MiB
// (profiles/r06/sum2_focus/, stripe512/). Unset, TIPS_STRIPE_KIB=0 also turns it off.
int64_t sum_stripe_of(int64_t tile) {
  static const int64_t v = [] {
    const char* g = getenv("TIPS_STRIPE_KIB");
    return env_kib_vecs("TIPS_SUM_STRIPE_KIB", g && *g && atol(g) == 0 ? 0 : 512);
  }();
  return v / std::max<int64_t>(1, tile);
}

// The grid that covers `tiles` tiles in stripes of C: whole rounds of 8 stripes once there are more
// than 8 stripes' worth of tiles.
int64_t stripe_grid(int64_t tiles, int64_t C) {
  if (C <= 0 || tiles <= 8 * C) return std::max<int64_t>(8, (tiles + 7) / 8 * 8);
  return (tiles + 8 * C - 1) / (8 * C) * (8 * C);
}

void stripe_slots(int64_t nslots, int64_t C, std::vector<int>* xcd, std::vector<int64_t>* pos) {
  xcd->assign((size_t)nslots, 0);
  pos->assign((size_t)nslots, 0);
  const int64_t grid = stripe_grid(nslots, C), R = grid >> 3;
  for (int64_t b = 0; b < grid; b++) {  // (host restatement of stripe_tile)
    const int64_t j = b >> 3;
    const int64_t t = (C <= 0 || R <= C) ? (b & 7) * R + j : ((j / C) * 8 + (b & 7)) * C + j % C;
    if (t < nslots) (*xcd)[t] = (int)(b & 7), (*pos)[t] = j;
  }
}

hipError_t launch_copy_buf(void* dst, const void* src, int64_t bytes, hipStream_t s) {
  if (bytes <= 0 || dst == src) return hipSuccess;
  if (((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) != 0)
    return hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, s);
  // TIPS_COPY_BUF_VARIANT (a sweep knob, read once; tools/copy_buf_sweep.sh): 0 = 4 KiB tiles, sc1
  // stores (shipped: 0.81-0.83 of HBM on config 3's 1 GiB, profiles/r04/z_copy_buf_sweep.txt);
  // 1 = 8 KiB tiles (0.71-0.75); 2 = 16 KiB tiles (0.73); 3 = 4 KiB tiles, nt stores;
  // 4 = hipMemcpyAsync (0.59-0.65); 5 / 6 = 128-lane workgroups (2 KiB tiles), sc1 / nt stores
  // (round 6: the 2-input sum's shipped shape)
  static const int variant = [] {
    const char* v = getenv("TIPS_COPY_BUF_VARIANT");
    return v && *v ? atoi(v) : 0;
  }();
  if (variant == 4) return hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, s);
  const int U = variant == 1 ? 2 : variant == 2 ? 4 : 1;
  const int64_t B = (variant == 5 || variant == 6) ? 128 : kBlock;
  const int64_t nvec = bytes / 16;
  const int64_t stripe = stripe_of(B * U);
  const int64_t grid = stripe_grid((nvec + B * U - 1) / (B * U), stripe);
  if (grid > 0x7fffffff) return hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, s);
  const dim3 g((unsigned)grid), b((unsigned)B);
  const auto kern = variant == 5   ? &copy_buf_kernel<1, 16, 128>
                    : variant == 6 ? &copy_buf_kernel<1, 2, 128>
                    : variant == 1 ? &copy_buf_kernel<2>
                    : variant == 2 ? &copy_buf_kernel<4>
                    : variant == 3 ? &copy_buf_kernel<1, 2>
                                   : &copy_buf_kernel<1>;
  hipLaunchKernelGGL(kern, g, b, 0, s, (u32x4*)dst, (const u32x4*)src, nvec, nvec * 16, bytes, stripe);
  return hipGetLastError();
}

// The scaled copy, dst = (src * pre) * post over n elements (tips_scale, and the scaled allreduce at
// one rank): launch_copy_buf's shipped shape (4 KiB tiles, nt loads, sc1 stores, 1 MiB stripes) with
// the multiplies between load and store; pointers that are not 16-B aligned take the scalar fold.
template <int DT>
hipError_t scale_buf_dispatch(void* dst, const void* src, int64_t n, double pre, double post, hipStream_t s) {
  using T = typename WorkOf<DT>::T;
  const ScaleArgs<DT> sc{(T)pre, (T)post, 1u};
  if (((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) != 0) {
    SrcList sl{};
    sl.p[0] = (const u32x4*)src;
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, 256 * 16));
    hipLaunchKernelGGL((multi_sum_scalar_kernel<DT, ScaleArgs<DT>>), dim3((unsigned)grid), dim3(kBlock), 0, s, dst, sl, 1,
                       n, sc);
    return hipGetLastError();
  }
  const int64_t bytes = n * dtype_size(DT), nvec = bytes / 16;
  const int64_t stripe = stripe_of(kBlock);
  const int64_t grid = stripe_grid((nvec + kBlock - 1) / kBlock, stripe);
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL((copy_buf_kernel<1, 16, kBlock, ScaleArgs<DT>>), dim3((unsigned)grid), dim3(kBlock), 0, s,
                     (u32x4*)dst, (const u32x4*)src, nvec, nvec * 16, bytes, stripe, sc);
  return hipGetLastError();
}

hipError_t launch_scale_buf(void* dst, const void* src, int64_t n, int dtype, double pre, double post, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (pre == 1.0 && post == 1.0) return launch_copy_buf(dst, src, n * dtype_size(dtype), s);
  switch (dtype) {
    case kF32: return scale_buf_dispatch<kF32>(dst, src, n, pre, post, s);
    case kF64: return scale_buf_dispatch<kF64>(dst, src, n, pre, post, s);
    case kF16: return scale_buf_dispatch<kF16>(dst, src, n, pre, post, s);
    case kBF16: return scale_buf_dispatch<kBF16>(dst, src, n, pre, post, s);
    default: return hipErrorInvalidValue;
  }
}

namespace {

// Default variant for the product path (chosen from the gfx950 sweeps): buffer ops,
// one 16-B vector per lane, 128-lane workgroups (a 2 KiB tile of each operand), nt loads and nt
// stores. Rounds 2-5 shipped 256 lanes with sc1 stores (nt index 1); under XCD stripes the
// 128-lane nt form is 1-3 % faster (profiles/r06/sum2_focus/). kDefMode and kDefNT are the launch's
// coordinates in tips_sum_variant's table (kernels_dev.hip): buffer ops, cache-policy pair 7.
constexpr int kDefMode = 3, kDefUnroll = 1, kDefNT = 7, kDefThreads = 128;
constexpr int kDefLoadAux = 2, kDefStoreAux = 2;  // nt, nt
static_assert(kDefMode == 3 && kDefNT == 7, "kDefLoadAux / kDefStoreAux spell out mode 3's cache-policy pair 7");

// The product launch of the 2-input sum, plain (sc empty) or scaled (one ScaleArgs<DT>): kDef* in
// 512 KiB stripes (sum_stripe_of); the scalar kernel when a pointer is not 16-B aligned.
template <int DT, class... SC>
hipError_t run_sum2_buf(void* dst, const void* a, const void* b, int64_t n, hipStream_t s, SC... sc) {
  if (!(aligned16(dst) && aligned16(a) && aligned16(b))) {
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, kNumCUs * 16));
    hipLaunchKernelGGL((sum2_scalar_kernel<DT, SC...>), dim3((unsigned)grid), dim3(kBlock), 0, s, dst, a, b, n, sc...);
    return hipGetLastError();
  }
  constexpr int64_t kTile = (int64_t)kDefUnroll * kDefThreads;
  const int64_t ve = 16 / (int64_t)dtype_size(DT);
  const int64_t nvec = n / ve;
  const int64_t stripe = sum_stripe_of(kTile);
  const int64_t grid = stripe_grid((nvec + kTile - 1) / kTile, stripe);
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL((sum2_buf_kernel<DT, kDefLoadAux, kDefStoreAux, kDefUnroll, kDefThreads, SC...>), dim3((unsigned)grid),
                     dim3(kDefThreads), 0, s, (u32x4*)dst, (const u32x4*)a, (const u32x4*)b, nvec, nvec * ve, n, stripe,
                     sc...);
  return hipGetLastError();
}

// Bytes the fold keeps in flight per CU (round 5, profiles/r05/): every wave-source pair has one
// 1 KiB wave-load outstanding, and with 9 streams the DRAM efficiency falls once a CU holds much more
// than the ~64 KiB the 2-input sum keeps in flight. Unused LDS reserved per workgroup caps the
// workgroups per CU (160 KiB / reservation): NSRC >= 6, 128 lanes x 5 workgroups = 10 waves
// (80 KiB for 8 sources: 8 x 32 MiB 48.1-49.2 -> 46.9-47.5 us on the sweep's boxes); NSRC 4-5,
// 128 lanes x 8 = 16 waves. 2-3 sources run uncapped (256 lanes x 8 = 32 waves: capping slowed
// 2 x 128 MiB). The reservation leaves the CU at least one RCCL transfer workgroup's worth (19.5
// KiB) at 5 workgroups; uncapped, the fold's 32 waves fill every wave slot anyway.
constexpr int kFoldLdsCap5 = 27648;  // floor(160 KiB / 27648) = 5, 25 KiB left
constexpr int kFoldLdsCap8 = 20480;  // 8

// The capped fold's store policy (TIPS_FOLD_STORE: sc1, the default, or nt; read once). The
// round-5 sweep under eighths found nt stores slower (0.72-0.74 vs 0.78-0.80); an A/B knob for
// the stripe map.
inline bool fold_store_nt() {
  static const bool v = [] {
    const char* e = getenv("TIPS_FOLD_STORE");
    return e && e[0] == 'n' && e[1] == 't' && e[2] == 0;
  }();
  return v;
}

// (sc: empty, or the scaled fold's ScaleArgs<DT> - the same launch shapes either way)
template <int DT, int NSRC, class... SC>
hipError_t run_multi(void* dst, const SrcList& sl, int64_t n, hipStream_t s, SC... sc) {
  // buffer loads, non-temporal for every source count. Round 1 kept plain loads beyond 4 sources
  // from a sweep that re-read one buffer set (plain 44.7 vs nt 47.3 us, 8 x 32 MiB, Infinity Cache
  // assisted); with operands from HBM, as the direct schedule's fold mostly reads them, nt wins
  // 48.6 vs 57.8 us (profiles/r02/multi_sum_variants.jsonl).
  constexpr int LAUX = 2;
  const int64_t ve = 16 / (int64_t)dtype_size(DT);
  const int64_t nvec = n / ve;
  const int64_t bytes = nvec * 16;
  // 256 lanes x 1 vector, except (each shape instantiated only for the source counts that can take it):
  auto kern = &multi_sum_buf_kernel<DT, NSRC, 1, LAUX, kBlock, 16, SC...>;
  int block = kBlock, vecs = 1, lds = 0;
  if constexpr (NSRC > 4) {
    // 4 vectors per lane for many sources of 3-12 MiB each (8 x 4 MiB: 7.0 vs 8.3 us, 8 x 8 MiB:
    // 12.6 vs 14.3 us; up to 4 sources, 1 vector wins or ties: profiles/r02/multi_sum_small.jsonl)
    if (bytes >= (3 << 20) && bytes <= (12 << 20)) kern = &multi_sum_buf_kernel<DT, NSRC, 4, LAUX, kBlock, 16, SC...>, vecs = 4;
  }
  if constexpr (NSRC >= 4) {
    if (bytes > (12 << 20)) {  // capped: 128 lanes, LDS reserved (kFoldLdsCap* above)
      kern = fold_store_nt() ? &multi_sum_buf_kernel<DT, NSRC, 1, LAUX, 128, 2, SC...>
                             : &multi_sum_buf_kernel<DT, NSRC, 1, LAUX, 128, 16, SC...>;
      block = 128, lds = NSRC >= 6 ? kFoldLdsCap5 : kFoldLdsCap8;
    }
  }
  const int64_t per = (int64_t)block * vecs;
  const int64_t stripe = stripe_of(per);
  const int64_t grid = stripe_grid((nvec + per - 1) / per, stripe);  // surplus workgroups fall off the bounds check
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(block), lds, s, (u32x4*)dst, sl, nvec, nvec * ve, n, stripe, sc...);
  return hipGetLastError();
}

// the pull-fold's launch (launch_multi_sum_remote): 4 vectors per lane, 256 lanes, uncapped
template <int DT, int NSRC>
hipError_t run_multi_remote(void* dst, const SrcList& sl, int64_t n, hipStream_t s) {
  const int64_t ve = 16 / (int64_t)dtype_size(DT);
  const int64_t nvec = n / ve;
  int64_t grid = (nvec + 4 * kBlock - 1) / (4 * kBlock);
  grid = std::max<int64_t>(8, (grid + 7) / 8 * 8);  // (xcd_tile: remote sources, not measured with stripes)
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL((multi_sum_buf_kernel<DT, NSRC, 4, 2>), dim3((unsigned)grid), dim3(kBlock), 0, s, (u32x4*)dst, sl,
                     nvec, nvec * ve, n, (int64_t)0);
  return hipGetLastError();
}

template <class T>
struct is_minmax : std::false_type {};
template <int DT, bool IS_MAX>
struct is_minmax<MinMaxArgs<DT, IS_MAX>> : std::true_type {};

template <int DT, class... SC>
hipError_t multi_dispatch(void* dst, const void* const* srcs, int nsrc, int64_t n, hipStream_t s, bool remote, SC... sc) {
  SrcList sl{};
  bool al = aligned16(dst);
  for (int j = 0; j < nsrc; j++) {
    sl.p[j] = (const u32x4*)srcs[j];
    al = al && aligned16(srcs[j]);
  }
  if (!al) {
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, kNumCUs * 16));
    hipLaunchKernelGGL((multi_sum_scalar_kernel<DT, SC...>), dim3((unsigned)grid), dim3(kBlock), 0, s, dst, sl, nsrc, n,
                       sc...);
    return hipGetLastError();
  }
  // Two sources: the fold is one add, i.e. the 2-input sum, whose launch (one 16-B vector per lane
  // per operand, buffer ops) runs 2 x 128 MiB at the sum's rate instead of the fold's 0.75 of HBM
  // (VERDICT r05 item 6). Storage-type arithmetic for these four types: bit-identical to the fold.
  // (MAX / MIN: every type - an exact compare has no accumulator width to differ in)
  constexpr bool kTwoIsSum = DT == kF32 || DT == kF64 || DT == kI32 || DT == kI64 || (is_minmax<SC>::value || ...);
  if constexpr (kTwoIsSum) {
    if (!remote && nsrc == 2) return run_sum2_buf<DT>(dst, srcs[0], srcs[1], n, s, sc...);
  }
  if (remote) {
    switch (nsrc) {
#define TIPS_REMOTE_CASE(K) \
  case K: return run_multi_remote<DT, K>(dst, sl, n, s);
      TIPS_REMOTE_CASE(2) TIPS_REMOTE_CASE(3) TIPS_REMOTE_CASE(4) TIPS_REMOTE_CASE(5) TIPS_REMOTE_CASE(6)
      TIPS_REMOTE_CASE(7) TIPS_REMOTE_CASE(8) TIPS_REMOTE_CASE(9) TIPS_REMOTE_CASE(10) TIPS_REMOTE_CASE(11)
      TIPS_REMOTE_CASE(12) TIPS_REMOTE_CASE(13) TIPS_REMOTE_CASE(14) TIPS_REMOTE_CASE(15) TIPS_REMOTE_CASE(16)
#undef TIPS_REMOTE_CASE
      default: return hipErrorInvalidValue;
    }
  }
  switch (nsrc) {
    case 2:  // (both callers handle one source themselves; two sources of a kTwoIsSum type went above)
      if constexpr (kTwoIsSum) return hipErrorInvalidValue;
      else return run_multi<DT, 2>(dst, sl, n, s, sc...);
#define TIPS_FOLD_CASE(K) \
  case K: return run_multi<DT, K>(dst, sl, n, s, sc...);
      TIPS_FOLD_CASE(3) TIPS_FOLD_CASE(4) TIPS_FOLD_CASE(5) TIPS_FOLD_CASE(6) TIPS_FOLD_CASE(7) TIPS_FOLD_CASE(8)
      TIPS_FOLD_CASE(9) TIPS_FOLD_CASE(10) TIPS_FOLD_CASE(11) TIPS_FOLD_CASE(12) TIPS_FOLD_CASE(13) TIPS_FOLD_CASE(14)
      TIPS_FOLD_CASE(15) TIPS_FOLD_CASE(16)
#undef TIPS_FOLD_CASE
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t launch_sum2(void* dst, const void* a, const void* b, int64_t n, int dtype, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  switch (dtype) {
    case kF32: return run_sum2_buf<kF32>(dst, a, b, n, s);
    case kF64: return run_sum2_buf<kF64>(dst, a, b, n, s);
    case kI32: return run_sum2_buf<kI32>(dst, a, b, n, s);
    case kI64: return run_sum2_buf<kI64>(dst, a, b, n, s);
    case kF16: return run_sum2_buf<kF16>(dst, a, b, n, s);
    case kBF16: return run_sum2_buf<kBF16>(dst, a, b, n, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_multi_sum(void* dst, const void* const* srcs, int nsrc, int64_t n, int dtype, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (nsrc < 1 || nsrc > kMaxSrcs) return hipErrorInvalidValue;
  if (nsrc == 1) {
    if (dst == srcs[0]) return hipSuccess;
    return hipMemcpyAsync(dst, srcs[0], (size_t)n * dtype_size(dtype), hipMemcpyDeviceToDevice, s);
  }
  switch (dtype) {
    case kF32: return multi_dispatch<kF32>(dst, srcs, nsrc, n, s, false);
    case kF64: return multi_dispatch<kF64>(dst, srcs, nsrc, n, s, false);
    case kI32: return multi_dispatch<kI32>(dst, srcs, nsrc, n, s, false);
    case kI64: return multi_dispatch<kI64>(dst, srcs, nsrc, n, s, false);
    case kF16: return multi_dispatch<kF16>(dst, srcs, nsrc, n, s, false);
    case kBF16: return multi_dispatch<kBF16>(dst, srcs, nsrc, n, s, false);
    default: return hipErrorInvalidValue;
  }
}

namespace {
// MAX / MIN through the sum's and the fold's launches (run_sum2_buf, multi_dispatch), per dtype
template <bool IS_MAX>
hipError_t minmax2(void* dst, const void* a, const void* b, int64_t n, int dtype, hipStream_t s) {
  switch (dtype) {
    case kF32: return run_sum2_buf<kF32>(dst, a, b, n, s, MinMaxArgs<kF32, IS_MAX>{});
    case kF64: return run_sum2_buf<kF64>(dst, a, b, n, s, MinMaxArgs<kF64, IS_MAX>{});
    case kI32: return run_sum2_buf<kI32>(dst, a, b, n, s, MinMaxArgs<kI32, IS_MAX>{});
    case kI64: return run_sum2_buf<kI64>(dst, a, b, n, s, MinMaxArgs<kI64, IS_MAX>{});
    case kF16: return run_sum2_buf<kF16>(dst, a, b, n, s, MinMaxArgs<kF16, IS_MAX>{});
    case kBF16: return run_sum2_buf<kBF16>(dst, a, b, n, s, MinMaxArgs<kBF16, IS_MAX>{});
    default: return hipErrorInvalidValue;
  }
}

template <bool IS_MAX>
hipError_t minmax_multi(void* dst, const void* const* srcs, int nsrc, int64_t n, int dtype, hipStream_t s) {
  switch (dtype) {
    case kF32: return multi_dispatch<kF32>(dst, srcs, nsrc, n, s, false, MinMaxArgs<kF32, IS_MAX>{});
    case kF64: return multi_dispatch<kF64>(dst, srcs, nsrc, n, s, false, MinMaxArgs<kF64, IS_MAX>{});
    case kI32: return multi_dispatch<kI32>(dst, srcs, nsrc, n, s, false, MinMaxArgs<kI32, IS_MAX>{});
    case kI64: return multi_dispatch<kI64>(dst, srcs, nsrc, n, s, false, MinMaxArgs<kI64, IS_MAX>{});
    case kF16: return multi_dispatch<kF16>(dst, srcs, nsrc, n, s, false, MinMaxArgs<kF16, IS_MAX>{});
    case kBF16: return multi_dispatch<kBF16>(dst, srcs, nsrc, n, s, false, MinMaxArgs<kBF16, IS_MAX>{});
    default: return hipErrorInvalidValue;
  }
}
}  // namespace

hipError_t launch_reduce2(void* dst, const void* a, const void* b, int64_t n, int dtype, int op, hipStream_t s) {
  if (op == kOpSum) return launch_sum2(dst, a, b, n, dtype, s);
  if (op != kOpMax && op != kOpMin) return hipErrorInvalidValue;
  if (n <= 0) return hipSuccess;
  return op == kOpMax ? minmax2<true>(dst, a, b, n, dtype, s) : minmax2<false>(dst, a, b, n, dtype, s);
}

hipError_t launch_multi_reduce(void* dst, const void* const* srcs, int nsrc, int64_t n, int dtype, int op, hipStream_t s) {
  if (op == kOpSum) return launch_multi_sum(dst, srcs, nsrc, n, dtype, s);
  if (op != kOpMax && op != kOpMin) return hipErrorInvalidValue;
  if (n <= 0) return hipSuccess;
  if (nsrc < 1 || nsrc > kMaxSrcs) return hipErrorInvalidValue;
  if (nsrc == 1) return launch_multi_sum(dst, srcs, nsrc, n, dtype, s);  // (the copy)
  return op == kOpMax ? minmax_multi<true>(dst, srcs, nsrc, n, dtype, s) : minmax_multi<false>(dst, srcs, nsrc, n, dtype, s);
}

namespace {
template <int DT>
ScaleArgs<DT> scale_args(double pre, double post, unsigned raw) {
  using T = typename WorkOf<DT>::T;
  return ScaleArgs<DT>{(T)pre, (T)post, raw};  // the factors' one conversion to the working type
}
}  // namespace

hipError_t launch_sum2_scaled(void* dst, const void* a, const void* b, int64_t n, int dtype, double pre, double post,
                              unsigned raw, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  raw &= 3u;
  if ((pre == 1.0 || raw == 0) && post == 1.0) return launch_sum2(dst, a, b, n, dtype, s);
  switch (dtype) {
    case kF32: return run_sum2_buf<kF32>(dst, a, b, n, s, scale_args<kF32>(pre, post, raw));
    case kF64: return run_sum2_buf<kF64>(dst, a, b, n, s, scale_args<kF64>(pre, post, raw));
    case kF16: return run_sum2_buf<kF16>(dst, a, b, n, s, scale_args<kF16>(pre, post, raw));
    case kBF16: return run_sum2_buf<kBF16>(dst, a, b, n, s, scale_args<kBF16>(pre, post, raw));
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_multi_sum_scaled(void* dst, const void* const* srcs, int nsrc, int64_t n, int dtype, double pre,
                                   double post, unsigned raw, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (nsrc < 1 || nsrc > kMaxSrcs) return hipErrorInvalidValue;
  raw &= (1u << nsrc) - 1u;
  if ((pre == 1.0 || raw == 0) && post == 1.0) return launch_multi_sum(dst, srcs, nsrc, n, dtype, s);
  if (nsrc == 1) return launch_scale_buf(dst, srcs[0], n, dtype, raw ? pre : 1.0, post, s);
  switch (dtype) {
    case kF32: return multi_dispatch<kF32>(dst, srcs, nsrc, n, s, false, scale_args<kF32>(pre, post, raw));
    case kF64: return multi_dispatch<kF64>(dst, srcs, nsrc, n, s, false, scale_args<kF64>(pre, post, raw));
    case kF16: return multi_dispatch<kF16>(dst, srcs, nsrc, n, s, false, scale_args<kF16>(pre, post, raw));
    case kBF16: return multi_dispatch<kBF16>(dst, srcs, nsrc, n, s, false, scale_args<kBF16>(pre, post, raw));
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_multi_sum_remote(void* dst, const void* const* srcs, int nsrc, int64_t n, int dtype, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (nsrc < 1 || nsrc > kMaxSrcs) return hipErrorInvalidValue;
  if (nsrc == 1) return launch_multi_sum(dst, srcs, nsrc, n, dtype, s);
  switch (dtype) {
    case kF32: return multi_dispatch<kF32>(dst, srcs, nsrc, n, s, true);
    case kF64: return multi_dispatch<kF64>(dst, srcs, nsrc, n, s, true);
    case kI32: return multi_dispatch<kI32>(dst, srcs, nsrc, n, s, true);
    case kI64: return multi_dispatch<kI64>(dst, srcs, nsrc, n, s, true);
    case kF16: return multi_dispatch<kF16>(dst, srcs, nsrc, n, s, true);
    case kBF16: return multi_dispatch<kBF16>(dst, srcs, nsrc, n, s, true);
    default: return hipErrorInvalidValue;
  }
}

namespace {

template <int U>
hipError_t run_copy_segs_groups(const CopySeg* tiles, const CopySeg* segs, const PackGroups& g, int pol, hipStream_t s) {
  const unsigned grid = g.blk0[g.n];
  switch (pol) {
    case 0: hipLaunchKernelGGL((copy_segs_groups_kernel<U, 0>), dim3(grid), dim3(kBlock), 0, s, tiles, segs, g); break;
    case 1: hipLaunchKernelGGL((copy_segs_groups_kernel<U, 1>), dim3(grid), dim3(kBlock), 0, s, tiles, segs, g); break;
    case 2: hipLaunchKernelGGL((copy_segs_groups_kernel<U, 2>), dim3(grid), dim3(kBlock), 0, s, tiles, segs, g); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <int U>
hipError_t run_copy_segs(const CopySeg* tiles, const CopySeg* segs, int tile0, int ntiles, int pol, hipStream_t s) {
  const int64_t C = pack_stripe_vecs() / ((int64_t)kBlock * U);  // tiles per stripe (0: xcd_tile)
  const unsigned grid = (unsigned)stripe_grid(ntiles, C);
  switch (pol) {
    case 0: hipLaunchKernelGGL((copy_segs_kernel<U, 0>), dim3(grid), dim3(kBlock), 0, s, tiles, segs, tile0, ntiles, C); break;
    case 1: hipLaunchKernelGGL((copy_segs_kernel<U, 1>), dim3(grid), dim3(kBlock), 0, s, tiles, segs, tile0, ntiles, C); break;
    case 2: hipLaunchKernelGGL((copy_segs_kernel<U, 2>), dim3(grid), dim3(kBlock), 0, s, tiles, segs, tile0, ntiles, C); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_copy_segs(const CopySeg* tiles, const CopySeg* segs, int tile0, int ntiles, int64_t tile_bytes,
                            int pol, hipStream_t s) {
  if (ntiles <= 0) return hipSuccess;
  switch (tile_bytes) {
    case 4096: return run_copy_segs<1>(tiles, segs, tile0, ntiles, pol, s);
    case 8192: return run_copy_segs<2>(tiles, segs, tile0, ntiles, pol, s);
    case 16384: return run_copy_segs<4>(tiles, segs, tile0, ntiles, pol, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_copy_segs_groups(const CopySeg* tiles, const CopySeg* segs, PackGroups g, int64_t tile_bytes, int pol,
                                   hipStream_t s) {
  if (g.n < 1 || g.n > kMaxPackGroups) return hipErrorInvalidValue;
  for (int k = 0; k < g.n; k++)
    if (g.done[k] && !g.counters) return hipErrorInvalidValue;
  int64_t blk = 0;
  for (int k = 0; k < g.n; k++) {  // each group's workgroups: whole XCD rounds (xcd_tile), at least 8
    if (g.ntiles[k] < 0) return hipErrorInvalidValue;
    g.blk0[k] = (unsigned)blk;
    blk += std::max<int64_t>(8, ((int64_t)g.ntiles[k] + 7) / 8 * 8);
  }
  if (blk > 0x7fffffff) return hipErrorInvalidValue;
  g.blk0[g.n] = (unsigned)blk;
  switch (tile_bytes) {
    case 4096: return run_copy_segs_groups<1>(tiles, segs, g, pol, s);
    case 8192: return run_copy_segs_groups<2>(tiles, segs, g, pol, s);
    case 16384: return run_copy_segs_groups<4>(tiles, segs, g, pol, s);
    default: return hipErrorInvalidValue;
  }
}

namespace {
// dynamic LDS per cast workgroup (an occupancy cap: 160 KiB / bytes workgroups per CU), per
// direction; TIPS_CAST_LDS_PACK / TIPS_CAST_LDS_UNPACK (bytes) for sweeps
int cast_lds_bytes(int dir) {
  static const int v[2] = {(int)std::min<long>(65536, std::max<long>(0, getenv("TIPS_CAST_LDS_PACK") ? atol(getenv("TIPS_CAST_LDS_PACK")) : 0)),
                           (int)std::min<long>(65536, std::max<long>(0, getenv("TIPS_CAST_LDS_UNPACK") ? atol(getenv("TIPS_CAST_LDS_UNPACK")) : 0))};
  return v[dir];
}

template <int U, int DIR>
hipError_t run_cast_segs(const CopySeg* tiles, const CopySeg* segs, int tile0, int ntiles, int wire, hipStream_t s) {
  const unsigned grid = (unsigned)std::max<int64_t>(8, ((int64_t)ntiles + 7) / 8 * 8);
  const int lds = cast_lds_bytes(DIR);
  static const int var = getenv("TIPS_CAST_VARIANT") ? atoi(getenv("TIPS_CAST_VARIANT")) : 8;
  if (wire != kF16 && wire != kBF16) return hipErrorInvalidValue;
  auto kern = wire == kF16 ? &cast_segs_kernel<U, DIR, kF16> : &cast_segs_kernel<U, DIR, kBF16>;
  if constexpr (U == 2) {  // (the load / store policy sweep: f16 wire, 8 KiB tiles)
    if (wire == kF16 && var != 8)
      kern = var == 0   ? &cast_segs_kernel<U, DIR, kF16, 0>
             : var == 1 ? &cast_segs_kernel<U, DIR, kF16, 1>
             : var == 2 ? &cast_segs_kernel<U, DIR, kF16, 2>
             : var == 3 ? &cast_segs_kernel<U, DIR, kF16, 3>
             : var == 4 ? &cast_segs_kernel<U, DIR, kF16, 4>
                        : &cast_segs_kernel<U, DIR, kF16, 5>;
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, s, tiles, segs, tile0, ntiles);
  return hipGetLastError();
}

template <int DIR>
hipError_t run_cast_range(void* dst, const void* src, int64_t n, int wire, hipStream_t s) {
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, (int64_t)kNumCUs * 16));
  if (wire == kF16) hipLaunchKernelGGL((cast_range_kernel<DIR, kF16>), dim3((unsigned)grid), dim3(kBlock), 0, s, dst, src, n);
  else if (wire == kBF16) hipLaunchKernelGGL((cast_range_kernel<DIR, kBF16>), dim3((unsigned)grid), dim3(kBlock), 0, s, dst, src, n);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}
}  // namespace

hipError_t launch_cast_segs(const CopySeg* tiles, const CopySeg* segs, int tile0, int ntiles, int64_t tile_bytes,
                            int dir, int wire, hipStream_t s) {
  if (ntiles <= 0) return hipSuccess;
  if (dir != 0 && dir != 1) return hipErrorInvalidValue;
  switch (tile_bytes) {
    case 4096: return dir ? run_cast_segs<1, 1>(tiles, segs, tile0, ntiles, wire, s) : run_cast_segs<1, 0>(tiles, segs, tile0, ntiles, wire, s);
    case 8192: return dir ? run_cast_segs<2, 1>(tiles, segs, tile0, ntiles, wire, s) : run_cast_segs<2, 0>(tiles, segs, tile0, ntiles, wire, s);
    case 16384: return dir ? run_cast_segs<4, 1>(tiles, segs, tile0, ntiles, wire, s) : run_cast_segs<4, 0>(tiles, segs, tile0, ntiles, wire, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_cast_range(void* dst, const void* src, int64_t n, int dir, int wire, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  return dir ? run_cast_range<1>(dst, src, n, wire, s) : run_cast_range<0>(dst, src, n, wire, s);
}

hipError_t launch_xfer(const XferSeg* segs, int nseg, hipStream_t s) {
  if (nseg < 0 || nseg > kMaxXferSegs) return hipErrorInvalidValue;
  XferList L{};
  int64_t max_tiles = 0;
  int m = 0;
  for (int i = 0; i < nseg; i++) {
    if (segs[i].bytes <= 0) continue;
    L.s[m++] = segs[i];
    max_tiles = std::max<int64_t>(max_tiles, (segs[i].bytes + kXferTileBytes - 1) / kXferTileBytes);
  }
  if (m == 0) return hipSuccess;
  const int64_t grid = max_tiles * m;
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(xfer_kernel, dim3((unsigned)grid), dim3(kBlock), 0, s, L, m);
  return hipGetLastError();
}

}  // namespace tips

