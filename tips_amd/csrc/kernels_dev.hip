// kernels_dev.hip — the kernels and launchers only the tuning sweeps run (libtips_hip_dev.so and
// the sanitizer build: tips_sum_variant, tips_multi_sum_variant, tips_copy_tiles_variant of
// include/tips_hip_dev.h). The forms rounds 1-5 measured against what kernels.hip ships; the kernel
// templates the two files share are in kernels_device.h. Never part of libtips_hip.so.
#include <algorithm>

#include "kernels_dev.h"
#include "kernels_device.h"

namespace tips {

// ---------------------------------------------------------------------------
// 2-input sum: dst = a + b
//
// The global_load / global_store form (round 1): UNROLL 16-B vectors per operand per lane, all
// loads issued before the first add; MODE 1 = one tile per workgroup, 0 = grid-stride over
// gridDim.x workgroups, 2 = one tile per workgroup in XCD-contiguous order.
template <int DT, int MODE, int UNROLL, bool NTL, bool NTS, int BLOCK>
__global__ __launch_bounds__(BLOCK) void sum2_kernel(u32x4* __restrict__ dst, const u32x4* __restrict__ a,
                                                    const u32x4* __restrict__ b, int64_t nvec, int64_t tail_begin,
                                                    int64_t n) {
  constexpr int64_t kTile = (int64_t)BLOCK * UNROLL;  // vectors per workgroup-iteration
  const int tid = threadIdx.x;
  // MODE 2: XCD-contiguous placement. Workgroups are dealt round-robin over the 8 XCDs
  // (b and b+8 share one), so tile = (b % 8) * (grid / 8) + b / 8 gives each XCD one
  // contiguous stretch of the bucket (speed only: any placement is correct).
  int64_t t = (MODE == 2) ? xcd_tile(blockIdx.x, gridDim.x) : (int64_t)blockIdx.x;
  const int64_t tstride = (MODE == 0) ? (int64_t)gridDim.x : 0;
  do {
    const int64_t base = t * kTile + tid;
    if (base + (UNROLL - 1) * BLOCK < nvec) {
      u32x4 x[UNROLL], y[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; u++) x[u] = ld16<NTL>(a + base + u * BLOCK);
#pragma unroll
      for (int u = 0; u < UNROLL; u++) y[u] = ld16<NTL>(b + base + u * BLOCK);
#pragma unroll
      for (int u = 0; u < UNROLL; u++) st16<NTS>(dst + base + u * BLOCK, add16<DT>(x[u], y[u]));
    } else {
#pragma unroll
      for (int u = 0; u < UNROLL; u++) {
        const int64_t i = base + u * BLOCK;
        if (i < nvec) st16<NTS>(dst + i, add16<DT>(ld16<NTL>(a + i), ld16<NTL>(b + i)));
      }
    }
    t += tstride;
  } while (MODE == 0 && t * kTile < nvec);
  if (blockIdx.x == 0 && tail_begin + tid < n) add_elem<DT>(dst, a, b, tail_begin + tid);
}

// The shipped sum with other workgroup -> tile maps (tuning sweep only, f32; the 128 MiB dip,
// DESIGN.md §3): stripe = 0 address order; else the tiles cut into stripes of `stripe` tiles dealt
// round-robin over the 8 XCDs (stripe s to XCD s % 8; the shipped map is one stripe per XCD), and
// workgroup j of XCD x takes the j-th tile of that XCD's stripes. The grid covers whole rounds of
// 8 stripes (the workgroups past the last tile exit at once).
__global__ __launch_bounds__(256) void sum2_map_kernel(u32x4* __restrict__ dst, const u32x4* __restrict__ a,
                                                       const u32x4* __restrict__ b, int64_t nvec, int64_t tail_begin,
                                                       int64_t n, int64_t stripe) {
  constexpr int64_t kTile = 256;
  const int64_t bx = blockIdx.x, x = bx & 7, j = bx >> 3;
  const int64_t t = stripe == 0 ? bx : (x + 8 * (j / stripe)) * stripe + j % stripe;
  const int64_t first = t * kTile;
  if (first < nvec) {
    const int rec = (int)(((nvec - first) < kTile ? (nvec - first) : kTile) * 16);
    __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)(a + first), (short)0, rec, 0x00020000);
    __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(b + first), (short)0, rec, 0x00020000);
    __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(dst + first), (short)0, rec, 0x00020000);
    const u32x4 xv = __builtin_amdgcn_raw_buffer_load_b128(ra, (int)threadIdx.x * 16, 0, 2);
    const u32x4 yv = __builtin_amdgcn_raw_buffer_load_b128(rb, (int)threadIdx.x * 16, 0, 2);
    __builtin_amdgcn_raw_buffer_store_b128(add16<kF32>(xv, yv), rd, (int)threadIdx.x * 16, 0, 16);
  }
  if (blockIdx.x == 0 && tail_begin + (int64_t)threadIdx.x < n) add_elem<kF32>(dst, a, b, tail_begin + threadIdx.x);
}

// LDS-staged 2-input sum (tuning sweep only, f32): both operand tiles go global -> LDS with
// gfx950's direct-to-LDS loads (global_load_lds_dwordx4 nt: no VGPR destination, each
// wave-instruction lands 1 KiB at a wave-uniform LDS base + lane x 16 B), then LDS -> VGPRs
// (ds_read_b128), add, sc1 buffer store as the shipped kernel. It measures what an LDS hop
// costs a stream that reads every byte once. Partial last tile: plain loads.
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef __attribute__((address_space(1))) void* gbl_ptr_t;

template <int U>
__global__ __launch_bounds__(256) void sum2_lds_kernel(u32x4* __restrict__ dst, const u32x4* __restrict__ a,
                                                       const u32x4* __restrict__ b, int64_t nvec, int64_t tail_begin,
                                                       int64_t n) {
  __shared__ u32x4 stage[2 * 256 * U];  // one array: [a tile | b tile]
  constexpr int64_t kTile = 256 * U;
  const int tid = threadIdx.x, wbase = tid & ~63;
  const int64_t first = xcd_tile(blockIdx.x, gridDim.x) * kTile;
  if (first + kTile <= nvec) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(a + first + u * 256 + tid), (lds_ptr_t)(stage + u * 256 + wbase),
                                       16, 0, 2);
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(b + first + u * 256 + tid),
                                       (lds_ptr_t)(stage + kTile + u * 256 + wbase), 16, 0, 2);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(dst + first), (short)0, (int)(kTile * 16),
                                                                  0x00020000);
#pragma unroll
    for (int u = 0; u < U; u++)
      __builtin_amdgcn_raw_buffer_store_b128(add16<kF32>(stage[u * 256 + tid], stage[kTile + u * 256 + tid]), rd,
                                             (u * 256 + tid) * 16, 0, 16);
  } else if (first < nvec) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t i = first + u * 256 + tid;
      if (i < nvec) dst[i] = add16<kF32>(a[i], b[i]);
    }
  }
  if (blockIdx.x == 0 && tail_begin + (int64_t)threadIdx.x < n) add_elem<kF32>(dst, a, b, tail_begin + threadIdx.x);
}

// Persistent streaming 2-input sum (tuning sweep only, f32): gridDim = 256 CUs x WPC
// workgroups, each owning one contiguous range of the bucket (XCD-contiguous order), walked
// 4 KiB per operand at a time with the next tile's loads issued before the current tile's add
// and sc1 store (2-deep software pipeline). Tests whether long sequential runs per CU beat one
// short tile per workgroup on DRAM efficiency.
__global__ __launch_bounds__(256) void sum2_stream_kernel(u32x4* __restrict__ dst, const u32x4* __restrict__ a,
                                                          const u32x4* __restrict__ b, int64_t nvec,
                                                          int64_t tail_begin, int64_t n) {
  const int64_t G = gridDim.x;
  const int64_t per = ((nvec + G - 1) / G + 255) / 256 * 256;
  const int64_t beg = xcd_tile(blockIdx.x, gridDim.x) * per;
  const int64_t end = beg + per < nvec ? beg + per : nvec;
  const int tid = threadIdx.x;
  if (beg < end) {
    __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(dst + beg), (short)0,
                                                                  (int)((end - beg) * 16), 0x00020000);
    const int64_t iters = (end - beg + 255) / 256;
    int64_t i = beg + tid;
    u32x4 x0 = {}, y0 = {};
    if (i < end) {
      x0 = ld16<true>(a + i);
      y0 = ld16<true>(b + i);
    }
    for (int64_t k = 0; k < iters; k++) {
      const int64_t j = i + 256;
      u32x4 x1 = {}, y1 = {};
      if (j < end) {
        x1 = ld16<true>(a + j);
        y1 = ld16<true>(b + j);
      }
      if (i < end) __builtin_amdgcn_raw_buffer_store_b128(add16<kF32>(x0, y0), rd, (int)((i - beg) * 16), 0, 16);
      x0 = x1;
      y0 = y1;
      i = j;
    }
  }
  if (blockIdx.x == 0 && tail_begin + (int64_t)threadIdx.x < n) add_elem<kF32>(dst, a, b, tail_begin + threadIdx.x);
}

template <int DT, int NSRC, int UNROLL>
__global__ __launch_bounds__(kBlock) void multi_sum_kernel(u32x4* __restrict__ dst, SrcList srcs, int64_t nvec,
                                                          int64_t tail_begin, int64_t n) {
  using W = Wide<DT>;
  constexpr int64_t kTile = (int64_t)kBlock * UNROLL;
  const int tid = threadIdx.x;
  const int64_t first = xcd_tile(blockIdx.x, gridDim.x) * kTile;
  const int64_t base = first + tid;
  // sc1 stores through a descriptor covering this tile (as sum2_buf_kernel)
  const int64_t left = nvec - first;
  __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(dst + first), (short)0, (int)((left < kTile ? (left > 0 ? left : 0) : kTile) * 16), 0x00020000);
#pragma unroll
  for (int u = 0; u < UNROLL; u++) {
    const int64_t i = base + u * kBlock;
    if (i < nvec) {
      u32x4 v[NSRC];
#pragma unroll
      for (int j = 0; j < NSRC; j++) v[j] = ld16<true>(srcs.p[j] + i);
      typename W::A acc = W::load(v[0]);
#pragma unroll
      for (int j = 1; j < NSRC; j++) acc = acc + W::load(v[j]);
      __builtin_amdgcn_raw_buffer_store_b128(W::store(acc), rd, (int)((i - first) * 16), 0, 16);
    }
  }
  if (blockIdx.x == 0 && NSRC > 1 && tail_begin + tid < n) {
    const void* s[NSRC];
#pragma unroll
    for (int j = 0; j < NSRC; j++) s[j] = srcs.p[j];
    fold_elem<DT>(dst, s, NSRC, tail_begin + tid);
  }
}

// Round-5 sweep form of the fold (f32): ORDER 0 = XCD-contiguous tiles, 1 = address order (the
// 8 XCDs on neighbouring tiles, so the chip reads NSRC + 1 moving windows instead of 8 x that),
// 2 = XCD-contiguous with each XCD's stretch cut into 8 interleaved runs; ITER consecutive tiles
// per workgroup, one after the other (longer-lived workgroups, fewer ramps); ROT: the sources'
// load order rotated by workgroup (the fold order is unchanged); SAUX store policy; BLOCK lanes.
template <int NSRC, int U, int SAUX, int ORDER, int ITER, int ROT, int BLOCK>
__global__ __launch_bounds__(BLOCK) void multi_sum_x_kernel(u32x4* __restrict__ dst, SrcList srcs, int64_t nvec,
                                                            int64_t tail_begin, int64_t n) {
  constexpr int64_t kTile = (int64_t)BLOCK * U;
  const int tid = threadIdx.x;
  int64_t g;
  if constexpr (ORDER == 0) {
    g = xcd_tile(blockIdx.x, gridDim.x);
  } else if constexpr (ORDER == 1) {
    g = blockIdx.x;
  } else {  // XCD x owns stretch x; inside it, its workgroups walk 8 sub-runs round-robin
    const int64_t per = gridDim.x >> 3, k = blockIdx.x >> 3, runs = per >= 64 ? 8 : 1;
    g = (int64_t)(blockIdx.x & 7u) * per + (k % runs) * (per / runs) + k / runs;
  }
  for (int it = 0; it < ITER; it++) {
    const int64_t first = (g * ITER + it) * kTile;
    if (first >= nvec) break;
    const int rec = (int)(((nvec - first) < kTile ? (nvec - first) : kTile) * 16);
    u32x4 v[U][NSRC];
#pragma unroll
    for (int jj = 0; jj < NSRC; jj++) {
      const int j = ROT ? (int)((jj + blockIdx.x) % NSRC) : jj;
      __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(srcs.p[j] + first), (short)0, rec, 0x00020000);
#pragma unroll
      for (int u = 0; u < U; u++) {
        u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rs, (u * BLOCK + tid) * 16, 0, 2);
        if constexpr (ROT) {
#pragma unroll
          for (int q = 0; q < NSRC; q++)
            if (q == j) v[u][q] = x;
        } else {
          v[u][jj] = x;
        }
      }
    }
    __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(dst + first), (short)0, rec, 0x00020000);
#pragma unroll
    for (int u = 0; u < U; u++) {
      f32x4 acc = __builtin_bit_cast(f32x4, v[u][0]);
#pragma unroll
      for (int j = 1; j < NSRC; j++) acc = acc + __builtin_bit_cast(f32x4, v[u][j]);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc), rd, (u * BLOCK + tid) * 16, 0, SAUX);
    }
  }
  if (blockIdx.x == 0 && NSRC > 1 && tail_begin + tid < n) {
    const void* s[NSRC];
#pragma unroll
    for (int j = 0; j < NSRC; j++) s[j] = srcs.p[j];
    fold_elem<kF32>(dst, s, NSRC, tail_begin + tid);
  }
}

// Grid-stride form (round-5 sweep, f32): gridDim = 256 CUs x W workgroups, XCD x walking its
// stretch with its grid / 8 workgroups side by side (tile = stretch start + k x grid / 8 + slot).
// The chip's loads in flight are capped by the grid, not by reserved LDS or registers, so a
// transfer kernel beside the fold still finds room on every CU. PIPE: the next tile's loads are
// issued before this tile's add and store.
template <int NSRC, int BLOCK, int PIPE>
__global__ __launch_bounds__(BLOCK) void multi_sum_gs_kernel(u32x4* __restrict__ dst, SrcList srcs, int64_t nvec,
                                                             int64_t tail_begin, int64_t n) {
  constexpr int64_t kTile = BLOCK;
  const int tid = threadIdx.x;
  const int64_t ntiles = (nvec + kTile - 1) / kTile;
  const int64_t per_xcd = (ntiles + 7) / 8, wg_xcd = gridDim.x >> 3;
  const int64_t x = blockIdx.x & 7u, slot = blockIdx.x >> 3;
  const int64_t beg = x * per_xcd, end = beg + per_xcd < ntiles ? beg + per_xcd : ntiles;
  auto load = [&](int64_t t, u32x4 (&v)[NSRC]) {
    const int64_t first = t * kTile;
    const int rec = (int)(((nvec - first) < kTile ? (nvec - first) : kTile) * 16);
#pragma unroll
    for (int j = 0; j < NSRC; j++) {
      __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(srcs.p[j] + first), (short)0, rec, 0x00020000);
      v[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, tid * 16, 0, 2);
    }
  };
  auto fold_store = [&](int64_t t, const u32x4 (&v)[NSRC]) {
    const int64_t first = t * kTile;
    const int rec = (int)(((nvec - first) < kTile ? (nvec - first) : kTile) * 16);
    __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(dst + first), (short)0, rec, 0x00020000);
    f32x4 acc = __builtin_bit_cast(f32x4, v[0]);
#pragma unroll
    for (int j = 1; j < NSRC; j++) acc = acc + __builtin_bit_cast(f32x4, v[j]);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc), rd, tid * 16, 0, 16);
  };
  int64_t t = beg + slot;
  if constexpr (PIPE) {
    u32x4 a[NSRC], b[NSRC];
    if (t < end) load(t, a);
    while (t < end) {
      const int64_t t2 = t + wg_xcd;
      if (t2 < end) load(t2, b);
      fold_store(t, a);
#pragma unroll
      for (int j = 0; j < NSRC; j++) a[j] = b[j];
      t = t2;
    }
  } else {
    for (; t < end; t += wg_xcd) {
      u32x4 v[NSRC];
      load(t, v);
      fold_store(t, v);
    }
  }
  if (blockIdx.x == 0 && NSRC > 1 && tail_begin + tid < n) {
    const void* s[NSRC];
#pragma unroll
    for (int j = 0; j < NSRC; j++) s[j] = srcs.p[j];
    fold_elem<kF32>(dst, s, NSRC, tail_begin + tid);
  }
}

// ---------------------------------------------------------------------------
// Batched copy of a tile list (rounds 1-2's fusion pack / unpack; the segment copy of kernels.hip
// replaced it in round 3): one workgroup per tile of at most kCopyTileBytes.

__global__ __launch_bounds__(kBlock) void copy_tiles_kernel(const CopyTile* __restrict__ tiles, int ntiles) {
  const int64_t ti = xcd_tile(blockIdx.x, gridDim.x);
  if (ti >= ntiles) return;
  const CopyTile t = tiles[ti];
  const int tid = threadIdx.x;
  if (((reinterpret_cast<uintptr_t>(t.src) | reinterpret_cast<uintptr_t>(t.dst) | (uintptr_t)t.bytes) & 15) == 0) {
    const u32x4* s = reinterpret_cast<const u32x4*>(t.src);
    __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(t.dst, (short)0, (int)t.bytes, 0x00020000);
    const int64_t nv = t.bytes >> 4;
    constexpr int U = 4;
    for (int64_t i = tid; i < nv; i += kBlock * U) {
      u32x4 v[U] = {};
#pragma unroll
      for (int u = 0; u < U; u++)
        if (i + u * kBlock < nv) v[u] = ld16<true>(s + i + u * kBlock);
#pragma unroll
      for (int u = 0; u < U; u++)  // sc1 stores; lanes past the tile fall off the descriptor's range
        __builtin_amdgcn_raw_buffer_store_b128(v[u], rd, (int)((i + u * kBlock) * 16), 0, 16);
    }
  } else if (((reinterpret_cast<uintptr_t>(t.src) | reinterpret_cast<uintptr_t>(t.dst) | (uintptr_t)t.bytes) & 3) == 0) {
    const unsigned* s = reinterpret_cast<const unsigned*>(t.src);
    unsigned* d = reinterpret_cast<unsigned*>(t.dst);
    for (int64_t i = tid; i < (t.bytes >> 2); i += kBlock) d[i] = s[i];
  } else {
    for (int64_t i = tid; i < t.bytes; i += kBlock) t.dst[i] = t.src[i];
  }
}

// Grouped variant (tuning sweep, tools/copy_sweep.py): each workgroup copies G consecutive tiles
// of at most 256 x U x 16 B. The G descriptors are read up front (independent scalar loads, one
// latency for all), then every lane issues its G x U 16-B loads before the first store, so one
// workgroup keeps G tiles in flight and the descriptor latency is paid once per G tiles. A tile
// whose ends are 16-B aligned moves its whole 16-B vectors through buffer ops (range = those
// vectors, so lanes past them fall off) and its < 16 trailing bytes bytewise; a misaligned tile
// goes bytewise whole.
template <int G, int U, int LAUX, int SAUX>
__global__ __launch_bounds__(kBlock) void copy_tiles_g_kernel(const CopyTile* __restrict__ tiles, int ntiles) {
  const int64_t t0 = xcd_tile(blockIdx.x, gridDim.x) * G;
  if (t0 >= ntiles) return;
  const int tid = threadIdx.x;
  CopyTile d[G];
  int vec[G];  // bytes moved as 16-B vectors
#pragma unroll
  for (int g = 0; g < G; g++) {
    d[g] = (t0 + g < ntiles) ? tiles[t0 + g] : CopyTile{nullptr, nullptr, 0};
    const bool al = ((reinterpret_cast<uintptr_t>(d[g].src) | reinterpret_cast<uintptr_t>(d[g].dst)) & 15) == 0;
    vec[g] = al ? (int)(d[g].bytes & ~(int64_t)15) : 0;
  }
  u32x4 v[G][U];
#pragma unroll
  for (int g = 0; g < G; g++) {
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)d[g].src, (short)0, vec[g], 0x00020000);
#pragma unroll
    for (int u = 0; u < U; u++) v[g][u] = __builtin_amdgcn_raw_buffer_load_b128(rs, (u * kBlock + tid) * 16, 0, LAUX);
  }
#pragma unroll
  for (int g = 0; g < G; g++) {
    __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(d[g].dst, (short)0, vec[g], 0x00020000);
#pragma unroll
    for (int u = 0; u < U; u++) __builtin_amdgcn_raw_buffer_store_b128(v[g][u], rd, (u * kBlock + tid) * 16, 0, SAUX);
    for (int64_t i = vec[g] + tid; i < d[g].bytes; i += kBlock) d[g].dst[i] = d[g].src[i];
  }
}

// ---------------------------------------------------------------------------
// Launchers

namespace {

template <int DT, int MODE, int UNROLL, bool NTL, bool NTS, int BLOCK>
hipError_t run_sum2(void* dst, const void* a, const void* b, int64_t n, int blocks, hipStream_t s) {
  const int64_t ve = 16 / (int64_t)dtype_size(DT);
  const int64_t nvec = n / ve;
  const int64_t tiles = (nvec + (int64_t)BLOCK * UNROLL - 1) / ((int64_t)BLOCK * UNROLL);
  int64_t grid = (MODE != 0) ? tiles : (blocks > 0 ? blocks : kNumCUs * 8);
  if (grid > tiles) grid = tiles;
  if (grid < 1) grid = 1;
  if (MODE == 2) grid = (grid + 7) / 8 * 8;  // whole XCD rounds; surplus tiles fall off the bounds checks
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL((sum2_kernel<DT, MODE, UNROLL, NTL, NTS, BLOCK>), dim3((unsigned)grid), dim3(BLOCK), 0, s,
                     (u32x4*)dst, (const u32x4*)a, (const u32x4*)b, nvec, nvec * ve, n);
  return hipGetLastError();
}

// nt: 0 = plain, 1 = non-temporal loads and stores, 2 = nt loads only, 3 = nt stores only
template <int DT>
hipError_t sum2_dispatch(void* dst, const void* a, const void* b, int64_t n, int mode, int unroll, int nt, int blocks,
                         int threads, hipStream_t s) {
  // (no variant of the unaligned fallback: the product's scalar launch)
  if (!(aligned16(dst) && aligned16(a) && aligned16(b))) return launch_sum2(dst, a, b, n, DT, s);
  if (mode == 5) {  // persistent streaming, f32, 256 threads; unroll = workgroups per CU (grid = 256 x unroll)
    if constexpr (DT == kF32) {
      if (threads == 256 && (unroll == 1 || unroll == 2 || unroll == 4 || unroll == 8)) {
        const int64_t nvec = n / 4;
        hipLaunchKernelGGL(sum2_stream_kernel, dim3((unsigned)(kNumCUs * unroll)), dim3(256), 0, s, (u32x4*)dst,
                           (const u32x4*)a, (const u32x4*)b, nvec, nvec * 4, n);
        return hipGetLastError();
      }
    }
    return hipErrorInvalidValue;
  }
  if (mode == 6) {  // other tile maps, f32, 256 threads; unroll = stripe in KiB of one operand (0: address order)
    if constexpr (DT == kF32) {
      const int64_t nvec = n / 4, T = (nvec + 255) / 256;
      const int64_t stripe = (int64_t)unroll * 1024 / 4096;  // tiles of 4 KiB
      if (unroll < 0 || (unroll > 0 && stripe < 1)) return hipErrorInvalidValue;
      const int64_t grid = stripe == 0 ? std::max<int64_t>(1, T) : ((T + stripe - 1) / stripe + 7) / 8 * 8 * stripe;
      hipLaunchKernelGGL(sum2_map_kernel, dim3((unsigned)grid), dim3(256), 0, s, (u32x4*)dst, (const u32x4*)a,
                         (const u32x4*)b, nvec, nvec * 4, n, stripe);
      return hipGetLastError();
    }
    return hipErrorInvalidValue;
  }
  if (mode == 4) {  // LDS-staged (direct-to-LDS loads), f32, 256 threads; unroll = 16-B vectors per lane
    if constexpr (DT == kF32) {
      const int64_t nvec = n / 4;
      auto grid_for = [&](int64_t tile) { return (unsigned)std::max<int64_t>(8, ((nvec + tile - 1) / tile + 7) / 8 * 8); };
      if (threads == 256 && unroll == 1) {
        hipLaunchKernelGGL((sum2_lds_kernel<1>), dim3(grid_for(256)), dim3(256), 0, s, (u32x4*)dst, (const u32x4*)a,
                           (const u32x4*)b, nvec, nvec * 4, n);
        return hipGetLastError();
      }
      if (threads == 256 && unroll == 2) {
        hipLaunchKernelGGL((sum2_lds_kernel<2>), dim3(grid_for(512)), dim3(256), 0, s, (u32x4*)dst, (const u32x4*)a,
                           (const u32x4*)b, nvec, nvec * 4, n);
        return hipGetLastError();
      }
      if (threads == 256 && unroll == 4) {
        hipLaunchKernelGGL((sum2_lds_kernel<4>), dim3(grid_for(1024)), dim3(256), 0, s, (u32x4*)dst, (const u32x4*)a,
                           (const u32x4*)b, nvec, nvec * 4, n);
        return hipGetLastError();
      }
    }
    return hipErrorInvalidValue;
  }
#define TIPS_SUM2_CASE(M, U, NTV, L, S_, B)                      \
  if (mode == M && unroll == U && nt == NTV && threads == B) \
    return run_sum2<DT, M, U, L, S_, B>(dst, a, b, n, blocks, s);
  if (mode == 3) {  // buffer-op variants: nt = index into (load aux, store aux); unroll x threads = tile
    const int64_t ve = 16 / (int64_t)dtype_size(DT);
    const int64_t nvec = n / ve;
    // blocks > 0: that many bytes of (unused) LDS reserved per workgroup, capping workgroups per CU
    // at 160 KiB / blocks (the occupancy sweep); 0 = no cap
    if (blocks < 0 || blocks > 65536) return hipErrorInvalidValue;
    const unsigned shmem = (unsigned)blocks;
#define TIPS_BUF_CASE(I, L, S_, U, B)                                                                          \
  if (nt == I && unroll == U && threads == B) {                                                            \
    hipLaunchKernelGGL((sum2_buf_kernel<DT, L, S_, U, B>),                                                    \
                       dim3((unsigned)stripe_grid((nvec + U * B - 1) / (U * B), sum_stripe_of(U * B))), dim3(B), shmem, s, \
                       (u32x4*)dst, (const u32x4*)a, (const u32x4*)b, nvec, nvec * ve, n, sum_stripe_of(U * B));      \
    return hipGetLastError();                                                                              \
  }
    TIPS_BUF_CASE(7, 2, 2, 1, 128)   // the product default (round 6): nt loads, nt stores, 1 x 16 B per lane, 128 lanes
    TIPS_BUF_CASE(1, 2, 16, 1, 256)  // rounds 2-5's default: nt loads, sc1 stores, 256 lanes
    if constexpr (DT == kF32) {
      TIPS_BUF_CASE(0, 2, 0, 1, 256)
      TIPS_BUF_CASE(2, 2, 17, 1, 256)
      TIPS_BUF_CASE(3, 18, 0, 1, 256)
      TIPS_BUF_CASE(4, 3, 0, 1, 256)
      TIPS_BUF_CASE(5, 16, 0, 1, 256)
      TIPS_BUF_CASE(6, 18, 16, 1, 256)
      TIPS_BUF_CASE(7, 2, 2, 1, 256)
      TIPS_BUF_CASE(8, 0, 16, 1, 256)
      TIPS_BUF_CASE(9, 3, 17, 1, 256)
      TIPS_BUF_CASE(1, 2, 16, 2, 256)
      TIPS_BUF_CASE(1, 2, 16, 4, 256)
      TIPS_BUF_CASE(1, 2, 16, 1, 512)
      TIPS_BUF_CASE(1, 2, 16, 2, 128)
      TIPS_BUF_CASE(1, 2, 16, 1, 1024)
      TIPS_BUF_CASE(1, 2, 16, 1, 128)
      TIPS_BUF_CASE(7, 2, 2, 1, 64)   // (round 6: one wave per workgroup, nt stores)
      TIPS_BUF_CASE(7, 2, 2, 2, 128)  // (round 6: 128 lanes, 2 vectors per lane, nt stores)
      TIPS_BUF_CASE(1, 2, 16, 2, 512)
      TIPS_BUF_CASE(7, 2, 2, 1, 512)  // nt loads + nt stores, other tile shapes (rotating-buffer sweep)
      TIPS_BUF_CASE(7, 2, 2, 1, 1024)
      TIPS_BUF_CASE(7, 2, 2, 2, 256)
      TIPS_BUF_CASE(7, 2, 2, 4, 256)
      TIPS_BUF_CASE(7, 2, 2, 2, 512)
      TIPS_BUF_CASE(10, 2, 18, 1, 256)  // nt loads; stores nt sc1, sc0 nt sc1, sc0, sc0 nt
      TIPS_BUF_CASE(11, 2, 19, 1, 256)
      TIPS_BUF_CASE(12, 2, 1, 1, 256)
      TIPS_BUF_CASE(13, 2, 3, 1, 256)
    }
#undef TIPS_BUF_CASE
    return hipErrorInvalidValue;
  }
  // global_load/store forms: the tuning sweep's other variants (f32 only)
  if constexpr (DT == kF32) {
    TIPS_SUM2_CASE(2, 1, 2, true, false, 256)
    TIPS_SUM2_CASE(1, 1, 2, true, false, 256)
    TIPS_SUM2_CASE(1, 4, 1, true, true, 256)
    TIPS_SUM2_CASE(1, 2, 2, true, false, 256)
    TIPS_SUM2_CASE(1, 8, 2, true, false, 256)
    TIPS_SUM2_CASE(1, 2, 2, true, false, 512)
    TIPS_SUM2_CASE(1, 2, 2, true, false, 128)
    TIPS_SUM2_CASE(1, 1, 2, true, false, 512)
    TIPS_SUM2_CASE(0, 2, 2, true, false, 256)
    TIPS_SUM2_CASE(0, 4, 2, true, false, 256)
    TIPS_SUM2_CASE(2, 2, 2, true, false, 256)
    TIPS_SUM2_CASE(2, 1, 2, true, false, 512)
    TIPS_SUM2_CASE(2, 4, 1, true, true, 256)
    TIPS_SUM2_CASE(1, 1, 0, false, false, 256)
    TIPS_SUM2_CASE(1, 2, 0, false, false, 256)
    TIPS_SUM2_CASE(1, 4, 0, false, false, 256)
    TIPS_SUM2_CASE(1, 8, 0, false, false, 256)
    TIPS_SUM2_CASE(1, 1, 1, true, true, 256)
    TIPS_SUM2_CASE(1, 2, 1, true, true, 256)
    TIPS_SUM2_CASE(1, 8, 1, true, true, 256)
    TIPS_SUM2_CASE(0, 1, 0, false, false, 256)
    TIPS_SUM2_CASE(0, 2, 0, false, false, 256)
    TIPS_SUM2_CASE(0, 4, 0, false, false, 256)
    TIPS_SUM2_CASE(0, 8, 0, false, false, 256)
    TIPS_SUM2_CASE(0, 1, 1, true, true, 256)
    TIPS_SUM2_CASE(0, 2, 1, true, true, 256)
    TIPS_SUM2_CASE(0, 4, 1, true, true, 256)
    TIPS_SUM2_CASE(0, 8, 1, true, true, 256)
    TIPS_SUM2_CASE(1, 4, 2, true, false, 256)
    TIPS_SUM2_CASE(1, 2, 3, false, true, 256)
    TIPS_SUM2_CASE(1, 4, 3, false, true, 256)
    TIPS_SUM2_CASE(1, 2, 1, true, true, 512)
    TIPS_SUM2_CASE(1, 4, 1, true, true, 512)
    TIPS_SUM2_CASE(1, 8, 1, true, true, 512)
    TIPS_SUM2_CASE(1, 1, 1, true, true, 1024)
    TIPS_SUM2_CASE(1, 2, 1, true, true, 1024)
    TIPS_SUM2_CASE(1, 4, 1, true, true, 1024)
    TIPS_SUM2_CASE(1, 4, 2, true, false, 512)
    TIPS_SUM2_CASE(1, 4, 3, false, true, 512)
    TIPS_SUM2_CASE(1, 16, 1, true, true, 256)
    TIPS_SUM2_CASE(1, 16, 1, true, true, 128)
    TIPS_SUM2_CASE(1, 8, 1, true, true, 128)
    TIPS_SUM2_CASE(1, 4, 1, true, true, 128)
    TIPS_SUM2_CASE(1, 8, 1, true, true, 64)
  }
#undef TIPS_SUM2_CASE
  return hipErrorInvalidValue;
}

template <int NSRC, int U, int SAUX, int ORDER, int ITER, int ROT, int BLOCK>
hipError_t launch_multi_x(void* dst, const SrcList& sl, int64_t nvec, int64_t n, unsigned shmem, hipStream_t s) {
  const int64_t per = (int64_t)BLOCK * U * ITER;
  int64_t grid = (nvec + per - 1) / per;
  grid = std::max<int64_t>(8, (grid + 7) / 8 * 8);
  if (ORDER == 2 && (grid >> 3) >= 64) grid = (grid + 63) / 64 * 64;  // every XCD's stretch splits into 8 runs
  hipLaunchKernelGGL((multi_sum_x_kernel<NSRC, U, SAUX, ORDER, ITER, ROT, BLOCK>), dim3((unsigned)grid), dim3(BLOCK),
                     shmem, s, (u32x4*)dst, sl, nvec, nvec * 4, n);
  return hipGetLastError();
}

template <int NSRC, int BLOCK, int PIPE>
hipError_t launch_multi_gs(void* dst, const SrcList& sl, int64_t nvec, int64_t n, int wpc, hipStream_t s) {
  const int64_t tiles = (nvec + BLOCK - 1) / BLOCK;
  const int64_t grid = std::max<int64_t>(8, std::min<int64_t>((int64_t)kNumCUs * wpc, (tiles + 7) / 8 * 8));
  hipLaunchKernelGGL((multi_sum_gs_kernel<NSRC, BLOCK, PIPE>), dim3((unsigned)grid), dim3(BLOCK), 0, s, (u32x4*)dst, sl,
                     nvec, nvec * 4, n);
  return hipGetLastError();
}

// Round-5 variants (f32), all nt loads: 8 = address-order tiles; 9 = nt stores; 10 = plain stores;
// 11 / 12 = 2 / 4 consecutive tiles per workgroup in turn; 13 / 14 = 512 / 128 lanes; 15 = load
// order rotated per workgroup; 16 = XCD stretches cut into 8 interleaved runs; 17 / 18 / 19 =
// 20 / 40 / 27 KiB of unused LDS per workgroup (8 / 4 / 5 workgroups per CU); 20 = address order,
// 4 tiles per workgroup; 21 = the shipped shape through this kernel (control); 22 = address order,
// 2 vectors per lane; 23 / 24 / 25 = 80 / 53 / 32 KiB of LDS (2 / 3 / 5 workgroups per CU);
// 26 / 27 / 30 / 34 = 128 lanes with 40 / 20 / 27 / 13 KiB (4 / 8 / 5 / 12 workgroups per CU);
// 28 / 29 = 2 vectors per lane with 40 / 80 KiB; 31 = address order with 40 KiB; 32 / 33 = 64
// lanes, uncapped / 10 KiB (16 per CU); 35 = 128 lanes, 2 vectors, 20 KiB; 40-49 = the grid-stride
// form (multi_sum_gs_kernel): 128 lanes x 4 / 5 / 6 / 8 / 12 workgroups per CU (40-43, 48), the
// same pipelined x 4 / 5 / 3 (44, 45, 49); 256 lanes x 3 (46), pipelined x 2 (47).
template <int NSRC>
hipError_t run_multi_x(void* dst, const SrcList& sl, int64_t n, int variant, hipStream_t s) {
  const int64_t nvec = n / 4;
  switch (variant) {
    case 8: return launch_multi_x<NSRC, 1, 16, 1, 1, 0, 256>(dst, sl, nvec, n, 0, s);
    case 9: return launch_multi_x<NSRC, 1, 2, 0, 1, 0, 256>(dst, sl, nvec, n, 0, s);
    case 10: return launch_multi_x<NSRC, 1, 0, 0, 1, 0, 256>(dst, sl, nvec, n, 0, s);
    case 11: return launch_multi_x<NSRC, 1, 16, 0, 2, 0, 256>(dst, sl, nvec, n, 0, s);
    case 12: return launch_multi_x<NSRC, 1, 16, 0, 4, 0, 256>(dst, sl, nvec, n, 0, s);
    case 13: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 512>(dst, sl, nvec, n, 0, s);
    case 14: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 128>(dst, sl, nvec, n, 0, s);
    case 15: return launch_multi_x<NSRC, 1, 16, 0, 1, 1, 256>(dst, sl, nvec, n, 0, s);
    case 16: return launch_multi_x<NSRC, 1, 16, 2, 1, 0, 256>(dst, sl, nvec, n, 0, s);
    case 17: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 256>(dst, sl, nvec, n, 20 << 10, s);
    case 18: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 256>(dst, sl, nvec, n, 40 << 10, s);
    case 19: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 256>(dst, sl, nvec, n, 27 << 10, s);
    case 20: return launch_multi_x<NSRC, 1, 16, 1, 4, 0, 256>(dst, sl, nvec, n, 0, s);
    case 21: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 256>(dst, sl, nvec, n, 0, s);
    case 22: return launch_multi_x<NSRC, 2, 16, 1, 1, 0, 256>(dst, sl, nvec, n, 0, s);
    case 23: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 256>(dst, sl, nvec, n, 80 << 10, s);
    case 24: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 256>(dst, sl, nvec, n, 53 << 10, s);
    case 25: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 256>(dst, sl, nvec, n, 32 << 10, s);
    case 26: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 128>(dst, sl, nvec, n, 40 << 10, s);
    case 27: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 128>(dst, sl, nvec, n, 20 << 10, s);
    case 28: return launch_multi_x<NSRC, 2, 16, 0, 1, 0, 256>(dst, sl, nvec, n, 40 << 10, s);
    case 29: return launch_multi_x<NSRC, 2, 16, 0, 1, 0, 256>(dst, sl, nvec, n, 80 << 10, s);
    case 30: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 128>(dst, sl, nvec, n, 27 << 10, s);
    case 31: return launch_multi_x<NSRC, 1, 16, 1, 1, 0, 256>(dst, sl, nvec, n, 40 << 10, s);
    case 32: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 64>(dst, sl, nvec, n, 0, s);
    case 33: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 64>(dst, sl, nvec, n, 10 << 10, s);
    case 34: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 128>(dst, sl, nvec, n, 13 << 10, s);
    case 35: return launch_multi_x<NSRC, 2, 16, 0, 1, 0, 128>(dst, sl, nvec, n, 20 << 10, s);
    case 50: {  // what tips_multi_sum launches
      const void* p[NSRC];
      for (int j = 0; j < NSRC; j++) p[j] = sl.p[j];
      return launch_multi_sum(dst, p, NSRC, n, kF32, s);
    }
    case 51: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 64>(dst, sl, nvec, n, 16384, s);   // 64 x 10
    case 52: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 64>(dst, sl, nvec, n, 13312, s);   // 64 x 12
    case 53: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 64>(dst, sl, nvec, n, 20480, s);   // 64 x 8
    case 54: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 128>(dst, sl, nvec, n, 26624, s);  // 128 x 6
    case 55: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 128>(dst, sl, nvec, n, 32768, s);  // 128 x 5 (no room)
    case 56: return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 192>(dst, sl, nvec, n, 32768, s);  // 192 x 5
    case 36:  // the round-4 shipped fold (no cap; 4 vectors per lane for > 4 sources of 3-24 MiB)
      if (NSRC > 4 && nvec * 16 >= (3 << 20) && nvec * 16 <= (24 << 20))
        return launch_multi_x<NSRC, 4, 16, 0, 1, 0, 256>(dst, sl, nvec, n, 0, s);
      return launch_multi_x<NSRC, 1, 16, 0, 1, 0, 256>(dst, sl, nvec, n, 0, s);
    case 40: return launch_multi_gs<NSRC, 128, 0>(dst, sl, nvec, n, 4, s);
    case 41: return launch_multi_gs<NSRC, 128, 0>(dst, sl, nvec, n, 5, s);
    case 42: return launch_multi_gs<NSRC, 128, 0>(dst, sl, nvec, n, 6, s);
    case 43: return launch_multi_gs<NSRC, 128, 0>(dst, sl, nvec, n, 8, s);
    case 44: return launch_multi_gs<NSRC, 128, 1>(dst, sl, nvec, n, 4, s);
    case 45: return launch_multi_gs<NSRC, 128, 1>(dst, sl, nvec, n, 5, s);
    case 46: return launch_multi_gs<NSRC, 256, 0>(dst, sl, nvec, n, 3, s);
    case 47: return launch_multi_gs<NSRC, 256, 1>(dst, sl, nvec, n, 2, s);
    case 48: return launch_multi_gs<NSRC, 128, 0>(dst, sl, nvec, n, 12, s);
    case 49: return launch_multi_gs<NSRC, 128, 1>(dst, sl, nvec, n, 3, s);
    default: return hipErrorInvalidValue;
  }
}

// Sweep entry (f32; nsrc 2, 4, 8): 0 = global nt loads (U 2 for nsrc <= 4, else 1),
// 1 = buffer nt loads U 1, 2 = buffer nt loads U 2, 3 = buffer plain loads U 1, 4 = buffer nt loads U 4.
template <int NSRC>
hipError_t run_multi_variant(void* dst, const SrcList& sl, int64_t n, int variant, hipStream_t s) {
  const int64_t nvec = n / 4;
  auto grid_for = [&](int u) {
    int64_t g = (nvec + (int64_t)kBlock * u - 1) / ((int64_t)kBlock * u);
    return (unsigned)std::max<int64_t>(8, (g + 7) / 8 * 8);
  };
  switch (variant) {
    case 0: {
      constexpr int U = NSRC <= 4 ? 2 : 1;
      hipLaunchKernelGGL((multi_sum_kernel<kF32, NSRC, U>), dim3(grid_for(U)), dim3(kBlock), 0, s, (u32x4*)dst, sl,
                         nvec, nvec * 4, n);
      break;
    }
    case 1:
      hipLaunchKernelGGL((multi_sum_buf_kernel<kF32, NSRC, 1, 2>), dim3(grid_for(1)), dim3(kBlock), 0, s,
                         (u32x4*)dst, sl, nvec, nvec * 4, n, (int64_t)0);
      break;
    case 2:
      hipLaunchKernelGGL((multi_sum_buf_kernel<kF32, NSRC, 2, 2>), dim3(grid_for(2)), dim3(kBlock), 0, s,
                         (u32x4*)dst, sl, nvec, nvec * 4, n, (int64_t)0);
      break;
    case 3:
      hipLaunchKernelGGL((multi_sum_buf_kernel<kF32, NSRC, 1, 0>), dim3(grid_for(1)), dim3(kBlock), 0, s,
                         (u32x4*)dst, sl, nvec, nvec * 4, n, (int64_t)0);
      break;
    case 4:
      hipLaunchKernelGGL((multi_sum_buf_kernel<kF32, NSRC, 4, 2>), dim3(grid_for(4)), dim3(kBlock), 0, s,
                         (u32x4*)dst, sl, nvec, nvec * 4, n, (int64_t)0);
      break;
    case 5:  // sc0 loads
      hipLaunchKernelGGL((multi_sum_buf_kernel<kF32, NSRC, 1, 1>), dim3(grid_for(1)), dim3(kBlock), 0, s,
                         (u32x4*)dst, sl, nvec, nvec * 4, n, (int64_t)0);
      break;
    case 6:  // sc1 loads
      hipLaunchKernelGGL((multi_sum_buf_kernel<kF32, NSRC, 1, 16>), dim3(grid_for(1)), dim3(kBlock), 0, s,
                         (u32x4*)dst, sl, nvec, nvec * 4, n, (int64_t)0);
      break;
    case 7:  // plain loads, 2 vectors per lane
      hipLaunchKernelGGL((multi_sum_buf_kernel<kF32, NSRC, 2, 0>), dim3(grid_for(2)), dim3(kBlock), 0, s,
                         (u32x4*)dst, sl, nvec, nvec * 4, n, (int64_t)0);
      break;
    default:
      return run_multi_x<NSRC>(dst, sl, n, variant, s);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_sum2_variant(void* dst, const void* a, const void* b, int64_t n, int dtype, int mode, int unroll,
                               int nt, int blocks, int threads, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  switch (dtype) {
    case kF32: return sum2_dispatch<kF32>(dst, a, b, n, mode, unroll, nt, blocks, threads, s);
    case kF64: return sum2_dispatch<kF64>(dst, a, b, n, mode, unroll, nt, blocks, threads, s);
    case kI32: return sum2_dispatch<kI32>(dst, a, b, n, mode, unroll, nt, blocks, threads, s);
    case kI64: return sum2_dispatch<kI64>(dst, a, b, n, mode, unroll, nt, blocks, threads, s);
    case kF16: return sum2_dispatch<kF16>(dst, a, b, n, mode, unroll, nt, blocks, threads, s);
    case kBF16: return sum2_dispatch<kBF16>(dst, a, b, n, mode, unroll, nt, blocks, threads, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_multi_sum_variant(void* dst, const void* const* srcs, int nsrc, int64_t n, int dtype, int variant,
                                   hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (dtype != kF32 || !aligned16(dst)) return hipErrorInvalidValue;
  SrcList sl{};
  for (int j = 0; j < nsrc && j < kMaxSrcs; j++) {
    if (!aligned16(srcs[j])) return hipErrorInvalidValue;
    sl.p[j] = (const u32x4*)srcs[j];
  }
  switch (nsrc) {
    case 2: return run_multi_variant<2>(dst, sl, n, variant, s);
    case 4: return run_multi_variant<4>(dst, sl, n, variant, s);
    case 8: return run_multi_variant<8>(dst, sl, n, variant, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_copy_tiles(const CopyTile* tiles_dev, int ntiles, hipStream_t s) {
  if (ntiles <= 0) return hipSuccess;
  const unsigned grid = (unsigned)((ntiles + 7) / 8 * 8);
  hipLaunchKernelGGL(copy_tiles_kernel, dim3(grid), dim3(kBlock), 0, s, tiles_dev, ntiles);
  return hipGetLastError();
}

namespace {

template <int G, int U, int LAUX, int SAUX>
hipError_t run_copy_g(const CopyTile* tiles, int ntiles, hipStream_t s) {
  const int64_t groups = (ntiles + G - 1) / G;
  const unsigned grid = (unsigned)std::max<int64_t>(8, (groups + 7) / 8 * 8);
  hipLaunchKernelGGL((copy_tiles_g_kernel<G, U, LAUX, SAUX>), dim3(grid), dim3(kBlock), 0, s, tiles, ntiles);
  return hipGetLastError();
}

template <int U>
hipError_t copy_variant_u(const CopyTile* tiles, int ntiles, int variant, hipStream_t s) {
  switch (variant) {
    case 1: return run_copy_g<1, U, 2, 16>(tiles, ntiles, s);
    case 2: return run_copy_g<2, U, 2, 16>(tiles, ntiles, s);
    case 3: return run_copy_g<4, U, 2, 16>(tiles, ntiles, s);
    case 4: return run_copy_g<8, U, 2, 16>(tiles, ntiles, s);
    case 5: return run_copy_g<2, U, 0, 16>(tiles, ntiles, s);  // plain loads
    case 6: return run_copy_g<2, U, 2, 2>(tiles, ntiles, s);   // nt stores
    case 7: return run_copy_g<2, U, 2, 0>(tiles, ntiles, s);   // plain stores
    case 8: return run_copy_g<4, U, 0, 0>(tiles, ntiles, s);   // plain both
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t launch_copy_tiles_variant(const CopyTile* tiles_dev, int ntiles, int variant, int64_t max_tile_bytes,
                                     hipStream_t s) {
  if (ntiles <= 0) return hipSuccess;
  if (variant == 0) return launch_copy_tiles(tiles_dev, ntiles, s);
  if (max_tile_bytes <= 4096) return copy_variant_u<1>(tiles_dev, ntiles, variant, s);
  if (max_tile_bytes <= 8192) return copy_variant_u<2>(tiles_dev, ntiles, variant, s);
  if (max_tile_bytes <= 16384) return copy_variant_u<4>(tiles_dev, ntiles, variant, s);
  return hipErrorInvalidValue;  // the grouped kernel holds a tile in registers: at most 16 KiB
}

}  // namespace tips
