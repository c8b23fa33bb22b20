// adasum.hip — the Adasum pair: out = ca a + cb b per segment.
//
// A call reduces a list of segments (one tensor each). For two operands a and b holding the same
// segments, for each segment s independently:
//
//   d  = SUM a_i b_i    na = SUM a_i a_i    nb = SUM b_i b_i        (over the elements of s, in f64)
//   ca = (na > 0) ? 1.0 - 0.5 (d / na) : 1.0                        (f64, each operation a separate IEEE op)
//   cb = (nb > 0) ? 1.0 - 0.5 (d / nb) : 1.0
//   out_i = round_S( fl_W( fl_W(ca_W a_i) + fl_W(cb_W b_i) ) )
//
// W is the working type (fp32 for f32 / f16 / bf16, f64 for f64), ca_W / cb_W the coefficients
// rounded once from f64 to W, S the storage type: one rounding at the store (bf16 through
// bf16_round_bits). The threshold is exact zero. Nothing is done about non-finite values: a NaN or an
// infinity anywhere in a segment of either operand makes that segment's coefficients non-finite and
// its whole result NaN; the other segments do not see it.
//
// The order of the three sums is a function of the segment's length and the dtype alone. With
// E = 16 / sizeof(element) elements per 16-B vector and K = 2048 E elements per chunk (32 KiB):
//   lane   element i of the segment belongs to chunk i / K and, inside it, to lane (i % K / E) % 256.
//          A lane adds its elements' products in ascending i to an accumulator that starts at +0
//          (f32 / f16 / bf16 products are exact in f64, so one fma per element; f64 inputs: a
//          multiply, then an add).
//   chunk  the 256 lane sums of a chunk: within each wave of 64 the halving tree x[l] += x[l + 32],
//          x[l] += x[l + 16], ... x[l] += x[l + 1]; then ((w0 + w1) + w2) + w3 over the four waves.
//   segment (coef pass) the chunk sums c_0 ... c_{m-1}: lane t adds c_t, c_{t + 256}, ... in that
//          order from +0, and the 256 lane sums go through the same wave tree and wave order.
// Which workgroup computes a chunk, the grid, the XCD map, the pointers' alignment, the segment's
// place in the buffer and its neighbours change none of it: a chunk's vectors are read 16 B per lane
// when a, b (and, for the combine, dst) are 16-B aligned at the segment's start and the vector lies
// wholly inside the segment, and element by element otherwise - into the same lane, the same order.
//
// Three launches, the kernel boundary the only synchronisation (no float atomics, no hand-off
// between workgroups): dots (one workgroup per chunk -> 3 doubles per chunk), coef (one workgroup
// per segment -> ca, cb in f64), combine (one workgroup per chunk, the dots' chunk map). 5 passes
// over a buffer's bytes: 2 reads for the dots, 2 reads and 1 write for the combine.
//
// Device helpers (16-B loads / stores, Wide, WorkOf, the separate multiply / add forms,
// bf16_round_bits, the XCD stripes) come from kernels_device.h.
#include <algorithm>

#include "adasum.h"
#include "kernels_device.h"

namespace tips {

namespace {

constexpr int kAdaU = 8;  // 16-B vectors per lane per chunk
static_assert(kAdaChunkBytes == (int64_t)kBlock * kAdaU * 16, "a chunk is 256 lanes x 8 vectors");

// the segment that chunk t belongs to: the last one whose chunk0 <= t (empty segments share their
// successor's chunk0 and sit before it)
__device__ __forceinline__ AdaSeg seg_of_chunk(const AdaSegs& segs, int64_t t, int* index) {
  if (!segs.table) {
    *index = 0;
    return segs.one;
  }
  int lo = 0, hi = segs.nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs.table[mid].chunk0 <= t) lo = mid;
    else hi = mid - 1;
  }
  *index = lo;
  return segs.table[lo];
}

// element j (0 <= j < E) of a 16-B vector, as a double (every storage value is exact in f64)
template <int DT>
__device__ __forceinline__ double vec_elem(u32x4 v, int j) {
  if constexpr (DT == kF32) return (double)__builtin_bit_cast(f32x4, v)[j];
  else if constexpr (DT == kF64) return __builtin_bit_cast(f64x2, v)[j];
  else if constexpr (DT == kF16) return (double)(float)__builtin_bit_cast(f16x8, v)[j];
  else {
    const unsigned w = v[j >> 1];
    return (double)__builtin_bit_cast(float, (j & 1) ? (w & 0xffff0000u) : (w << 16));
  }
}

struct Dots {
  double d, na, nb;
};

template <int DT>
__device__ __forceinline__ void dots_add(Dots& acc, double x, double y) {
#pragma clang fp contract(off)
  if constexpr (DT == kF64) {
    const double xy = x * y, xx = x * x, yy = y * y;
    acc.d = acc.d + xy;
    acc.na = acc.na + xx;
    acc.nb = acc.nb + yy;
  } else {  // the products are exact: the fma rounds once, as the separate add would
    acc.d = __builtin_fma(x, y, acc.d);
    acc.na = __builtin_fma(x, x, acc.na);
    acc.nb = __builtin_fma(y, y, acc.nb);
  }
}

// The 256 lanes' values to one, in the fixed order of the head comment; the result is valid in lane 0
// of the workgroup. lds: 4 doubles per value in flight.
__device__ __forceinline__ double wave_tree(double x) {
#pragma clang fp contract(off)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x = x + __shfl_down(x, d, 64);
  return x;
}

__device__ __forceinline__ Dots block_tree(Dots v, double (*lds)[3]) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  v.d = wave_tree(v.d);
  v.na = wave_tree(v.na);
  v.nb = wave_tree(v.nb);
  if (lane == 0) {
    lds[w][0] = v.d;
    lds[w][1] = v.na;
    lds[w][2] = v.nb;
  }
  __syncthreads();
  Dots r;
  r.d = ((lds[0][0] + lds[1][0]) + lds[2][0]) + lds[3][0];
  r.na = ((lds[0][1] + lds[1][1]) + lds[2][1]) + lds[3][1];
  r.nb = ((lds[0][2] + lds[1][2]) + lds[2][2]) + lds[3][2];
  return r;
}

template <int DT>
__global__ __launch_bounds__(kBlock) void adasum_dots_kernel(const void* a, const void* b, AdaSegs segs, int64_t nchunks,
                                                             int64_t stripe, double* __restrict__ partials) {
  using T = typename ScalarOf<DT>::T;
  constexpr int E = 16 / (int)sizeof(T);
  constexpr int64_t K = (int64_t)kBlock * kAdaU * E;
  __shared__ double lds[kBlock / 64][3];
  const int64_t t = stripe_tile(blockIdx.x, gridDim.x, stripe);
  if (t >= nchunks) return;  // (whole workgroups: nobody waits at the barrier below)
  int si;
  const AdaSeg sg = seg_of_chunk(segs, t, &si);
  const int64_t base = (t - sg.chunk0) * K;
  const int64_t rem = sg.count - base;  // elements of the segment from this chunk's first one on
  const T* pa = (const T*)a + sg.off + base;
  const T* pb = (const T*)b + sg.off + base;
  const bool vec = ((reinterpret_cast<uintptr_t>(pa) | reinterpret_cast<uintptr_t>(pb)) & 15) == 0;
  const int tid = threadIdx.x;
  Dots acc = {0.0, 0.0, 0.0};
  if (vec && rem >= K) {  // a whole chunk of aligned vectors: all 16 loads in flight, then the sums
    u32x4 x[kAdaU], y[kAdaU];
#pragma unroll
    for (int u = 0; u < kAdaU; u++) x[u] = ld16<false>((const u32x4*)pa + u * kBlock + tid);
#pragma unroll
    for (int u = 0; u < kAdaU; u++) y[u] = ld16<false>((const u32x4*)pb + u * kBlock + tid);
#pragma unroll
    for (int u = 0; u < kAdaU; u++)
#pragma unroll
      for (int j = 0; j < E; j++) dots_add<DT>(acc, vec_elem<DT>(x[u], j), vec_elem<DT>(y[u], j));
  } else if (rem > 0) {
#pragma unroll 2
    for (int u = 0; u < kAdaU; u++) {
      const int64_t i0 = ((int64_t)u * kBlock + tid) * E;
      if (i0 >= rem) break;
      if (vec && i0 + E <= rem) {
        const u32x4 x = ld16<false>((const u32x4*)pa + u * kBlock + tid), y = ld16<false>((const u32x4*)pb + u * kBlock + tid);
#pragma unroll
        for (int j = 0; j < E; j++) dots_add<DT>(acc, vec_elem<DT>(x, j), vec_elem<DT>(y, j));
      } else {
        for (int j = 0; j < E && i0 + j < rem; j++)
          dots_add<DT>(acc, (double)load_work<DT>(pa, i0 + j), (double)load_work<DT>(pb, i0 + j));
      }
    }
  }
  const Dots r = block_tree(acc, lds);
  if (tid == 0) {
    partials[3 * t] = r.d;
    partials[3 * t + 1] = r.na;
    partials[3 * t + 2] = r.nb;
  }
}

// One workgroup per segment: its chunks' partials to (d, na, nb), then the coefficients.
__global__ __launch_bounds__(kBlock) void adasum_coef_kernel(AdaSegs segs, int64_t chunk_elems,
                                                             const double* __restrict__ partials,
                                                             double* __restrict__ coef) {
#pragma clang fp contract(off)
  __shared__ double lds[kBlock / 64][3];
  const int si = blockIdx.x;
  const AdaSeg sg = segs.table ? segs.table[si] : segs.one;
  const int64_t m = (sg.count + chunk_elems - 1) / chunk_elems;
  const double* p = partials + 3 * sg.chunk0;
  Dots acc = {0.0, 0.0, 0.0};
  for (int64_t c = threadIdx.x; c < m; c += kBlock) {
    acc.d = acc.d + p[3 * c];
    acc.na = acc.na + p[3 * c + 1];
    acc.nb = acc.nb + p[3 * c + 2];
  }
  const Dots r = block_tree(acc, lds);
  if (threadIdx.x == 0) {
    double ca = 1.0, cb = 1.0;
    if (r.na > 0) {
      const double q = r.d / r.na;
      const double h = 0.5 * q;
      ca = 1.0 - h;
    }
    if (r.nb > 0) {
      const double q = r.d / r.nb;
      const double h = 0.5 * q;
      cb = 1.0 - h;
    }
    coef[2 * si] = ca;
    coef[2 * si + 1] = cb;
  }
}

template <int DT>
__device__ __forceinline__ u32x4 combine16(u32x4 x, u32x4 y, typename WorkOf<DT>::T ca, typename WorkOf<DT>::T cb) {
  return Wide<DT>::store(separate_add<DT>(scaled_load<DT>(x, ca), scaled_load<DT>(y, cb)));
}

template <int DT>
__device__ __forceinline__ void combine_elem(void* dst, const void* a, const void* b, int64_t i,
                                             typename WorkOf<DT>::T ca, typename WorkOf<DT>::T cb) {
#pragma clang fp contract(off)
  const typename WorkOf<DT>::T x = load_work<DT>(a, i) * ca;
  const typename WorkOf<DT>::T y = load_work<DT>(b, i) * cb;
  store_work<DT>(dst, i, x + y);
}

// dst may be a or b: every lane stores only where it has already loaded both operands.
template <int DT>
__global__ __launch_bounds__(kBlock) void adasum_combine_kernel(void* dst, const void* a, const void* b, AdaSegs segs,
                                                                int64_t nchunks, int64_t stripe,
                                                                const double* __restrict__ coef) {
  using T = typename ScalarOf<DT>::T;
  using F = typename WorkOf<DT>::T;
  constexpr int E = 16 / (int)sizeof(T);
  constexpr int64_t K = (int64_t)kBlock * kAdaU * E;
  const int64_t t = stripe_tile(blockIdx.x, gridDim.x, stripe);
  if (t >= nchunks) return;
  int si;
  const AdaSeg sg = seg_of_chunk(segs, t, &si);
  const F ca = (F)coef[2 * si], cb = (F)coef[2 * si + 1];  // (the one rounding f64 -> W)
  const int64_t base = (t - sg.chunk0) * K;
  const int64_t rem = sg.count - base;
  const T* pa = (const T*)a + sg.off + base;
  const T* pb = (const T*)b + sg.off + base;
  T* pd = (T*)dst + sg.off + base;
  const bool vec =
      ((reinterpret_cast<uintptr_t>(pa) | reinterpret_cast<uintptr_t>(pb) | reinterpret_cast<uintptr_t>(pd)) & 15) == 0;
  const int tid = threadIdx.x;
  if (vec && rem >= K) {
    u32x4 x[kAdaU], y[kAdaU];
#pragma unroll
    for (int u = 0; u < kAdaU; u++) x[u] = ld16<true>((const u32x4*)pa + u * kBlock + tid);
#pragma unroll
    for (int u = 0; u < kAdaU; u++) y[u] = ld16<true>((const u32x4*)pb + u * kBlock + tid);
#pragma unroll
    for (int u = 0; u < kAdaU; u++) st16<false>((u32x4*)pd + u * kBlock + tid, combine16<DT>(x[u], y[u], ca, cb));
  } else if (rem > 0) {
#pragma unroll 2
    for (int u = 0; u < kAdaU; u++) {
      const int64_t i0 = ((int64_t)u * kBlock + tid) * E;
      if (i0 >= rem) break;
      if (vec && i0 + E <= rem) {
        const u32x4 x = ld16<true>((const u32x4*)pa + u * kBlock + tid), y = ld16<true>((const u32x4*)pb + u * kBlock + tid);
        st16<false>((u32x4*)pd + u * kBlock + tid, combine16<DT>(x, y, ca, cb));
      } else {
        for (int j = 0; j < E && i0 + j < rem; j++) combine_elem<DT>(pd, pa, pb, i0 + j, ca, cb);
      }
    }
  }
}

// the chunk launches' grid: the 2-input sum's XCD stripes (512 KiB of each operand = 16 chunks per
// stripe), whole rounds of 8 stripes; workgroups past the last chunk leave at once
hipError_t chunk_grid(int64_t nchunks, unsigned* grid, int64_t* stripe) {
  *stripe = sum_stripe_of((int64_t)kBlock * kAdaU);
  const int64_t g = stripe_grid(nchunks, *stripe);
  if (nchunks <= 0 || g > 0x7fffffff) return hipErrorInvalidValue;
  *grid = (unsigned)g;
  return hipSuccess;
}

bool bad_segs(const AdaSegs& segs) { return segs.nseg < 1 || (!segs.table && segs.nseg != 1); }

}  // namespace

int64_t adasum_chunk_elems(int dtype) {
  switch (dtype) {
    case kF32: return kAdaChunkBytes / 4;
    case kF64: return kAdaChunkBytes / 8;
    case kF16:
    case kBF16: return kAdaChunkBytes / 2;
    default: return 0;
  }
}

hipError_t launch_adasum_dots(const void* a, const void* b, AdaSegs segs, int64_t nchunks, int dtype, double* partials,
                              hipStream_t s) {
  unsigned grid;
  int64_t stripe;
  if (bad_segs(segs) || !a || !b || !partials) return hipErrorInvalidValue;
  hipError_t err = chunk_grid(nchunks, &grid, &stripe);
  if (err != hipSuccess) return err;
  switch (dtype) {
    case kF32: hipLaunchKernelGGL(adasum_dots_kernel<kF32>, dim3(grid), dim3(kBlock), 0, s, a, b, segs, nchunks, stripe, partials); break;
    case kF64: hipLaunchKernelGGL(adasum_dots_kernel<kF64>, dim3(grid), dim3(kBlock), 0, s, a, b, segs, nchunks, stripe, partials); break;
    case kF16: hipLaunchKernelGGL(adasum_dots_kernel<kF16>, dim3(grid), dim3(kBlock), 0, s, a, b, segs, nchunks, stripe, partials); break;
    case kBF16: hipLaunchKernelGGL(adasum_dots_kernel<kBF16>, dim3(grid), dim3(kBlock), 0, s, a, b, segs, nchunks, stripe, partials); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_adasum_coef(AdaSegs segs, int dtype, const double* partials, double* coef, hipStream_t s) {
  const int64_t K = adasum_chunk_elems(dtype);
  if (bad_segs(segs) || K <= 0 || !partials || !coef) return hipErrorInvalidValue;
  hipLaunchKernelGGL(adasum_coef_kernel, dim3((unsigned)segs.nseg), dim3(kBlock), 0, s, segs, K, partials, coef);
  return hipGetLastError();
}

hipError_t launch_adasum_combine(void* dst, const void* a, const void* b, AdaSegs segs, int64_t nchunks, int dtype,
                                 const double* coef, hipStream_t s) {
  unsigned grid;
  int64_t stripe;
  if (bad_segs(segs) || !dst || !a || !b || !coef) return hipErrorInvalidValue;
  hipError_t err = chunk_grid(nchunks, &grid, &stripe);
  if (err != hipSuccess) return err;
  switch (dtype) {
    case kF32: hipLaunchKernelGGL(adasum_combine_kernel<kF32>, dim3(grid), dim3(kBlock), 0, s, dst, a, b, segs, nchunks, stripe, coef); break;
    case kF64: hipLaunchKernelGGL(adasum_combine_kernel<kF64>, dim3(grid), dim3(kBlock), 0, s, dst, a, b, segs, nchunks, stripe, coef); break;
    case kF16: hipLaunchKernelGGL(adasum_combine_kernel<kF16>, dim3(grid), dim3(kBlock), 0, s, dst, a, b, segs, nchunks, stripe, coef); break;
    case kBF16: hipLaunchKernelGGL(adasum_combine_kernel<kBF16>, dim3(grid), dim3(kBlock), 0, s, dst, a, b, segs, nchunks, stripe, coef); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_adasum_pair(void* dst, const void* a, const void* b, AdaSegs segs, int64_t nchunks, int dtype,
                              void* workspace, hipStream_t s) {
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return hipErrorInvalidValue;
  double* partials = (double*)workspace;
  double* coef = partials + 3 * nchunks;
  hipError_t err = launch_adasum_dots(a, b, segs, nchunks, dtype, partials, s);
  if (err != hipSuccess) return err;
  if ((err = launch_adasum_coef(segs, dtype, partials, coef, s)) != hipSuccess) return err;
  return launch_adasum_combine(dst, a, b, segs, nchunks, dtype, coef, s);
}

}  // namespace tips
