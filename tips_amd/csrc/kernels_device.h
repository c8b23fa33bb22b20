// kernels_device.h — the device vocabulary of the reduction kernels (16-byte vectors, per-dtype
// arithmetic, the scaled forms, the workgroup -> tile maps) and the kernel templates that both
// kernels.hip (what the product launches) and kernels_dev.hip (the tuning sweeps of
// libtips_hip_dev.so) instantiate. HIP translation units only. Design: kernels.hip's head comment.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.h"

namespace tips {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

enum { kF32 = 0, kF64 = 1, kI32 = 2, kI64 = 3, kF16 = 4, kBF16 = 5 };
constexpr int kBlock = 256;  // 4 waves of 64

// ---------------------------------------------------------------------------
// 16-byte loads / stores

template <bool NT>
__device__ __forceinline__ u32x4 ld16(const u32x4* p) {
  if constexpr (NT) {
    return __builtin_nontemporal_load(p);
  } else {
    return *p;
  }
}

template <bool NT>
__device__ __forceinline__ void st16(u32x4* p, u32x4 v) {
  if constexpr (NT) {
    __builtin_nontemporal_store(v, p);
  } else {
    *p = v;
  }
}

// ---------------------------------------------------------------------------
// bf16 helpers: exact same rounding as oracle_float_to_bf16 (oracle/oracle.c)

__device__ __forceinline__ unsigned bf16_round_bits(unsigned x) {
  return ((x & 0x7fffffffu) > 0x7f800000u) ? ((x >> 16) | 0x40u) : ((x + 0x7fffu + ((x >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ u32x4 bf16_pack(f32x4 lo, f32x4 hi) {
  u32x4 l = __builtin_bit_cast(u32x4, lo), h = __builtin_bit_cast(u32x4, hi);
  u32x4 r;
#pragma unroll
  for (int i = 0; i < 4; i++) r[i] = bf16_round_bits(l[i]) | (bf16_round_bits(h[i]) << 16);
  return r;
}

__device__ __forceinline__ f32x4 bf16_lo(u32x4 v) { return __builtin_bit_cast(f32x4, v << 16u); }
__device__ __forceinline__ f32x4 bf16_hi(u32x4 v) { return __builtin_bit_cast(f32x4, v & 0xffff0000u); }

// ---------------------------------------------------------------------------
// 16-byte vector add per dtype (storage-precision result: one MPI_SUM step)

template <int DT>
__device__ __forceinline__ u32x4 add16(u32x4 a, u32x4 b);

template <>
__device__ __forceinline__ u32x4 add16<kF32>(u32x4 a, u32x4 b) {
  return __builtin_bit_cast(u32x4, __builtin_bit_cast(f32x4, a) + __builtin_bit_cast(f32x4, b));
}
template <>
__device__ __forceinline__ u32x4 add16<kF64>(u32x4 a, u32x4 b) {
  return __builtin_bit_cast(u32x4, __builtin_bit_cast(f64x2, a) + __builtin_bit_cast(f64x2, b));
}
template <>
__device__ __forceinline__ u32x4 add16<kI32>(u32x4 a, u32x4 b) {
  return a + b;
}
template <>
__device__ __forceinline__ u32x4 add16<kI64>(u32x4 a, u32x4 b) {
  return __builtin_bit_cast(u32x4, __builtin_bit_cast(u64x2, a) + __builtin_bit_cast(u64x2, b));
}
template <>
__device__ __forceinline__ u32x4 add16<kF16>(u32x4 a, u32x4 b) {
  return __builtin_bit_cast(u32x4, __builtin_bit_cast(f16x8, a) + __builtin_bit_cast(f16x8, b));
}
template <>
__device__ __forceinline__ u32x4 add16<kBF16>(u32x4 a, u32x4 b) {
  return bf16_pack(bf16_lo(a) + bf16_lo(b), bf16_hi(a) + bf16_hi(b));
}

// Scalar element add for the tail (same arithmetic as add16, one element).
template <int DT>
__device__ __forceinline__ void add_elem(void* dst, const void* a, const void* b, int64_t i);

template <>
__device__ __forceinline__ void add_elem<kF32>(void* d, const void* a, const void* b, int64_t i) {
  ((float*)d)[i] = ((const float*)a)[i] + ((const float*)b)[i];
}
template <>
__device__ __forceinline__ void add_elem<kF64>(void* d, const void* a, const void* b, int64_t i) {
  ((double*)d)[i] = ((const double*)a)[i] + ((const double*)b)[i];
}
template <>
__device__ __forceinline__ void add_elem<kI32>(void* d, const void* a, const void* b, int64_t i) {
  ((unsigned*)d)[i] = ((const unsigned*)a)[i] + ((const unsigned*)b)[i];
}
template <>
__device__ __forceinline__ void add_elem<kI64>(void* d, const void* a, const void* b, int64_t i) {
  ((unsigned long long*)d)[i] = ((const unsigned long long*)a)[i] + ((const unsigned long long*)b)[i];
}
template <>
__device__ __forceinline__ void add_elem<kF16>(void* d, const void* a, const void* b, int64_t i) {
  ((_Float16*)d)[i] = ((const _Float16*)a)[i] + ((const _Float16*)b)[i];
}
template <>
__device__ __forceinline__ void add_elem<kBF16>(void* d, const void* a, const void* b, int64_t i) {
  unsigned x = (unsigned)((const unsigned short*)a)[i] << 16, y = (unsigned)((const unsigned short*)b)[i] << 16;
  float s = __builtin_bit_cast(float, x) + __builtin_bit_cast(float, y);
  ((unsigned short*)d)[i] = (unsigned short)bf16_round_bits(__builtin_bit_cast(unsigned, s));
}

// The accumulation type of a 16-byte vector per dtype (the multi-input fold and the scaled forms):
// f16/bf16 widen to fp32 and round once at the store; the others stay in their storage type.
template <int DT>
struct Wide;
template <>
struct Wide<kF32> {
  using A = f32x4;
  static __device__ A load(u32x4 v) { return __builtin_bit_cast(f32x4, v); }
  static __device__ u32x4 store(A a) { return __builtin_bit_cast(u32x4, a); }
};
template <>
struct Wide<kF64> {
  using A = f64x2;
  static __device__ A load(u32x4 v) { return __builtin_bit_cast(f64x2, v); }
  static __device__ u32x4 store(A a) { return __builtin_bit_cast(u32x4, a); }
};
template <>
struct Wide<kI32> {
  using A = u32x4;
  static __device__ A load(u32x4 v) { return v; }
  static __device__ u32x4 store(A a) { return a; }
};
template <>
struct Wide<kI64> {
  using A = u64x2;
  static __device__ A load(u32x4 v) { return __builtin_bit_cast(u64x2, v); }
  static __device__ u32x4 store(A a) { return __builtin_bit_cast(u32x4, a); }
};
template <>
struct Wide<kF16> {
  using A = f32x8;
  static __device__ A load(u32x4 v) { return __builtin_convertvector(__builtin_bit_cast(f16x8, v), f32x8); }
  static __device__ u32x4 store(A a) { return __builtin_bit_cast(u32x4, __builtin_convertvector(a, f16x8)); }
};
template <>
struct Wide<kBF16> {
  using A = f32x8;
  static __device__ A load(u32x4 v) {
    f32x4 lo = bf16_lo(v), hi = bf16_hi(v);
    return A{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  }
  static __device__ u32x4 store(A a) {
    return bf16_pack(f32x4{a[0], a[1], a[2], a[3]}, f32x4{a[4], a[5], a[6], a[7]});
  }
};

template <int DT>
struct ScalarOf;
template <>
struct ScalarOf<kF32> {
  using T = float;
};
template <>
struct ScalarOf<kF64> {
  using T = double;
};
template <>
struct ScalarOf<kI32> {
  using T = unsigned;
};
template <>
struct ScalarOf<kI64> {
  using T = unsigned long long;
};
template <>
struct ScalarOf<kF16> {
  using T = _Float16;
};
template <>
struct ScalarOf<kBF16> {
  using T = unsigned short;
};

// ---------------------------------------------------------------------------
// Scaled forms (DESIGN.md §Scaled allreduce): result = post * SUM_r (pre * x_r). The sum, fold and
// copy kernels below take an optional trailing ScaleArgs<DT>; without it they are the plain kernels,
// instruction for instruction. With it every operand whose bit of `raw` is set is multiplied by pre
// where it is read, the operands are added in source order, the sum is multiplied by post, and the
// result is rounded to the storage type once, at the store. All of it in the working type W (fp32
// for f32 / f16 / bf16, f64 for f64), every multiply and add its own IEEE operation: contraction
// is off in these helpers, or a*s + b*s would become a fused multiply-add. An operand that is not raw
// (a partial sum a peer already scaled) and a sum that is not final (post = 1) are multiplied by 1,
// which changes no bit. Float dtypes only.
template <int DT>
struct WorkOf {
  using T = float;
};
template <>
struct WorkOf<kF64> {
  using T = double;
};

template <int DT>
struct ScaleArgs {
  typename WorkOf<DT>::T pre, post;
  unsigned raw;  // bit j: source j is a rank's raw input (not yet multiplied by pre)
  __device__ __forceinline__ typename WorkOf<DT>::T in(int j) const { return ((raw >> j) & 1u) ? pre : 1; }
};

template <int DT>
__device__ __forceinline__ typename Wide<DT>::A scaled_load(u32x4 v, typename WorkOf<DT>::T f) {
#pragma clang fp contract(off)
  return Wide<DT>::load(v) * f;
}
template <int DT>
__device__ __forceinline__ typename Wide<DT>::A separate_add(typename Wide<DT>::A a, typename Wide<DT>::A b) {
#pragma clang fp contract(off)
  return a + b;
}
template <int DT>
__device__ __forceinline__ u32x4 scaled_store(typename Wide<DT>::A a, typename WorkOf<DT>::T f) {
#pragma clang fp contract(off)
  return Wide<DT>::store(a * f);
}

// one element in W, and its single rounding back to the storage type
template <int DT>
__device__ __forceinline__ typename WorkOf<DT>::T load_work(const void* p, int64_t i) {
  if constexpr (DT == kBF16) return __builtin_bit_cast(float, (unsigned)((const unsigned short*)p)[i] << 16);
  else return (typename WorkOf<DT>::T)((const typename ScalarOf<DT>::T*)p)[i];
}
template <int DT>
__device__ __forceinline__ void store_work(void* p, int64_t i, typename WorkOf<DT>::T v) {
  if constexpr (DT == kBF16) ((unsigned short*)p)[i] = (unsigned short)bf16_round_bits(__builtin_bit_cast(unsigned, v));
  else if constexpr (DT == kF16) {
    // the fp32 product is a value of its own before it is rounded to half: without this the compiler
    // folds the last multiply and the conversion into one v_fma_mixlo_f16, which the vector path
    // (v_pk_mul_f32, then v_cvt_pk_f16_f32) does not do - tails and the scalar fallback must match it
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(v));
#endif
    ((_Float16*)p)[i] = (_Float16)v;
  } else ((typename ScalarOf<DT>::T*)p)[i] = (typename ScalarOf<DT>::T)v;
}

// dst[i] = (((s0 * f0) + (s1 * f1)) + ...) * post for one element (tails and the unaligned fallback)
template <int DT>
__device__ __forceinline__ void fold_elem(void* dst, const void* const* srcs, int nsrc, int64_t i, ScaleArgs<DT> sc) {
#pragma clang fp contract(off)
  typename WorkOf<DT>::T acc = load_work<DT>(srcs[0], i) * sc.in(0);
  for (int j = 1; j < nsrc; j++) {
    const typename WorkOf<DT>::T x = load_work<DT>(srcs[j], i) * sc.in(j);
    acc = acc + x;
  }
  store_work<DT>(dst, i, acc * sc.post);
}

// the 2-input sum's vector and element: plain, or scaled
template <int DT>
__device__ __forceinline__ u32x4 sum16(u32x4 a, u32x4 b) {
  return add16<DT>(a, b);
}
template <int DT>
__device__ __forceinline__ u32x4 sum16(u32x4 a, u32x4 b, ScaleArgs<DT> sc) {
  return scaled_store<DT>(separate_add<DT>(scaled_load<DT>(a, sc.in(0)), scaled_load<DT>(b, sc.in(1))), sc.post);
}
template <int DT>
__device__ __forceinline__ void sum_elem(void* dst, const void* a, const void* b, int64_t i) {
  add_elem<DT>(dst, a, b, i);
}
template <int DT>
__device__ __forceinline__ void sum_elem(void* dst, const void* a, const void* b, int64_t i, ScaleArgs<DT> sc) {
  const void* s[2] = {a, b};
  fold_elem<DT>(dst, s, 2, i, sc);
}

// the fold's steps: plain, or scaled
template <int DT>
__device__ __forceinline__ typename Wide<DT>::A fold_first(u32x4 v) {
  return Wide<DT>::load(v);
}
template <int DT>
__device__ __forceinline__ typename Wide<DT>::A fold_first(u32x4 v, ScaleArgs<DT> sc) {
  return scaled_load<DT>(v, sc.in(0));
}
template <int DT>
__device__ __forceinline__ typename Wide<DT>::A fold_next(typename Wide<DT>::A acc, u32x4 v, int) {
  return acc + Wide<DT>::load(v);
}
template <int DT>
__device__ __forceinline__ typename Wide<DT>::A fold_next(typename Wide<DT>::A acc, u32x4 v, int j, ScaleArgs<DT> sc) {
  return separate_add<DT>(acc, scaled_load<DT>(v, sc.in(j)));
}
template <int DT>
__device__ __forceinline__ u32x4 fold_store(typename Wide<DT>::A acc) {
  return Wide<DT>::store(acc);
}
template <int DT>
__device__ __forceinline__ u32x4 fold_store(typename Wide<DT>::A acc, ScaleArgs<DT> sc) {
  return scaled_store<DT>(acc, sc.post);
}

// ---------------------------------------------------------------------------
// MAX / MIN forms (DESIGN.md §MAX and MIN): result = the largest (smallest) of the operands, in the
// storage type, exact. The sum, fold and scalar kernels take one MinMaxArgs<DT, IS_MAX> in the place of
// a ScaleArgs<DT>: an empty tag, the op a template parameter, so each op's compare is one instruction
// (v_maximum3_f32 / v_pk_maximum3_f16 / v_max_i32 ...) and not a select between two. Floats follow
// IEEE 754-2019 maximum / minimum: a NaN operand gives a NaN, -0 < +0, subnormals are kept
// (__builtin_elementwise_maximum; __builtin_elementwise_max would drop the NaN). Integers compare
// signed - the sums' unsigned vectors are cast first. bf16 compares as f32 after the << 16 and keeps the
// winner's upper half (nothing to round); the fold widens f16 to fp32 like the sum's fold, which is
// exact for a compare, the 2-input form compares packed halves. No operand order can change a bit
// of the result (a NaN's payload excepted), so every schedule returns the same bits.
template <int DT, bool IS_MAX>
struct MinMaxArgs {};

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef long long i64x2 __attribute__((ext_vector_type(2)));

template <bool IS_MAX, class V>
__device__ __forceinline__ V pick_float(V a, V b) {
  if constexpr (IS_MAX) return __builtin_elementwise_maximum(a, b);
  else return __builtin_elementwise_minimum(a, b);
}
template <bool IS_MAX, class V>
__device__ __forceinline__ V pick_int(V a, V b) {
  if constexpr (IS_MAX) return __builtin_elementwise_max(a, b);
  else return __builtin_elementwise_min(a, b);
}

// the compare in the fold's accumulator type Wide<DT>::A (unsigned vectors for the integers)
template <int DT, bool IS_MAX>
__device__ __forceinline__ typename Wide<DT>::A pick_wide(typename Wide<DT>::A a, typename Wide<DT>::A b) {
  if constexpr (DT == kI32) return __builtin_bit_cast(u32x4, pick_int<IS_MAX>(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b)));
  else if constexpr (DT == kI64) return __builtin_bit_cast(u64x2, pick_int<IS_MAX>(__builtin_bit_cast(i64x2, a), __builtin_bit_cast(i64x2, b)));
  else return pick_float<IS_MAX>(a, b);
}

// two bf16 halves' winners (f32 values whose low 16 bits are zero) back into one word per pair
__device__ __forceinline__ u32x4 bf16_pack_exact(f32x4 lo, f32x4 hi) {
  return (__builtin_bit_cast(u32x4, lo) >> 16u) | (__builtin_bit_cast(u32x4, hi) & 0xffff0000u);
}

template <int DT, bool IS_MAX>
__device__ __forceinline__ u32x4 sum16(u32x4 a, u32x4 b, MinMaxArgs<DT, IS_MAX>) {
  if constexpr (DT == kF16) {
    return __builtin_bit_cast(u32x4, pick_float<IS_MAX>(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b)));
  } else if constexpr (DT == kBF16) {
    return bf16_pack_exact(pick_float<IS_MAX>(bf16_lo(a), bf16_lo(b)), pick_float<IS_MAX>(bf16_hi(a), bf16_hi(b)));
  } else {
    return Wide<DT>::store(pick_wide<DT, IS_MAX>(Wide<DT>::load(a), Wide<DT>::load(b)));
  }
}

template <int DT, bool IS_MAX>
__device__ __forceinline__ typename Wide<DT>::A fold_first(u32x4 v, MinMaxArgs<DT, IS_MAX>) {
  return Wide<DT>::load(v);
}
template <int DT, bool IS_MAX>
__device__ __forceinline__ typename Wide<DT>::A fold_next(typename Wide<DT>::A acc, u32x4 v, int, MinMaxArgs<DT, IS_MAX>) {
  return pick_wide<DT, IS_MAX>(acc, Wide<DT>::load(v));
}
template <int DT, bool IS_MAX>
__device__ __forceinline__ u32x4 fold_store(typename Wide<DT>::A acc, MinMaxArgs<DT, IS_MAX>) {
  if constexpr (DT == kBF16) {
    return bf16_pack_exact(f32x4{acc[0], acc[1], acc[2], acc[3]}, f32x4{acc[4], acc[5], acc[6], acc[7]});
  } else {
    return Wide<DT>::store(acc);  // (f16: every winner is a half's value, the conversion rounds nothing)
  }
}

// one element (tails and the unaligned fallback): the same compares, signed for the integers
template <int DT>
struct CmpOf {
  using T = typename ScalarOf<DT>::T;
};
template <>
struct CmpOf<kI32> {
  using T = int;
};
template <>
struct CmpOf<kI64> {
  using T = long long;
};
template <int DT, bool IS_MAX>
__device__ __forceinline__ void fold_elem(void* dst, const void* const* srcs, int nsrc, int64_t i, MinMaxArgs<DT, IS_MAX>) {
  if constexpr (DT == kBF16) {
    float acc = load_work<kBF16>(srcs[0], i);
    for (int j = 1; j < nsrc; j++) acc = pick_float<IS_MAX>(acc, load_work<kBF16>(srcs[j], i));
    ((unsigned short*)dst)[i] = (unsigned short)(__builtin_bit_cast(unsigned, acc) >> 16);
  } else {
    using T = typename CmpOf<DT>::T;
    T acc = ((const T*)srcs[0])[i];
    for (int j = 1; j < nsrc; j++) {
      if constexpr (DT == kI32 || DT == kI64) acc = pick_int<IS_MAX>(acc, ((const T*)srcs[j])[i]);
      else acc = pick_float<IS_MAX>(acc, ((const T*)srcs[j])[i]);
    }
    ((T*)dst)[i] = acc;
  }
}
template <int DT, bool IS_MAX>
__device__ __forceinline__ void sum_elem(void* dst, const void* a, const void* b, int64_t i, MinMaxArgs<DT, IS_MAX> mm) {
  const void* s[2] = {a, b};
  fold_elem<DT>(dst, s, 2, i, mm);
}

// the contiguous copy's vector and trailing bytes: plain, or scaled (source 0 is raw)
__device__ __forceinline__ u32x4 copy16(u32x4 v) { return v; }
template <int DT>
__device__ __forceinline__ u32x4 copy16(u32x4 v, ScaleArgs<DT> sc) {
  return scaled_store<DT>(scaled_load<DT>(v, sc.in(0)), sc.post);
}
__device__ __forceinline__ void copy_tail(void* dst, const void* src, int64_t tail_begin, int64_t bytes, int tid) {
  if (tail_begin + tid < bytes)
    reinterpret_cast<char*>(dst)[tail_begin + tid] = reinterpret_cast<const char*>(src)[tail_begin + tid];
}
template <int DT>
__device__ __forceinline__ void copy_tail(void* dst, const void* src, int64_t tail_begin, int64_t bytes, int tid,
                                          ScaleArgs<DT> sc) {
  constexpr int64_t es = sizeof(typename ScalarOf<DT>::T);
  const int64_t i = tail_begin / es + tid;
  if (i < bytes / es) fold_elem<DT>(dst, &src, 1, i, sc);
}

// XCD-contiguous tile order: workgroups are dealt round-robin over the 8 XCDs
// (b and b+8 share one), so tile = (b % 8) * (grid / 8) + b / 8 hands each XCD
// one contiguous stretch. Needs grid % 8 == 0; speed only, never correctness.
__device__ __forceinline__ int64_t xcd_tile(unsigned b, unsigned grid) {
  return (int64_t)(b & 7u) * (grid >> 3) + (b >> 3);
}

// XCD stripes (round 6): the tiles cut into stripes of C tiles (1 MiB of each operand), stripe s
// on XCD s % 8, and workgroup j of an XCD takes the j-th tile of that XCD's stripes. With one
// contiguous eighth per XCD (xcd_tile) the 8 XCDs' streams sit at the same offset of their
// eighths, all 3 operands' alike; at 128 MiB operands that cost the 2-input sum 6 % (0.774 against
// 0.820 in 1 MiB stripes, profiles/r06/stripes/sum2_map_sweep.jsonl), at 256 MiB it ties. C <= 0, or one
// stripe per XCD or fewer (the grid's eighth R <= C), is xcd_tile. The grid must then cover whole
// rounds of 8 stripes (stripe_grid): R a multiple of C, so the map is a bijection onto [0, grid).
__device__ __forceinline__ int64_t stripe_tile(unsigned b, unsigned grid, int64_t C) {
  const int64_t R = grid >> 3;
  if (C <= 0 || R <= C) return xcd_tile(b, grid);
  const int64_t j = b >> 3;
  return ((j / C) * 8 + (b & 7u)) * C + j % C;
}

// ---------------------------------------------------------------------------
// 2-input sum: dst = a + b
//
// The shipped 2-input sum (and, with other CPol bits, the cache-policy sweep
// variants): one tile of U x BLOCK vectors per operand per workgroup, placed by stripe_tile,
// through buffer_load/store_dwordx4 with explicit CPol bits (aux: 1 = sc0,
// 2 = nt, 16 = sc1). The product launch (kernels.hip kDef*): BLOCK = 128, nt loads and nt stores,
// 512 KiB stripes (round 6; rounds 2-5: 256 lanes with sc1 stores, which won when one buffer
// triple was re-read, 7.46 vs 7.10 TB/s, profiles/r01_sum_sweep_f.jsonl). Each workgroup's
// descriptors cover exactly its tile, so the hardware range check drops lanes past the end.
// SC: empty (the plain sum), one ScaleArgs<DT> (the scaled sum, see "Scaled forms" above), or one
// MinMaxArgs<DT, IS_MAX> (MAX / MIN, see "MAX / MIN forms").
template <int DT, int LAUX, int SAUX, int U = 1, int BLOCK = 256, class... SC>
__global__ __launch_bounds__(BLOCK) void sum2_buf_kernel(u32x4* __restrict__ dst, const u32x4* __restrict__ a,
                                                        const u32x4* __restrict__ b, int64_t nvec,
                                                        int64_t tail_begin, int64_t n, int64_t stripe, SC... sc) {
  constexpr int64_t kTile = (int64_t)BLOCK * U;
  const int64_t t = stripe_tile(blockIdx.x, gridDim.x, stripe);
  const int64_t first = t * kTile;
  if (first < nvec) {
    const int rec = (int)(((nvec - first) < kTile ? (nvec - first) : kTile) * 16);
    __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)(a + first), (short)0, rec, 0x00020000);
    __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(b + first), (short)0, rec, 0x00020000);
    __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(dst + first), (short)0, rec, 0x00020000);
    u32x4 x[U], y[U];
#pragma unroll
    for (int u = 0; u < U; u++) x[u] = __builtin_amdgcn_raw_buffer_load_b128(ra, (u * BLOCK + (int)threadIdx.x) * 16, 0, LAUX);
#pragma unroll
    for (int u = 0; u < U; u++) y[u] = __builtin_amdgcn_raw_buffer_load_b128(rb, (u * BLOCK + (int)threadIdx.x) * 16, 0, LAUX);
#pragma unroll
    for (int u = 0; u < U; u++)
      __builtin_amdgcn_raw_buffer_store_b128(sum16<DT>(x[u], y[u], sc...), rd, (u * BLOCK + (int)threadIdx.x) * 16, 0, SAUX);
  }
  if (blockIdx.x == 0 && tail_begin + (int64_t)threadIdx.x < n) sum_elem<DT>(dst, a, b, tail_begin + threadIdx.x, sc...);
}

// Unaligned fallback (any pointer not 16-B aligned): one element per lane.
template <int DT, class... SC>
__global__ __launch_bounds__(kBlock) void sum2_scalar_kernel(void* dst, const void* a, const void* b, int64_t n, SC... sc) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    sum_elem<DT>(dst, a, b, i, sc...);
}

// ---------------------------------------------------------------------------
// Multi-input sum: dst = ((s0 + s1) + s2) + ...  (rank-order fold)
// f16/bf16 accumulate in fp32 and round once; others accumulate in storage type.

template <int DT>
__device__ __forceinline__ void fold_elem(void* dst, const void* const* srcs, int nsrc, int64_t i) {
  if constexpr (DT == kF16) {
    float acc = (float)((const _Float16*)srcs[0])[i];
    for (int j = 1; j < nsrc; j++) acc += (float)((const _Float16*)srcs[j])[i];
    ((_Float16*)dst)[i] = (_Float16)acc;
  } else if constexpr (DT == kBF16) {
    float acc = __builtin_bit_cast(float, (unsigned)((const unsigned short*)srcs[0])[i] << 16);
    for (int j = 1; j < nsrc; j++) acc += __builtin_bit_cast(float, (unsigned)((const unsigned short*)srcs[j])[i] << 16);
    ((unsigned short*)dst)[i] = (unsigned short)bf16_round_bits(__builtin_bit_cast(unsigned, acc));
  } else {
    // storage-type fold in a register (dst may alias one of srcs: in-place)
    using T = typename ScalarOf<DT>::T;
    T acc = ((const T*)srcs[0])[i];
    for (int j = 1; j < nsrc; j++) acc = acc + ((const T*)srcs[j])[i];
    ((T*)dst)[i] = acc;
  }
}

struct SrcList {
  const u32x4* p[kMaxSrcs];
};

// Buffer-op form of the multi-input sum: one descriptor per source covering
// this workgroup's tile, cache-policy bits on the loads (LAUX) and sc1 stores,
// every source's vectors in flight before the fold (as sum2_buf_kernel).
// SC: empty (the plain fold), one ScaleArgs<DT> (the scaled fold), or one MinMaxArgs<DT, IS_MAX>.
template <int DT, int NSRC, int U, int LAUX, int BLOCK = kBlock, int SAUX = 16, class... SC>
__global__ __launch_bounds__(BLOCK) void multi_sum_buf_kernel(u32x4* __restrict__ dst, SrcList srcs, int64_t nvec,
                                                             int64_t tail_begin, int64_t n, int64_t stripe, SC... sc) {
  using W = Wide<DT>;
  constexpr int64_t kTile = (int64_t)BLOCK * U;
  const int tid = threadIdx.x;
  const int64_t first = stripe_tile(blockIdx.x, gridDim.x, stripe) * kTile;
  if (first < nvec) {
    const int rec = (int)(((nvec - first) < kTile ? (nvec - first) : kTile) * 16);
    u32x4 v[U][NSRC];
#pragma unroll
    for (int j = 0; j < NSRC; j++) {
      __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(srcs.p[j] + first), (short)0, rec, 0x00020000);
#pragma unroll
      for (int u = 0; u < U; u++) v[u][j] = __builtin_amdgcn_raw_buffer_load_b128(rs, (u * BLOCK + tid) * 16, 0, LAUX);
    }
    __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(dst + first), (short)0, rec, 0x00020000);
#pragma unroll
    for (int u = 0; u < U; u++) {
      typename W::A acc = fold_first<DT>(v[u][0], sc...);
#pragma unroll
      for (int j = 1; j < NSRC; j++) acc = fold_next<DT>(acc, v[u][j], j, sc...);
      __builtin_amdgcn_raw_buffer_store_b128(fold_store<DT>(acc, sc...), rd, (u * BLOCK + tid) * 16, 0, SAUX);
    }
  }
  if (blockIdx.x == 0 && NSRC > 1 && tail_begin + tid < n) {
    const void* s[NSRC];
#pragma unroll
    for (int j = 0; j < NSRC; j++) s[j] = srcs.p[j];
    fold_elem<DT>(dst, s, NSRC, tail_begin + tid, sc...);
  }
}

template <int DT, class... SC>
__global__ __launch_bounds__(kBlock) void multi_sum_scalar_kernel(void* dst, SrcList srcs, int nsrc, int64_t n, SC... sc) {
  const void* s[kMaxSrcs];
  for (int j = 0; j < nsrc; j++) s[j] = srcs.p[j];
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    fold_elem<DT>(dst, s, nsrc, i, sc...);
}

// ---------------------------------------------------------------------------
// Contiguous copy: the out-of-place allreduce at one rank (MPI_Allreduce returns the input). Shaped
// as sum2_buf_kernel with one operand: one 4 KiB tile per 256-lane workgroup in XCD-contiguous
// order, buffer loads nt, buffer stores sc1 (the line leaves the XCD's L2), descriptors covering
// exactly the tile; the < 16 trailing bytes go bytewise in workgroup 0. (hipMemcpyAsync's D2D blit
// moved config 3's 1 GiB at 0.62 of HBM, profiles/r04/n_bench_n1.jsonl.)
// SC: empty (the copy), or one ScaleArgs<DT>: dst = (src * pre) * post (in place allowed: every lane
// stores only what it loaded), the trailing elements by workgroup 0 one per lane.
template <int U, int SAUX = 16, int BLOCK = kBlock, class... SC>
__global__ __launch_bounds__(BLOCK) void copy_buf_kernel(u32x4* __restrict__ dst, const u32x4* __restrict__ src,
                                                         int64_t nvec, int64_t tail_begin, int64_t bytes, int64_t stripe,
                                                         SC... sc) {
  constexpr int64_t kTile = (int64_t)BLOCK * U;
  const int64_t first = stripe_tile(blockIdx.x, gridDim.x, stripe) * kTile;
  const int tid = threadIdx.x;
  if (first < nvec) {
    const int rec = (int)(((nvec - first) < kTile ? (nvec - first) : kTile) * 16);
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(src + first), (short)0, rec, 0x00020000);
    __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)(dst + first), (short)0, rec, 0x00020000);
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, (u * BLOCK + tid) * 16, 0, 2);
#pragma unroll
    for (int u = 0; u < U; u++)
      __builtin_amdgcn_raw_buffer_store_b128(copy16(v[u], sc...), rd, (u * BLOCK + tid) * 16, 0, SAUX);
  }
  if (blockIdx.x == 0) copy_tail(dst, src, tail_begin, bytes, tid, sc...);
}

// ---------------------------------------------------------------------------
// Host helpers of kernels.hip that the sweep launchers use too (described there).
int64_t sum_stripe_of(int64_t tile);
int64_t stripe_grid(int64_t tiles, int64_t C);

constexpr int kNumCUs = 256;

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace tips
