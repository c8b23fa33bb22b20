// sparse_rows.hip — ordered "sum rows by index" for sparse gradients.
//
//   dst[j][:] = post * (e(x1) + e(x2) + ... + e(xk)),  e(x) = pre * x
//
// x1 ... xk are the rows values[e][:] with indices[e] == j in ascending entry order, folded left to
// right from the first row itself in the working type (fp32 for f32 / f16 / bf16, f64 for f64, the
// integer type for integers), every multiply and add a separate IEEE operation, one rounding at the
// store. A row no entry names is +0; an entry whose index is outside [0, rows) is skipped before any
// address is formed from it and counted in g_bad_indices. Nothing but the inputs decides a bit of
// the result: the only unordered step (place) is followed by a sort of each row's entry ids.
//
// Five passes on one stream, after a memset of the counters:
//   count  one pass over the indices, integer atomicAdd into count[rows] (integer atomics give
//          deterministic totals)
//   scan   exclusive prefix sum of count in place -> offset[rows + 1]: one looped workgroup up to
//          8192 entries, above that three launches (tile totals, their scan, the tiles in parallel)
//   place  entry e takes slot offset[idx] + atomicAdd(cursor[idx], 1): each row's entries now sit
//          in one segment, in arbitrary order
//   order  one lane per placed entry counts the ids of its segment that are smaller than its own
//          (rank counting) and writes its id at that rank: segments ascending. O(k) reads per entry
//          of a segment of k (all served by L1 / L2: a wave's lanes mostly share the segment), so
//          O(k^2 / lanes of the whole device) per row, G^2 / lanes when every entry names one row
//   fold   per output row, the values rows in segment order; lanes across the row, 16 B per lane
//          (several short rows per wave), or one element per lane when a base or the row length is
//          not 16-B aligned; every row of dst written exactly once, empty rows as zeros
//
// Device helpers (16-B loads / stores, Wide, the separate multiply / add forms, bf16_round_bits)
// come from kernels_device.h.
#include <algorithm>

#include "kernels_device.h"
#include "sparse_rows.h"

namespace tips {

namespace {

typedef unsigned long long u64;

// entries skipped because their index was outside [0, rows), on this device, since load
__device__ u64 g_bad_indices;

__global__ __launch_bounds__(kBlock) void rows_count_kernel(const int64_t* __restrict__ indices, int64_t n, int64_t rows,
                                                            u64* __restrict__ count) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += (int64_t)gridDim.x * kBlock) {
    const int64_t j = indices[e];
    if (j >= 0 && j < rows) atomicAdd(&count[j], 1ull);
    else atomicAdd(&g_bad_indices, 1ull);
  }
}

// In-place exclusive prefix sum of a[0, m). One workgroup (TILED false): tiles of BLOCK * kScanItems
// entries in turn, each lane its kScanItems consecutive ones, the lanes' totals scanned across the
// wave by cross-lane reads and across the waves through LDS, the tile's total carried into the next.
// That loop is latency-bound (788 us for 1 Mi + 1 entries, 80 % of the whole row sum,
// profiles/sparse/), so above kScanSingle entries the tiles run in parallel (TILED true): workgroup t
// scans tile t alone, starting from carry[t] = the total of the tiles before it, which
// rows_tile_total_kernel and a one-workgroup scan of its totals leave there. The carries live in the
// first entries of the cursor array, which place needs zero: each workgroup zeroes its own after
// reading it (no other workgroup touches that entry).
constexpr int kScanItems = 8, kScanBlock = 1024, kTileBlock = 256;
constexpr int64_t kScanTile = (int64_t)kTileBlock * kScanItems;  // 2048 entries per parallel tile
constexpr int64_t kScanSingle = 8192;

__global__ __launch_bounds__(kTileBlock) void rows_tile_total_kernel(const u64* __restrict__ a, int64_t m,
                                                                     u64* __restrict__ total) {
  __shared__ u64 wsum[kTileBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * kScanTile + (int64_t)tid * kScanItems;
  u64 t = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; k++)
    if (i0 + k < m) t += a[i0 + k];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) t += __shfl_down(t, d, 64);
  if (lane == 0) wsum[w] = t;
  __syncthreads();
  if (tid == 0) {
    u64 sum = 0;
#pragma unroll
    for (int i = 0; i < kTileBlock / 64; i++) sum += wsum[i];
    total[blockIdx.x] = sum;
  }
}

template <int BLOCK, bool TILED>
__global__ __launch_bounds__(BLOCK) void rows_scan_kernel(u64* __restrict__ a, int64_t m, u64* __restrict__ carries) {
  constexpr int kWaves = BLOCK / 64;
  __shared__ u64 wsum[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  u64 carry = 0;
  int64_t begin = 0, end = m;
  if constexpr (TILED) {
    begin = (int64_t)blockIdx.x * BLOCK * kScanItems;
    end = begin + (int64_t)BLOCK * kScanItems < m ? begin + (int64_t)BLOCK * kScanItems : m;
    carry = carries[blockIdx.x];
    __syncthreads();
    if (tid == 0) carries[blockIdx.x] = 0;
  }
  for (int64_t base = begin; base < end; base += (int64_t)BLOCK * kScanItems) {
    const int64_t i0 = base + (int64_t)tid * kScanItems;
    u64 x[kScanItems];
    u64 t = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
      const u64 v = (i0 + k < end) ? a[i0 + k] : 0;
      x[k] = t;
      t += v;
    }
    u64 inc = t;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const u64 y = __shfl_up(inc, d, 64);
      if (lane >= d) inc += y;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    u64 wbase = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < kWaves; i++) {
      const u64 sw = wsum[i];
      if (i < w) wbase += sw;
      tot += sw;
    }
    const u64 before = carry + wbase + (inc - t);
#pragma unroll
    for (int k = 0; k < kScanItems; k++)
      if (i0 + k < end) a[i0 + k] = before + x[k];
    carry += tot;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void rows_place_kernel(const int64_t* __restrict__ indices, int64_t n, int64_t rows,
                                                            const u64* __restrict__ offset, u64* __restrict__ cursor,
                                                            int64_t* __restrict__ ids) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += (int64_t)gridDim.x * kBlock) {
    const int64_t j = indices[e];
    if (j >= 0 && j < rows) {
      const u64 slot = offset[j] + atomicAdd(&cursor[j], 1ull);
      if (slot < (u64)n) ids[slot] = e;
    }
  }
}

// Slot s of the placed ids holds entry id = ids[s] of row indices[id], whose segment is
// [offset[row], offset[row + 1]). The ids of a segment are distinct, so "how many are smaller" is
// a permutation of the segment's positions.
__global__ __launch_bounds__(kBlock) void rows_order_kernel(const int64_t* __restrict__ indices, int64_t n, int64_t rows,
                                                            const u64* __restrict__ offset,
                                                            const int64_t* __restrict__ ids,
                                                            int64_t* __restrict__ sorted) {
  const u64 placed = offset[rows] < (u64)n ? offset[rows] : (u64)n;
  for (u64 s = (u64)blockIdx.x * kBlock + threadIdx.x; s < placed; s += (u64)gridDim.x * kBlock) {
    const int64_t id = ids[s];
    if (id < 0 || id >= n) continue;
    const int64_t j = indices[id];
    if (j < 0 || j >= rows) continue;
    const u64 b = offset[j];
    u64 e = offset[j + 1];
    if (e > placed) e = placed;
    u64 rank = 0;
    for (u64 t = b; t < e; t++) rank += (ids[t] < id) ? 1u : 0u;
    if (b + rank < placed) sorted[b + rank] = id;
  }
}

// ---------------------------------------------------------------------------
// fold

// one element's working type: WorkOf for the floats, the storage type for the integers
template <int DT>
struct RowWork {
  using T = typename WorkOf<DT>::T;
};
template <>
struct RowWork<kI32> {
  using T = unsigned;
};
template <>
struct RowWork<kI64> {
  using T = u64;
};

template <int DT>
__device__ __forceinline__ typename RowWork<DT>::T row_load(const void* p, int64_t i) {
  if constexpr (DT == kI32 || DT == kI64) return ((const typename RowWork<DT>::T*)p)[i];
  else return load_work<DT>(p, i);
}
template <int DT>
__device__ __forceinline__ void row_store(void* p, int64_t i, typename RowWork<DT>::T v) {
  if constexpr (DT == kI32 || DT == kI64) ((typename RowWork<DT>::T*)p)[i] = v;
  else store_work<DT>(p, i, v);
}

// the entry id at position t of the ordered ids (always inside [0, n): what place wrote)
__device__ __forceinline__ int64_t entry_at(const int64_t* __restrict__ sorted, u64 t, int64_t n) {
  const int64_t id = sorted[t];
  return (id >= 0 && id < n) ? id : 0;
}

template <int DT, bool SCALED>
__device__ __forceinline__ typename Wide<DT>::A row_term(u32x4 v, typename WorkOf<DT>::T pre) {
  if constexpr (SCALED) return scaled_load<DT>(v, pre);
  else return Wide<DT>::load(v);
}
template <int DT, bool SCALED>
__device__ __forceinline__ typename Wide<DT>::A row_add(typename Wide<DT>::A acc, u32x4 v, typename WorkOf<DT>::T pre) {
  if constexpr (SCALED) return separate_add<DT>(acc, scaled_load<DT>(v, pre));
  else return acc + Wide<DT>::load(v);
}

// Vector form: rows of rowvecs 16-B vectors, dst and values 16-B aligned. 2^lpr_log2 lanes share a
// row (the power of two that covers rowvecs, at most a wave), so a wave holds 64 >> lpr_log2 rows;
// values are read once (nt), four entries' vectors in flight before they are added in order.
template <int DT, bool SCALED>
__global__ __launch_bounds__(kBlock) void rows_fold_vec_kernel(u32x4* __restrict__ dst, const u32x4* __restrict__ values,
                                                               const u64* __restrict__ offset,
                                                               const int64_t* __restrict__ sorted, int64_t rows,
                                                               int64_t rowvecs, int64_t n, int lpr_log2,
                                                               typename WorkOf<DT>::T pre, typename WorkOf<DT>::T post) {
  using W = Wide<DT>;
  const int lpr = 1 << lpr_log2;
  const int sub = (int)threadIdx.x & (lpr - 1);
  const int64_t rpb = kBlock >> lpr_log2;
  for (int64_t j = (int64_t)blockIdx.x * rpb + ((int)threadIdx.x >> lpr_log2); j < rows; j += (int64_t)gridDim.x * rpb) {
    const u64 b = offset[j];
    u64 e = offset[j + 1];
    if (e > (u64)n) e = (u64)n;
    for (int64_t v = sub; v < rowvecs; v += lpr) {
      u32x4 out = {0u, 0u, 0u, 0u};
      if (b < e) {
        typename W::A acc = row_term<DT, SCALED>(ld16<true>(values + entry_at(sorted, b, n) * rowvecs + v), pre);
        u64 t = b + 1;
        for (; t + 4 <= e; t += 4) {
          const u32x4 x0 = ld16<true>(values + entry_at(sorted, t, n) * rowvecs + v);
          const u32x4 x1 = ld16<true>(values + entry_at(sorted, t + 1, n) * rowvecs + v);
          const u32x4 x2 = ld16<true>(values + entry_at(sorted, t + 2, n) * rowvecs + v);
          const u32x4 x3 = ld16<true>(values + entry_at(sorted, t + 3, n) * rowvecs + v);
          acc = row_add<DT, SCALED>(acc, x0, pre);
          acc = row_add<DT, SCALED>(acc, x1, pre);
          acc = row_add<DT, SCALED>(acc, x2, pre);
          acc = row_add<DT, SCALED>(acc, x3, pre);
        }
        for (; t < e; t++) acc = row_add<DT, SCALED>(acc, ld16<true>(values + entry_at(sorted, t, n) * rowvecs + v), pre);
        if constexpr (SCALED) out = scaled_store<DT>(acc, post);
        else out = W::store(acc);
      }
      st16<true>(dst + j * rowvecs + v, out);
    }
  }
}

// Element form (a base not 16-B aligned, or a row length that is no multiple of 16 B): one output
// element per lane, lanes across the flattened table so a wave's loads of one entry are contiguous.
template <int DT, bool SCALED>
__global__ __launch_bounds__(kBlock) void rows_fold_elem_kernel(void* __restrict__ dst, const void* __restrict__ values,
                                                                const u64* __restrict__ offset,
                                                                const int64_t* __restrict__ sorted, int64_t rows,
                                                                int64_t row_elems, int64_t n,
                                                                typename WorkOf<DT>::T pre, typename WorkOf<DT>::T post) {
#pragma clang fp contract(off)
  using T = typename RowWork<DT>::T;
  const int64_t total = rows * row_elems;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
    const int64_t j = i / row_elems, c = i - j * row_elems;
    const u64 b = offset[j];
    u64 e = offset[j + 1];
    if (e > (u64)n) e = (u64)n;
    T acc = 0;
    if (b < e) {
      acc = row_load<DT>(values, entry_at(sorted, b, n) * row_elems + c);
      if constexpr (SCALED) acc = acc * pre;
      for (u64 t = b + 1; t < e; t++) {
        T x = row_load<DT>(values, entry_at(sorted, t, n) * row_elems + c);
        if constexpr (SCALED) x = x * pre;
        acc = acc + x;
      }
      if constexpr (SCALED) acc = acc * post;
    }
    row_store<DT>(dst, i, acc);
  }
}

inline unsigned grid_for(int64_t items, int64_t per_block, int64_t cap) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, cap));
}

template <int DT, bool SCALED>
hipError_t run_fold(void* dst, int64_t rows, int64_t row_elems, const void* values, const u64* offset,
                    const int64_t* sorted, int64_t n, double pre, double post, hipStream_t s) {
  using F = typename WorkOf<DT>::T;
  const int64_t row_bytes = row_elems * dtype_size(DT);
  if (aligned16(dst) && aligned16(values) && row_bytes % 16 == 0) {
    const int64_t rowvecs = row_bytes / 16;
    int lpr_log2 = 0;
    while (lpr_log2 < 6 && ((int64_t)1 << lpr_log2) < rowvecs) lpr_log2++;
    const int64_t rpb = kBlock >> lpr_log2;
    hipLaunchKernelGGL((rows_fold_vec_kernel<DT, SCALED>), dim3(grid_for(rows, rpb, (int64_t)1 << 20)), dim3(kBlock), 0, s,
                       (u32x4*)dst, (const u32x4*)values, offset, sorted, rows, rowvecs, n, lpr_log2, (F)pre, (F)post);
  } else {
    hipLaunchKernelGGL((rows_fold_elem_kernel<DT, SCALED>), dim3(grid_for(rows * row_elems, kBlock, (int64_t)1 << 20)),
                       dim3(kBlock), 0, s, dst, values, offset, sorted, rows, row_elems, n, (F)pre, (F)post);
  }
  return hipGetLastError();
}

template <int DT>
hipError_t run_fold_float(void* dst, int64_t rows, int64_t row_elems, const void* values, const u64* offset,
                          const int64_t* sorted, int64_t n, double pre, double post, hipStream_t s) {
  if (pre == 1.0 && post == 1.0) return run_fold<DT, false>(dst, rows, row_elems, values, offset, sorted, n, 1.0, 1.0, s);
  return run_fold<DT, true>(dst, rows, row_elems, values, offset, sorted, n, pre, post, s);
}

}  // namespace

hipError_t launch_rows_sum(void* dst, int64_t rows, int64_t row_elems, const void* values, const int64_t* indices,
                           int64_t n, int dtype, double pre, double post, void* workspace, hipStream_t s) {
  if (rows <= 0 || row_elems <= 0 || n < 0 || !dst || !workspace || (n > 0 && (!values || !indices)))
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return hipErrorInvalidValue;
  const bool integer = dtype == kI32 || dtype == kI64;
  if (integer && (pre != 1.0 || post != 1.0)) return hipErrorInvalidValue;
  u64* offset = (u64*)workspace;         // [rows + 1]: the counts, then their exclusive prefix sums
  u64* cursor = offset + (rows + 1);     // [rows + 1]
  int64_t* ids = (int64_t*)(cursor + (rows + 1));  // [n], placed
  int64_t* sorted = ids + n;                       // [n], each row's segment ascending
  hipError_t err = hipMemsetAsync(workspace, 0, (size_t)(8 * (2 * rows + 2)), s);
  if (err != hipSuccess) return err;
  if (n > 0) {
    const unsigned g = grid_for(n, kBlock, (int64_t)kNumCUs * 32);
    hipLaunchKernelGGL(rows_count_kernel, dim3(g), dim3(kBlock), 0, s, indices, n, rows, offset);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    const int64_t m = rows + 1;
    if (m <= kScanSingle) {
      hipLaunchKernelGGL((rows_scan_kernel<kScanBlock, false>), dim3(1), dim3(kScanBlock), 0, s, offset, m, (u64*)nullptr);
    } else {
      static_assert(kScanTile == (int64_t)kTileBlock * kScanItems, "the totals' tiles are the tiled scan's");
      const int64_t tiles = (m + kScanTile - 1) / kScanTile;  // (<= rows + 1: they fit the cursor array)
      if (tiles > 0x7fffffff) return hipErrorInvalidValue;
      hipLaunchKernelGGL(rows_tile_total_kernel, dim3((unsigned)tiles), dim3(kTileBlock), 0, s, (const u64*)offset, m, cursor);
      if ((err = hipGetLastError()) != hipSuccess) return err;
      hipLaunchKernelGGL((rows_scan_kernel<kScanBlock, false>), dim3(1), dim3(kScanBlock), 0, s, cursor, tiles, (u64*)nullptr);
      if ((err = hipGetLastError()) != hipSuccess) return err;
      hipLaunchKernelGGL((rows_scan_kernel<kTileBlock, true>), dim3((unsigned)tiles), dim3(kTileBlock), 0, s, offset, m, cursor);
    }
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(rows_place_kernel, dim3(g), dim3(kBlock), 0, s, indices, n, rows, (const u64*)offset, cursor, ids);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    hipLaunchKernelGGL(rows_order_kernel, dim3(g), dim3(kBlock), 0, s, indices, n, rows, (const u64*)offset,
                       (const int64_t*)ids, sorted);
    if ((err = hipGetLastError()) != hipSuccess) return err;
  }
  switch (dtype) {
    case kF32: return run_fold_float<kF32>(dst, rows, row_elems, values, offset, sorted, n, pre, post, s);
    case kF64: return run_fold_float<kF64>(dst, rows, row_elems, values, offset, sorted, n, pre, post, s);
    case kF16: return run_fold_float<kF16>(dst, rows, row_elems, values, offset, sorted, n, pre, post, s);
    case kBF16: return run_fold_float<kBF16>(dst, rows, row_elems, values, offset, sorted, n, pre, post, s);
    case kI32: return run_fold<kI32, false>(dst, rows, row_elems, values, offset, sorted, n, 1.0, 1.0, s);
    case kI64: return run_fold<kI64, false>(dst, rows, row_elems, values, offset, sorted, n, 1.0, 1.0, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t rows_sum_bad_indices(int64_t* out) {
  hipError_t err = hipDeviceSynchronize();
  if (err != hipSuccess) return err;
  u64 v = 0;
  err = hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_bad_indices), sizeof(v), 0, hipMemcpyDeviceToHost);
  *out = (int64_t)v;
  return err;
}

}  // namespace tips
