// sparse.cc — the sparse-gradient entry points of the C-ABI: tips_rows_sum, the
// local ordered row sum (sparse_rows.hip), and tips_sparse_allreduce, the collective around it - the
// other half of the reference's allreduce, its tf.IndexedSlices branch (tips/tensorflow/__init__.py:
// 59-74), which allgathers values and indices and leaves the sums to the consumer.
#include <atomic>
#include <vector>

#include "rt.h"
#include "side.h"
#include "sparse_rows.h"

using namespace tips::rt;

namespace {

std::atomic<int64_t> g_calls{0}, g_entries{0};  // row sums launched by this process, and their entries

// the argument checks both entry points share; *active = there is a table to write
int check_rows_args(int64_t rows, int64_t row_elems, int64_t n, int dtype, double pre, double post, bool* active) {
  TRY(check_dtype(dtype));
  if (rows < 0 || row_elems < 0 || n < 0)
    return fail(TIPS_ERR_INVALID_ARG, "negative size (rows %lld, row_elems %lld, n %lld)", (long long)rows,
                (long long)row_elems, (long long)n);
  TRY(check_scale(dtype, pre, post));
  int64_t a, b, c;
  const int64_t es = tips::dtype_size(dtype);
  if (__builtin_mul_overflow(rows, row_elems, &a) || __builtin_mul_overflow(a, es, &b) ||
      __builtin_mul_overflow(n, row_elems, &a) || __builtin_mul_overflow(a, es, &b) ||
      __builtin_mul_overflow(rows, (int64_t)64, &c) || __builtin_mul_overflow(n, (int64_t)64, &c))
    return fail(TIPS_ERR_INVALID_ARG, "sizes overflow (rows %lld, row_elems %lld, n %lld)", (long long)rows,
                (long long)row_elems, (long long)n);
  *active = rows > 0 && row_elems > 0;
  return 0;
}

const char kTakes[] = "the sparse row sum takes";  // need_device's phrase

int launch(void* dst, int64_t rows, int64_t row_elems, const void* values, const int64_t* indices, int64_t n, int dtype,
           double pre, double post, void* ws, hipStream_t s) {
  HIP_TRY(tips::launch_rows_sum(dst, rows, row_elems, values, indices, n, dtype, pre, post, ws, s));
  g_calls.fetch_add(1, std::memory_order_relaxed);
  g_entries.fetch_add(n, std::memory_order_relaxed);
  return 0;
}

}  // namespace

extern "C" {

int64_t tips_rows_sum_workspace(int64_t rows, int64_t n) {
  if (rows < 0 || n < 0 || rows > ((int64_t)1 << 56) || n > ((int64_t)1 << 56))
    return fail(TIPS_ERR_INVALID_ARG, "bad sizes (rows %lld, n %lld)", (long long)rows, (long long)n);
  return tips::rows_sum_workspace_bytes(rows, n);
}

int tips_rows_sum(void* dst, int64_t rows, int64_t row_elems, const void* values, const int64_t* indices, int64_t n,
                  int dtype, double prescale, double postscale, void* workspace, int64_t workspace_bytes, void* stream) {
  bool active;
  TRY(check_rows_args(rows, row_elems, n, dtype, prescale, postscale, &active));
  if (workspace_bytes < 0) return fail(TIPS_ERR_INVALID_ARG, "negative workspace size");
  if (!active) return 0;
  const int64_t need = tips::rows_sum_workspace_bytes(rows, n);
  if (workspace_bytes < need)
    return fail(TIPS_ERR_INVALID_ARG, "workspace of %lld B is too small: %lld rows and %lld entries need %lld B",
                (long long)workspace_bytes, (long long)rows, (long long)n, (long long)need);
  TRY(need_device(dst, "dst", kTakes));
  TRY(need_device(workspace, "workspace", kTakes));
  if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return fail(TIPS_ERR_INVALID_ARG, "workspace must be 8-B aligned");
  if (n > 0) {
    TRY(need_device(values, "values", kTakes));
    TRY(need_device(indices, "indices", kTakes));
  }
  return launch(dst, rows, row_elems, values, indices, n, dtype, prescale, postscale, workspace, (hipStream_t)stream);
}

int tips_sparse_allreduce(const void* values, const int64_t* indices, int64_t n, int64_t rows, int64_t row_elems,
                          int dtype, double prescale, double postscale, void* dense_out, void* stream) {
  bool active;
  TRY(check_rows_args(rows, row_elems, n, dtype, prescale, postscale, &active));
  State& st = S();
  std::unique_lock<std::mutex> one;
  int size;
  TRY(side_open(st, st.sparse, "tips_sparse_allreduce", "sparse", nullptr, /*rccl_only=*/false, &one, &size));
  hipStream_t s = (hipStream_t)stream;
  int own = 0;
  if (active) {
    own = need_device(dense_out, "dense_out", kTakes);
    if (own == 0 && n > 0) own = need_device(values, "values", kTakes);
    if (own == 0 && n > 0) own = need_device(indices, "indices", kTakes);
  }
  const int64_t mine[5] = {n, rows, row_elems, dtype, own};
  SideRecords rec;
  TRY(side_exchange(size, mine, 5, &rec));
  // reported in this order: this rank's own refusal, a mismatch, another rank's refusal
  TRY(rec.report_own());
  if (const int r = rec.first_differing(1, 4); r >= 0) {
    const int64_t *q = rec.of(r), *q0 = rec.of(0);
    return fail(TIPS_ERR_MISMATCH,
                "Mismatched sparse allreduce: rank %d has rows %lld, row_elems %lld, dtype %lld; rank 0 has rows %lld, "
                "row_elems %lld, dtype %lld",
                r, (long long)q[1], (long long)q[2], (long long)q[3], (long long)q0[1], (long long)q0[2], (long long)q0[3]);
  }
  TRY(rec.report_refusing("sparse allreduce"));
  if (!active) return 0;
  const int64_t es = tips::dtype_size(dtype);
  std::vector<int64_t> counts(size), vcounts(size);
  int64_t G = 0;
  for (int r = 0; r < size; r++) {
    counts[r] = rec.of(r)[0];
    if (counts[r] < 0 || __builtin_add_overflow(G, counts[r], &G))
      return fail(TIPS_ERR_MISMATCH, "sparse allreduce: bad entry count on rank %d", r);
    vcounts[r] = counts[r] * row_elems;
  }
  bool act2;
  TRY(check_rows_args(rows, row_elems, G, dtype, prescale, postscale, &act2));  // (the gathered sizes)
  const int64_t ws_bytes = tips::rows_sum_workspace_bytes(rows, G);
  const int64_t idx_bytes = size == 1 ? 0 : round_up(8 * G, kAlignBytes);
  const int64_t val_bytes = size == 1 ? 0 : round_up(G * row_elems * es, kAlignBytes);
  char* base;
  {
    std::lock_guard<std::mutex> lk(st.mu);
    if (!st.initialized) return fail(TIPS_ERR_NOT_INITIALIZED, "tips_init has not been called");
    TRY(st.sparse.open(s, (size_t)(idx_bytes + val_bytes + ws_bytes)));
    base = (char*)st.sparse.scratch.p;
  }
  const int64_t* g_idx = indices;
  const void* g_val = values;
  if (size > 1) {
    TRY(tips_allgatherv(indices, n, base, counts.data(), TIPS_INT64, stream));
    TRY(tips_allgatherv(values, n * row_elems, base + idx_bytes, vcounts.data(), dtype, stream));
    g_idx = (const int64_t*)base;
    g_val = base + idx_bytes;
  }
  TRY(launch(dense_out, rows, row_elems, g_val, g_idx, G, dtype, prescale, postscale, base + idx_bytes + val_bytes, s));
  std::lock_guard<std::mutex> lk(st.mu);
  return st.sparse.close(s);
}

int tips_sparse_stats(int64_t* calls, int64_t* entries, int64_t* bad_indices) {
  const int64_t c = g_calls.load(std::memory_order_relaxed);
  if (calls) *calls = c;
  if (entries) *entries = g_entries.load(std::memory_order_relaxed);
  if (bad_indices) {
    *bad_indices = 0;
    if (c > 0) HIP_TRY(tips::rows_sum_bad_indices(bad_indices));  // (no launch yet: nothing to read, no device touched)
  }
  return 0;
}

}  // extern "C"
