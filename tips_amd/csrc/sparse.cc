// sparse.cc — the sparse-gradient entry points of the C-ABI: tips_rows_sum, the
// local ordered row sum (sparse_rows.hip), and tips_sparse_allreduce, the collective around it - the
// other half of the reference's allreduce, its tf.IndexedSlices branch (tips/tensorflow/__init__.py:
// 59-74), which allgathers values and indices and leaves the sums to the consumer.
#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "rt.h"
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

int need_device(const void* p, const char* what) {
  if (!p) return fail(TIPS_ERR_INVALID_ARG, "null pointer (%s)", what);
  if (!is_device_ptr(p))
    return fail(TIPS_ERR_UNSUPPORTED, "%s is host memory: the sparse row sum takes device pointers only (nothing is staged)",
                what);
  return 0;
}

int launch(void* dst, int64_t rows, int64_t row_elems, const void* values, const int64_t* indices, int64_t n, int dtype,
           double pre, double post, void* ws, hipStream_t s) {
  HIP_TRY(tips::launch_rows_sum(dst, rows, row_elems, values, indices, n, dtype, pre, post, ws, s));
  g_calls.fetch_add(1, std::memory_order_relaxed);
  g_entries.fetch_add(n, std::memory_order_relaxed);
  return 0;
}

}  // namespace

namespace tips {
namespace rt {

void sparse_release(State& st) {
  st.sparse_scratch.release();
  if (st.ev_sparse) {
    (void)hipEventDestroy(st.ev_sparse);
    st.ev_sparse = nullptr;
  }
  st.sparse_chain_valid = false;
}

}  // namespace rt
}  // namespace tips

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
  TRY(need_device(dst, "dst"));
  TRY(need_device(workspace, "workspace"));
  if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return fail(TIPS_ERR_INVALID_ARG, "workspace must be 8-B aligned");
  if (n > 0) {
    TRY(need_device(values, "values"));
    TRY(need_device(indices, "indices"));
  }
  return launch(dst, rows, row_elems, values, indices, n, dtype, prescale, postscale, workspace, (hipStream_t)stream);
}

int tips_sparse_allreduce(const void* values, const int64_t* indices, int64_t n, int64_t rows, int64_t row_elems,
                          int dtype, double prescale, double postscale, void* dense_out, void* stream) {
  bool active;
  TRY(check_rows_args(rows, row_elems, n, dtype, prescale, postscale, &active));
  if (on_negotiation_thread() || negotiation_running())
    return fail(TIPS_ERR_UNSUPPORTED,
                "tips_sparse_allreduce does not go through a running negotiation (named sparse requests are not "
                "implemented): call it before the first named request or after tips_shutdown / tips_init");
  State& st = S();
  std::lock_guard<std::mutex> one(st.sparse_mu);
  int size;
  {
    std::lock_guard<std::mutex> lk(st.mu);
    if (!st.initialized) return fail(TIPS_ERR_NOT_INITIALIZED, "tips_init has not been called");
    TRY(set_device(st));
    size = st.size;
  }
  hipStream_t s = (hipStream_t)stream;
  // this rank's own verdict on its pointers travels with the record, so a rank that refuses its
  // arguments does not leave the others waiting in the exchange
  int own = 0;
  if (active) {
    own = need_device(dense_out, "dense_out");
    if (own == 0 && n > 0) own = need_device(values, "values");
    if (own == 0 && n > 0) own = need_device(indices, "indices");
  }
  const std::string own_msg = own ? last_error() : std::string();
  std::vector<int64_t> all((size_t)5 * size);
  const int64_t mine[5] = {n, rows, row_elems, dtype, own};
  if (size == 1) {
    std::copy(mine, mine + 5, all.begin());
  } else {
    TRY(tips_allgather_i64(mine, 5, all.data()));
  }
  if (own) return fail(own, "%s", own_msg.c_str());
  for (int r = 0; r < size; r++) {
    const int64_t* q = &all[(size_t)5 * r];
    if (q[1] != all[1] || q[2] != all[2] || q[3] != all[3])
      return fail(TIPS_ERR_MISMATCH,
                  "Mismatched sparse allreduce: rank %d has rows %lld, row_elems %lld, dtype %lld; rank 0 has rows %lld, "
                  "row_elems %lld, dtype %lld",
                  r, (long long)q[1], (long long)q[2], (long long)q[3], (long long)all[1], (long long)all[2],
                  (long long)all[3]);
  }
  for (int r = 0; r < size; r++)
    if (all[(size_t)5 * r + 4] != 0)
      return fail(TIPS_ERR_MISMATCH, "sparse allreduce: rank %d refused its arguments (status %lld)", r,
                  (long long)all[(size_t)5 * r + 4]);
  if (!active) return 0;
  const int64_t es = tips::dtype_size(dtype);
  std::vector<int64_t> counts(size), vcounts(size);
  int64_t G = 0;
  for (int r = 0; r < size; r++) {
    counts[r] = all[(size_t)5 * r];
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
    TRY(st.sparse_scratch.ensure((size_t)(idx_bytes + val_bytes + ws_bytes)));
    base = (char*)st.sparse_scratch.p;
    if (!st.ev_sparse) HIP_TRY(hipEventCreateWithFlags(&st.ev_sparse, hipEventDisableTiming));
    if (st.sparse_chain_valid) HIP_TRY(hipStreamWaitEvent(s, st.ev_sparse, 0));
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
  if (st.ev_sparse) {
    HIP_TRY(hipEventRecord(st.ev_sparse, s));
    st.sparse_chain_valid = true;
  }
  return 0;
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
