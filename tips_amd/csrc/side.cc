// side.cc — the protocol the collectives beside the negotiation share (side.h).
#include "side.h"

#include <math.h>

#include <algorithm>

namespace tips {
namespace rt {

int need_device(const void* p, const char* what, const char* feature) {
  if (!p) return fail(TIPS_ERR_INVALID_ARG, "null pointer (%s)", what);
  if (!is_device_ptr(p))
    return fail(TIPS_ERR_UNSUPPORTED, "%s is host memory: %s device pointers only (nothing is staged)", what, feature);
  return 0;
}

int check_counts(const int64_t* counts, int n, const char* noun, int64_t* total) {
  if (n < 0 || (n > 0 && !counts)) return fail(TIPS_ERR_INVALID_ARG, "bad %s list (n %d)", noun, n);
  *total = 0;
  for (int i = 0; i < n; i++) {
    if (counts[i] < 0) return fail(TIPS_ERR_INVALID_ARG, "negative count (%s %d: %lld)", noun, i, (long long)counts[i]);
    if (__builtin_add_overflow(*total, counts[i], total) || *total > ((int64_t)1 << 56))
      return fail(TIPS_ERR_INVALID_ARG, "sizes overflow (%s %d)", noun, i);
  }
  return 0;
}

uint64_t hash_counts(const int64_t* counts, int n) {
  uint64_t h = kFnvBasis;
  for (int i = 0; i < n; i++)
    for (int k = 0; k < 8; k++) h = (h ^ (((uint64_t)counts[i] >> (8 * k)) & 0xff)) * kFnvPrime;
  return h;
}

int check_factor(double factor) {
  if (!isfinite(factor) || !isfinite((float)factor)) return fail(TIPS_ERR_INVALID_ARG, "factor %g is not a finite float", factor);
  return 0;
}

int refuse_capture(const char* what, hipStream_t s) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  if (cs == hipStreamCaptureStatusNone) return 0;
  return fail(TIPS_ERR_UNSUPPORTED, "%s is never captured into a graph (its stream is capturing)", what);
}

int side_open(State& st, SideChain& chain, const char* what, const char* noun, RankRule ranks, bool rccl_only,
              std::unique_lock<std::mutex>* one, int* size) {
  if (on_negotiation_thread() || negotiation_running())
    return fail(TIPS_ERR_UNSUPPORTED,
                "%s does not go through a running negotiation (named %s requests are not implemented): call it before the "
                "first named request or after tips_shutdown / tips_init",
                what, noun);
  *one = std::unique_lock<std::mutex>(chain.mu);
  std::lock_guard<std::mutex> lk(st.mu);
  if (!st.initialized) return fail(TIPS_ERR_NOT_INITIALIZED, "tips_init has not been called");
  TRY(set_device(st));
  *size = st.size;
  if (ranks) TRY(ranks(what, st.size));
  if (rccl_only && st.size > 1 && resolve_algo(st.algo, st.size, 0) == TIPS_ALGO_PEER)
    return fail(TIPS_ERR_UNSUPPORTED, "%s has one schedule, over RCCL send / recv: not available under TIPS_ALGO_PEER", what);
  return 0;
}

int side_exchange(int size, const int64_t* mine, int words, SideRecords* rec) {
  rec->size = size;
  rec->words = words;
  rec->own = (int)mine[words - 1];
  if (rec->own) rec->own_msg = last_error();
  rec->all.assign(mine, mine + words);  // (one rank: its own record is all of them)
  if (size == 1) return 0;
  rec->all.resize((size_t)words * size);
  return tips_allgather_i64(mine, words, rec->all.data());
}

int SideRecords::first_differing(int lo, int hi) const {
  for (int r = 1; r < size; r++)
    if (!std::equal(of(r) + lo, of(r) + hi, of(0) + lo)) return r;
  return -1;
}

int SideRecords::first_refusing() const {
  for (int r = 0; r < size; r++)
    if (of(r)[words - 1] != 0) return r;
  return -1;
}

int SideRecords::report_refusing(const char* call) const {
  const int r = first_refusing();
  if (r < 0) return 0;
  return fail(TIPS_ERR_MISMATCH, "%s: rank %d refused its arguments (status %lld)", call, r, (long long)of(r)[words - 1]);
}

}  // namespace rt
}  // namespace tips
