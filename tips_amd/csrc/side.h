// side.h — what the collectives that run beside the negotiation share (sparse.cc, adasum.cc,
// mxfp8.cc, reducescatter.cc): the argument checks (pointers, counts, the f32 factor,
// the capturing stream), how a call opens, and the record exchange in which
// every rank learns whether all ranks bring the same call and accept their own pointers before any
// of them enters a device exchange. The scratch they chain their calls on is rt.h's SideChain.
#pragma once

#include "rt.h"

namespace tips {
namespace rt {

// null: TIPS_ERR_INVALID_ARG; host memory: TIPS_ERR_UNSUPPORTED, "<what> is host memory: <feature> device pointers only"
int need_device(const void* p, const char* what, const char* feature);
// the counts of a list of `noun`s ("segment", "tensor"): none negative, the total (at most 2^56) in *total
int check_counts(const int64_t* counts, int n, const char* noun, int64_t* total);
uint64_t hash_counts(const int64_t* counts, int n);  // FNV-1a over the counts' bytes
// a factor the f32 kernels multiply by: finite as a double and as a float, or TIPS_ERR_INVALID_ARG
int check_factor(double factor);
// 0, or TIPS_ERR_UNSUPPORTED "<what> is never captured into a graph" where the stream is capturing:
// this rank's refusal, like a pointer it does not accept (a query that fails counts as not capturing)
int refuse_capture(const char* what, hipStream_t s);

// How a call opens. Refuses a call on, or beside, a running negotiation (`noun`: "sparse", "Adasum",
// "MXFP8"); takes the chain's mutex into *one; then, under st.mu: the lifecycle, the device, *size,
// the caller's rule on the rank count (`ranks`: 0 or fail(...); may be null) and, with `rccl_only`,
// the refusal under TIPS_ALGO_PEER. st.mu is not held on return.
using RankRule = int (*)(const char* what, int size);
int side_open(State& st, SideChain& chain, const char* what, const char* noun, RankRule ranks, bool rccl_only,
              std::unique_lock<std::mutex>* one, int* size);

// Every rank's record: the words the caller compares and, last, the rank's own verdict on its
// pointers - it travels with the record so that a rank which refuses its arguments does not leave
// the others waiting in the exchange. The caller runs the scans and the reports in its own order.
struct SideRecords {
  int size = 0, words = 0, own = 0;
  std::string own_msg;  // last_error() as the verdict left it
  std::vector<int64_t> all;
  const int64_t* of(int r) const { return &all[(size_t)words * r]; }
  int first_differing(int lo, int hi) const;  // the first rank whose words [lo, hi) are not rank 0's, or -1
  int first_refusing() const;                 // the first rank whose verdict is not 0, or -1
  int report_own() const { return own ? fail(own, "%s", own_msg.c_str()) : 0; }
  // TIPS_ERR_MISMATCH "<call>: rank r refused its arguments" (`call`: "sparse allreduce", "reduce-scatter", ...), or 0
  int report_refusing(const char* call) const;
};
// mine[words - 1] is the verdict; st.mu must not be held (tips_allgather_i64; one rank: a copy)
int side_exchange(int size, const int64_t* mine, int words, SideRecords* rec);

}  // namespace rt
}  // namespace tips
