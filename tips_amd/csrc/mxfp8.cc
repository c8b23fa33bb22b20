// mxfp8.cc — the MXFP8 wire's entry points of the C-ABI: the three local operations
// (tips_mxfp8_quantize, tips_mxfp8_fold, tips_mxfp8_dequantize over mxfp8.hip's kernels) and the two
// collectives around them, tips_allreduce_mxfp8 and tips_fused_allreduce_mxfp8_flat: every rank
// quantises its input once, the blocks are cut into p chunks, chunk q of every rank goes to rank q,
// which folds the p sources in rank order and requantises once, and the reduced chunks are gathered.
// A value is quantised twice whatever p is (a ring would requantise at every step).
#include <math.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mxfp8.h"
#include "rt.h"

using namespace tips::rt;

namespace {

int need_device(const void* p, const char* what) {
  if (!p) return fail(TIPS_ERR_INVALID_ARG, "null pointer (%s)", what);
  if (!is_device_ptr(p))
    return fail(TIPS_ERR_UNSUPPORTED, "%s is host memory: the MXFP8 calls take device pointers only (nothing is staged)", what);
  return 0;
}

int check_factor(double factor) {
  if (!isfinite(factor) || !isfinite((float)factor)) return fail(TIPS_ERR_INVALID_ARG, "factor %g is not a finite float", factor);
  return 0;
}

// The list's flat layout: the tensors' element offsets, the flat element count E, and the segments a
// quantise (cover = true: every flat position up to round_up(E, 256), padding included) or a
// dequantise (the tensors' own elements) launches over. ptrs[i] may be null for an empty tensor.
struct Flat {
  int64_t elems = 0, total = 0;
  std::vector<tips::MxSeg> segs;
};

int flat_of(const void* const* ptrs, const int64_t* counts, int n, bool cover, Flat* f) {
  if (n < 0 || (n > 0 && (!counts || !ptrs))) return fail(TIPS_ERR_INVALID_ARG, "bad tensor list (n %d)", n);
  for (int i = 0; i < n; i++) {
    if (counts[i] < 0) return fail(TIPS_ERR_INVALID_ARG, "negative count (tensor %d: %lld)", i, (long long)counts[i]);
    if (__builtin_add_overflow(f->total, counts[i], &f->total) || f->total > ((int64_t)1 << 56))
      return fail(TIPS_ERR_INVALID_ARG, "sizes overflow (tensor %d)", i);
  }
  if (f->total == 0) return 0;
  std::vector<int64_t> offs((size_t)n);
  f->elems = fused_layout(counts, n, TIPS_FLOAT32, offs.data()) / 4;
  for (int i = 0; i < n; i++)
    if (counts[i] > 0) {
      if (!ptrs[i]) return fail(TIPS_ERR_INVALID_ARG, "null pointer (tensor %d)", i);
      if ((reinterpret_cast<uintptr_t>(ptrs[i]) & 3) != 0) return fail(TIPS_ERR_INVALID_ARG, "tensor %d is not 4-B aligned", i);
      f->segs.push_back(tips::MxSeg{ptrs[i], offs[i] / 4, counts[i], (counts[i] + 31) / 32 * 32});
    }
  std::sort(f->segs.begin(), f->segs.end(), [](const tips::MxSeg& a, const tips::MxSeg& b) { return a.off < b.off; });
  if (cover) {
    const int64_t end = tips::mxfp8_scales_offset(f->elems);
    for (size_t i = 0; i < f->segs.size(); i++)
      f->segs[i].span = (i + 1 < f->segs.size() ? f->segs[i + 1].off : end) - f->segs[i].off;
    if (f->segs[0].off > 0) f->segs.insert(f->segs.begin(), tips::MxSeg{nullptr, 0, 0, f->segs[0].off});
  }
  return 0;
}

int check_wire(const void* wire, const char* what) {
  TRY(need_device(wire, what));
  if ((reinterpret_cast<uintptr_t>(wire) & 15) != 0) return fail(TIPS_ERR_INVALID_ARG, "%s must be 16-B aligned", what);
  return 0;
}

int quantize_into(const Flat& f, unsigned char* wire, hipStream_t s) {
  const int64_t so = tips::mxfp8_scales_offset(f.elems);
  HIP_TRY(tips::launch_mxfp8_quantize(f.segs.data(), (int)f.segs.size(), wire, wire + so, so / tips::kMxBlock,
                                      tips::mxfp8_wire_bytes(f.elems) - so, s));
  return 0;
}

int dequantize_from(const Flat& f, const unsigned char* wire, double factor, hipStream_t s) {
  HIP_TRY(tips::launch_mxfp8_dequantize(f.segs.data(), (int)f.segs.size(), wire, wire + tips::mxfp8_scales_offset(f.elems),
                                        (float)factor, s));
  return 0;
}

uint64_t hash_counts(const int64_t* counts, int n) {  // FNV-1a over the counts' bytes
  uint64_t h = 1469598103934665603ull;
  for (int i = 0; i < n; i++)
    for (int k = 0; k < 8; k++) h = (h ^ (((uint64_t)counts[i] >> (8 * k)) & 0xff)) * 1099511628211ull;
  return h;
}

const char kBusy[] =
    "%s does not go through a running negotiation (named MXFP8 requests are not implemented): call it before the "
    "first named request or after tips_shutdown / tips_init";

// What both collectives check before any device exchange: the lifecycle, the rank count, the
// algorithm, and that every rank brings the same list and accepts its own pointers
// (`own`: this rank's verdict, which travels with the record so that no rank waits in the exchange).
int agree(State& st, const char* what, int n, int64_t total, const int64_t* counts, int own, int* size) {
  const std::string own_msg = own ? last_error() : std::string();
  {
    std::lock_guard<std::mutex> lk(st.mu);
    if (!st.initialized) return fail(TIPS_ERR_NOT_INITIALIZED, "tips_init has not been called");
    TRY(set_device(st));
    *size = st.size;
    if (st.size > tips::kMxMaxSrcs)
      return fail(TIPS_ERR_UNSUPPORTED, "%s folds at most %d ranks, not %d", what, tips::kMxMaxSrcs, st.size);
    if (st.size > 1 && resolve_algo(st.algo, st.size, 0) == TIPS_ALGO_PEER)
      return fail(TIPS_ERR_UNSUPPORTED, "%s has one schedule, over RCCL send / recv: not available under TIPS_ALGO_PEER", what);
  }
  const std::string& msg = own_msg;
  if (*size > 1) {
    const int64_t mine[4] = {n, total, (int64_t)hash_counts(counts, n), own};
    std::vector<int64_t> all((size_t)4 * *size);
    TRY(tips_allgather_i64(mine, 4, all.data()));
    for (int r = 0; r < *size; r++) {
      const int64_t* q = &all[(size_t)4 * r];
      if (q[0] != all[0] || q[1] != all[1] || q[2] != all[2])
        return fail(TIPS_ERR_MISMATCH,
                    "Mismatched MXFP8 allreduce: rank %d has %lld tensors, %lld elements, count hash %llx; rank 0 has %lld "
                    "tensors, %lld elements, count hash %llx",
                    r, (long long)q[0], (long long)q[1], (unsigned long long)q[2], (long long)all[0], (long long)all[1],
                    (unsigned long long)all[2]);
    }
    for (int r = 0; r < *size; r++)
      if (all[(size_t)4 * r + 3] != 0 && !own)
        return fail(TIPS_ERR_MISMATCH, "MXFP8 allreduce: rank %d refused its arguments (status %lld)", r,
                    (long long)all[(size_t)4 * r + 3]);
  }
  if (own) return fail(own, "%s", msg.c_str());
  return 0;
}

// The schedule: `in` (the segments of this rank's input) -> `out` (the segments of the result), both
// over the same flat layout. Caller holds st.mu and st.mxfp8_mu.
int run_collective(State& st, const Flat& in, const Flat& out, double factor, hipStream_t s) {
  const int p = st.size, rank = st.rank;
  const int64_t E = in.elems, B = tips::mxfp8_blocks(E), so = tips::mxfp8_scales_offset(E);
  const int64_t wire = tips::mxfp8_wire_bytes(E);
  // chunk q: blocks chunk_of(B, p, 8, q) - a function of (E, p) alone, payload starts 256-B aligned
  const int64_t per = p > 1 ? chunk_of(B, p, 8, 0).len() : 0;
  const int64_t slot = round_up(per * tips::kMxBlock + per, kAlignBytes);  // a staged chunk: payload, then scales
  TRY(st.mxfp8_scratch.ensure((size_t)(2 * wire + (p - 1) * slot)));
  unsigned char* w0 = (unsigned char*)st.mxfp8_scratch.p;
  unsigned char* w1 = w0 + wire;
  unsigned char* stage = w1 + wire;
  if (!st.ev_mxfp8) HIP_TRY(hipEventCreateWithFlags(&st.ev_mxfp8, hipEventDisableTiming));
  if (st.mxfp8_chain_valid) HIP_TRY(hipStreamWaitEvent(s, st.ev_mxfp8, 0));
  TRY(quantize_into(in, w0, s));
  const unsigned char* reduced = w0;
  if (p > 1) {
    TRY(ensure_comm(st));
    auto slot_of = [&](int r) { return stage + (int64_t)(r < rank ? r : r - 1) * slot; };
    const Range mine = chunk_of(B, p, 8, rank);
    TRY(rccl_enter(st, s));
    NCCL_TRY(ncclGroupStart());
    for (int q = 0; q < p; q++) {
      if (q == rank) continue;
      const Range c = chunk_of(B, p, 8, q);
      if (c.len() > 0) {
        NCCL_TRY(ncclSend(w0 + c.b * tips::kMxBlock, (size_t)(c.len() * tips::kMxBlock), ncclInt8, q, st.comm, s));
        NCCL_TRY(ncclSend(w0 + so + c.b, (size_t)c.len(), ncclInt8, q, st.comm, s));
      }
      if (mine.len() > 0) {
        NCCL_TRY(ncclRecv(slot_of(q), (size_t)(mine.len() * tips::kMxBlock), ncclInt8, q, st.comm, s));
        NCCL_TRY(ncclRecv(slot_of(q) + per * tips::kMxBlock, (size_t)mine.len(), ncclInt8, q, st.comm, s));
      }
    }
    NCCL_TRY(ncclGroupEnd());
    TRY(rccl_leave(st, s));
    if (mine.len() > 0) {
      tips::MxSrcs srcs = {};
      for (int r = 0; r < p; r++) {
        srcs.payload[r] = r == rank ? w0 + mine.b * tips::kMxBlock : slot_of(r);
        srcs.scales[r] = r == rank ? w0 + so + mine.b : slot_of(r) + per * tips::kMxBlock;
      }
      HIP_TRY(tips::launch_mxfp8_fold(w1 + mine.b * tips::kMxBlock, w1 + so + mine.b, srcs, p, mine.len(), s));
    }
    TRY(rccl_enter(st, s));
    NCCL_TRY(ncclGroupStart());
    for (int q = 0; q < p; q++) {
      if (q == rank) continue;
      const Range c = chunk_of(B, p, 8, q);
      if (mine.len() > 0) {
        NCCL_TRY(ncclSend(w1 + mine.b * tips::kMxBlock, (size_t)(mine.len() * tips::kMxBlock), ncclInt8, q, st.comm, s));
        NCCL_TRY(ncclSend(w1 + so + mine.b, (size_t)mine.len(), ncclInt8, q, st.comm, s));
      }
      if (c.len() > 0) {
        NCCL_TRY(ncclRecv(w1 + c.b * tips::kMxBlock, (size_t)(c.len() * tips::kMxBlock), ncclInt8, q, st.comm, s));
        NCCL_TRY(ncclRecv(w1 + so + c.b, (size_t)c.len(), ncclInt8, q, st.comm, s));
      }
    }
    NCCL_TRY(ncclGroupEnd());
    TRY(rccl_leave(st, s));
    reduced = w1;
  }
  TRY(dequantize_from(out, reduced, factor, s));
  HIP_TRY(hipEventRecord(st.ev_mxfp8, s));
  st.mxfp8_chain_valid = true;
  return 0;
}

int collective(const char* what, const void* const* ins, const int64_t* counts, int n, void* const* outs, double factor,
               hipStream_t s) {
  TRY(check_factor(factor));
  Flat in, out;
  TRY(flat_of(ins, counts, n, true, &in));
  TRY(flat_of(outs, counts, n, false, &out));
  if (on_negotiation_thread() || negotiation_running()) return fail(TIPS_ERR_UNSUPPORTED, kBusy, what);
  State& st = S();
  std::lock_guard<std::mutex> one(st.mxfp8_mu);
  // a capturing stream is refused before anything else touches the runtime
  int own = 0;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess) (void)hipGetLastError();
  else if (cs != hipStreamCaptureStatusNone)
    own = fail(TIPS_ERR_UNSUPPORTED, "%s is never captured into a graph (its stream is capturing)", what);
  for (size_t i = 0; i < in.segs.size() && own == 0; i++)
    if (in.segs[i].ptr) own = need_device(in.segs[i].ptr, "an input");
  for (size_t i = 0; i < out.segs.size() && own == 0; i++) own = need_device(out.segs[i].ptr, "an output");
  int size;
  TRY(agree(st, what, n, in.total, counts, own, &size));
  if (in.total == 0) return 0;
  std::lock_guard<std::mutex> lk(st.mu);
  if (!st.initialized) return fail(TIPS_ERR_NOT_INITIALIZED, "tips_init has not been called");
  TRY(set_device(st));
  return run_collective(st, in, out, factor, s);
}

}  // namespace

namespace tips {
namespace rt {

void mxfp8_release(State& st) {
  st.mxfp8_scratch.release();
  if (st.ev_mxfp8) {
    (void)hipEventDestroy(st.ev_mxfp8);
    st.ev_mxfp8 = nullptr;
  }
  st.mxfp8_chain_valid = false;
}

}  // namespace rt
}  // namespace tips

extern "C" {

int64_t tips_mxfp8_wire_bytes(int64_t flat_elems, int64_t* scales_offset) {
  if (flat_elems < 0 || flat_elems > ((int64_t)1 << 56)) return fail(TIPS_ERR_INVALID_ARG, "bad size (%lld elements)", (long long)flat_elems);
  if (scales_offset) *scales_offset = tips::mxfp8_scales_offset(flat_elems);
  return tips::mxfp8_wire_bytes(flat_elems);
}

int tips_mxfp8_quantize(const void* const* ins, const int64_t* counts, int n, void* wire, void* stream) {
  Flat f;
  TRY(flat_of(ins, counts, n, true, &f));
  if (f.total == 0) return 0;
  TRY(check_wire(wire, "wire"));
  for (const tips::MxSeg& sg : f.segs)
    if (sg.ptr) TRY(need_device(sg.ptr, "a tensor of the list"));
  return quantize_into(f, (unsigned char*)wire, (hipStream_t)stream);
}

int tips_mxfp8_fold(void* dst_wire, const void* const* src_wires, int nsrc, int64_t flat_elems, int64_t block_begin,
                    int64_t block_count, void* stream) {
  if (nsrc < 1 || nsrc > tips::kMxMaxSrcs) return fail(TIPS_ERR_INVALID_ARG, "nsrc must be 1 ... %d (got %d)", tips::kMxMaxSrcs, nsrc);
  if (flat_elems < 0 || flat_elems > ((int64_t)1 << 56) || block_begin < 0 || block_count < 0)
    return fail(TIPS_ERR_INVALID_ARG, "negative size (elements %lld, blocks %lld + %lld)", (long long)flat_elems,
                (long long)block_begin, (long long)block_count);
  if (block_count > tips::mxfp8_blocks(flat_elems) - block_begin)
    return fail(TIPS_ERR_INVALID_ARG, "blocks %lld + %lld lie outside the buffer's %lld", (long long)block_begin,
                (long long)block_count, (long long)tips::mxfp8_blocks(flat_elems));
  if (!src_wires) return fail(TIPS_ERR_INVALID_ARG, "null pointer (src_wires)");
  if (block_count == 0) return 0;
  TRY(check_wire(dst_wire, "dst_wire"));
  const int64_t so = tips::mxfp8_scales_offset(flat_elems);
  tips::MxSrcs srcs = {};
  for (int j = 0; j < nsrc; j++) {
    TRY(check_wire(src_wires[j], "a source wire buffer"));
    srcs.payload[j] = (const unsigned char*)src_wires[j] + block_begin * tips::kMxBlock;
    srcs.scales[j] = (const unsigned char*)src_wires[j] + so + block_begin;
  }
  unsigned char* d = (unsigned char*)dst_wire;
  HIP_TRY(tips::launch_mxfp8_fold(d + block_begin * tips::kMxBlock, d + so + block_begin, srcs, nsrc, block_count,
                                  (hipStream_t)stream));
  return 0;
}

int tips_mxfp8_dequantize(void* const* outs, const int64_t* counts, int n, const void* wire, double factor, void* stream) {
  TRY(check_factor(factor));
  Flat f;
  TRY(flat_of(outs, counts, n, false, &f));
  if (f.total == 0) return 0;
  TRY(check_wire(wire, "wire"));
  for (const tips::MxSeg& sg : f.segs) TRY(need_device(sg.ptr, "a tensor of the list"));
  return dequantize_from(f, (const unsigned char*)wire, factor, (hipStream_t)stream);
}

int tips_allreduce_mxfp8(const void* in, void* out, int64_t count, double factor, void* stream) {
  if (count < 0) return fail(TIPS_ERR_INVALID_ARG, "negative count");
  return collective("tips_allreduce_mxfp8", &in, &count, 1, &out, factor, (hipStream_t)stream);
}

int tips_fused_allreduce_mxfp8_flat(const void* const* ins, const int64_t* counts, int n, void* flat, double factor,
                                    void* stream) {
  if (n < 0 || (n > 0 && (!counts || !ins))) return fail(TIPS_ERR_INVALID_ARG, "bad tensor list (n %d)", n);
  // the outputs: every tensor at its layout offset in `flat`
  std::vector<int64_t> offs((size_t)n);
  std::vector<void*> outs((size_t)n, nullptr);
  int64_t total = 0;
  for (int i = 0; i < n; i++) {
    if (counts[i] < 0) return fail(TIPS_ERR_INVALID_ARG, "negative count (tensor %d: %lld)", i, (long long)counts[i]);
    total += counts[i] > 0;
  }
  if (total > 0) {
    if (!flat) return fail(TIPS_ERR_INVALID_ARG, "null pointer (flat)");
    fused_layout(counts, n, TIPS_FLOAT32, offs.data());
    for (int i = 0; i < n; i++)
      if (counts[i] > 0) outs[i] = (char*)flat + offs[i];
  }
  return collective("tips_fused_allreduce_mxfp8_flat", ins, counts, n, outs.data(), factor, (hipStream_t)stream);
}

}  // extern "C"
