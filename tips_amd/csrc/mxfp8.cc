// mxfp8.cc — the MXFP8 wire's entry points of the C-ABI: the three local operations
// (tips_mxfp8_quantize, tips_mxfp8_fold, tips_mxfp8_dequantize over mxfp8.hip's kernels) and the two
// collectives around them, tips_allreduce_mxfp8 and tips_fused_allreduce_mxfp8_flat: every rank
// quantises its input once, the blocks are cut into p chunks, chunk q of every rank goes to rank q,
// which folds the p sources in rank order and requantises once, and the reduced chunks are gathered.
// A value is quantised twice whatever p is (a ring would requantise at every step).
// The calls with error feedback (tips_mxfp8_ef_bytes, tips_mxfp8_quantize_ef,
// tips_mxfp8_fold_ef, tips_allreduce_mxfp8_ef, tips_fused_allreduce_mxfp8_ef_flat) are the same
// code with a residual: the launchers take it as an argument that is null for the plain calls - the
// quantise over the state's sender part, the owner's fold over its owner part. The factor check, the
// capturing-stream verdict and the record exchange are side.h's, the segment cover mxfp8.h's.
#include <algorithm>
#include <vector>

#include "mxfp8.h"
#include "rt.h"
#include "side.h"

using namespace tips::rt;

namespace {

const char kTakes[] = "the MXFP8 calls take";  // need_device's phrase

// The list's flat layout: the tensors' element offsets, the flat element count E, and the segments a
// quantise (cover = true: every flat position up to round_up(E, 256), padding included) or a
// dequantise (the tensors' own elements) launches over. ptrs[i] may be null for an empty tensor.
struct Flat {
  int64_t elems = 0, total = 0;
  std::vector<tips::MxSeg> segs;
};

int flat_of(const void* const* ptrs, const int64_t* counts, int n, bool cover, Flat* f) {
  if (n > 0 && !ptrs) return fail(TIPS_ERR_INVALID_ARG, "bad tensor list (n %d)", n);
  TRY(check_counts(counts, n, "tensor", &f->total));
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
  if (cover) tips::mxfp8_cover(f->segs, tips::mxfp8_scales_offset(f->elems));
  return 0;
}

int check_wire(const void* wire, const char* what) {
  TRY(need_device(wire, what, kTakes));
  if ((reinterpret_cast<uintptr_t>(wire) & 15) != 0) return fail(TIPS_ERR_INVALID_ARG, "%s must be 16-B aligned", what);
  return 0;
}

// `residual`: the sender residual of the feedback form, or null for the plain quantise
int quantize_into(const Flat& f, unsigned char* wire, float* residual, hipStream_t s) {
  const int64_t so = tips::mxfp8_scales_offset(f.elems);
  const int64_t tail_begin = so / tips::kMxBlock, tail_end = tips::mxfp8_wire_bytes(f.elems) - so;
  HIP_TRY(tips::launch_mxfp8_quantize(f.segs.data(), (int)f.segs.size(), wire, wire + so, residual, tail_begin, tail_end, s));
  return 0;
}

// The feedback state of a list of E flat elements on p ranks, in f32 elements: the sender residual
// (one per flat position up to round_up(E, 256)), then the owner residual of a chunk (32 per block of
// the largest chunk, chunk 0 - the `per` that sizes a staged slot)
int64_t ef_sender_elems(int64_t E) { return tips::mxfp8_scales_offset(E); }
int64_t ef_elems(int64_t E, int p) {
  const int64_t per = p > 1 ? chunk_of(tips::mxfp8_blocks(E), p, 8, 0).len() : 0;
  return ef_sender_elems(E) + tips::kMxBlock * per;
}

// [a, a + an) and [b, b + bn) share a byte
bool overlaps(const void* a, int64_t an, const void* b, int64_t bn) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return an > 0 && bn > 0 && x < y + (uintptr_t)bn && y < x + (uintptr_t)an;
}

// a residual / state buffer of `bytes` bytes: a 16-B aligned device pointer that overlaps no tensor of the lists
int check_residual(const void* r, int64_t bytes, const char* what, const Flat* a, const Flat* b) {
  TRY(need_device(r, what, kTakes));
  if ((reinterpret_cast<uintptr_t>(r) & 15) != 0) return fail(TIPS_ERR_INVALID_ARG, "%s must be 16-B aligned", what);
  for (const Flat* f : {a, b})
    if (f)
      for (const tips::MxSeg& sg : f->segs)
        if (sg.ptr && overlaps(r, bytes, sg.ptr, sg.count * 4)) return fail(TIPS_ERR_INVALID_ARG, "%s overlaps a tensor of the list", what);
  return 0;
}

int dequantize_from(const Flat& f, const unsigned char* wire, double factor, hipStream_t s) {
  HIP_TRY(tips::launch_mxfp8_dequantize(f.segs.data(), (int)f.segs.size(), wire, wire + tips::mxfp8_scales_offset(f.elems),
                                        (float)factor, s));
  return 0;
}

int at_most_max_srcs(const char* what, int size) {
  if (size > tips::kMxMaxSrcs)
    return fail(TIPS_ERR_UNSUPPORTED, "%s folds at most %d ranks, not %d", what, tips::kMxMaxSrcs, size);
  return 0;
}

// What both collectives check once open, before any device exchange: that every rank brings the
// same list and accepts its own pointers and stream (`own`: this rank's verdict)
// (`with_ef`: the call kind is folded into the feedback calls' count-hash word, so that a feedback call
// paired with a plain call is a mismatch; the plain call's record is what it was)
int agree(int size, int n, int64_t total, const int64_t* counts, int own, bool with_ef) {
  const uint64_t h = hash_counts(counts, n);
  const int64_t mine[4] = {n, total, (int64_t)(with_ef ? (h ^ 0xEFull) * kFnvPrime : h), own};
  SideRecords rec;
  TRY(side_exchange(size, mine, 4, &rec));
  // reported in this order: a mismatch, another rank's refusal, this rank's own
  if (const int r = rec.first_differing(0, 3); r >= 0) {
    const int64_t *q = rec.of(r), *q0 = rec.of(0);
    return fail(TIPS_ERR_MISMATCH,
                "Mismatched MXFP8 allreduce: rank %d has %lld tensors, %lld elements, count hash %llx; rank 0 has %lld "
                "tensors, %lld elements, count hash %llx",
                r, (long long)q[0], (long long)q[1], (unsigned long long)q[2], (long long)q0[0], (long long)q0[1],
                (unsigned long long)q0[2]);
  }
  if (!own) TRY(rec.report_refusing("MXFP8 allreduce"));
  return rec.report_own();
}

// Blocks of a wire buffer, or of a staged chunk: where their payload and their scales start
struct Part {
  unsigned char *payload, *scales;
  int64_t blocks;
};

// One RCCL group with every peer q: to(q) goes to q and q's blocks land in from(q), payload then
// scales each way; a part of no blocks is not exchanged.
template <class To, class From>
int exchange(State& st, hipStream_t s, To&& to, From&& from) {
  TRY(rccl_enter(st, s));
  NCCL_TRY(ncclGroupStart());
  for (int q = 0; q < st.size; q++) {
    if (q == st.rank) continue;
    const Part t = to(q), f = from(q);
    if (t.blocks > 0) {
      NCCL_TRY(ncclSend(t.payload, (size_t)(t.blocks * tips::kMxBlock), ncclInt8, q, st.comm, s));
      NCCL_TRY(ncclSend(t.scales, (size_t)t.blocks, ncclInt8, q, st.comm, s));
    }
    if (f.blocks > 0) {
      NCCL_TRY(ncclRecv(f.payload, (size_t)(f.blocks * tips::kMxBlock), ncclInt8, q, st.comm, s));
      NCCL_TRY(ncclRecv(f.scales, (size_t)f.blocks, ncclInt8, q, st.comm, s));
    }
  }
  NCCL_TRY(ncclGroupEnd());
  return rccl_leave(st, s);
}

// The schedule: `in` (the segments of this rank's input) -> `out` (the segments of the result), both
// over the same flat layout. `ef`: the feedback state (sender residual, then this rank's owner
// residual), or null for the plain collective. Caller holds st.mu and st.mxfp8.mu.
int run_collective(State& st, const Flat& in, const Flat& out, double factor, float* ef, hipStream_t s) {
  const int p = st.size, rank = st.rank;
  const int64_t E = in.elems, B = tips::mxfp8_blocks(E), so = tips::mxfp8_scales_offset(E);
  const int64_t wire = tips::mxfp8_wire_bytes(E);
  // chunk q: blocks chunk_of(B, p, 8, q) - a function of (E, p) alone, payload starts 256-B aligned
  const int64_t per = p > 1 ? chunk_of(B, p, 8, 0).len() : 0;
  const int64_t slot = round_up(per * tips::kMxBlock + per, kAlignBytes);  // a staged chunk: payload, then scales
  TRY(st.mxfp8.open(s, (size_t)(2 * wire + (p - 1) * slot)));
  unsigned char* w0 = (unsigned char*)st.mxfp8.scratch.p;
  unsigned char* w1 = w0 + wire;
  unsigned char* stage = w1 + wire;
  TRY(quantize_into(in, w0, ef, s));
  const unsigned char* reduced = w0;
  if (p > 1) {
    TRY(ensure_comm(st));
    auto slot_of = [&](int r) { return stage + (int64_t)(r < rank ? r : r - 1) * slot; };
    auto staged = [&](int r, int64_t blocks) { return Part{slot_of(r), slot_of(r) + per * tips::kMxBlock, blocks}; };
    auto blocks_of = [&](unsigned char* w, Range c) { return Part{w + c.b * tips::kMxBlock, w + so + c.b, c.len()}; };
    const Range mine = chunk_of(B, p, 8, rank);
    // scatter: chunk q of this rank's buffer to its owner q, the peers' chunks `mine` into their slots
    TRY(exchange(
        st, s, [&](int q) { return blocks_of(w0, chunk_of(B, p, 8, q)); }, [&](int q) { return staged(q, mine.len()); }));
    if (mine.len() > 0) {
      tips::MxSrcs srcs = {};
      for (int r = 0; r < p; r++) {
        const Part src = r == rank ? blocks_of(w0, mine) : staged(r, mine.len());
        srcs.payload[r] = src.payload;
        srcs.scales[r] = src.scales;
      }
      const Part dst = blocks_of(w1, mine);
      HIP_TRY(tips::launch_mxfp8_fold(dst.payload, dst.scales, srcs, p, mine.len(), ef ? ef + ef_sender_elems(E) : nullptr, s));
    }
    // gather: the reduced chunk `mine` to every peer, every peer's reduced chunk into its place
    TRY(exchange(
        st, s, [&](int) { return blocks_of(w1, mine); }, [&](int q) { return blocks_of(w1, chunk_of(B, p, 8, q)); }));
    reduced = w1;
  }
  TRY(dequantize_from(out, reduced, factor, s));
  return st.mxfp8.close(s);
}

// `with_ef`: the feedback form over the state `ef` of `ef_bytes` bytes
int collective(const char* what, const void* const* ins, const int64_t* counts, int n, void* const* outs, double factor,
               bool with_ef, void* ef, int64_t ef_bytes, hipStream_t s) {
  TRY(check_factor(factor));
  Flat in, out;
  TRY(flat_of(ins, counts, n, true, &in));
  TRY(flat_of(outs, counts, n, false, &out));
  State& st = S();
  std::unique_lock<std::mutex> one;
  int size;
  TRY(side_open(st, st.mxfp8, what, "MXFP8", at_most_max_srcs, /*rccl_only=*/true, &one, &size));
  int own = refuse_capture(what, s);
  for (size_t i = 0; i < in.segs.size() && own == 0; i++)
    if (in.segs[i].ptr) own = need_device(in.segs[i].ptr, "an input", kTakes);
  for (size_t i = 0; i < out.segs.size() && own == 0; i++) own = need_device(out.segs[i].ptr, "an output", kTakes);
  if (with_ef && in.total > 0 && own == 0) {
    const int64_t need = 4 * ef_elems(in.elems, size);
    if (ef_bytes < need)  // the state was sized for another list or rank count: this rank's verdict
      own = fail(TIPS_ERR_MISMATCH, "%s: ef_bytes %lld is below tips_mxfp8_ef_bytes(%lld, %d) = %lld", what, (long long)ef_bytes,
                 (long long)in.elems, size, (long long)need);
    else own = check_residual(ef, need, "ef", &in, &out);
  }
  TRY(agree(size, n, in.total, counts, own, with_ef));
  if (in.total == 0) return 0;
  std::lock_guard<std::mutex> lk(st.mu);
  if (!st.initialized) return fail(TIPS_ERR_NOT_INITIALIZED, "tips_init has not been called");
  TRY(set_device(st));
  return run_collective(st, in, out, factor, with_ef ? (float*)ef : nullptr, s);
}

// tips_mxfp8_fold and, `with_ef`, tips_mxfp8_fold_ef over `residual` (32 f32 per block of the range)
int fold_blocks(void* dst_wire, const void* const* src_wires, int nsrc, int64_t flat_elems, int64_t block_begin,
                int64_t block_count, bool with_ef, void* residual, hipStream_t s) {
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
  if (with_ef) {
    const int64_t rbytes = 4 * tips::kMxBlock * block_count, wbytes = tips::mxfp8_wire_bytes(flat_elems);
    TRY(check_residual(residual, rbytes, "residual", nullptr, nullptr));
    bool hit = overlaps(residual, rbytes, dst_wire, wbytes);
    for (int j = 0; j < nsrc; j++) hit = hit || overlaps(residual, rbytes, src_wires[j], wbytes);
    if (hit) return fail(TIPS_ERR_INVALID_ARG, "residual overlaps a wire buffer");
  }
  unsigned char* d = (unsigned char*)dst_wire;
  HIP_TRY(tips::launch_mxfp8_fold(d + block_begin * tips::kMxBlock, d + so + block_begin, srcs, nsrc, block_count,
                                  with_ef ? (float*)residual : nullptr, s));
  return 0;
}

// the flat list calls: every tensor's result at its layout offset in `flat`
int flat_collective(const char* what, const void* const* ins, const int64_t* counts, int n, void* flat, double factor,
                    bool with_ef, void* ef, int64_t ef_bytes, hipStream_t s) {
  if (n < 0 || (n > 0 && (!counts || !ins))) return fail(TIPS_ERR_INVALID_ARG, "bad tensor list (n %d)", n);
  // the outputs: every tensor at its layout offset in `flat`
  std::vector<int64_t> offs((size_t)n);
  std::vector<void*> outs((size_t)n, nullptr);
  int64_t total;
  TRY(check_counts(counts, n, "tensor", &total));
  if (total > 0) {
    if (!flat) return fail(TIPS_ERR_INVALID_ARG, "null pointer (flat)");
    fused_layout(counts, n, TIPS_FLOAT32, offs.data());
    for (int i = 0; i < n; i++)
      if (counts[i] > 0) outs[i] = (char*)flat + offs[i];
  }
  return collective(what, ins, counts, n, outs.data(), factor, with_ef, ef, ef_bytes, s);
}

}  // namespace

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
    if (sg.ptr) TRY(need_device(sg.ptr, "a tensor of the list", kTakes));
  return quantize_into(f, (unsigned char*)wire, nullptr, (hipStream_t)stream);
}

int64_t tips_mxfp8_ef_bytes(int64_t flat_elems, int nranks) {
  if (flat_elems < 0 || flat_elems > ((int64_t)1 << 56)) return fail(TIPS_ERR_INVALID_ARG, "bad size (%lld elements)", (long long)flat_elems);
  if (nranks < 1 || nranks > tips::kMxMaxSrcs) return fail(TIPS_ERR_INVALID_ARG, "nranks must be 1 ... %d (got %d)", tips::kMxMaxSrcs, nranks);
  return 4 * ef_elems(flat_elems, nranks);
}

int tips_mxfp8_quantize_ef(const void* const* ins, const int64_t* counts, int n, void* wire, void* residual, void* stream) {
  Flat f;
  TRY(flat_of(ins, counts, n, true, &f));
  if (f.total == 0) return 0;
  TRY(check_wire(wire, "wire"));
  for (const tips::MxSeg& sg : f.segs)
    if (sg.ptr) TRY(need_device(sg.ptr, "a tensor of the list", kTakes));
  const int64_t rbytes = 4 * ef_sender_elems(f.elems);
  TRY(check_residual(residual, rbytes, "residual", &f, nullptr));
  if (overlaps(residual, rbytes, wire, tips::mxfp8_wire_bytes(f.elems))) return fail(TIPS_ERR_INVALID_ARG, "residual overlaps the wire buffer");
  return quantize_into(f, (unsigned char*)wire, (float*)residual, (hipStream_t)stream);
}

int tips_mxfp8_fold(void* dst_wire, const void* const* src_wires, int nsrc, int64_t flat_elems, int64_t block_begin,
                    int64_t block_count, void* stream) {
  return fold_blocks(dst_wire, src_wires, nsrc, flat_elems, block_begin, block_count, false, nullptr, (hipStream_t)stream);
}

int tips_mxfp8_fold_ef(void* dst_wire, const void* const* src_wires, int nsrc, int64_t flat_elems, int64_t block_begin,
                       int64_t block_count, void* residual, void* stream) {
  return fold_blocks(dst_wire, src_wires, nsrc, flat_elems, block_begin, block_count, true, residual, (hipStream_t)stream);
}

int tips_mxfp8_dequantize(void* const* outs, const int64_t* counts, int n, const void* wire, double factor, void* stream) {
  TRY(check_factor(factor));
  Flat f;
  TRY(flat_of(outs, counts, n, false, &f));
  if (f.total == 0) return 0;
  TRY(check_wire(wire, "wire"));
  for (const tips::MxSeg& sg : f.segs) TRY(need_device(sg.ptr, "a tensor of the list", kTakes));
  return dequantize_from(f, (const unsigned char*)wire, factor, (hipStream_t)stream);
}

int tips_allreduce_mxfp8(const void* in, void* out, int64_t count, double factor, void* stream) {
  if (count < 0) return fail(TIPS_ERR_INVALID_ARG, "negative count");
  return collective("tips_allreduce_mxfp8", &in, &count, 1, &out, factor, false, nullptr, 0, (hipStream_t)stream);
}

int tips_allreduce_mxfp8_ef(const void* in, void* out, int64_t count, double factor, void* ef, int64_t ef_bytes, void* stream) {
  if (count < 0) return fail(TIPS_ERR_INVALID_ARG, "negative count");
  return collective("tips_allreduce_mxfp8_ef", &in, &count, 1, &out, factor, true, ef, ef_bytes, (hipStream_t)stream);
}

int tips_fused_allreduce_mxfp8_flat(const void* const* ins, const int64_t* counts, int n, void* flat, double factor,
                                    void* stream) {
  return flat_collective("tips_fused_allreduce_mxfp8_flat", ins, counts, n, flat, factor, false, nullptr, 0, (hipStream_t)stream);
}

int tips_fused_allreduce_mxfp8_ef_flat(const void* const* ins, const int64_t* counts, int n, void* flat, double factor,
                                       void* ef, int64_t ef_bytes, void* stream) {
  return flat_collective("tips_fused_allreduce_mxfp8_ef_flat", ins, counts, n, flat, factor, true, ef, ef_bytes,
                         (hipStream_t)stream);
}

}  // extern "C"
