// reducescatter.cc — the reduce-scatter entry points of the C-ABI: the two pure-host
// layout calls, tips_reducescatter_fold (reducescatter.hip's kernel alone) and the collectives
// tips_reducescatter / tips_grouped_reducescatter around it: every rank sends slice q of its tensors to
// rank q in one RCCL group and folds the p sources of its own slices in rank order, straight into the
// callers' outputs. It is the direct schedule's first half: the same fold over the same operands, so a
// shard is bit-identical to that slice of the direct allreduce.
// The MXFP8 reduce-scatter (tips_reducescatter_mxfp8_layout, tips_reducescatter_mxfp8_fold,
// tips_reducescatter_mxfp8, tips_grouped_reducescatter_mxfp8) is the same exchange with the peer
// regions quantised once (mxfp8.hip's quantise) and the owner's fold reading wire bytes beside its
// own f32 slices (mxfp8.hip's fold-dequantise).
// Both kinds of collective go through one entry path, enter(): an entry keeps its own checks on its
// scalar arguments, its words of the record, its mismatch text and its schedule.
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mxfp8.h"
#include "reducescatter.h"
#include "rt.h"
#include "side.h"

using namespace tips::rt;

namespace {

const char kTakes[] = "the reduce-scatter takes";  // need_device's phrase

int at_most_max_srcs(const char* what, int size) {
  if (size > tips::kMaxSrcs) return fail(TIPS_ERR_UNSUPPORTED, "%s folds at most %d ranks, not %d", what, tips::kMaxSrcs, size);
  return 0;
}

// dtype, op and factors: what every entry checks the same way
int check_op(int dtype, int op, double pre, double post) {
  TRY(check_dtype(dtype));
  if (op != TIPS_OP_SUM && op != TIPS_OP_MAX && op != TIPS_OP_MIN) return fail(TIPS_ERR_INVALID_ARG, "unknown op %d", op);
  TRY(check_scale(dtype, pre, post));
  if (op != TIPS_OP_SUM && (pre != 1.0 || post != 1.0))
    return fail(TIPS_ERR_INVALID_ARG, "there is no scaled MAX / MIN (prescale %g, postscale %g)", pre, post);
  return 0;
}

tips::Scale scale_of(int op, double pre, double post) {
  tips::Scale sc;
  sc.pre = pre;
  sc.post = post;
  sc.op = op;
  return sc;
}

// rows and row_elems of a list: none negative, no tensor's or region's bytes overflow; *total = elements
int check_shapes(const int64_t* rows, const int64_t* row_elems, int n, int es, int64_t* total) {
  if (n < 0 || (n > 0 && (!rows || !row_elems))) return fail(TIPS_ERR_INVALID_ARG, "bad tensor list (n %d)", n);
  *total = 0;
  for (int i = 0; i < n; i++) {
    int64_t elems;
    if (rows[i] < 0 || row_elems[i] < 0)
      return fail(TIPS_ERR_INVALID_ARG, "negative size (tensor %d: rows %lld, row_elems %lld)", i, (long long)rows[i],
                  (long long)row_elems[i]);
    if (__builtin_mul_overflow(rows[i], row_elems[i], &elems) || __builtin_add_overflow(*total, elems, total) ||
        *total > ((int64_t)1 << 56) / es)
      return fail(TIPS_ERR_INVALID_ARG, "sizes overflow (tensor %d)", i);
  }
  return 0;
}

uint64_t bits_of(double x) {
  uint64_t u;
  memcpy(&u, &x, 8);
  return u;
}

struct Span {
  uintptr_t b, e;
};

// some output [b, e) shares a byte with some input
bool outputs_meet_inputs(std::vector<Span> ins, const std::vector<Span>& outs) {
  std::sort(ins.begin(), ins.end(), [](const Span& x, const Span& y) { return x.b < y.b; });
  std::vector<uintptr_t> reach(ins.size());  // the furthest end among the inputs up to this one
  for (size_t i = 0; i < ins.size(); i++) reach[i] = std::max(ins[i].e, i ? reach[i - 1] : 0);
  for (const Span& o : outs) {
    const size_t k = std::lower_bound(ins.begin(), ins.end(), o.e, [](const Span& x, uintptr_t v) { return x.b < v; }) - ins.begin();
    if (k > 0 && reach[k - 1] > o.b) return true;  // (the inputs that begin before the output's end)
  }
  return false;
}

// What a call brings: the list, and this rank's slices of it on p ranks
struct Call {
  const void* const* ins;
  void* const* outs;
  const int64_t *rows, *row_elems;
  int n, dtype, es;
  tips::Scale sc;
};

const char* slice_of(const Call& c, int i, int p, int q, int64_t* elems) {
  int64_t begin;
  *elems = tips::rs_rows(c.rows[i], p, q, &begin) * c.row_elems[i];
  return (const char*)c.ins[i] + begin * c.row_elems[i] * c.es;
}

// this rank's verdict on its pointers (device memory, element-aligned, no output over an input)
int check_pointers(const Call& c, int p, int rank) {
  if (!c.ins || !c.outs) return fail(TIPS_ERR_INVALID_ARG, "null pointer list");
  std::vector<Span> ins, outs;
  for (int i = 0; i < c.n; i++) {
    const int64_t bytes = c.rows[i] * c.row_elems[i] * c.es;
    if (bytes == 0) continue;
    TRY(need_device(c.ins[i], "an input", kTakes));
    const uintptr_t a = reinterpret_cast<uintptr_t>(c.ins[i]);
    if (a & (uintptr_t)(c.es - 1)) return fail(TIPS_ERR_INVALID_ARG, "input %d is not %d-B aligned", i, c.es);
    ins.push_back(Span{a, a + (uintptr_t)bytes});
    int64_t own;
    slice_of(c, i, p, rank, &own);
    if (own == 0) continue;
    TRY(need_device(c.outs[i], "an output", kTakes));
    const uintptr_t o = reinterpret_cast<uintptr_t>(c.outs[i]);
    if (o & (uintptr_t)(c.es - 1)) return fail(TIPS_ERR_INVALID_ARG, "output %d is not %d-B aligned", i, c.es);
    outs.push_back(Span{o, o + (uintptr_t)(own * c.es)});
  }
  if (outputs_meet_inputs(ins, outs)) return fail(TIPS_ERR_INVALID_ARG, "an output overlaps an input (the reduce-scatter is out of place)");
  return 0;
}

// The schedule. Caller holds st.mu and st.rscatter.mu.
int run_collective(State& st, const Call& c, hipStream_t s) {
  const int p = st.size, rank = st.rank, n = c.n;
  std::vector<int64_t> offs((size_t)n);
  std::vector<tips::FoldSeg> segs;
  auto region = [&](int q) { return tips::rs_layout(c.rows, c.row_elems, n, c.es, p, q, offs.data()); };
  const int64_t slot = round_up(region(0), kAlignBytes);  // region 0 is the largest
  const bool packed = p > 1 && n > 1;
  TRY(st.rscatter.open(s, (size_t)((packed ? 2 : 1) * (int64_t)(p - 1) * slot)));
  char* stage = (char*)st.rscatter.scratch.p;  // the peers' regions `rank`, then (packed) this rank's regions for them
  char* send = stage + (int64_t)(p - 1) * slot;
  auto slot_of = [&](char* base, int r) { return base + (int64_t)(r < rank ? r : r - 1) * slot; };
  std::vector<int64_t> bytes_of((size_t)p);
  for (int q = 0; q < p; q++) bytes_of[q] = region(q);
  if (p > 1) {
    TRY(ensure_comm(st));
    if (packed) {
      // the pack: the kernel's one-source form, the peers' send slots laid end to end as its byte space
      for (int q = 0; q < p; q++) {
        if (q == rank || bytes_of[q] == 0) continue;
        region(q);
        char* to = slot_of(send, q);
        for (int i = 0; i < n; i++) {
          int64_t elems;
          const char* from = slice_of(c, i, p, q, &elems);
          if (elems > 0) segs.push_back(tips::FoldSeg{from, to + offs[i], (int64_t)(to - send) + offs[i], elems});
        }
      }
      HIP_TRY(tips::launch_fold_segs(segs.data(), (int)segs.size(), nullptr, 1, 0, c.dtype, tips::Scale(), s));
      segs.clear();
    }
    TRY(rccl_enter(st, s));
    NCCL_TRY(ncclGroupStart());
    for (int q = 0; q < p; q++) {
      if (q == rank) continue;
      if (bytes_of[q] > 0) {
        int64_t elems;
        const void* from = packed ? slot_of(send, q) : slice_of(c, 0, p, q, &elems);
        NCCL_TRY(ncclSend(from, (size_t)bytes_of[q], ncclInt8, q, st.comm, s));
      }
      if (bytes_of[rank] > 0) NCCL_TRY(ncclRecv(slot_of(stage, q), (size_t)bytes_of[rank], ncclInt8, q, st.comm, s));
    }
    NCCL_TRY(ncclGroupEnd());
    TRY(rccl_leave(st, s));
  }
  if (bytes_of[rank] > 0) {
    region(rank);
    for (int i = 0; i < n; i++) {
      int64_t elems;
      const char* own = slice_of(c, i, p, rank, &elems);
      if (elems > 0) segs.push_back(tips::FoldSeg{own, c.outs[i], offs[i], elems});
    }
    const void* stages[tips::kMaxSrcs] = {};
    for (int r = 0; r < p; r++)
      if (r != rank) stages[r] = slot_of(stage, r);
    HIP_TRY(tips::launch_fold_segs(segs.data(), (int)segs.size(), stages, p, rank, c.dtype, c.sc, s));
  }
  return st.rscatter.close(s);
}

// What a collective entry brings beside its Call. Every rank's record is eight words: the tensor
// count (-1 where the list cannot be read), the element count, the shape hash, `words` and, last,
// the rank's verdict. A call of one kind paired with a call of the other on another rank is a
// mismatch on both sides: `kind` is folded into the shape hash.
struct Entry {
  const char *what, *noun;  // "tips_reducescatter", "reduce-scatter"
  uint64_t kind;            // 0: the plain calls, their record as it always was; 0xF8: the MXFP8 calls
  int64_t words[4];         // the record's words 3 ... 6
  int (*mismatch)(int r, const int64_t* q, const int64_t* q0);  // fail(TIPS_ERR_MISMATCH, ...) on rank r's record and rank 0's
};

// The path every collective entry takes. `own`: the verdict of the entry's own checks on its scalar
// arguments; run(st) is its schedule, called under st.mu and st.rscatter.mu.
template <class Run>
int enter(const Entry& e, const Call& c, int own, hipStream_t s, Run run) {
  // What needs no device comes first; once the call is open it is part of this rank's verdict, so
  // that a rank which refuses its arguments does not leave the others waiting in the exchange.
  const int n = c.n;
  int64_t total = 0;
  if (own == 0) own = check_shapes(c.rows, c.row_elems, n, c.es, &total);
  if (own == 0 && n > 0 && (!c.ins || !c.outs)) own = fail(TIPS_ERR_INVALID_ARG, "null pointer list");
  const bool usable = own == 0;  // the list can be read
  const std::string early = own ? last_error() : std::string();
  State& st = S();
  std::unique_lock<std::mutex> one;
  int size;
  if (const int rc = side_open(st, st.rscatter, e.what, e.noun, at_most_max_srcs, /*rccl_only=*/true, &one, &size))
    return own ? fail(own, "%s", early.c_str()) : rc;
  if (own) (void)fail(own, "%s", early.c_str());
  else own = refuse_capture(e.what, s);
  if (own == 0) {
    int rank;
    {
      std::lock_guard<std::mutex> lk(st.mu);
      rank = st.rank;
    }
    own = check_pointers(c, size, rank);
  }
  uint64_t h = kFnvBasis;
  if (usable) {
    std::vector<int64_t> shape((size_t)2 * n);
    for (int i = 0; i < n; i++) shape[2 * i] = c.rows[i], shape[2 * i + 1] = c.row_elems[i];
    h = hash_counts(shape.data(), 2 * n);
  }
  if (e.kind) h = (h ^ e.kind) * kFnvPrime;
  const int64_t mine[8] = {usable ? n : -1, total, (int64_t)h, e.words[0], e.words[1], e.words[2], e.words[3], own};
  SideRecords rec;
  TRY(side_exchange(size, mine, 8, &rec));
  // reported in this order: a mismatch, another rank's refusal, this rank's own
  if (const int r = rec.first_differing(0, 7); r >= 0) return e.mismatch(r, rec.of(r), rec.of(0));
  if (!own) TRY(rec.report_refusing(e.noun));
  TRY(rec.report_own());
  if (total == 0) return 0;
  std::lock_guard<std::mutex> lk(st.mu);
  if (!st.initialized) return fail(TIPS_ERR_NOT_INITIALIZED, "tips_init has not been called");
  TRY(set_device(st));
  return run(st);
}

int mismatch(int r, const int64_t* q, const int64_t* q0) {
  return fail(TIPS_ERR_MISMATCH,
              "Mismatched reduce-scatter: rank %d has %lld tensors, %lld elements, shape hash %llx, dtype %lld, op %lld, "
              "factor bits %llx / %llx; rank 0 has %lld tensors, %lld elements, shape hash %llx, dtype %lld, op %lld, "
              "factor bits %llx / %llx",
              r, (long long)q[0], (long long)q[1], (unsigned long long)q[2], (long long)q[3], (long long)q[4],
              (unsigned long long)q[5], (unsigned long long)q[6], (long long)q0[0], (long long)q0[1],
              (unsigned long long)q0[2], (long long)q0[3], (long long)q0[4], (unsigned long long)q0[5],
              (unsigned long long)q0[6]);
}

int collective(const char* what, const void* const* ins, void* const* outs, const int64_t* rows, const int64_t* row_elems,
               int n, int dtype, int op, double pre, double post, hipStream_t s) {
  const Call c{ins, outs, rows, row_elems, n, dtype, tips::dtype_size(dtype), scale_of(op, pre, post)};
  const Entry e{what, "reduce-scatter", 0, {dtype, op, (int64_t)bits_of(pre), (int64_t)bits_of(post)}, mismatch};
  return enter(e, c, check_op(dtype, op, pre, post), s, [&](State& st) { return run_collective(st, c, s); });
}

// ---- the MXFP8 reduce-scatter ----

uint32_t float_bits_of(double x) {
  const float f = (float)x;
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

// A count list as the MXFP8 wire sees it: the tensors' element counts, their flat element offsets
// under tips_fused_layout(counts, n, FLOAT32) and the flat element count E (all 0 for an empty list)
struct MxRegion {
  std::vector<int64_t> counts, offs;
  int64_t elems = 0;
};

MxRegion mx_region_of(std::vector<int64_t> counts) {
  MxRegion r;
  r.counts = std::move(counts);
  r.offs.assign(r.counts.size(), 0);
  int64_t total = 0;
  for (const int64_t c : r.counts) total += c;
  if (total > 0) {
    r.elems = fused_layout(r.counts.data(), (int)r.counts.size(), TIPS_FLOAT32, r.offs.data()) / 4;
    for (int64_t& o : r.offs) o /= 4;
  }
  return r;
}

// region q of a list: its slices' counts
MxRegion mx_region(const int64_t* rows, const int64_t* row_elems, int n, int p, int q) {
  std::vector<int64_t> counts((size_t)n);
  for (int i = 0; i < n; i++) counts[i] = tips::rs_rows(rows[i], p, q, nullptr) * row_elems[i];
  return mx_region_of(std::move(counts));
}

// the order the kernels want: ascending flat offset (the layout puts a tensor of at least the fusion
// threshold behind the others, whatever its place in the list)
std::vector<int> by_offset(const MxRegion& r) {
  std::vector<int> idx;
  for (int i = 0; i < (int)r.counts.size(); i++)
    if (r.counts[i] > 0) idx.push_back(i);
  std::sort(idx.begin(), idx.end(), [&](int a, int b) { return r.offs[a] < r.offs[b]; });
  return idx;
}

tips::MxSrcs wires_of(const void* const* wires, int nsrc, int own_pos, int64_t elems) {
  tips::MxSrcs w = {};
  for (int j = 0; j < nsrc; j++)
    if (j != own_pos) {
      w.payload[j] = (const unsigned char*)wires[j];
      w.scales[j] = w.payload[j] + tips::mxfp8_scales_offset(elems);
    }
  return w;
}

// The schedule. Caller holds st.mu and st.rscatter.mu.
int run_mx_collective(State& st, const Call& c, double factor, hipStream_t s) {
  const int p = st.size, rank = st.rank, n = c.n;
  std::vector<MxRegion> reg;
  for (int q = 0; q < p; q++) reg.push_back(mx_region(c.rows, c.row_elems, n, p, q));
  const MxRegion& mine = reg[rank];
  // The send buffer is one wire buffer over the peers' regions laid end to end, each from a multiple
  // of 256 flat elements: region q's payload and scale bytes are then exactly its own wire buffer's,
  // at payload byte base[q] and scale byte base[q] / 32, and one quantise (a launch per 48 slices) fills it.
  std::vector<int64_t> base((size_t)p, 0);
  int64_t send_elems = 0;
  for (int q = 0; q < p; q++)
    if (q != rank) base[q] = send_elems, send_elems += tips::mxfp8_scales_offset(reg[q].elems);
  const int64_t send_bytes = send_elems ? tips::mxfp8_wire_bytes(send_elems) : 0;
  const int64_t slot = p > 1 ? tips::mxfp8_wire_bytes(mine.elems) : 0;  // a peer's region `rank`: a whole wire buffer
  TRY(st.rscatter.open(s, (size_t)(send_bytes + (int64_t)(p - 1) * slot)));
  unsigned char* send = (unsigned char*)st.rscatter.scratch.p;
  unsigned char* stage = send + send_bytes;
  auto slot_of = [&](int r) { return stage + (int64_t)(r < rank ? r : r - 1) * slot; };
  if (p > 1) {
    TRY(ensure_comm(st));
    if (send_elems > 0) {
      std::vector<tips::MxSeg> segs;
      for (int q = 0; q < p; q++) {
        if (q == rank) continue;
        for (int i : by_offset(reg[q])) {
          int64_t elems;
          const char* from = slice_of(c, i, p, q, &elems);
          segs.push_back(tips::MxSeg{from, base[q] + reg[q].offs[i], elems, 0});
        }
      }
      tips::mxfp8_cover(segs, send_elems);
      HIP_TRY(tips::launch_mxfp8_quantize(segs.data(), (int)segs.size(), send, send + send_elems, nullptr,
                                          send_elems / tips::kMxBlock, send_bytes - send_elems, s));
    }
    const int64_t in_blocks = tips::mxfp8_blocks(mine.elems);
    TRY(rccl_enter(st, s));
    NCCL_TRY(ncclGroupStart());
    for (int q = 0; q < p; q++) {
      if (q == rank) continue;
      if (const int64_t b = tips::mxfp8_blocks(reg[q].elems); b > 0) {
        NCCL_TRY(ncclSend(send + base[q], (size_t)(b * tips::kMxBlock), ncclInt8, q, st.comm, s));
        NCCL_TRY(ncclSend(send + send_elems + base[q] / tips::kMxBlock, (size_t)b, ncclInt8, q, st.comm, s));
      }
      if (in_blocks > 0) {
        NCCL_TRY(ncclRecv(slot_of(q), (size_t)(in_blocks * tips::kMxBlock), ncclInt8, q, st.comm, s));
        NCCL_TRY(ncclRecv(slot_of(q) + tips::mxfp8_scales_offset(mine.elems), (size_t)in_blocks, ncclInt8, q, st.comm, s));
      }
    }
    NCCL_TRY(ncclGroupEnd());
    TRY(rccl_leave(st, s));
  }
  if (mine.elems > 0) {
    std::vector<tips::MxFoldSeg> segs;
    for (int i : by_offset(mine)) {
      int64_t elems;
      const char* own = slice_of(c, i, p, rank, &elems);
      segs.push_back(tips::MxFoldSeg{own, c.outs[i], mine.offs[i], elems});
    }
    const void* slots[tips::kMxMaxSrcs] = {};
    for (int r = 0; r < p; r++)
      if (r != rank) slots[r] = slot_of(r);
    HIP_TRY(tips::launch_mxfp8_fold_segs(segs.data(), (int)segs.size(), wires_of(slots, p, rank, mine.elems), p, rank,
                                         (float)factor, s));
  }
  return st.rscatter.close(s);
}

int mx_mismatch(int r, const int64_t* q, const int64_t* q0) {
  return fail(TIPS_ERR_MISMATCH,
              "Mismatched MXFP8 reduce-scatter: rank %d has %lld tensors, %lld elements, call and shape hash %llx, factor bits "
              "%llx; rank 0 has %lld tensors, %lld elements, call and shape hash %llx, factor bits %llx",
              r, (long long)q[0], (long long)q[1], (unsigned long long)q[2], (unsigned long long)q[5], (long long)q0[0],
              (long long)q0[1], (unsigned long long)q0[2], (unsigned long long)q0[5]);
}

int mx_collective(const char* what, const void* const* ins, void* const* outs, const int64_t* rows, const int64_t* row_elems,
                  int n, double factor, hipStream_t s) {
  const Call c{ins, outs, rows, row_elems, n, TIPS_FLOAT32, 4, tips::Scale()};
  // the plain record's words with the factor's float bits where the prescale's stand
  const Entry e{what, "MXFP8 reduce-scatter", 0xF8, {TIPS_FLOAT32, TIPS_OP_SUM, (int64_t)float_bits_of(factor), 0}, mx_mismatch};
  return enter(e, c, check_factor(factor), s, [&](State& st) { return run_mx_collective(st, c, factor, s); });
}

}  // namespace

extern "C" {

int64_t tips_reducescatter_rows(int64_t rows, int nranks, int rank, int64_t* begin) {
  if (rows < 0 || nranks < 1 || rank < 0 || rank >= nranks)
    return fail(TIPS_ERR_INVALID_ARG, "bad split (rows %lld, rank %d of %d)", (long long)rows, rank, nranks);
  return tips::rs_rows(rows, nranks, rank, begin);
}

int64_t tips_reducescatter_layout(const int64_t* rows, const int64_t* row_elems, int n, int dtype, int nranks, int rank,
                                  int64_t* offsets) {
  TRY(check_dtype(dtype));
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(TIPS_ERR_INVALID_ARG, "bad rank (%d of %d)", rank, nranks);
  int64_t total;
  TRY(check_shapes(rows, row_elems, n, tips::dtype_size(dtype), &total));
  return tips::rs_layout(rows, row_elems, n, tips::dtype_size(dtype), nranks, rank, offsets);
}

int tips_reducescatter_fold(void* const* outs, const void* const* own, const int64_t* counts, const int64_t* offsets, int n,
                            const void* const* stages, int nsrc, int own_pos, int dtype, int op, double prescale,
                            double postscale, void* stream) {
  TRY(check_op(dtype, op, prescale, postscale));
  if (nsrc < 1 || nsrc > tips::kMaxSrcs) return fail(TIPS_ERR_INVALID_ARG, "nsrc must be 1 ... %d (got %d)", tips::kMaxSrcs, nsrc);
  if (own_pos < 0 || own_pos >= nsrc) return fail(TIPS_ERR_INVALID_ARG, "own_pos %d is outside 0 ... %d", own_pos, nsrc - 1);
  int64_t total;
  TRY(check_counts(counts, n, "segment", &total));
  if (n > 0 && (!outs || !own || !offsets)) return fail(TIPS_ERR_INVALID_ARG, "null pointer list");
  if (nsrc > 1 && !stages) return fail(TIPS_ERR_INVALID_ARG, "null pointer (stages)");
  const int64_t es = tips::dtype_size(dtype);
  std::vector<tips::FoldSeg> segs;
  int64_t end = 0;  // the region byte behind the last non-empty segment
  for (int i = 0; i < n; i++) {
    if (counts[i] == 0) continue;
    if (offsets[i] < 0 || offsets[i] % kAlignBytes != 0)
      return fail(TIPS_ERR_INVALID_ARG, "offset %lld of segment %d is not a multiple of %lld", (long long)offsets[i], i,
                  (long long)kAlignBytes);
    if (offsets[i] < end) return fail(TIPS_ERR_INVALID_ARG, "segment %d begins inside an earlier one (offsets ascend)", i);
    if (!outs[i] || !own[i]) return fail(TIPS_ERR_INVALID_ARG, "null pointer (segment %d)", i);
    if ((reinterpret_cast<uintptr_t>(outs[i]) | reinterpret_cast<uintptr_t>(own[i])) & (uintptr_t)(es - 1))
      return fail(TIPS_ERR_INVALID_ARG, "segment %d is not %lld-B aligned", i, (long long)es);
    end = offsets[i] + counts[i] * es;
    segs.push_back(tips::FoldSeg{own[i], outs[i], offsets[i], counts[i]});
  }
  if (segs.empty()) return 0;
  for (int j = 0; j < nsrc; j++)
    if (j != own_pos) {
      if (!stages[j]) return fail(TIPS_ERR_INVALID_ARG, "null pointer (stage %d)", j);
      if (reinterpret_cast<uintptr_t>(stages[j]) & 15) return fail(TIPS_ERR_INVALID_ARG, "stage %d is not 16-B aligned", j);
    }
  // (like tips_multi_sum, the kernel's own entry does not probe its pointers: two lookups per segment
  // cost a 214-segment call more than its launches)
  HIP_TRY(tips::launch_fold_segs(segs.data(), (int)segs.size(), stages, nsrc, own_pos, dtype, scale_of(op, prescale, postscale),
                                 (hipStream_t)stream));
  return 0;
}

int tips_reducescatter(const void* in, void* out, int64_t rows, int64_t row_elems, int dtype, int op, double prescale,
                       double postscale, void* stream) {
  return collective("tips_reducescatter", &in, &out, &rows, &row_elems, 1, dtype, op, prescale, postscale, (hipStream_t)stream);
}

int tips_grouped_reducescatter(const void* const* ins, void* const* outs, const int64_t* rows, const int64_t* row_elems, int n,
                               int dtype, int op, double prescale, double postscale, void* stream) {
  return collective("tips_grouped_reducescatter", ins, outs, rows, row_elems, n, dtype, op, prescale, postscale,
                    (hipStream_t)stream);
}

int64_t tips_reducescatter_mxfp8_layout(const int64_t* rows, const int64_t* row_elems, int n, int nranks, int rank,
                                        int64_t* offsets) {
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(TIPS_ERR_INVALID_ARG, "bad rank (%d of %d)", rank, nranks);
  int64_t total;
  TRY(check_shapes(rows, row_elems, n, 4, &total));
  const MxRegion r = mx_region(rows, row_elems, n, nranks, rank);
  if (offsets) std::copy(r.offs.begin(), r.offs.end(), offsets);
  return r.elems;
}

int tips_reducescatter_mxfp8_fold(void* const* outs, const void* const* own, const int64_t* counts, int n,
                                  const void* const* wires, int nsrc, int own_pos, double factor, void* stream) {
  TRY(check_factor(factor));
  if (nsrc < 1 || nsrc > tips::kMxMaxSrcs) return fail(TIPS_ERR_INVALID_ARG, "nsrc must be 1 ... %d (got %d)", tips::kMxMaxSrcs, nsrc);
  if (own_pos < 0 || own_pos >= nsrc) return fail(TIPS_ERR_INVALID_ARG, "own_pos %d is outside 0 ... %d", own_pos, nsrc - 1);
  int64_t total;
  TRY(check_counts(counts, n, "tensor", &total));
  if (n > 0 && (!outs || !own)) return fail(TIPS_ERR_INVALID_ARG, "null pointer list");
  if (nsrc > 1 && !wires) return fail(TIPS_ERR_INVALID_ARG, "null pointer (wires)");
  for (int i = 0; i < n; i++) {
    if (counts[i] == 0) continue;
    if (!outs[i] || !own[i]) return fail(TIPS_ERR_INVALID_ARG, "null pointer (tensor %d)", i);
    if ((reinterpret_cast<uintptr_t>(outs[i]) | reinterpret_cast<uintptr_t>(own[i])) & 3)
      return fail(TIPS_ERR_INVALID_ARG, "tensor %d is not 4-B aligned", i);
  }
  if (total == 0) return 0;
  for (int j = 0; j < nsrc; j++)
    if (j != own_pos) {
      if (!wires[j]) return fail(TIPS_ERR_INVALID_ARG, "null pointer (wire %d)", j);
      if (reinterpret_cast<uintptr_t>(wires[j]) & 15) return fail(TIPS_ERR_INVALID_ARG, "wire %d is not 16-B aligned", j);
    }
  const MxRegion r = mx_region_of(std::vector<int64_t>(counts, counts + n));
  std::vector<tips::MxFoldSeg> segs;
  for (int i : by_offset(r)) segs.push_back(tips::MxFoldSeg{own[i], outs[i], r.offs[i], counts[i]});
  // (like tips_reducescatter_fold, the kernel's own entry does not probe its pointers)
  HIP_TRY(tips::launch_mxfp8_fold_segs(segs.data(), (int)segs.size(), wires_of(wires, nsrc, own_pos, r.elems), nsrc, own_pos,
                                       (float)factor, (hipStream_t)stream));
  return 0;
}

int tips_reducescatter_mxfp8(const void* in, void* out, int64_t rows, int64_t row_elems, double factor, void* stream) {
  return mx_collective("tips_reducescatter_mxfp8", &in, &out, &rows, &row_elems, 1, factor, (hipStream_t)stream);
}

int tips_grouped_reducescatter_mxfp8(const void* const* ins, void* const* outs, const int64_t* rows, const int64_t* row_elems,
                                     int n, double factor, void* stream) {
  return mx_collective("tips_grouped_reducescatter_mxfp8", ins, outs, rows, row_elems, n, factor, (hipStream_t)stream);
}

}  // extern "C"
