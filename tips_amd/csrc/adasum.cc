// adasum.cc — the Adasum entry points of the C-ABI: tips_adasum_pair, the local
// operation out = ca a + cb b per segment (adasum.hip), and the two collectives around it -
// tips_allreduce_adasum (one segment) and tips_fused_allreduce_adasum_flat (one segment per tensor of
// a list, over the fused flat layout) - which fold the ranks' values by recursive doubling: at level k
// rank r exchanges its whole buffer with rank r XOR 2^k and both compute the same pair. The op the
// reference's allreduce names and never calls ("# TODO: Need to fix this to actuall call Adasum",
// tips/tensorflow/__init__.py:62).
#include <algorithm>
#include <string>
#include <vector>

#include "adasum.h"
#include "rt.h"

using namespace tips::rt;

namespace {

bool float_dtype(int dtype) {
  return dtype == TIPS_FLOAT32 || dtype == TIPS_FLOAT64 || dtype == TIPS_FLOAT16 || dtype == TIPS_BFLOAT16;
}

int check_float(int dtype, const char* what) {
  TRY(check_dtype(dtype));
  if (!float_dtype(dtype))
    return fail(TIPS_ERR_UNSUPPORTED, "%s is defined for float dtypes only (dtype %d)", what, dtype);
  return 0;
}

int need_device(const void* p, const char* what) {
  if (!p) return fail(TIPS_ERR_INVALID_ARG, "null pointer (%s)", what);
  if (!is_device_ptr(p))
    return fail(TIPS_ERR_UNSUPPORTED, "%s is host memory: Adasum takes device pointers only (nothing is staged)", what);
  return 0;
}

// ---------------------------------------------------------------------------
// Segment tables: {offset, count, first chunk} per segment, uploaded once per layout (device, chunk
// size, offsets, counts) and kept - like the fusion tables, a training step brings the same list
// every time. A single segment travels by value and needs no table.

struct SegLayout {
  int device = -1;
  int64_t chunk = 0;
  std::vector<int64_t> offs, counts;
  tips::AdaSeg* dev = nullptr;
  uint64_t stamp = 0;
};
constexpr size_t kMaxSegLayouts = 32;
std::mutex g_seg_mu;
std::vector<SegLayout> g_seg_layouts;
uint64_t g_seg_clock = 0;

// offs[i] / counts[i]: segment i's first element and length (offs == nullptr: back to back from 0)
int find_segs(const int64_t* offs, const int64_t* counts, int nseg, int dtype, tips::AdaSegs* out, int64_t* nchunks) {
  const int64_t K = tips::adasum_chunk_elems(dtype);
  std::vector<int64_t> o((size_t)nseg);
  int64_t run = 0, chunks = 0;
  for (int i = 0; i < nseg; i++) {
    o[i] = offs ? offs[i] : run;
    run += counts[i];
    chunks += tips::adasum_chunks(counts[i], K);
  }
  *nchunks = chunks;
  if (nseg == 1) {
    *out = tips::AdaSegs{nullptr, 1, tips::AdaSeg{o[0], counts[0], 0}};
    return 0;
  }
  int device = -1;
  HIP_TRY(hipGetDevice(&device));
  std::lock_guard<std::mutex> lk(g_seg_mu);
  for (SegLayout& L : g_seg_layouts)
    if (L.device == device && L.chunk == K && (int)L.counts.size() == nseg && L.offs == o &&
        std::equal(counts, counts + nseg, L.counts.begin())) {
      L.stamp = ++g_seg_clock;
      *out = tips::AdaSegs{L.dev, nseg, tips::AdaSeg{0, 0, 0}};
      return 0;
    }
  if (g_seg_layouts.size() >= kMaxSegLayouts) {  // the least recently used one goes (hipFree waits for the device)
    auto old = std::min_element(g_seg_layouts.begin(), g_seg_layouts.end(),
                                [](const SegLayout& x, const SegLayout& y) { return x.stamp < y.stamp; });
    (void)hipFree(old->dev);
    g_seg_layouts.erase(old);
  }
  std::vector<tips::AdaSeg> host((size_t)nseg);
  int64_t c0 = 0;
  for (int i = 0; i < nseg; i++) {
    host[i] = tips::AdaSeg{o[i], counts[i], c0};
    c0 += tips::adasum_chunks(counts[i], K);
  }
  SegLayout L;
  L.device = device;
  L.chunk = K;
  L.offs = std::move(o);
  L.counts.assign(counts, counts + nseg);
  L.stamp = ++g_seg_clock;
  HIP_TRY(hipMalloc((void**)&L.dev, sizeof(tips::AdaSeg) * (size_t)nseg));
  if (hipError_t e = hipMemcpy(L.dev, host.data(), sizeof(tips::AdaSeg) * (size_t)nseg, hipMemcpyHostToDevice);
      e != hipSuccess) {
    (void)hipFree(L.dev);
    return fail(TIPS_ERR_HIP, "segment table upload failed: %s", hipGetErrorString(e));
  }
  *out = tips::AdaSegs{L.dev, nseg, tips::AdaSeg{0, 0, 0}};
  g_seg_layouts.push_back(std::move(L));
  return 0;
}

// the counts of a list: none negative, the total in *total
int check_counts(const int64_t* counts, int n, int64_t* total) {
  if (n < 0 || (n > 0 && !counts)) return fail(TIPS_ERR_INVALID_ARG, "bad segment list (n %d)", n);
  *total = 0;
  for (int i = 0; i < n; i++) {
    if (counts[i] < 0) return fail(TIPS_ERR_INVALID_ARG, "negative count (segment %d: %lld)", i, (long long)counts[i]);
    if (__builtin_add_overflow(*total, counts[i], total) || *total > ((int64_t)1 << 56))
      return fail(TIPS_ERR_INVALID_ARG, "sizes overflow (segment %d)", i);
  }
  return 0;
}

uint64_t hash_counts(const int64_t* counts, int n) {  // FNV-1a over the counts' bytes
  uint64_t h = 1469598103934665603ull;
  for (int i = 0; i < n; i++)
    for (int k = 0; k < 8; k++) h = (h ^ (((uint64_t)counts[i] >> (8 * k)) & 0xff)) * 1099511628211ull;
  return h;
}

const char kBusy[] =
    "%s does not go through a running negotiation (named Adasum requests are not implemented): call it before the "
    "first named request or after tips_shutdown / tips_init";

// What both collectives check before any device exchange: the lifecycle, the rank count, the
// algorithm, and that every rank brings the same list and accepts its own pointers (`own`: this
// rank's verdict, which travels with the record so that no rank is left waiting in the exchange).
int agree(State& st, const char* what, int n, int64_t total, int dtype, const int64_t* counts, int own, int* size) {
  const std::string own_msg = own ? last_error() : std::string();
  {
    std::lock_guard<std::mutex> lk(st.mu);
    if (!st.initialized) return fail(TIPS_ERR_NOT_INITIALIZED, "tips_init has not been called");
    TRY(set_device(st));
    *size = st.size;
    if ((st.size & (st.size - 1)) != 0)
      return fail(TIPS_ERR_UNSUPPORTED, "%s needs a power-of-two number of ranks (recursive doubling), not %d", what, st.size);
    if (st.size > 1 && resolve_algo(st.algo, st.size, 0) == TIPS_ALGO_PEER)
      return fail(TIPS_ERR_UNSUPPORTED, "%s has one schedule, over RCCL send / recv: not available under TIPS_ALGO_PEER", what);
  }
  if (*size > 1) {
    const int64_t mine[5] = {n, total, dtype, (int64_t)hash_counts(counts, n), own};
    std::vector<int64_t> all((size_t)5 * *size);
    TRY(tips_allgather_i64(mine, 5, all.data()));
    for (int r = 0; r < *size; r++) {
      const int64_t* q = &all[(size_t)5 * r];
      if (q[0] != all[0] || q[1] != all[1] || q[2] != all[2] || q[3] != all[3])
        return fail(TIPS_ERR_MISMATCH,
                    "Mismatched Adasum allreduce: rank %d has %lld tensors, %lld elements, dtype %lld, count hash %llx; rank "
                    "0 has %lld tensors, %lld elements, dtype %lld, count hash %llx",
                    r, (long long)q[0], (long long)q[1], (long long)q[2], (unsigned long long)q[3], (long long)all[0],
                    (long long)all[1], (long long)all[2], (unsigned long long)all[3]);
    }
    for (int r = 0; r < *size; r++)
      if (all[(size_t)5 * r + 4] != 0 && !own)
        return fail(TIPS_ERR_MISMATCH, "Adasum allreduce: rank %d refused its arguments (status %lld)", r,
                    (long long)all[(size_t)5 * r + 4]);
  }
  if (own) return fail(own, "%s", own_msg.c_str());
  return 0;
}

// The levels. `buf` holds this rank's value in its first span_bytes (segments at offs / counts,
// elements) and receives the result; `first` is what level 0 reads as this rank's value (the input
// of an out-of-place call, or buf). Caller holds st.mu and st.adasum_mu; size a power of two > 1.
int run_levels(State& st, const void* first, void* buf, int64_t span_bytes, const int64_t* offs, const int64_t* counts,
               int nseg, int64_t total, int dtype, hipStream_t s) {
  tips::AdaSegs segs;
  int64_t nchunks;
  TRY(find_segs(offs, counts, nseg, dtype, &segs, &nchunks));
  const int64_t recv_bytes = round_up(span_bytes, kAlignBytes);
  TRY(st.adasum_scratch.ensure((size_t)(recv_bytes + tips::adasum_workspace_bytes(total, nseg))));
  char* recv = (char*)st.adasum_scratch.p;
  void* ws = recv + recv_bytes;
  if (!st.ev_adasum) HIP_TRY(hipEventCreateWithFlags(&st.ev_adasum, hipEventDisableTiming));
  if (st.adasum_chain_valid) HIP_TRY(hipStreamWaitEvent(s, st.ev_adasum, 0));
  TRY(ensure_comm(st));
  const void* mine = first;
  for (int bit = 1; bit < st.size; bit <<= 1) {
    const int partner = st.rank ^ bit;
    TRY(rccl_enter(st, s));
    NCCL_TRY(ncclGroupStart());
    NCCL_TRY(ncclSend(mine, (size_t)span_bytes, ncclInt8, partner, st.comm, s));
    NCCL_TRY(ncclRecv(recv, (size_t)span_bytes, ncclInt8, partner, st.comm, s));
    NCCL_TRY(ncclGroupEnd());
    TRY(rccl_leave(st, s));
    // a = the value of the partner whose bit is clear, b = the other's: the same call on both
    const bool low = (st.rank & bit) == 0;
    HIP_TRY(tips::launch_adasum_pair(buf, low ? mine : recv, low ? recv : mine, segs, nchunks, dtype, ws, s));
    mine = buf;
  }
  HIP_TRY(hipEventRecord(st.ev_adasum, s));
  st.adasum_chain_valid = true;
  return 0;
}

}  // namespace

namespace tips {
namespace rt {

void adasum_release(State& st) {
  st.adasum_scratch.release();
  if (st.ev_adasum) {
    (void)hipEventDestroy(st.ev_adasum);
    st.ev_adasum = nullptr;
  }
  st.adasum_chain_valid = false;
  std::lock_guard<std::mutex> lk(g_seg_mu);
  for (SegLayout& L : g_seg_layouts) (void)hipFree(L.dev);
  g_seg_layouts.clear();
}

}  // namespace rt
}  // namespace tips

extern "C" {

int64_t tips_adasum_workspace(int64_t count, int nseg) {
  if (count < 0 || nseg < 0 || count > ((int64_t)1 << 56))
    return fail(TIPS_ERR_INVALID_ARG, "bad sizes (count %lld, nseg %d)", (long long)count, nseg);
  return tips::adasum_workspace_bytes(count, nseg);
}

int tips_adasum_pair(void* dst, const void* a, const void* b, const int64_t* seg_counts, int nseg, int dtype,
                     void* workspace, int64_t workspace_bytes, void* stream) {
  TRY(check_float(dtype, "tips_adasum_pair"));
  int64_t total;
  TRY(check_counts(seg_counts, nseg, &total));
  if (workspace_bytes < 0) return fail(TIPS_ERR_INVALID_ARG, "negative workspace size");
  if (total == 0) return 0;
  const int64_t need = tips::adasum_workspace_bytes(total, nseg);
  if (workspace_bytes < need)
    return fail(TIPS_ERR_INVALID_ARG, "workspace of %lld B is too small: %lld elements in %d segments need %lld B",
                (long long)workspace_bytes, (long long)total, nseg, (long long)need);
  TRY(need_device(dst, "dst"));
  TRY(need_device(a, "a"));
  TRY(need_device(b, "b"));
  TRY(need_device(workspace, "workspace"));
  if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return fail(TIPS_ERR_INVALID_ARG, "workspace must be 8-B aligned");
  tips::AdaSegs segs;
  int64_t nchunks;
  TRY(find_segs(nullptr, seg_counts, nseg, dtype, &segs, &nchunks));
  HIP_TRY(tips::launch_adasum_pair(dst, a, b, segs, nchunks, dtype, workspace, (hipStream_t)stream));
  return 0;
}

int tips_allreduce_adasum(const void* in, void* out, int64_t count, int dtype, void* stream) {
  TRY(check_float(dtype, "tips_allreduce_adasum"));
  if (count < 0) return fail(TIPS_ERR_INVALID_ARG, "negative count");
  if (on_negotiation_thread() || negotiation_running()) return fail(TIPS_ERR_UNSUPPORTED, kBusy, "tips_allreduce_adasum");
  State& st = S();
  std::lock_guard<std::mutex> one(st.adasum_mu);
  int own = 0;
  if (count > 0) {
    own = need_device(in, "in");
    if (own == 0) own = need_device(out, "out");
  }
  int size;
  TRY(agree(st, "tips_allreduce_adasum", 1, count, dtype, &count, own, &size));
  if (count == 0) return 0;
  const int64_t bytes = count * tips::dtype_size(dtype);
  hipStream_t s = (hipStream_t)stream;
  std::lock_guard<std::mutex> lk(st.mu);
  if (!st.initialized) return fail(TIPS_ERR_NOT_INITIALIZED, "tips_init has not been called");
  if (size == 1) {  // one rank: the copy
    HIP_TRY(tips::launch_copy_buf(out, in, bytes, s));
    return 0;
  }
  return run_levels(st, in, out, bytes, nullptr, &count, 1, count, dtype, s);
}

int tips_fused_allreduce_adasum_flat(const void* const* ins, const int64_t* counts, int n, int dtype, void* flat,
                                     void* stream) {
  TRY(check_float(dtype, "tips_fused_allreduce_adasum_flat"));
  int64_t total;
  TRY(check_counts(counts, n, &total));
  if (n > 0 && !ins) return fail(TIPS_ERR_INVALID_ARG, "bad tensor list");
  if (on_negotiation_thread() || negotiation_running())
    return fail(TIPS_ERR_UNSUPPORTED, kBusy, "tips_fused_allreduce_adasum_flat");
  State& st = S();
  std::lock_guard<std::mutex> one(st.adasum_mu);
  int own = 0;
  if (total > 0) own = need_device(flat, "flat");
  for (int i = 0; i < n && own == 0; i++)
    if (counts[i] > 0) own = need_device(ins[i], "a tensor of the list");
  int size;
  TRY(agree(st, "tips_fused_allreduce_adasum_flat", n, total, dtype, counts, own, &size));
  if (total == 0) return 0;
  return list_collective(ins, counts, n, dtype, dtype, kOutsFlat, nullptr, flat, /*route=*/false,
                         [&](State& st2, std::vector<BatchItem>& items) -> int {
                           for (auto& it : items) it.out = it.count ? flat : nullptr;
                           hipStream_t s = (hipStream_t)stream;
                           TRY(fused_pack_flat(st2, items.data(), n, dtype, flat, s));
                           if (size == 1) return 0;  // one rank: the packed copy
                           // one segment per tensor at its layout offset: the padding between them is
                           // exchanged with the buffer and never read by a kernel
                           const int64_t es = tips::dtype_size(dtype);
                           std::vector<int64_t> offs((size_t)n);
                           const int64_t span = fused_layout(counts, n, dtype, offs.data());
                           for (auto& o : offs) o /= es;
                           return run_levels(st2, flat, flat, span, offs.data(), counts, n, total, dtype, s);
                         });
}

}  // extern "C"
