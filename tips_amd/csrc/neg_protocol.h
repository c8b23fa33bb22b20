// neg_protocol.h — the negotiation's protocol core: the wire records, rank 0's table and decision,
// the response cache and the linger's expected set. Pure data in, bytes out: no HIP, socket or
// thread (negotiate.cc has those), so it is driven on its own by tests/c/neg_protocol_check.cc.
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/tips_hip.h"
#include "err.h"

namespace tips {
namespace rt {

// ---- wire format: flat little-endian records ----------------------------------
struct Writer {
  std::string b;
  template <class T>
  void put(T v) {
    b.append(reinterpret_cast<const char*>(&v), sizeof v);
  }
  void str(const std::string& s) {
    put<uint32_t>((uint32_t)s.size());
    b += s;
  }
};

struct Reader {
  const std::string& b;
  size_t off = 0;
  bool ok = true;
  explicit Reader(const std::string& s) : b(s) {}
  template <class T>
  T get() {
    T v{};
    if (off + sizeof v > b.size()) {
      ok = false;
      return v;
    }
    memcpy(&v, b.data() + off, sizeof v);
    off += sizeof v;
    return v;
  }
  std::string str() {
    std::string s;
    str_into(s);
    return s;
  }
  void str_into(std::string& s) {  // (into a reused string: no allocation once its capacity fits)
    const uint32_t n = get<uint32_t>();
    if (!ok || off + n > b.size()) {
      ok = false;
      s.clear();
      return;
    }
    s.assign(b.data() + off, n);
    off += n;
  }
};

struct Announce {
  int type = TIPS_REQ_ALLREDUCE, root = 0;
  bool bad = false;  // the announcing rank found the request unusable (its pointers disagree)
  int dtype;
  int64_t count;
  std::vector<int64_t> shape;
  std::string name;
};

struct Decision {
  bool ok;
  std::string name, err;
  std::vector<int64_t> sizes;
};

// The name tables' key carries the name's hash, made by the enqueuing thread (Req::name_hash): the
// negotiation thread admits a request without reading the name's bytes, which another core wrote
// (an insertion compares the cached hash first, the strings only when the hashes are equal).
struct NameKey {
  uint64_t h;
  std::string s;
  bool operator==(const NameKey& o) const { return h == o.h && s == o.s; }
};
struct NameKeyHash {
  size_t operator()(const NameKey& k) const { return (size_t)k.h; }
};

// a routed synchronous call's name (route_collective), one per call: never cached or expected
inline bool sync_name(const std::string& name) { return name.compare(0, 6, "~sync.") == 0; }

constexpr uint8_t kCachedOk = 2;  // a response entry's tag: a cached name decided OK (then its id)

// announce (rank -> rank 0): u8 shutdown, u32 n,
//   n x {i32 type, i32 root, u8 bad, i32 dtype, i64 count, u32 ndim, ndim x i64 dim, str name},
//   u32 k, k x u32 cache id
//   (a full record: the fields of the reference's RequestMessage, collective_messages.fbs: request
//   type, dtype, name, shape; plus the broadcast root, which the reference never sends, and `bad`,
//   see Announce. An id: a request the response cache holds with this dtype and shape.)
// response (rank 0 -> all): u8 shutdown, u32 n, n x entry, an entry one of
//   {u8 0 | 1 (ok), str name, str error, u32 m, m x i64 size}
//   {u8 kCachedOk, u32 cache id}
//   (sizes: an allgather's first dimension per rank, the ResponseMessage's tensor_sizes)
// str: u32 length, bytes.
// Each message's writer next to its reader; Coordinator::decide reads an announce's id list itself.
inline void put_announce_head(Writer& w, bool shutdown, uint32_t nfull) {
  w.put<uint8_t>(shutdown ? 1 : 0);
  w.put<uint32_t>(nfull);
}
inline void get_announce_head(Reader& rd, bool* shutdown, uint32_t* nfull) {
  *shutdown = rd.get<uint8_t>() != 0;
  *nfull = rd.get<uint32_t>();
}
void put_announce_record(Writer& w, int type, int root, bool bad, int dtype, int64_t count,
                         const std::vector<int64_t>& shape, const std::string& name);
void get_announce_record(Reader& rd, Announce& a);  // (a reused: its shape and name keep their allocations)
inline void put_announce_ids(Writer& w, const std::vector<uint32_t>& ids) {
  w.put<uint32_t>((uint32_t)ids.size());
  for (uint32_t id : ids) w.put<uint32_t>(id);
}

inline size_t put_response_head(Writer& w, bool shutdown) {  // returns where the entry count goes
  w.put<uint8_t>(shutdown ? 1 : 0);
  w.put<uint32_t>(0);
  return w.b.size() - sizeof(uint32_t);
}
inline void put_response_count(Writer& w, size_t at, uint32_t n) { memcpy(&w.b[at], &n, sizeof n); }
// sizes: m values `stride` words apart (the table's records)
void put_response_entry(Writer& w, bool ok, const std::string& name, const std::string& err, const int64_t* sizes,
                        uint32_t m, size_t stride);
inline void put_response_cached(Writer& w, uint32_t id) {
  w.put<uint8_t>(kCachedOk);
  w.put<uint32_t>(id);
}
struct ResponseCache;
// Into ds[0, *nd) (kept slots: their strings keep their capacity); a cached entry's name comes from
// `cache`, *ncached counts them. False: malformed (or an id the cache does not hold).
bool get_response(const std::string& resp, const ResponseCache& cache, bool* shutdown, std::vector<Decision>& ds,
                  size_t* nd, int64_t* ncached);

// ConstructResponseMessage's rules over p request records (TIPS_REQUEST_WORDS each)
int check_records(const int64_t* t, int p);
std::string shape_str(const int64_t* rec);

// ---- rank 0's table (IncreTensorCount + ConstructResponseMessage) ---------------
// A name joins the ready queue the moment its last rank announces it (or a
// rank announces it twice), as IncreTensorCount feeds ready_to_reduce
// (coordinator.cc:15-38, 451-455): rank 0's readiness order, O(1) per announce.
struct Table {
  struct Row {
    std::vector<int64_t> rec;  // p records of TIPS_REQUEST_WORDS
    std::vector<int> roots;    // broadcast root each rank named
    std::vector<char> seen;
    int nseen = 0;
    bool queued = false;
    std::string dup;  // set when a rank announced this name twice while unresolved
    std::string bad;  // set when a rank announced this name as unusable (failed once all announced)
  };
  int p = 1;
  std::unordered_map<std::string, Row> rows;
  std::vector<std::string> ready_q;  // [0, nready): names that became ready (slots reused across cycles)
  size_t nready = 0;
  // Rows resolved in earlier cycles, kept with their map node, key and vectors: a new name reuses
  // one instead of allocating all four (a 1000-gradient step resolves 1000 names a cycle).
  std::vector<std::unordered_map<std::string, Row>::node_type> spare;

  void announce(int rank, const Announce& a);
  // The names that became ready since the last call, in readiness order, each with its verdict,
  // written straight into rank 0's response (ok, name, error, allgather sizes): no per-name
  // Decision objects on the way. Returns how many.
  uint32_t write_ready(Writer& w);
};

// ---- response cache (every rank) ------------------------------------------------
// An allreduce decided OK is cached on every rank under an id: the position of its first OK
// decision in the response stream, which every rank reads in the same order (note()), so the
// ids agree without being sent. A later request with that name, dtype and shape is announced
// by id; when every rank announced an id by id, rank 0 answers "cached OK" without the table:
// the checks ConstructResponseMessage makes (coordinator.cc:90-186) passed for exactly these
// parameters. Any full record of the name (changed shape, an unusable pointer, a rank with the
// cache off) sends the round's ids of that name through the table, which then checks and
// words every failure as before. A failure drops the name from the cache on every rank.
struct ReqParams {  // what note() keeps of the request a decision resolved
  int type, dtype;
  int64_t count;
  const std::vector<int64_t>& shape;
};

struct ResponseCache {
  static constexpr size_t kCacheCap = 1 << 16;
  struct Entry {
    std::string name;
    int dtype;
    int64_t count;
    std::vector<int64_t> shape;
    bool live;
  };
  std::vector<Entry> entries;  // by id, dropped ones included
  std::unordered_map<NameKey, uint32_t, NameKeyHash> ids;
  NameKey look{0, std::string()};  // (a kept key: no allocation per lookup)
  const bool by_id;
  const size_t cap;
  // by_id false: this rank announces every request in full (it keeps the bookkeeping either way, so
  // ranks may differ in this). Rank 0 counts ids in a 64-bit rank mask: above 64 ranks everything
  // travels in full.
  explicit ResponseCache(int ranks, bool by_id = true, size_t cap = kCacheCap) : by_id(by_id && ranks <= 64), cap(cap) {}

  int32_t lookup(const std::string& name, uint64_t h) {
    look.h = h;
    look.s.assign(name);
    auto it = ids.find(look);
    return it == ids.end() ? -1 : (int32_t)it->second;
  }
  // the id to announce this request by, or -1: in full
  int32_t cached_id(const std::string& name, uint64_t hash, int type, int dtype, const std::vector<int64_t>& shape,
                    bool bad) {
    if (!by_id || type != TIPS_REQ_ALLREDUCE || bad || ids.empty()) return -1;
    const int32_t id = lookup(name, hash);
    if (id < 0) return -1;
    const Entry& e = entries[(size_t)id];
    return e.dtype == dtype && e.shape == shape ? id : -1;
  }
  bool live(uint32_t id) const { return id < entries.size() && entries[id].live; }
  Announce expand(uint32_t id) const;
  // (every rank, in response order) an OK allreduce joins the cache or refreshes its parameters; a
  // failure leaves it. r: the request the decision resolved, or none.
  void note(const Decision& d, const ReqParams* r);
};

// ---- rank 0's decision ----------------------------------------------------------
struct Coordinator {
  Coordinator(int ranks, ResponseCache& cache) : p(ranks), cache(cache) { table.p = ranks; }
  // Fold every rank's announce (all[0, p), rank order) into the table, answer with the ready list
  // in *resp (the previous response's buffer, reused). -1, or the rank whose announce was malformed.
  int decide(const std::string* all, std::string* resp);
  // this round's announces of id go to the table from now on, the ones counted so far too
  void to_table(int32_t id);

  struct IdState {  // this round's announces of a cached name
    uint64_t mask = 0;   // the ranks that announced it by id
    int n = 0;
    bool table = false;  // a full record came: the rest of the round goes through the table
  };
  const int p;
  ResponseCache& cache;  // the rank's own (the negotiation thread notes decisions into it)
  Table table;
  std::vector<IdState> idst;
  std::vector<uint32_t> id_ready;
  Announce a;  // (one, reused: its shape and name keep their allocations)
};

// ---- the linger's expected set --------------------------------------------------
// The names the last two cycles announced (routed ~sync requests aside) and how many of them the
// next announce holds so far: a training step enqueues the same gradients every step, and once
// all of them are in the linger need not wait out its quiet time (Negotiator::loop).
// (sorted name hashes, made by the enqueuing threads: admitted() compares integers, and a collision
// only ends a linger early or late, never changes what runs)
struct ExpectSet {
  std::vector<uint64_t> want, prev, cur;  // expected (sorted); the previous cycle's; the batch being rolled
  size_t hits = 0;

  void admitted(uint64_t name_hash) {
    if (!want.empty() && std::binary_search(want.begin(), want.end(), name_hash)) hits++;
  }
  bool complete() const { return !want.empty() && hits == want.size(); }
  // After a batch (cur cleared, roll_add for each of its requests): the next cycle expects this
  // one's names and the previous one's (two cycles, not one: Negotiator::loop).
  void roll_add(const std::string& name, uint64_t name_hash) {
    if (!sync_name(name)) cur.push_back(name_hash);
  }
  void roll() {
    // (kept as it is when this cycle named exactly the expected set: the previous one's
    // names are in it already)
    if (!cur.empty() && !(hits == want.size() && cur.size() == want.size())) {
      want.assign(cur.begin(), cur.end());
      want.insert(want.end(), prev.begin(), prev.end());
      std::sort(want.begin(), want.end());
      want.erase(std::unique(want.begin(), want.end()), want.end());
    }
    if (!cur.empty()) prev.swap(cur);
    cur.clear();
    hits = 0;
  }
};

}  // namespace rt
}  // namespace tips
