// neg_protocol_check.cc — the negotiation's protocol unit (tips_amd/csrc/neg_protocol.h) driven
// on its own: p ranks simulated in one process, each with its own response cache, one Coordinator;
// announces built with the encoder, the response decoded with the decoder and noted on every rank
// in response order. Links neg_protocol.cc and err.cc only (no HIP, socket or thread), built with
// AddressSanitizer and UBSan (Makefile: tools/_bin/neg_protocol_check; tests/test_neg_protocol.py).
// The cache's capacity rule is checked with a reduced cap (ResponseCache's constructor argument).
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <memory>

#include "../../tips_amd/csrc/neg_protocol.h"

using namespace tips::rt;

namespace {

int g_checks = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    g_checks++;                                                          \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

void check_eq(const std::string& got, const std::string& want, int line) {
  g_checks++;
  if (got != want) {
    fprintf(stderr, "%s:%d: got  \"%s\"\n%*swant \"%s\"\n", __FILE__, line, got.c_str(), 4, "", want.c_str());
    exit(1);
  }
}
#define CHECK_EQ(got, want) check_eq((got), (want), __LINE__)

const int AR = TIPS_REQ_ALLREDUCE, AG = TIPS_REQ_ALLGATHER, BC = TIPS_REQ_BROADCAST;
using Shape = std::vector<int64_t>;
uint64_t H(const std::string& s) { return std::hash<std::string>()(s); }

struct Rq {
  std::string name;
  Shape shape{8};
  int type = AR, dtype = 0, root = 0;
  bool bad = false;
  int64_t count() const {
    int64_t c = 1;
    for (int64_t d : shape) c *= d;
    return c;
  }
};
using Lines = std::vector<std::string>;
using PerRank = std::vector<std::vector<Rq>>;

struct Sim {
  int p;
  std::vector<std::unique_ptr<ResponseCache>> cache;
  std::unique_ptr<Coordinator> coord;
  std::vector<std::map<std::string, Rq>> pending;  // what each rank has announced and not seen decided
  std::vector<std::vector<Decision>> ds;
  std::string resp;
  int64_t ncached = 0;           // cached-OK entries of the last response
  std::vector<size_t> by_id;     // how many requests each rank announced by id in the last cycle
  int malformed = -1;            // the last decide()'s verdict

  // off: the rank that announces everything in full (TIPS_RESPONSE_CACHE=0 there), or -1
  explicit Sim(int ranks, int off = -1, size_t cap = ResponseCache::kCacheCap) : p(ranks), pending(ranks), ds(ranks), by_id(ranks) {
    for (int r = 0; r < p; r++) cache.emplace_back(new ResponseCache(p, r != off, cap));
    coord.reset(new Coordinator(p, *cache[0]));
  }

  std::string announce(int r, const std::vector<Rq>& rqs, bool shutdown = false) {
    std::vector<uint32_t> ids;
    std::vector<const Rq*> full;
    for (const Rq& q : rqs) {
      const int32_t id = cache[r]->cached_id(q.name, H(q.name), q.type, q.dtype, q.shape, q.bad);
      if (id >= 0) ids.push_back((uint32_t)id);
      else full.push_back(&q);
      pending[r].emplace(q.name, q);
    }
    by_id[r] = ids.size();
    Writer w;
    put_announce_head(w, shutdown, (uint32_t)full.size());
    for (const Rq* q : full) put_announce_record(w, q->type, q->root, q->bad, q->dtype, q->count(), q->shape, q->name);
    put_announce_ids(w, ids);
    return w.b;
  }

  // Rank 0 decides over these announce bytes; every rank decodes and notes. The decisions as the
  // dry run logs them ("name OK[ sizes=a,b]" / "name ERR text"), the same on every rank.
  Lines decide(const std::vector<std::string>& all) {
    malformed = coord->decide(all.data(), &resp);
    Lines first;
    if (malformed >= 0) return first;
    for (int r = 0; r < p; r++) {
      bool shutdown = true;
      size_t nd = 0;
      ncached = 0;
      CHECK(get_response(resp, *cache[r], &shutdown, ds[r], &nd, &ncached));
      CHECK(!shutdown);
      Lines lines;
      for (size_t i = 0; i < nd; i++) {
        const Decision& d = ds[r][i];
        std::string sz;
        for (size_t k = 0; k < d.sizes.size(); k++) sz += (k ? "," : " sizes=") + std::to_string(d.sizes[k]);
        lines.push_back(d.name + (d.ok ? " OK" + sz : " ERR " + d.err));
        auto it = pending[r].find(d.name);
        if (it == pending[r].end()) {
          cache[r]->note(d, nullptr);
        } else {
          const ReqParams rp{it->second.type, it->second.dtype, it->second.count(), it->second.shape};
          cache[r]->note(d, &rp);
          pending[r].erase(it);
        }
      }
      if (r == 0) first = lines;
      else CHECK(lines == first);
    }
    return first;
  }

  Lines cycle(const PerRank& per) {
    CHECK((int)per.size() == p);
    std::vector<std::string> all;
    for (int r = 0; r < p; r++) all.push_back(announce(r, per[r]));
    return decide(all);
  }
  Lines all_ranks(const std::vector<Rq>& rqs) { return cycle(PerRank((size_t)p, rqs)); }
  // every rank holds `name` under `id` (-1: not at all)
  void check_id(const std::string& name, int32_t id) {
    for (int r = 0; r < p; r++) CHECK(cache[r]->lookup(name, H(name)) == id);
  }
};

Rq rq(const std::string& name, Shape shape = {8}, int type = AR, int dtype = 0, int root = 0, bool bad = false) {
  Rq q;
  q.name = name;
  q.shape = shape;
  q.type = type;
  q.dtype = dtype;
  q.root = root;
  q.bad = bad;
  return q;
}

// Names announced over several cycles in different per-rank orders come back in the order their
// last announce was folded (ranks 0..p-1 within a cycle), never before their last rank.
void readiness_order() {
  Sim s(3);
  CHECK(s.cycle({{rq("a"), rq("b"), rq("c")}, {rq("c")}, {rq("b")}}).empty());
  CHECK((s.cycle({{}, {rq("b"), rq("a")}, {rq("a"), rq("c")}}) == Lines{"b OK", "a OK", "c OK"}));
  CHECK((s.cycle({{rq("x"), rq("y")}, {rq("y")}, {}}).empty()));
  CHECK((s.cycle({{rq("z")}, {rq("z")}, {rq("z"), rq("y")}}) == Lines{"z OK", "y OK"}));
  CHECK((s.cycle({{}, {rq("x")}, {rq("x")}}) == Lines{"x OK"}));
  Sim one(1);
  CHECK((one.all_ranks({rq("q"), rq("r")}) == Lines{"q OK", "r OK"}));
}

// one name, rank r announcing per[r]: the single verdict
std::string verdict(const std::vector<Rq>& per) {
  Sim s((int)per.size());
  PerRank pr;
  for (const Rq& q : per) pr.push_back({q});
  const Lines l = s.cycle(pr);
  CHECK(l.size() == 1);
  return l[0];
}

void verdicts() {
  CHECK_EQ(verdict({rq("b", {8}, AR, 0), rq("b", {8}, AR, 1)}), "b ERR Mismatch data types found: 0 vs 1.");
  CHECK_EQ(verdict({rq("op"), rq("op", {8}, AG)}), "op ERR Mismatched operations found: 0 vs 1.");
  CHECK_EQ(verdict({rq("a", {8}), rq("a", {8}), rq("a", {9})}), "a ERR Mismatched allreduce tensor shapes: [8] vs [9]");
  CHECK_EQ(verdict({rq("w", {2, 4}), rq("w", {4, 2})}), "w ERR Mismatched allreduce tensor shapes: [2,4] vs [4,2]");
  CHECK_EQ(verdict({rq("a", {4}), rq("a", {4, 1})}), "a ERR Mismatched allreduce tensor shapes: [4] vs [4,1]");
  CHECK_EQ(verdict({rq("bs", {2, 4}, BC), rq("bs", {4, 2}, BC)}), "bs ERR Mismatched broadcast tensor shapes: [2,4] vs [4,2]");
  CHECK_EQ(verdict({rq("g", {2, 4}, AG), rq("g", {2, 4, 1}, AG)}), "g ERR Mismatched allgather tensor shapes: rank 2 vs 3");
  CHECK_EQ(verdict({rq("s", {2, 4}, AG), rq("s", {3, 3}, AG)}), "s ERR Mismatched allgather tensor shapes: 1-th dimension 4 vs 3");
  CHECK_EQ(verdict({rq("e", {}, AG), rq("e", {}, AG)}), "e ERR An empty tensor found");
  CHECK_EQ(verdict({rq("br", {4}, BC, 0, 0), rq("br", {4}, BC, 0, 0), rq("br", {4}, BC, 0, 2)}),
           "br ERR Mismatched broadcast root ranks: 0 vs 2");
  CHECK_EQ(verdict({rq("bo", {4}, BC, 0, 1), rq("bo", {4}, BC, 0, 1)}), "bo OK");
  CHECK_EQ(verdict({rq("x"), rq("x", {8}, AR, 0, 0, true), rq("x")}),
           "x ERR named request x: one device and one host pointer on rank 1");
  CHECK_EQ(verdict({rq("t", {8}, 7), rq("t", {8}, 7)}), "t ERR Not supported request type: 7");
  CHECK_EQ(verdict({rq("ag", {2, 4}, AG), rq("ag", {5, 4}, AG), rq("ag", {1, 4}, AG)}), "ag OK sizes=2,5,1");
  CHECK_EQ(verdict({rq("ag1", {3}, AG)}), "ag1 OK sizes=3");
  // a name announced twice by one rank before it resolves: answered at once, with that text
  Sim s(2);
  CHECK((s.cycle({{rq("d"), rq("d")}, {rq("d")}}) == Lines{"d ERR rank 0 enqueued d twice"}));
  Sim t(2);
  CHECK(t.cycle({{}, {rq("d")}}).empty());
  CHECK((t.cycle({{}, {rq("d")}}) == Lines{"d ERR rank 1 enqueued d twice"}));
}

void cache_basics(int p) {
  Sim s(p);
  const std::vector<Rq> step{rq("g0"), rq("g1", {2, 3}), rq("~sync.0"), rq("bc", {4}, BC), rq("g2", {1}, AR, 1), rq("ag", {2}, AG)};
  const Lines l = s.all_ranks(step);
  CHECK(l.size() == 6 && s.ncached == 0);
  CHECK_EQ(l[0], "g0 OK");
  // ids in response order; ~sync. names and non-allreduce requests never get one
  s.check_id("g0", 0);
  s.check_id("g1", 1);
  s.check_id("g2", 2);
  s.check_id("~sync.0", -1);
  s.check_id("bc", -1);
  s.check_id("ag", -1);
  // by id on every rank (64 at the most), plus a new name: the table's entries come first, then the cached ones
  std::vector<Rq> again{rq("g2", {1}, AR, 1), rq("g0"), rq("n"), rq("g1", {2, 3})};
  const Lines m = s.all_ranks(again);
  if (p <= 64) {
    for (int r = 0; r < p; r++) CHECK(s.by_id[r] == 3);
    CHECK(s.ncached == 3);
    CHECK((m == Lines{"n OK", "g2 OK", "g0 OK", "g1 OK"}));
  } else {  // nothing travels by id
    for (int r = 0; r < p; r++) CHECK(s.by_id[r] == 0);
    CHECK(s.ncached == 0);
    CHECK((m == Lines{"g2 OK", "g0 OK", "n OK", "g1 OK"}));
  }
  s.check_id("n", 3);
  // a changed dtype travels in full and refreshes the entry under its id
  CHECK((s.all_ranks({rq("g0", {8}, AR, 1)}) == Lines{"g0 OK"}));
  CHECK(s.ncached == 0);
  s.check_id("g0", 0);
  CHECK((s.all_ranks({rq("g0", {8}, AR, 1)}) == Lines{"g0 OK"}));
  CHECK(s.ncached == (p <= 64 ? 1 : 0));
}

void cache_cap() {
  Sim s(2, -1, /*cap=*/4);
  std::vector<Rq> step;
  for (int i = 0; i < 5; i++) step.push_back(rq("n" + std::to_string(i)));
  CHECK(s.all_ranks(step).size() == 5);
  s.check_id("n3", 3);
  s.check_id("n4", -1);  // decided, not cached
  CHECK((s.all_ranks(step) == Lines{"n4 OK", "n0 OK", "n1 OK", "n2 OK", "n3 OK"}));
  CHECK(s.ncached == 4 && s.cache[0]->entries.size() == 4);
}

// Some ranks by id, one in full with a changed shape (rank `odd`: first or last in the fold)
void mixed_changed_shape(int odd) {
  Sim s(3);
  CHECK((s.all_ranks({rq("w")}) == Lines{"w OK"}));
  PerRank per(3, {rq("w")});
  per[odd] = {rq("w", {9})};
  const Lines l = s.cycle(per);
  for (int r = 0; r < 3; r++) CHECK(s.by_id[r] == (r == odd ? 0u : 1u));
  CHECK(l.size() == 1 && s.ncached == 0);
  CHECK_EQ(l[0], odd == 0 ? "w ERR Mismatched allreduce tensor shapes: [9] vs [8]" : "w ERR Mismatched allreduce tensor shapes: [8] vs [9]");
  s.check_id("w", -1);  // dropped everywhere
  for (int r = 0; r < 3; r++) CHECK(!s.cache[r]->live(0));
  CHECK((s.all_ranks({rq("w")}) == Lines{"w OK"}));  // in full
  for (int r = 0; r < 3; r++) CHECK(s.by_id[r] == 0);
  CHECK(s.ncached == 0);
  s.check_id("w", 1);
  CHECK((s.all_ranks({rq("w")}) == Lines{"w OK"}));  // by id again
  CHECK(s.ncached == 1);
}

// The same with an equal full record (a rank with the cache off): OK through the table, refreshed
void mixed_equal_full(int off) {
  Sim s(3, off);
  CHECK((s.all_ranks({rq("w"), rq("v")}) == Lines{"w OK", "v OK"}));
  for (int step = 0; step < 2; step++) {
    CHECK((s.all_ranks({rq("v"), rq("w")}) == Lines{"v OK", "w OK"}));
    for (int r = 0; r < 3; r++) CHECK(s.by_id[r] == (r == off ? 0u : 2u));
    CHECK(s.ncached == 0);
    s.check_id("w", 0);
    s.check_id("v", 1);
    for (int r = 0; r < 3; r++) CHECK(s.cache[r]->live(0) && s.cache[r]->live(1));
  }
}

void mixed_duplicates_and_spread() {
  {  // rank 1 announces the id twice before the others
    Sim s(3);
    s.all_ranks({rq("w")});
    CHECK((s.cycle({{}, {rq("w"), rq("w")}, {}}) == Lines{"w ERR rank 1 enqueued w twice"}));
    CHECK(s.by_id[1] == 2);
    s.check_id("w", -1);
  }
  {  // ... and after them, over two cycles
    Sim s(3);
    s.all_ranks({rq("w")});
    CHECK(s.cycle({{}, {rq("w")}, {}}).empty());
    CHECK((s.cycle({{rq("w")}, {rq("w")}, {rq("w")}}) == Lines{"w ERR rank 1 enqueued w twice"}));
    for (int r = 0; r < 3; r++) CHECK(s.by_id[r] == 1);
    s.check_id("w", -1);
  }
  {  // an id spread over two cycles is answered once, in the second
    Sim s(2);
    s.all_ranks({rq("w")});
    CHECK(s.cycle({{rq("w")}, {}}).empty());
    CHECK(s.ncached == 0);
    CHECK((s.cycle({{}, {rq("w")}}) == Lines{"w OK"}));
    CHECK(s.ncached == 1);
    CHECK(s.cycle({{}, {}}).empty());
  }
}

// rank 1's announce bytes against a fresh 2-rank negotiation that has g0, g1 cached (and dropped
// g2): the rank decide() names, -1 if it took them
int decide_raw(const std::string& bytes) {
  Sim s(2);
  s.all_ranks({rq("g0"), rq("g1"), rq("g2")});
  s.cycle({{rq("g2", {9})}, {rq("g2")}});  // (fails: id 2 is dropped)
  CHECK(!s.cache[0]->live(2) && s.cache[0]->entries.size() == 3);
  s.decide({s.announce(0, {}), bytes});
  return s.malformed;
}

std::string raw_record(uint32_t ndim, uint32_t ndims_present, uint32_t name_len, const std::string& name_bytes) {
  Writer w;
  put_announce_head(w, false, 1);
  w.put<int32_t>(AR);
  w.put<int32_t>(0);
  w.put<uint8_t>(0);
  w.put<int32_t>(0);
  w.put<int64_t>(8);
  w.put<uint32_t>(ndim);
  for (uint32_t d = 0; d < ndims_present; d++) w.put<int64_t>(2);
  w.put<uint32_t>(name_len);
  w.b += name_bytes;
  put_announce_ids(w, {});
  return w.b;
}

void malformed() {
  Sim b(2);
  b.all_ranks({rq("g0"), rq("g1")});
  const std::string good = b.announce(1, {rq("x", {2, 3}), rq("g1"), rq("y", {}, AG), rq("g0")});
  CHECK(b.by_id[1] == 2);
  CHECK(decide_raw(good) == -1);
  for (size_t n = 0; n < good.size(); n++) CHECK(decide_raw(good.substr(0, n)) == 1);  // every strict prefix
  CHECK(decide_raw(raw_record(TIPS_MAX_DIMS, TIPS_MAX_DIMS, 1, "n")) == -1);
  CHECK(decide_raw(raw_record(TIPS_MAX_DIMS + 1, TIPS_MAX_DIMS + 1, 1, "n")) == 1);
  CHECK(decide_raw(raw_record(1, 1, 1000, "short")) == 1);       // a string length past the buffer
  CHECK(decide_raw(raw_record(1, 1, 0xffffffffu, "short")) == 1);
  auto ids = [](std::vector<uint32_t> v) {
    Writer w;
    put_announce_head(w, false, 0);
    put_announce_ids(w, v);
    return w.b;
  };
  CHECK(decide_raw(ids({1, 0})) == -1);
  CHECK(decide_raw(ids({3})) == 1);            // an id >= the cache size
  CHECK(decide_raw(ids({0xffffffffu})) == 1);
  CHECK(decide_raw(ids({2})) == 1);            // a dropped entry's id

  // the response: an OK entry, a failure, an allgather's sizes, a cached entry
  ResponseCache c(2);
  Decision d{true, "g0", "", {}};
  const Shape sh{8};
  const ReqParams rp{AR, 0, 8, sh};
  c.note(d, &rp);
  d.name = "gone";
  c.note(d, &rp);
  d.ok = false;
  c.note(d, &rp);  // (id 1: dropped)
  const int64_t sizes[2] = {2, 5};
  Writer w;
  const size_t at = put_response_head(w, false);
  put_response_entry(w, true, "a", "", nullptr, 0, 1);
  put_response_entry(w, false, "b", "why", nullptr, 0, 1);
  put_response_entry(w, true, "ag", "", sizes, 2, 1);
  put_response_cached(w, 0);
  put_response_count(w, at, 4);
  std::vector<Decision> ds;
  bool shutdown;
  size_t nd;
  int64_t nc = 0;
  CHECK(get_response(w.b, c, &shutdown, ds, &nd, &nc) && nd == 4 && nc == 1 && !shutdown);
  CHECK(ds[1].err == "why" && !ds[1].ok && (ds[2].sizes == Shape{2, 5}) && ds[3].name == "g0" && ds[3].ok);
  for (size_t n = 0; n < w.b.size(); n++) CHECK(!get_response(w.b.substr(0, n), c, &shutdown, ds, &nd, &nc));
  auto cached = [&](uint32_t id) {
    Writer v;
    const size_t a = put_response_head(v, false);
    put_response_cached(v, id);
    put_response_count(v, a, 1);
    return get_response(v.b, c, &shutdown, ds, &nd, &nc);
  };
  CHECK(cached(0) && !cached(1) && !cached(2) && !cached(0xffffffffu));
  Writer v;  // a size count of 2^32 - 1 on a short buffer
  const size_t a = put_response_head(v, false);
  v.put<uint8_t>(1);
  v.str("ag");
  v.str("");
  v.put<uint32_t>(0xffffffffu);
  v.put<int64_t>(7);
  put_response_count(v, a, 1);
  CHECK(!get_response(v.b, c, &shutdown, ds, &nd, &nc));
}

// one cycle of the linger's set: admits in order, then the roll; whether the set was complete
// after each admit
std::vector<bool> expect_cycle(ExpectSet& e, const std::vector<std::string>& names) {
  std::vector<bool> complete;
  for (auto& n : names) {
    e.admitted(H(n));
    complete.push_back(e.complete());
  }
  for (auto& n : names) e.roll_add(n, H(n));
  e.roll();
  return complete;
}

void expected_set() {
  using B = std::vector<bool>;
  ExpectSet e;
  CHECK(!e.complete());
  CHECK((expect_cycle(e, {"a", "b", "c"}) == B{false, false, false}));
  CHECK(e.want.size() == 3);
  // the same names: kept, complete at the last admit
  CHECK((expect_cycle(e, {"c", "a", "b"}) == B{false, false, true}));
  CHECK((expect_cycle(e, {"b", "c", "a"}) == B{false, false, true}));
  CHECK(e.want.size() == 3 && e.hits == 0);
  // ~sync. names are ignored
  CHECK((expect_cycle(e, {"a", "~sync.4", "b", "c", "~sync.5"}) == B{false, false, false, true, true}));
  CHECK(e.want.size() == 3);
  CHECK(expect_cycle(e, {"~sync.6"}) == B{false});
  CHECK(e.want.size() == 3 && e.prev.size() == 3);
  // a subset cycle: the union with the previous cycle, so the full set again is complete
  CHECK((expect_cycle(e, {"a", "b"}) == B{false, false}));
  CHECK(e.want.size() == 3 && e.prev.size() == 2);
  CHECK((expect_cycle(e, {"a", "b", "c"}) == B{false, false, true}));
  CHECK(e.want.size() == 3 && e.prev.size() == 3);
  // a cycle that adds names: the union
  CHECK((expect_cycle(e, {"a", "b", "c", "d"}) == B{false, false, true, true}));
  CHECK(e.want.size() == 4);
  CHECK((expect_cycle(e, {"e"}) == B{false}));
  CHECK(e.want.size() == 5 && std::is_sorted(e.want.begin(), e.want.end()));
  CHECK((expect_cycle(e, {"e"}) == B{false}));  // (d..a were two cycles ago)
  CHECK(e.want.size() == 1);
}

}  // namespace

int main() {
  readiness_order();
  verdicts();
  for (int p : {1, 2, 3, 5, 65}) cache_basics(p);
  cache_cap();
  for (int odd : {2, 0}) mixed_changed_shape(odd);  // id-then-full, full-then-id
  for (int off : {2, 0}) mixed_equal_full(off);
  mixed_duplicates_and_spread();
  malformed();
  expected_set();
  printf("neg_protocol_check: %d checks ok\n", g_checks);
  return 0;
}
