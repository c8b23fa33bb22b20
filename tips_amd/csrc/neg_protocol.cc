// neg_protocol.cc — the negotiation's protocol core (neg_protocol.h): record codecs, rank 0's
// checks (the reference's ConstructResponseMessage, tips/core/collective/coordinator.cc:90-186),
// its table and decision, the response cache.
#include "neg_protocol.h"

namespace tips {
namespace rt {

// ---- the messages' parts that are not inline (format: neg_protocol.h) ----------
void put_announce_record(Writer& w, int type, int root, bool bad, int dtype, int64_t count,
                         const std::vector<int64_t>& shape, const std::string& name) {
  w.put<int32_t>(type);
  w.put<int32_t>(root);
  w.put<uint8_t>(bad ? 1 : 0);
  w.put<int32_t>(dtype);
  w.put<int64_t>(count);
  w.put<uint32_t>((uint32_t)shape.size());
  for (int64_t d : shape) w.put<int64_t>(d);
  w.str(name);
}
void get_announce_record(Reader& rd, Announce& a) {
  a.shape.clear();
  a.type = rd.get<int32_t>();
  a.root = rd.get<int32_t>();
  a.bad = rd.get<uint8_t>() != 0;
  a.dtype = rd.get<int32_t>();
  a.count = rd.get<int64_t>();
  const uint32_t ndim = rd.get<uint32_t>();
  if (ndim > TIPS_MAX_DIMS) rd.ok = false;
  for (uint32_t d = 0; d < ndim && rd.ok; d++) a.shape.push_back(rd.get<int64_t>());
  rd.str_into(a.name);
}

void put_response_entry(Writer& w, bool ok, const std::string& name, const std::string& err, const int64_t* sizes,
                        uint32_t m, size_t stride) {
  w.put<uint8_t>(ok ? 1 : 0);
  w.str(name);
  w.str(ok ? std::string() : err);
  w.put<uint32_t>(m);
  for (uint32_t i = 0; i < m; i++) w.put<int64_t>(sizes[(size_t)i * stride]);
}
bool get_response(const std::string& resp, const ResponseCache& cache, bool* shutdown, std::vector<Decision>& ds,
                  size_t* nd, int64_t* ncached) {
  Reader rd(resp);
  *shutdown = rd.get<uint8_t>() != 0;
  const uint32_t n = rd.get<uint32_t>();
  *nd = 0;
  for (uint32_t i = 0; i < n && rd.ok; i++) {
    if (*nd == ds.size()) ds.emplace_back();
    Decision& d = ds[(*nd)++];  // (a kept slot: its strings keep their capacity)
    const uint8_t tag = rd.get<uint8_t>();
    d.sizes.clear();
    d.err.clear();
    if (tag == kCachedOk) {  // a cached allreduce every rank announced by id
      const uint32_t id = rd.get<uint32_t>();
      if (!cache.live(id)) return false;
      d.ok = true;
      d.name.assign(cache.entries[id].name);
      ++*ncached;
      continue;
    }
    d.ok = tag != 0;
    rd.str_into(d.name);
    rd.str_into(d.err);
    const uint32_t m = rd.get<uint32_t>();
    for (uint32_t k = 0; k < m && rd.ok && k < (1u << 20); k++) d.sizes.push_back(rd.get<int64_t>());
  }
  return rd.ok;
}

// ---- the rules ---------------------------------------------------------------------
std::string shape_str(const int64_t* rec) {  // tensorflow::TensorShape::DebugString() form: [2,4]
  std::string s = "[";
  for (int64_t d = 0; d < rec[2]; d++) s += (d ? "," : "") + std::to_string(rec[3 + d]);
  return s + "]";
}

// ConstructResponseMessage (coordinator.cc:90-186) + GatherFirstRankSizes (:40-88): every
// record is compared with rank 0's; the first mismatch is reported with the reference's text.
int check_records(const int64_t* t, int p) {
  const int W = TIPS_REQUEST_WORDS;
  const int64_t* r0 = t;
  for (int i = 1; i < p; i++)
    if (t[i * W + 1] != r0[1])
      return fail(TIPS_ERR_MISMATCH, "Mismatch data types found: %lld vs %lld.", (long long)r0[1], (long long)t[i * W + 1]);
  for (int i = 1; i < p; i++)  // (the reference compares requests[0] with itself here, coordinator.cc:123-129)
    if (t[i * W + 0] != r0[0])
      return fail(TIPS_ERR_MISMATCH, "Mismatched operations found: %lld vs %lld.", (long long)r0[0], (long long)t[i * W]);
  for (int i = 0; i < p; i++)
    if (t[i * W + 2] < 0 || t[i * W + 2] > TIPS_MAX_DIMS) return fail(TIPS_ERR_INVALID_ARG, "bad ndim in request %d", i);
  if (r0[0] == TIPS_REQ_ALLREDUCE || r0[0] == TIPS_REQ_BROADCAST) {
    for (int i = 1; i < p; i++) {
      const int64_t* ri = t + i * W;
      bool same = ri[2] == r0[2];
      for (int64_t d = 0; same && d < r0[2]; d++) same = ri[3 + d] == r0[3 + d];
      if (!same)
        return fail(TIPS_ERR_MISMATCH, "Mismatched %s tensor shapes: %s vs %s",
                    r0[0] == TIPS_REQ_BROADCAST ? "broadcast" : "allreduce", shape_str(r0).c_str(), shape_str(ri).c_str());
    }
  } else if (r0[0] == TIPS_REQ_ALLGATHER) {
    if (r0[2] == 0) return fail(TIPS_ERR_MISMATCH, "An empty tensor found");
    for (int i = 1; i < p; i++) {
      const int64_t* ri = t + i * W;
      if (ri[2] != r0[2])
        return fail(TIPS_ERR_MISMATCH, "Mismatched allgather tensor shapes: rank %lld vs %lld", (long long)r0[2],
                    (long long)ri[2]);
      for (int64_t d = 1; d < r0[2]; d++)
        if (ri[3 + d] != r0[3 + d])
          return fail(TIPS_ERR_MISMATCH, "Mismatched allgather tensor shapes: %lld-th dimension %lld vs %lld",
                      (long long)d, (long long)r0[3 + d], (long long)ri[3 + d]);
    }
  } else {
    return fail(TIPS_ERR_INVALID_ARG, "Not supported request type: %lld", (long long)r0[0]);
  }
  return 0;
}

// ---- rank 0's table ------------------------------------------------------------------
void Table::announce(int rank, const Announce& a) {
  auto it = rows.find(a.name);
  if (it == rows.end()) {
    if (!spare.empty()) {
      auto nh = std::move(spare.back());
      spare.pop_back();
      nh.key() = a.name;
      Row& r = nh.mapped();
      r.rec.assign((size_t)p * TIPS_REQUEST_WORDS, 0);
      r.seen.assign(p, 0);
      r.roots.assign(p, 0);
      r.nseen = 0;
      r.queued = false;
      r.dup.clear();
      r.bad.clear();
      it = rows.insert(std::move(nh)).position;
    } else {
      Row r;
      r.rec.assign((size_t)p * TIPS_REQUEST_WORDS, 0);
      r.seen.assign(p, 0);
      r.roots.assign(p, 0);
      it = rows.emplace(a.name, std::move(r)).first;
    }
  }
  Row& r = it->second;
  if (r.seen[rank]) {
    if (r.dup.empty()) r.dup = "rank " + std::to_string(rank) + " enqueued " + a.name + " twice";
  } else {
    r.seen[rank] = 1;
    r.nseen++;
    if (a.bad && r.bad.empty())
      r.bad = "named request " + a.name + ": one device and one host pointer on rank " + std::to_string(rank);
    int64_t* rec = &r.rec[(size_t)rank * TIPS_REQUEST_WORDS];
    rec[0] = a.type;
    rec[1] = a.dtype;
    r.roots[rank] = a.root;
    rec[2] = (int64_t)a.shape.size();  // (<= TIPS_MAX_DIMS: checked at enqueue and on decode)
    for (size_t d = 0; d < a.shape.size(); d++) rec[3 + d] = a.shape[d];
  }
  if (!r.queued && (!r.dup.empty() || r.nseen == p)) {
    r.queued = true;
    if (nready < ready_q.size()) ready_q[nready] = a.name;  // (assign into a kept string: no allocation)
    else ready_q.push_back(a.name);
    nready++;
  }
}

uint32_t Table::write_ready(Writer& w) {
  const int W = TIPS_REQUEST_WORDS;
  for (size_t q = 0; q < nready; q++) {
    const std::string& name = ready_q[q];
    auto it = rows.find(name);
    Row& r = it->second;
    const std::string* err = &r.dup;
    std::string why;
    bool ok = false;
    if (r.dup.empty() && !r.bad.empty()) {
      err = &r.bad;
    } else if (r.dup.empty()) {
      ok = check_records(r.rec.data(), p) == 0;
      if (!ok) why = last_error();
      if (ok && r.rec[0] == TIPS_REQ_BROADCAST)
        for (int i = 1; i < p && ok; i++)
          if (r.roots[i] != r.roots[0]) {
            ok = false;
            why = "Mismatched broadcast root ranks: " + std::to_string(r.roots[0]) + " vs " + std::to_string(r.roots[i]);
          }
      err = &why;
    }
    // (an allgather's sizes: GatherFirstRankSizes, coordinator.cc:40-88)
    put_response_entry(w, ok, name, *err, &r.rec[3], ok && r.rec[0] == TIPS_REQ_ALLGATHER ? (uint32_t)p : 0, W);
    if (spare.size() < 4096) spare.push_back(rows.extract(it));
    else rows.erase(it);
  }
  const uint32_t n = (uint32_t)nready;
  nready = 0;
  return n;
}

// ---- the response cache ----------------------------------------------------------------
Announce ResponseCache::expand(uint32_t id) const {
  const Entry& e = entries[id];
  Announce a;
  a.type = TIPS_REQ_ALLREDUCE;
  a.dtype = e.dtype;
  a.count = e.count;
  a.shape = e.shape;
  a.name = e.name;
  return a;
}

void ResponseCache::note(const Decision& d, const ReqParams* r) {
  if (sync_name(d.name)) return;  // (routed calls: never cached)
  const int32_t id = lookup(d.name, std::hash<std::string>()(d.name));
  if (!d.ok || !r || r->type != TIPS_REQ_ALLREDUCE) {
    if (id >= 0) {
      entries[(size_t)id].live = false;
      ids.erase(look);
    }
    return;
  }
  if (id >= 0) {
    Entry& e = entries[(size_t)id];
    e.dtype = r->dtype;
    e.count = r->count;
    e.shape = r->shape;
    return;
  }
  if (entries.size() >= cap) return;  // (full: later names travel in full, on every rank alike)
  ids.emplace(NameKey{std::hash<std::string>()(d.name), d.name}, (uint32_t)entries.size());
  entries.push_back(Entry{d.name, r->dtype, r->count, r->shape, true});
}

// ---- rank 0's decision -----------------------------------------------------------------
void Coordinator::to_table(int32_t id) {
  if ((size_t)id >= idst.size()) idst.resize(cache.entries.size());
  IdState& st = idst[(size_t)id];
  if (st.table) return;
  st.table = true;
  for (int q = 0; q < 64 && st.mask; q++)
    if (st.mask & (1ull << q)) {
      st.mask &= ~(1ull << q);
      table.announce(q, cache.expand((uint32_t)id));
    }
  st.n = 0;
}

int Coordinator::decide(const std::string* all, std::string* resp) {
  bool everyone_stops = true;
  for (int r = 0; r < p; r++) {
    Reader rd(all[r]);
    bool stops;
    uint32_t n;
    get_announce_head(rd, &stops, &n);
    everyone_stops &= stops;
    for (uint32_t i = 0; i < n && rd.ok; i++) {
      get_announce_record(rd, a);
      if (!rd.ok) break;
      // a full record of a name others announced by id this round: theirs join the table too
      if (!cache.ids.empty()) {
        const int32_t id = cache.lookup(a.name, std::hash<std::string>()(a.name));
        if (id >= 0) to_table(id);
      }
      table.announce(r, a);
    }
    const uint32_t k = rd.get<uint32_t>();
    for (uint32_t i = 0; i < k && rd.ok; i++) {
      const uint32_t id = rd.get<uint32_t>();
      if (!cache.live(id)) {
        rd.ok = false;
        break;
      }
      if (idst.size() < cache.entries.size()) idst.resize(cache.entries.size());
      IdState& st = idst[id];
      const uint64_t bit = 1ull << r;
      if (st.table || (st.mask & bit)) {  // (a rank's second announce: the table names the duplicate)
        to_table(id);
        table.announce(r, cache.expand(id));
        continue;
      }
      st.mask |= bit;
      if (++st.n == p) {  // every rank, every one by id: ready, valid as cached
        st.mask = 0;
        st.n = 0;
        id_ready.push_back(id);
      }
    }
    if (!rd.ok) return r;
  }
  for (size_t q = 0; q < table.nready; q++) {  // (decided now: later ids of these names count anew)
    const int32_t id = idst.empty() ? -1 : cache.lookup(table.ready_q[q], std::hash<std::string>()(table.ready_q[q]));
    if (id >= 0 && (size_t)id < idst.size()) idst[id].table = false;
  }
  Writer w;
  w.b.swap(*resp);  // (the previous response's buffer, reused)
  w.b.clear();
  const size_t count_at = put_response_head(w, everyone_stops);
  uint32_t n = table.write_ready(w);
  for (uint32_t id : id_ready) put_response_cached(w, id);  // after the table's: readiness order among themselves
  n += (uint32_t)id_ready.size();
  id_ready.clear();
  put_response_count(w, count_at, n);
  resp->swap(w.b);
  return -1;
}

}  // namespace rt
}  // namespace tips
