// ivfflat.hpp -- C++ host-side mirror of vers's IVFFlatIndex<N> / Index<N> on top of the C ABI (include/vers_hip.h).
//
// The reference host is Rust (vers/src/indexes/{base,ivfflat}.rs); no Rust toolchain exists in this environment, so
// the compiled-language host side is written in C++ with the SAME names, argument meaning and error behaviour:
//   Vector<N>                      base.rs:14-17   (#[repr(align(256))] [f32; N])
//   IVFFlatIndex<N>::build_index   ivfflat.rs:102-136
//   Index::add / search_approximate ivfflat.rs:200-213 / 153-198
//   Index::save_index / load_index base.rs:31-58   (bincode 1.3 layout, see vers_amd/index.py)
// A reference panic becomes a thrown vers::Panic.  The five fields stay host-owned (serde); the handle is a cache.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vers_hip.h"

namespace vers {

struct Panic : std::runtime_error {
  int32_t status;
  Panic(int32_t s, const std::string& m) : std::runtime_error(m), status(s) {}
};
inline void check(int32_t status) {
  if (status != VERS_OK) throw Panic(status, std::string("vers status ") + std::to_string(status) + ": " + vers_last_error());
}

template <size_t N>
struct alignas(256) Vector {  // base.rs:14-17
  float v[N];
};

template <size_t N>
class IVFFlatIndex {
 public:
  // the reference's fields, in its order (ivfflat.rs:9-15)
  size_t num_centroids = 0;
  std::vector<Vector<N>> values;
  std::vector<Vector<N>> centroids;
  std::vector<size_t> assignments;
  std::vector<std::vector<size_t>> ids;

  IVFFlatIndex() = default;
  IVFFlatIndex(const IVFFlatIndex&) = delete;
  IVFFlatIndex& operator=(const IVFFlatIndex&) = delete;
  IVFFlatIndex(IVFFlatIndex&& o) noexcept { *this = std::move(o); }
  IVFFlatIndex& operator=(IVFFlatIndex&& o) noexcept {
    if (h_) vers_ivf_destroy(h_);
    num_centroids = o.num_centroids; values = std::move(o.values); centroids = std::move(o.centroids);
    assignments = std::move(o.assignments); ids = std::move(o.ids); h_ = o.h_; device_ = o.device_; o.h_ = nullptr;
    return *this;
  }
  ~IVFFlatIndex() { if (h_) vers_ivf_destroy(h_); }

  // ivfflat.rs:102-136.  `init_indices` (optional) injects the draws of initialize_centroids (ivfflat.rs:18-27);
  // without it they are drawn like the reference does: k indices WITH replacement per attempt from an unseeded RNG.
  static IVFFlatIndex build_index(size_t num_clusters, size_t num_attempts, size_t max_iterations,
                                  const std::vector<Vector<N>>& vectors, const std::vector<uint64_t>* init_indices = nullptr,
                                  int device = 0) {
    IVFFlatIndex ix;
    ix.device_ = device;
    check(vers_ivf_create(device, (uint32_t)N, &ix.h_));
    std::vector<uint64_t> draws;
    if (init_indices) draws = *init_indices;
    else {
      std::random_device rd;
      std::mt19937_64 rng(rd());
      draws.resize(num_attempts * num_clusters);
      for (auto& x : draws) x = vectors.empty() ? 0 : rng() % vectors.size();
    }
    // centroids are written straight into the Vec<Vector<N>> with ITS pitch (sizeof(Vector<N>) = round_up(4N, 256))
    std::vector<Vector<N>> cent(num_clusters);
    std::vector<uint64_t> asg(vectors.size() ? vectors.size() : 1);
    float cost = 0; int32_t kept = 0;
    check(vers_ivf_build(ix.h_, vectors.empty() ? nullptr : vectors[0].v, vectors.size(), sizeof(Vector<N>), num_clusters,
                         num_attempts, max_iterations, draws.data(), cent.empty() ? nullptr : cent[0].v, sizeof(Vector<N>),
                         asg.data(), &cost, &kept, nullptr));
    ix.num_centroids = num_clusters;
    ix.values = vectors;  // ivfflat.rs:131 vectors.clone()
    if (kept) {
      ix.centroids = std::move(cent);
      ix.assignments.assign(asg.begin(), asg.begin() + vectors.size());
    }  // else: nothing beat +inf -> empty centroids / assignments (ivfflat.rs:109-110)
    ix.ids.assign(num_clusters, {});
    for (size_t vec_id = 0; vec_id < ix.assignments.size(); ++vec_id) ix.ids[ix.assignments[vec_id]].push_back(vec_id);  // :123-127
    return ix;
  }

  // Index::add (ivfflat.rs:200-213): vec_id is accepted and ignored, like the reference (:209).
  void add(const Vector<N>& embedding, size_t /*vec_id*/) {
    uint64_t c = 0, id = 0;
    check(vers_ivf_add(handle(), embedding.v, &c, &id));
    values.push_back(embedding);
    assignments.push_back((size_t)c);
    ids[(size_t)c].push_back((size_t)id);
  }

  // add for many vectors in one call (vers_ivf_add_batch): the same fields as embeddings.size() calls of add.  On an error (a NaN
  // distance at row i) the rows before it are added, mirrored here, and the error is thrown.
  void add_batch(const std::vector<Vector<N>>& embeddings) {
    std::vector<uint64_t> cl(embeddings.size() ? embeddings.size() : 1);
    uint64_t first = 0, added = 0;
    const int32_t rc = vers_ivf_add_batch(handle(), embeddings.empty() ? nullptr : embeddings[0].v, embeddings.size(), sizeof(Vector<N>),
                                          cl.data(), &first, &added);
    for (uint64_t i = 0; i < added; ++i) {
      values.push_back(embeddings[i]);
      assignments.push_back((size_t)cl[i]);
      ids[(size_t)cl[i]].push_back((size_t)(first + i));
    }
    check(rc);
  }

  // Removal (extension, vers_ivf_remove_batch): ids[assignments[v]].retain(|&x| x != v) for every listed v.  values and assignments keep
  // their entries (positions are vec ids).  An id >= assignments.size() throws and removes nothing.  Returns the rows that left the index.
  size_t remove_batch(const std::vector<size_t>& vec_ids) {
    std::vector<uint64_t> v(vec_ids.begin(), vec_ids.end());
    uint64_t removed = 0;
    check(vers_ivf_remove_batch(handle(), v.data(), v.size(), &removed));
    size_t gone = 0;
    std::vector<bool> mark(assignments.size(), false);
    for (size_t x : vec_ids) mark[x] = true;
    for (auto& l : ids) {
      size_t w = 0;
      for (size_t x : l)
        if (!mark[x]) l[w++] = x;
      gone += l.size() - w;
      l.resize(w);
    }
    if (gone != removed) throw Panic(VERS_ERR_INVALID, "remove_batch: the device removed another number of rows than the host lists hold");
    return gone;
  }

  // Update (extension, vers_ivf_update_batch): values[v] = embeddings[i] for v = vec_ids[i], under the id the vector already has.  A row
  // whose first-minimum centroid is still its list keeps its position; one that changes cluster leaves its list and enters the new one at
  // its sorted place by vec id (every list stays ascending); an id that is in no list is skipped.  All or nothing: an id >=
  // assignments.size(), an id twice in the call or a NaN distance throws and nothing changes.  Returns the status per update
  // (0 stayed, 1 moved, 2 skipped).
  std::vector<uint8_t> update_batch(const std::vector<size_t>& vec_ids, const std::vector<Vector<N>>& embeddings) {
    if (vec_ids.size() != embeddings.size()) throw Panic(VERS_ERR_INVALID, "update_batch: one embedding per vec id");
    const size_t n = vec_ids.size();
    std::vector<uint64_t> v(vec_ids.begin(), vec_ids.end()), cl(n ? n : 1);
    std::vector<uint8_t> st(n ? n : 1);
    check(vers_ivf_update_batch(handle(), v.data(), n ? embeddings[0].v : nullptr, n, sizeof(Vector<N>), cl.data(), st.data(), nullptr));
    st.resize(n);
    for (size_t i = 0; i < n; ++i) {
      const size_t id = vec_ids[i], old = assignments[id], c = (size_t)cl[i];
      auto& from = ids[old];
      const auto at = std::lower_bound(from.begin(), from.end(), id);
      const bool listed = at != from.end() && *at == id;
      const uint8_t want = !listed ? 2 : c == old ? 0 : 1;
      if (st[i] != want) throw Panic(VERS_ERR_INVALID, "update_batch: the device's status differs from the host lists'");
      if (!listed) continue;
      values[id] = embeddings[i];
      if (c == old) continue;
      from.erase(at);
      assignments[id] = c;
      auto& to = ids[c];
      to.insert(std::lower_bound(to.begin(), to.end(), id), id);
    }
    return st;
  }

  // Compaction (extension, vers_ivf_compact): the device storage goes back to the capacities a fresh upload of the current lists plans and
  // the certificate maxima are recomputed; none of the five fields changes.  Returns {storage rows before, storage rows after}.
  std::pair<uint64_t, uint64_t> compact() {
    uint64_t before = 0, after = 0;
    check(vers_ivf_compact(handle(), &before, &after));
    return {before, after};
  }

  // Recluster (extension, vers_ivf_recluster): build_index over the vectors that are in some list, taken in ascending vec id (L), the vec ids
  // kept.  `init_indices` (optional) are POSITIONS in L, num_attempts * num_clusters of them; without it they are drawn as build_index draws
  // them.  When an attempt is kept, centroids, assignments (0 for an id in no list), ids and num_centroids follow the call's outputs; values,
  // assignments.size() and the live count do not change.  When none is kept nothing changes; a refusal throws and nothing changes.
  // Returns {cost, an attempt was kept}.
  std::pair<float, bool> recluster(size_t num_clusters, size_t num_attempts, size_t max_iterations, const std::vector<uint64_t>* init_indices = nullptr) {
    std::vector<size_t> live;
    for (const auto& l : ids) live.insert(live.end(), l.begin(), l.end());
    std::sort(live.begin(), live.end());
    std::vector<uint64_t> draws;
    if (init_indices) draws = *init_indices;
    else {
      std::random_device rd;
      std::mt19937_64 rng(rd());
      draws.resize(num_attempts * num_clusters);
      for (auto& x : draws) x = live.empty() ? 0 : rng() % live.size();
    }
    std::vector<Vector<N>> cent(num_clusters);
    std::vector<uint64_t> asg(assignments.size() ? assignments.size() : 1);
    float cost = 0; int32_t kept = 0;
    check(vers_ivf_recluster(handle(), num_clusters, num_attempts, max_iterations, draws.empty() ? nullptr : draws.data(), cent.empty() ? nullptr : cent[0].v,
                             sizeof(Vector<N>), asg.data(), &cost, &kept, nullptr));
    if (kept) {
      num_centroids = num_clusters;
      centroids = std::move(cent);
      assignments.assign(asg.begin(), asg.begin() + assignments.size());
      ids.assign(num_clusters, {});
      for (size_t v : live) ids[assignments[v]].push_back(v);  // ascending vec id: every list ascending
    }
    return {cost, kept != 0};
  }

  // Fetch (extension, vers_ivf_fetch): what the DEVICE holds under each listed vec id -- the stored vector, its cluster and a status (0 found,
  // 2 in no list: the vector is zeros, the cluster SIZE_MAX).  Any order, repeats allowed.  An id >= assignments.size() throws and nothing
  // is written.  The rows arrive with the pitch of Vec<Vector<N>>; the padding behind N floats is left as it is.
  struct Fetched {
    std::vector<Vector<N>> rows;
    std::vector<size_t> clusters;
    std::vector<uint8_t> status;
    size_t found = 0, in_no_list = 0;
  };
  Fetched fetch(const std::vector<size_t>& vec_ids) const {
    const size_t n = vec_ids.size();
    std::vector<uint64_t> v(vec_ids.begin(), vec_ids.end()), cl(n ? n : 1);
    Fetched f;
    f.rows.resize(n);
    f.status.resize(n ? n : 1);
    uint64_t counts[2] = {0, 0};
    check(vers_ivf_fetch(handle(), v.data(), n, n ? f.rows[0].v : nullptr, sizeof(Vector<N>), cl.data(), f.status.data(), counts));
    f.status.resize(n);
    f.clusters.assign(cl.begin(), cl.begin() + n);
    f.found = (size_t)counts[0];
    f.in_no_list = (size_t)counts[1];
    return f;
  }

  // Search by stored id (extension, vers_ivf_search_by_id): search with values[vec_id] as the query, which never leaves the device.
  // nprobe == 0: search_approximate's own semantics; exclude_self (nprobe >= 1): the result on the index without vec_id itself.  An id that
  // is in no list throws.
  std::vector<std::pair<size_t, float>> search_by_id(size_t vec_id, size_t top_k, size_t nprobe = 0, bool exclude_self = false) const {
    std::vector<uint64_t> oi(top_k ? top_k : 1);
    std::vector<float> od(top_k ? top_k : 1);
    uint32_t cnt = 0;
    const uint64_t v = vec_id;
    check(vers_ivf_search_by_id(handle(), &v, 1, (uint32_t)top_k, (uint32_t)nprobe, exclude_self ? VERS_BYID_EXCLUDE_SELF : 0u, oi.data(), od.data(), &cnt));
    std::vector<std::pair<size_t, float>> out;
    for (uint32_t i = 0; i < cnt; ++i) out.emplace_back((size_t)oi[i], od[i]);
    return out;
  }

  // vectors currently in the lists (vers_ivf_live_count)
  size_t live_count() const {
    uint64_t live = 0;
    check(vers_ivf_live_count(handle(), &live));
    return (size_t)live;
  }

  // Index::search_approximate (ivfflat.rs:153-198)
  std::vector<std::pair<size_t, float>> search_approximate(const Vector<N>& query, size_t top_k) const {
    std::vector<uint64_t> oi(top_k ? top_k : 1);
    std::vector<float> od(top_k ? top_k : 1);
    uint32_t cnt = 0;
    check(vers_ivf_search(handle(), query.v, sizeof(Vector<N>), 1, (uint32_t)top_k, 0 /* reference semantics */, oi.data(),
                          od.data(), &cnt));
    std::vector<std::pair<size_t, float>> out;
    for (uint32_t i = 0; i < cnt; ++i) out.emplace_back((size_t)oi[i], od[i]);
    return out;
  }

  // Range search (extension, vers_ivf_range_search): every row of the min(nprobe, k) nearest lists with distance <= radius, ascending by
  // (distance, probe rank, list position) -- the head of the nprobe mode's order; walk_order: probe rank, then list position.
  std::vector<std::pair<size_t, float>> range_search(const Vector<N>& query, float radius, size_t nprobe, bool walk_order = false) const {
    const uint32_t flags = walk_order ? VERS_RANGE_WALK_ORDER : 0u;
    uint64_t lims[2] = {0, 0}, total = 0;
    check(vers_ivf_range_search(handle(), query.v, sizeof(Vector<N>), 1, &radius, (uint32_t)nprobe, flags, lims, nullptr, nullptr, 0, &total));  // size query
    std::vector<uint64_t> oi(total ? total : 1);
    std::vector<float> od(total ? total : 1);
    if (total) check(vers_ivf_range_search(handle(), query.v, sizeof(Vector<N>), 1, &radius, (uint32_t)nprobe, flags, lims, oi.data(), od.data(), total, &total));
    std::vector<std::pair<size_t, float>> out;
    for (uint64_t i = 0; i < total && i < oi.size(); ++i) out.emplace_back((size_t)oi[i], od[i]);
    return out;
  }

  // Exhaustive range search (extension, vers_ivf_range_search_exhaustive): EVERY row in a list now with distance <= radius under `metric`,
  // ascending by (distance, vec id) -- the head of utils::search_exhaustive's order; walk_order: list by list, ascending list position.
  std::vector<std::pair<size_t, float>> range_search_exhaustive(const Vector<N>& query, float radius, uint32_t metric = VERS_METRIC_L2SQ,
                                                                bool walk_order = false) const {
    const uint32_t flags = walk_order ? VERS_RANGE_WALK_ORDER : 0u;
    uint64_t lims[2] = {0, 0}, total = 0;
    check(vers_ivf_range_search_exhaustive(handle(), query.v, sizeof(Vector<N>), 1, &radius, metric, flags, lims, nullptr, nullptr, 0, &total));  // size query
    std::vector<uint64_t> oi(total ? total : 1);
    std::vector<float> od(total ? total : 1);
    if (total) check(vers_ivf_range_search_exhaustive(handle(), query.v, sizeof(Vector<N>), 1, &radius, metric, flags, lims, oi.data(), od.data(), total, &total));
    std::vector<std::pair<size_t, float>> out;
    for (uint64_t i = 0; i < total && i < oi.size(); ++i) out.emplace_back((size_t)oi[i], od[i]);
    return out;
  }

  // Filtered search (extension, vers_ivf_search_filtered): the top_k nearest among the allowed rows of the min(nprobe, k) nearest lists,
  // nprobe >= 1 -- what search over those lists returns once every vec id with allowed[v] == false (or v >= allowed.size()) has been
  // removed; the index is not touched.  Ascending by (distance, probe rank, list position); fewer than top_k entries when fewer are allowed.
  std::vector<std::pair<size_t, float>> search_filtered(const Vector<N>& query, size_t top_k, size_t nprobe, const std::vector<bool>& allowed) const {
    const std::vector<uint64_t> bits = allowed_bitmap(allowed);
    std::vector<uint64_t> oi(top_k ? top_k : 1);
    std::vector<float> od(top_k ? top_k : 1);
    uint32_t cnt = 0;
    check(vers_ivf_search_filtered(handle(), query.v, sizeof(Vector<N>), 1, (uint32_t)top_k, (uint32_t)nprobe, bits.data(), allowed.size(), oi.data(), od.data(),
                                   &cnt));
    std::vector<std::pair<size_t, float>> out;
    for (uint32_t i = 0; i < cnt; ++i) out.emplace_back((size_t)oi[i], od[i]);
    return out;
  }

  // Filtered search to an adaptive depth (extension, vers_ivf_search_filtered_adaptive): search_filtered(query, top_k, P, allowed) with P the
  // smallest depth in [min(nprobe_min, k), min(nprobe_max, k)] whose lists hold min_allowed allowed rows, or the upper end when none does;
  // *depth (nullable) receives P.
  std::vector<std::pair<size_t, float>> search_filtered_adaptive(const Vector<N>& query, size_t top_k, size_t nprobe_min, size_t nprobe_max, size_t min_allowed,
                                                                 const std::vector<bool>& allowed, size_t* depth = nullptr) const {
    const std::vector<uint64_t> bits = allowed_bitmap(allowed);
    std::vector<uint64_t> oi(top_k ? top_k : 1);
    std::vector<float> od(top_k ? top_k : 1);
    uint32_t cnt = 0, np = 0;
    check(vers_ivf_search_filtered_adaptive(handle(), query.v, sizeof(Vector<N>), 1, (uint32_t)top_k, (uint32_t)nprobe_min, (uint32_t)nprobe_max,
                                            (uint32_t)min_allowed, bits.data(), allowed.size(), oi.data(), od.data(), &cnt, &np));
    if (depth) *depth = np;
    std::vector<std::pair<size_t, float>> out;
    for (uint32_t i = 0; i < cnt; ++i) out.emplace_back((size_t)oi[i], od[i]);
    return out;
  }

  // Exhaustive filtered search (extension, vers_ivf_search_exhaustive_filtered): the top_k nearest among the allowed rows that are in a list
  // now, under `metric`, ascending by (distance, vec id).
  std::vector<std::pair<size_t, float>> search_exhaustive_filtered(const Vector<N>& query, size_t top_k, const std::vector<bool>& allowed,
                                                                   uint32_t metric = VERS_METRIC_L2SQ) const {
    const std::vector<uint64_t> bits = allowed_bitmap(allowed);
    std::vector<uint64_t> oi(top_k ? top_k : 1);
    std::vector<float> od(top_k ? top_k : 1);
    uint32_t cnt = 0;
    check(vers_ivf_search_exhaustive_filtered(handle(), query.v, sizeof(Vector<N>), 1, (uint32_t)top_k, metric, bits.data(), allowed.size(), oi.data(),
                                              od.data(), &cnt));
    std::vector<std::pair<size_t, float>> out;
    for (uint32_t i = 0; i < cnt; ++i) out.emplace_back((size_t)oi[i], od[i]);
    return out;
  }

  // Filtered range search (extension, vers_ivf_range_search_filtered): range_search over the lists once every vec id with allowed[v] == false
  // (or v >= allowed.size()) has been removed; the index is not touched.  Order as range_search.
  std::vector<std::pair<size_t, float>> range_search_filtered(const Vector<N>& query, float radius, size_t nprobe, const std::vector<bool>& allowed,
                                                              bool walk_order = false) const {
    const std::vector<uint64_t> bits = allowed_bitmap(allowed);
    const uint32_t flags = walk_order ? VERS_RANGE_WALK_ORDER : 0u;
    uint64_t lims[2] = {0, 0}, total = 0;
    check(vers_ivf_range_search_filtered(handle(), query.v, sizeof(Vector<N>), 1, &radius, (uint32_t)nprobe, flags, bits.data(), allowed.size(), lims, nullptr,
                                         nullptr, 0, &total));  // size query
    std::vector<uint64_t> oi(total ? total : 1);
    std::vector<float> od(total ? total : 1);
    if (total)
      check(vers_ivf_range_search_filtered(handle(), query.v, sizeof(Vector<N>), 1, &radius, (uint32_t)nprobe, flags, bits.data(), allowed.size(), lims, oi.data(),
                                           od.data(), total, &total));
    std::vector<std::pair<size_t, float>> out;
    for (uint64_t i = 0; i < total && i < oi.size(); ++i) out.emplace_back((size_t)oi[i], od[i]);
    return out;
  }

  // Exhaustive filtered range search (extension, vers_ivf_range_search_exhaustive_filtered): every allowed row in a list now with distance <=
  // radius under `metric`.  Order as range_search_exhaustive.
  std::vector<std::pair<size_t, float>> range_search_exhaustive_filtered(const Vector<N>& query, float radius, const std::vector<bool>& allowed,
                                                                         uint32_t metric = VERS_METRIC_L2SQ, bool walk_order = false) const {
    const std::vector<uint64_t> bits = allowed_bitmap(allowed);
    const uint32_t flags = walk_order ? VERS_RANGE_WALK_ORDER : 0u;
    uint64_t lims[2] = {0, 0}, total = 0;
    check(vers_ivf_range_search_exhaustive_filtered(handle(), query.v, sizeof(Vector<N>), 1, &radius, metric, flags, bits.data(), allowed.size(), lims, nullptr,
                                                    nullptr, 0, &total));  // size query
    std::vector<uint64_t> oi(total ? total : 1);
    std::vector<float> od(total ? total : 1);
    if (total)
      check(vers_ivf_range_search_exhaustive_filtered(handle(), query.v, sizeof(Vector<N>), 1, &radius, metric, flags, bits.data(), allowed.size(), lims, oi.data(),
                                                      od.data(), total, &total));
    std::vector<std::pair<size_t, float>> out;
    for (uint64_t i = 0; i < total && i < oi.size(); ++i) out.emplace_back((size_t)oi[i], od[i]);
    return out;
  }

  // allowed[v] -> the u64 words of the C ABI: bit (v & 63) of word (v >> 6); at least one word, so that the array has an address
  static std::vector<uint64_t> allowed_bitmap(const std::vector<bool>& allowed) {
    std::vector<uint64_t> bits((allowed.size() + 63) / 64 + 1, 0);
    for (size_t v = 0; v < allowed.size(); ++v)
      if (allowed[v]) bits[v >> 6] |= 1ull << (v & 63);
    return bits;
  }

  // Index::save_index (base.rs:31-43): bincode 1.3 default options -- LE, u64 lengths, fields in order, no tags
  void save_index(const std::string& path) const {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("save_index: cannot create " + path);
    auto u64 = [&](uint64_t x) { std::fwrite(&x, 8, 1, f); };
    u64(num_centroids);
    u64(values.size());
    for (auto& r : values) std::fwrite(r.v, sizeof(float), N, f);
    u64(centroids.size());
    for (auto& r : centroids) std::fwrite(r.v, sizeof(float), N, f);
    u64(assignments.size());
    for (size_t a : assignments) u64(a);
    u64(ids.size());
    for (auto& l : ids) { u64(l.size()); for (size_t x : l) u64(x); }
    std::fclose(f);
  }

  // Index::load_index (base.rs:45-58); the device cache is rebuilt on first use
  static IVFFlatIndex load_index(const std::string& path, int device = 0) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("load_index: cannot open " + path);
    auto u64 = [&]() { uint64_t x = 0; if (std::fread(&x, 8, 1, f) != 1) { std::fclose(f); throw std::runtime_error("Deserialization error: unexpected end of file"); } return x; };
    auto rows = [&](std::vector<Vector<N>>& m) { m.resize(u64()); for (auto& r : m) if (std::fread(r.v, sizeof(float), N, f) != N) { std::fclose(f); throw std::runtime_error("Deserialization error: unexpected end of file"); } };
    IVFFlatIndex ix;
    ix.device_ = device;
    ix.num_centroids = u64();
    rows(ix.values);
    rows(ix.centroids);
    ix.assignments.resize(u64());
    for (auto& a : ix.assignments) a = u64();
    ix.ids.resize(u64());
    for (auto& l : ix.ids) { l.resize(u64()); for (auto& x : l) x = u64(); }
    std::fclose(f);
    return ix;
  }

 private:
  mutable vers_ivf_t* h_ = nullptr;
  int device_ = 0;
  vers_ivf_t* handle() const {  // after load_index: upload the host fields once
    if (!h_) {
      check(vers_ivf_create(device_, (uint32_t)N, &h_));
      std::vector<uint64_t> a(assignments.begin(), assignments.end());
      check(vers_ivf_upload(h_, values.empty() ? nullptr : values[0].v, values.size(), sizeof(Vector<N>),
                            centroids.empty() ? nullptr : centroids[0].v, centroids.size(), sizeof(Vector<N>), a.data()));
      // vers_ivf_upload implies ids[c] = every position with assignments == c: positions missing from the loaded lists were removed
      // before the index was saved and leave the cache again (none in a file the reference wrote)
      std::vector<bool> in_list(assignments.size(), false);
      for (auto& l : ids)
        for (size_t x : l)
          if (x < in_list.size()) in_list[x] = true;
      std::vector<uint64_t> gone;
      for (size_t v = 0; v < in_list.size(); ++v)
        if (!in_list[v]) gone.push_back(v);
      if (!gone.empty() && !centroids.empty()) check(vers_ivf_remove_batch(h_, gone.data(), gone.size(), nullptr));
    }
    return h_;
  }
};

// utils::search_exhaustive (utils.rs:68-82)
template <size_t N>
std::vector<std::pair<size_t, float>> search_exhaustive(const std::vector<Vector<N>>& data, const Vector<N>& query, size_t top_k,
                                                        int device = 0) {
  vers_flat_t* h = nullptr;
  check(vers_flat_create(device, (uint32_t)N, &h));
  std::vector<uint64_t> oi(top_k ? top_k : 1);
  std::vector<float> od(top_k ? top_k : 1);
  uint32_t cnt = 0;
  int32_t rc = vers_flat_upload(h, data.empty() ? nullptr : data[0].v, data.size(), sizeof(Vector<N>));
  if (rc == VERS_OK) rc = vers_flat_search(h, query.v, sizeof(Vector<N>), 1, (uint32_t)top_k, VERS_METRIC_L2SQ, oi.data(), od.data(), &cnt);
  vers_flat_destroy(h);
  check(rc);
  std::vector<std::pair<size_t, float>> out;
  for (uint32_t i = 0; i < cnt; ++i) out.emplace_back((size_t)oi[i], od[i]);
  return out;
}

}  // namespace vers
