// Marginalizing node removal of the pose-graph SPA solver (kh_spa_marginalize_nodes): the constraints of a leaving node composed
// through it, a round of nodes per launch (marginalize.hip, marginalize.hpp).  A round is packed on the host,
// run on the device and applied to the graph store; nothing of a round is applied unless all of it can be.
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_set>

#include "spa_private.hpp"

using namespace kh;
using namespace kh::spa;

namespace
{
// the live constraints of node v, grouped by neighbour in the order of v's first constraint to each: nb[i] and, flat,
// ks[kp[i] .. kp[i + 1]).  Returns the number of neighbours, or cap + 1 as soon as there are more than cap.
int32_t neighbour_entries(const kh_spa * s, int32_t v, int32_t cap, std::vector<int32_t> & nb, std::vector<int32_t> & kp, std::vector<int32_t> & ks)
{
  nb.clear(); kp.assign(1, 0); ks.clear();
  auto inc = s->incident.find(v);
  if (inc == s->incident.end()) {return 0;}
  // (two passes over a short list: the neighbours first, then each one's constraints, so that ks comes out grouped)
  for (int32_t k : inc->second) {
    const Constraint & c = s->cons[k];
    if (c.dead) {continue;}
    const int32_t o = c.a == v ? c.b : c.a;
    if (std::find(nb.begin(), nb.end(), o) == nb.end()) {
      if (static_cast<int32_t>(nb.size()) == cap) {return cap + 1;}
      nb.push_back(o);
    }
  }
  for (int32_t o : nb) {
    for (int32_t k : inc->second) {
      const Constraint & c = s->cons[k];
      if (!c.dead && (c.a == v ? c.b : c.a) == o) {ks.push_back(k);}
    }
    kp.push_back(static_cast<int32_t>(ks.size()));
  }
  return static_cast<int32_t>(nb.size());
}

// everything that can be refused is refused on the graph as it stands, before the first edit
int check_listed_nodes(const kh_spa * s, int32_t n, const int32_t * ids)
{
  std::vector<int32_t> nb, kp, ks;
  std::unordered_set<int32_t> seen;
  for (int32_t i = 0; i < n; ++i) {
    const int32_t id = ids[i];
    if (!s->index_of.count(id)) {set_error("kh_spa_marginalize_nodes: no node " + std::to_string(id)); return KH_ERR_NOT_FOUND;}
    if (!seen.insert(id).second) {set_error("kh_spa_marginalize_nodes: node " + std::to_string(id) + " is listed twice"); return KH_ERR_INVALID_ARG;}
    if (s->has_first && id == s->first_id) {
      set_error("kh_spa_marginalize_nodes: node " + std::to_string(id) + " is the gauge node, which cannot be handed on");
      return KH_ERR_INVALID_ARG;
    }
    if (neighbour_entries(s, id, kMargMaxDegree, nb, kp, ks) > kMargMaxDegree) {
      set_error("kh_spa_marginalize_nodes: node " + std::to_string(id) + " has more than 64 neighbours");
      return KH_ERR_INVALID_ARG;
    }
  }
  return KH_OK;
}

// A round, packed: per member (list order) its id and, for those that go to the device, their number there (-1: plain removal);
// the device's input as marginalize.hpp lays it out; the device's answer.  The vectors keep their capacity from round to round.
struct Round
{
  std::vector<int32_t> member, member_dev;
  std::vector<int32_t> ent_ptr, ent_id, con_ptr, con_dir, pair_ptr, pair_ent, pair_con, out_ptr, ints;
  std::vector<double> dbl, pair_dbl;
  std::vector<char> blob, result;
  int32_t n_dev() const {return static_cast<int32_t>(ent_ptr.size()) - 1;}
  int32_t n_out() const {return out_ptr.back();}
};

// The nodes of `pending` whose closed neighbourhoods are disjoint become the round, the others go to `waiting` in their order.
int pack_round(const kh_spa * s, const std::vector<int32_t> & pending, Round & r, std::vector<int32_t> & waiting, kh_marginalize_summary & sum)
{
  std::vector<int32_t> nb, kp, ks;
  std::unordered_set<int32_t> blocked;
  r.member.clear(); r.member_dev.clear(); waiting.clear();
  r.ent_ptr.assign(1, 0); r.ent_id.clear(); r.con_ptr.assign(1, 0); r.con_dir.clear(); r.pair_ptr.assign(1, 0); r.pair_ent.clear(); r.pair_con.clear();
  r.out_ptr.assign(1, 0); r.dbl.clear(); r.pair_dbl.clear();
  auto put9 = [](std::vector<double> & to, const Constraint & c) {
    to.insert(to.end(), c.z, c.z + 3);
    to.insert(to.end(), c.omega, c.omega + 6);
  };
  for (int32_t v : pending) {
    const int32_t d = neighbour_entries(s, v, kMargMaxDegree, nb, kp, ks);
    if (d > kMargMaxDegree) {
      set_error("kh_spa_marginalize_nodes: node " + std::to_string(v) + " has grown past 64 neighbours through the nodes listed before it");
      return KH_ERR_INVALID_ARG;
    }
    // the node waits when its closed neighbourhood meets that of an earlier node of this pass, in the round or waiting itself
    bool meets = blocked.count(v) != 0;
    for (int32_t o : nb) {meets = meets || blocked.count(o) != 0;}
    blocked.insert(v);
    blocked.insert(nb.begin(), nb.end());
    if (meets) {waiting.push_back(v); continue;}
    sum.max_degree = std::max(sum.max_degree, d);
    r.member.push_back(v);
    if (d < 2) {r.member_dev.push_back(-1); continue;}
    r.member_dev.push_back(r.n_dev());
    for (int32_t i = 0; i < d; ++i) {
      r.ent_id.push_back(nb[i]);
      for (int32_t q = kp[i]; q < kp[i + 1]; ++q) {
        const Constraint & c = s->cons[ks[q]];
        r.con_dir.push_back(c.a == v ? 0 : 1);
        put9(r.dbl, c);
      }
      r.con_ptr.push_back(static_cast<int32_t>(r.con_dir.size()));
    }
    // the first existing constraint of every pair of neighbours (the host knows the topology, not the hub)
    const size_t pair_begin = r.pair_ent.size();
    for (int32_t i = 0; i < d; ++i) {
      auto inc = s->incident.find(nb[i]);
      if (inc == s->incident.end()) {continue;}
      for (int32_t k : inc->second) {
        const Constraint & c = s->cons[k];
        if (c.dead) {continue;}
        const int32_t o = c.a == nb[i] ? c.b : c.a;
        if (o == v) {continue;}
        const int32_t j = static_cast<int32_t>(std::find(nb.begin(), nb.end(), o) - nb.begin());
        if (j >= d || j <= i) {continue;}
        const int32_t key = i | (j << 8);
        bool known = false;
        for (size_t p = pair_begin; p < r.pair_ent.size(); ++p) {known = known || (r.pair_ent[p] & 0xffff) == key;}
        if (known) {continue;}
        r.pair_ent.push_back(key | ((c.a == nb[i] ? 0 : 1) << 16));
        r.pair_con.push_back(k);
        put9(r.pair_dbl, c);
      }
    }
    r.ent_ptr.push_back(static_cast<int32_t>(r.ent_id.size()));
    r.pair_ptr.push_back(static_cast<int32_t>(r.pair_ent.size()));
    r.out_ptr.push_back(r.out_ptr.back() + d - 1);
  }
  return KH_OK;
}

// One upload (the doubles -- incident constraints, then pairs -- then the index arrays), one launch, one download into r.result.
int run_round(kh_spa * s, Round & r, kh_marginalize_summary & sum, std::chrono::steady_clock::time_point t_pack)
{
  hipStream_t st = s->stream;
  const int32_t n_dev = r.n_dev(), n_out = r.n_out();
  const size_t n_con = r.con_dir.size(), n_ent = r.ent_id.size();
  r.dbl.insert(r.dbl.end(), r.pair_dbl.begin(), r.pair_dbl.end());
  r.ints.clear();
  const size_t o_ent_ptr = 0, o_out_ptr = o_ent_ptr + n_dev + 1, o_pair_ptr = o_out_ptr + n_dev + 1, o_ent_id = o_pair_ptr + n_dev + 1,
    o_con_ptr = o_ent_id + n_ent, o_con_dir = o_con_ptr + n_ent + 1, o_pair_ent = o_con_dir + n_con;
  r.ints.insert(r.ints.end(), r.ent_ptr.begin(), r.ent_ptr.end());
  r.ints.insert(r.ints.end(), r.out_ptr.begin(), r.out_ptr.end());
  r.ints.insert(r.ints.end(), r.pair_ptr.begin(), r.pair_ptr.end());
  r.ints.insert(r.ints.end(), r.ent_id.begin(), r.ent_id.end());
  r.ints.insert(r.ints.end(), r.con_ptr.begin(), r.con_ptr.end());
  r.ints.insert(r.ints.end(), r.con_dir.begin(), r.con_dir.end());
  r.ints.insert(r.ints.end(), r.pair_ent.begin(), r.pair_ent.end());
  const size_t dbl_bytes = r.dbl.size() * sizeof(double), int_bytes = r.ints.size() * sizeof(int32_t);
  r.blob.resize(dbl_bytes + int_bytes);
  std::memcpy(r.blob.data(), r.dbl.data(), dbl_bytes);
  std::memcpy(r.blob.data() + dbl_bytes, r.ints.data(), int_bytes);
  const size_t out_dbl_bytes = static_cast<size_t>(n_out) * 9 * sizeof(double), out_bytes = out_dbl_bytes + static_cast<size_t>(n_out) * 2 * sizeof(int32_t);
  sum.pack_ms += ms_since(t_pack);
  const auto t_kernel = std::chrono::steady_clock::now();
  int rc = s->d_marg_in.ensure(r.blob.size());
  if (rc) {return rc;}
  rc = s->d_marg_out.ensure(out_bytes);
  if (rc) {return rc;}
  KS_HIP(hipMemcpyAsync(s->d_marg_in.p, r.blob.data(), r.blob.size(), hipMemcpyHostToDevice, st));
  const double * dd = reinterpret_cast<const double *>(s->d_marg_in.p);
  const int32_t * di = reinterpret_cast<const int32_t *>(s->d_marg_in.p + dbl_bytes);
  MargDev g;
  g.n_nodes = n_dev;
  g.ent_ptr = di + o_ent_ptr; g.out_ptr = di + o_out_ptr; g.pair_ptr = di + o_pair_ptr; g.ent_id = di + o_ent_id;
  g.con_ptr = di + o_con_ptr; g.con_dir = di + o_con_dir; g.pair_ent = di + o_pair_ent;
  g.con_d = dd; g.pair_d = dd + 9 * n_con;
  g.out_d = reinterpret_cast<double *>(s->d_marg_out.p);
  g.out_i = reinterpret_cast<int32_t *>(s->d_marg_out.p + out_dbl_bytes);
  marginalize_launch_round(g, st);
  KS_HIP(hipGetLastError());
  r.result.resize(out_bytes);
  KS_HIP(hipMemcpyAsync(r.result.data(), s->d_marg_out.p, out_bytes, hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));
  sum.kernel_ms += ms_since(t_kernel);
  return KH_OK;
}

// The round's edits to the graph store, recorded in s->marg_edits in the order they are made: per member the composed constraints
// (fused into an existing one, or added), then the node's removal.
int apply_round(kh_spa * s, const Round & r, kh_marginalize_summary & sum)
{
  const int32_t n_dev = r.n_dev(), n_out = r.n_out();
  const size_t n_pair = r.pair_ent.size();
  const double * out_d = reinterpret_cast<const double *>(r.result.data());
  const int32_t * out_i = reinterpret_cast<const int32_t *>(r.result.data() + static_cast<size_t>(n_out) * 9 * sizeof(double));
  // nothing of the round is applied unless all of it can be: every result finite, every information positive definite
  for (int32_t q = 0; q < (n_dev > 0 ? n_out : 0); ++q) {
    double u[9];
    sqrt_information(out_d + 9 * q + 3, u);
    bool ok = u[0] > 0.0 && u[4] > 0.0 && u[8] > 0.0;
    for (int k = 0; k < 3; ++k) {ok = ok && std::isfinite(out_d[9 * q + k]);}
    if (!ok) {
      set_error("kh_spa_marginalize_nodes: a composed constraint is not finite or its information is not positive definite");
      return KH_ERR_SOLVER;
    }
  }
  for (size_t w = 0; w < r.member.size(); ++w) {
    const int32_t v = r.member[w], dev = r.member_dev[w];
    MargEdit ed;
    std::memset(&ed, 0, sizeof(ed));
    ed.via = v;
    if (dev >= 0) {
      const int32_t d = r.ent_ptr[dev + 1] - r.ent_ptr[dev];
      for (int32_t row = 0; row < d - 1; ++row) {
        const int32_t q = r.out_ptr[dev] + row;
        const int32_t h = out_i[2 * q], p = out_i[2 * q + 1];
        if (h < 0 || h >= d || p < -1 || p >= static_cast<int32_t>(n_pair)) {set_error("kh_spa_marginalize_nodes: the device returned an index out of range"); return KH_ERR_SOLVER;}
        const int32_t i = row < h ? row : row + 1;
        const double * z = out_d + 9 * q; const double * omega = z + 3;
        std::copy(z, z + 3, ed.z); std::copy(omega, omega + 6, ed.omega);
        if (p >= 0) {
          Constraint & c = s->cons[r.pair_con[p]];
          std::copy(z, z + 3, c.z); std::copy(omega, omega + 6, c.omega);
          sqrt_information(c.omega, c.u);
          ed.kind = 1; ed.a = c.a; ed.b = c.b;
          ++sum.n_fused;
        } else {
          ed.kind = 0; ed.a = r.ent_id[r.ent_ptr[dev] + h]; ed.b = r.ent_id[r.ent_ptr[dev] + i];
          const int rc = add_constraint_information(s, ed.a, ed.b, z, omega);
          if (rc) {return rc;}
          ++sum.n_added;
        }
        s->marg_edits.push_back(ed);
      }
      ++sum.n_marginalized;
    } else {
      ++sum.n_plain;
    }
    ed.kind = 2; ed.a = ed.b = v;
    s->marg_edits.push_back(ed);
    remove_found_node(s, s->index_of.find(v));
  }
  s->cov_valid = false;
  s->topology_dirty = true;
  return KH_OK;
}
}  // namespace

extern "C" int kh_spa_marginalize_nodes(kh_spa * s, int32_t n, const int32_t * ids, kh_marginalize_summary * summary)
{
  if (s) {s->marg_edits.clear();}                        // (whatever the call answers, the edits on record are its own)
  if (n < 0 || (n > 0 && !ids)) {return KH_ERR_INVALID_ARG;}
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!s) {return KH_ERR_INVALID_ARG;}
  kh_marginalize_summary sum;
  std::memset(&sum, 0, sizeof(sum));
  const auto t_begin = std::chrono::steady_clock::now();
  auto finish = [&](int rc) {sum.total_ms = ms_since(t_begin); if (summary) {*summary = sum;} return rc;};
  int rc = check_listed_nodes(s, n, ids);
  if (rc) {return finish(rc);}
  KS_HIP(hipSetDevice(s->device));
  std::vector<int32_t> pending(ids, ids + n), waiting;
  Round round;
  while (!pending.empty()) {
    const auto t_pack = std::chrono::steady_clock::now();
    ++sum.n_rounds;
    rc = pack_round(s, pending, round, waiting, sum);
    if (rc) {return finish(rc);}
    if (round.n_dev() > 0) {
      rc = run_round(s, round, sum, t_pack);
      if (rc) {return finish(rc);}
    } else {
      sum.pack_ms += ms_since(t_pack);
    }
    const auto t_apply = std::chrono::steady_clock::now();
    rc = apply_round(s, round, sum);
    if (rc) {return finish(rc);}
    sum.apply_ms += ms_since(t_apply);
    pending.swap(waiting);
  }
  return finish(KH_OK);
}

namespace kh
{
// what the last kh_spa_marginalize_nodes did, edit by edit (the mapper mirrors it in its own topology)
const std::vector<MargEdit> & spa_marginalize_edits(const kh_spa * s) {return s->marg_edits;}
// whether kh_spa_marginalize_nodes would refuse the node on the graph as it stands (unknown, the gauge, more than 64 neighbours)
bool spa_marginalize_refuses(const kh_spa * s, int32_t id)
{
  if (!s->index_of.count(id) || (s->has_first && id == s->first_id)) {return true;}
  std::vector<int32_t> nb, kp, ks;
  return neighbour_entries(s, id, kMargMaxDegree, nb, kp, ks) > kMargMaxDegree;
}
}  // namespace kh
