// Covariances of the pose-graph SPA solver (hot path B): Sigma = (J^T J)^-1 on the pattern of H from the selected inverse of the
// factor, block columns of Sigma for query nodes, their getters, and the constraint audit that reads them (DESIGN.md sections 7e, 7g and 7i).
// All numeric work runs on the GPU (spa_selinv.hip, spa_cov_columns.hip, spa_audit.hip); the columns' plan is covariance_columns_plan.hpp's.
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>

#include "spa_private.hpp"

using namespace kh;
using namespace kh::spa;

namespace
{
// how every getter opens: its own argument check, then the device, then the handle
int enter(bool args_ok, const kh_spa * s)
{
  if (!args_ok) {return KH_ERR_INVALID_ARG;}
  if (require_device(0) != KH_OK) {return KH_ERR_NO_DEVICE;}
  if (!s) {return KH_ERR_INVALID_ARG;}
  return KH_OK;
}

// `pass`: the call that would have had to run
int stale(const char * pass)
{
  set_error(std::string("kh_spa: the covariances are stale (the graph or a pose has changed since ") + pass + ", or it never ran)");
  return KH_ERR_SOLVER;
}

// a getter's list of nodes: ids[0 .. n), or without ids all nodes in insertion order
int check_listed(const kh_spa * s, const char * who, int32_t n, const int32_t * ids)
{
  if (!ids && n != static_cast<int32_t>(s->nodes.size())) {
    set_error(std::string(who) + ": without ids, n must be kh_spa_num_nodes");
    return KH_ERR_INVALID_ARG;
  }
  return KH_OK;
}

// block (p, q) of the 6 x 6 joint covariance <- the 3 x 3 block blk, or its transpose
void place_block(double cov[36], int p, int q, const double * blk, bool transposed = false)
{
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {cov[(3 * p + r) * 6 + 3 * q + c] = transposed ? blk[3 * c + r] : blk[3 * r + c];}
  }
}

// What the last covariance pass left resident on the device, as far as the getters' kernels and the audit read it: the sizes, the
// edge arrays, the free numbering and the BSR pattern.  (The pass left the analysis, the edge arrays and the poses it linearised at
// -- d_x -- on the device: cov_valid falls with every change of the graph or of a pose.)
SpaDev resident_view(const kh_spa * s)
{
  SpaDev dev;
  std::memset(&dev, 0, sizeof(dev));
  dev.n_nodes = static_cast<int32_t>(s->nodes.size()); dev.n_free = static_cast<int32_t>(s->node_of_free.size());
  dev.n_edges = static_cast<int32_t>(s->cons.size());
  dev.edge_a = s->d_edge_a.p; dev.edge_b = s->d_edge_b.p; dev.edge_z = s->d_edge_z.p; dev.edge_u = s->d_edge_u.p;
  dev.free_of_node = s->d_free_of_node.p; dev.node_of_free = s->d_node_of_free.p;
  dev.n_slots = s->n_slots; dev.bsr_row_ptr = s->d_bsr_row_ptr.p; dev.bsr_col = s->d_bsr_col.p; dev.bsr_diag_slot = s->d_bsr_diag.p;
  return dev;
}

// ---- the stages of the covariance pass ----
// Every free node must reach the gauge node through constraints, or J^T J is singular.  Checked on the graph itself: the
// last pivot of a floating component is zero only up to rounding, so the fail word of the factorisation (checked after the launches
// as well) sees it only when the rounding falls that way.
int check_tied_to_gauge(const kh_spa * s, const std::string & who)
{
  const int32_t nf = static_cast<int32_t>(s->node_of_free.size());
  std::vector<int32_t> root(nf);
  for (int32_t f = 0; f < nf; ++f) {root[f] = f;}
  auto find = [&](int32_t f) {while (root[f] != f) {root[f] = root[root[f]]; f = root[f];} return f;};
  std::vector<uint8_t> tied(nf, 0);
  for (size_t e = 0; e < s->cached_ea.size(); ++e) {
    const int32_t fa = s->free_of_node[s->cached_ea[e]], fb = s->free_of_node[s->cached_eb[e]];
    if (fa >= 0 && fb >= 0) {root[find(fa)] = find(fb);}
  }
  for (size_t e = 0; e < s->cached_ea.size(); ++e) {
    const int32_t pa = s->cached_ea[e], pb = s->cached_eb[e];
    if (pa == s->fixed_index && s->free_of_node[pb] >= 0) {tied[find(s->free_of_node[pb])] = 1;}
    if (pb == s->fixed_index && s->free_of_node[pa] >= 0) {tied[find(s->free_of_node[pa])] = 1;}
  }
  for (int32_t f = 0; f < nf; ++f) {
    if (!tied[find(f)]) {
      set_error(who + ": node " + std::to_string(s->nodes[s->node_of_free[f]].id) +
        " belongs to a free component of the graph that is not tied to the gauge node: J^T J is singular");
      return KH_ERR_SOLVER;
    }
  }
  return KH_OK;
}

// The columns' plan: the fronts of every level on the union of the paths from a query's front to its root, and which queries
// each carries; [query -> elimination position | the levels' lists] go to the device in one piece.  R: the right-hand sides' padded
// width; col_level_off[l]: where level l's list begins in the lists.
int plan_and_upload_columns(kh_spa * s, const SpaDev & dev, const std::string & who, const std::vector<int32_t> & query_free, int32_t R,
                            std::vector<int32_t> & col_level_off, kh_spa_cov_columns_summary & csum)
{
  const Symbolic & sym = s->sym;
  const int n_levels = static_cast<int>(sym.levels.size());
  const int32_t n_queries = static_cast<int32_t>(query_free.size());
  col_level_off.assign(n_levels + 1, n_queries);
  if (n_queries == 0) {return KH_OK;}
  if (!plan_covariance_columns(sym.parent, sym.level, n_levels, sym.sn_of_elim, sym.elim_of_free, query_free, s->col_plan)) {
    set_error(who + ": the queries do not fit the analysis");
    return KH_ERR_SOLVER;
  }
  const CovColumnsPlan & plan = s->col_plan;
  s->h_col_lists.clear();
  for (int32_t k = 0; k < n_queries; ++k) {s->h_col_lists.push_back(query_free[k] < 0 ? -1 : sym.elim_of_free[query_free[k]]);}
  for (int l = 0; l < n_levels; ++l) {
    col_level_off[l] = static_cast<int32_t>(s->h_col_lists.size());
    s->h_col_lists.insert(s->h_col_lists.end(), plan.level_fronts[l].begin(), plan.level_fronts[l].end());
  }
  col_level_off[n_levels] = static_cast<int32_t>(s->h_col_lists.size());
  csum.n_queries = n_queries; csum.path_fronts = plan.n_path_fronts;
  for (int32_t k = 0; k < sym.n_fronts; ++k) {
    const int64_t ns = sym.front_ns[k], nu = sym.front_m[k] - ns;
    csum.column_flops += (ns * ns + 2 * nu * ns) * R * (plan.front_mask[k] ? 2 : 1);
  }
  if (s->d_col_rhs.ensure(3 * static_cast<size_t>(dev.n_free) * R + 16) || s->d_columns.ensure(9 * static_cast<size_t>(dev.n_free) * n_queries + 16) ||
      s->d_col_lists.upload(s->h_col_lists, s->stream) || s->d_col_masks.upload(plan.front_mask, s->stream)) {return KH_ERR_HIP;}
  return KH_OK;
}

// The launches behind the linearisation: the undamped factorisation, the selected inverse down the tree, its blocks on H's pattern,
// the queries' columns, and the cleaning of the fronts; the fail word's copy rides behind them.
int launch_pass(kh_spa * s, const SpaDev & dev, int32_t n_queries, int32_t R, const std::vector<int32_t> & col_level_off, bool events)
{
  hipStream_t st = s->stream;
  const kh_spa_options & opt = s->opt;
  const int n_levels = static_cast<int>(s->sym.levels.size());
  int rc = zero_fronts(s, dev); if (rc) {return rc;}
  // undamped: inv_radius = 0.  The LM diagonal is formed on the way into a scratch vector (d_delta: every iteration of a Compute
  // overwrites it), so that 0 * diagonal is 0 whatever d_diag holds -- it may never have been formed
  spa_launch_assemble(dev, s->d_scale.p, s->d_delta.p, 0.0, true, opt.min_lm_diagonal, opt.max_lm_diagonal, s->d_rhs.p, s->d_fail.p, st);
  rc = launch_factor_levels(s, dev, true); if (rc) {return rc;}
  if (events) {KS_HIP(hipEventRecord(s->ev_cov[0], st));}
  for (int l = n_levels - 1; l >= 0; --l) {
    spa_launch_selinv_level(dev, s->level_offsets[l], s->level_offsets[l + 1] - s->level_offsets[l], s->level_max_m[l], s->level_max_ns[l], s->d_zbuf.p, st);
  }
  if (events) {KS_HIP(hipEventRecord(s->ev_cov[1], st));}
  spa_launch_cov_gather(dev, s->d_zbuf.p, s->d_scale.p, s->d_cov.p, st);
  if (events) {KS_HIP(hipEventRecord(s->ev_cov[2], st));}
  if (n_queries > 0) {
    // the fronts still hold G where L21 was, winv holds W: forward up the paths, backward over every front, then the blocks
    if (events) {KS_HIP(hipEventRecord(s->ev_col[0], st));}
    spa_launch_cov_columns_init(dev, s->d_col_lists.p, n_queries, R, s->d_scale.p, s->d_col_rhs.p, st);
    for (int l = 0; l < n_levels; ++l) {
      spa_launch_cov_columns_forward(dev, s->d_col_lists.p + col_level_off[l], col_level_off[l + 1] - col_level_off[l], s->d_col_masks.p, R, s->d_col_rhs.p, st);
    }
    if (events) {KS_HIP(hipEventRecord(s->ev_col[1], st));}
    for (int l = n_levels - 1; l >= 0; --l) {
      spa_launch_cov_columns_backward(dev, s->level_offsets[l], s->level_offsets[l + 1] - s->level_offsets[l], R, s->d_col_rhs.p, st);
    }
    if (events) {KS_HIP(hipEventRecord(s->ev_col[2], st));}
    spa_launch_cov_columns_gather(dev, n_queries, R, s->d_scale.p, s->d_col_rhs.p, s->d_columns.p, st);
  }
  if (dev.scatter) {
    // the pass stands where the backward sweep stands in a solve: the last reader of what the factorisation left in the fronts
    spa_launch_selinv_clean(dev, st);
    spa_launch_zero_update_blocks(dev, s->d_deferred.p, s->n_deferred_fronts, s->deferred_max_m, st);
  }
  KS_HIP(hipMemcpyAsync(s->h_fail, s->d_fail.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  KS_HIP(hipGetLastError());
  return KH_OK;
}

// behind the drain: the fail word of the factorisation, then what the pass left in the self-cleaning fronts
int check_pass(kh_spa * s, const SpaDev & dev, const std::string & who)
{
  if (s->h_fail[0] != 0) {
    // (a failed front has handed NaNs up the tree: the fronts are not trusted to be clean, the next factorisation memsets)
    set_error(who + ": non-positive pivot: a free component of the graph is not tied to the gauge node");
    return KH_ERR_SOLVER;
  }
  if (dev.scatter) {
    s->clean_a = dev.fronts; s->clean_b = dev.fronts_b;
    // (as behind a Compute())
    if (s->debug_flags & 1) {return check_fronts_clean(s, dev, "the covariance pass");}
  }
  return KH_OK;
}

void fold_event_times(kh_spa * s, int32_t n_queries, kh_spa_cov_summary & sum, kh_spa_cov_columns_summary & csum)
{
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, s->ev_cov[0], s->ev_cov[1]) == hipSuccess) {sum.inverse_ms = ms;}
  if (hipEventElapsedTime(&ms, s->ev_cov[1], s->ev_cov[2]) == hipSuccess) {sum.gather_ms = ms;}
  if (n_queries > 0) {
    if (hipEventElapsedTime(&ms, s->ev_col[0], s->ev_col[1]) == hipSuccess) {csum.forward_ms = ms;}
    if (hipEventElapsedTime(&ms, s->ev_col[1], s->ev_col[2]) == hipSuccess) {csum.backward_ms = ms;}
  }
}
}  // namespace

// ---- covariances: Sigma = (J^T J)^-1 on the pattern of H, from the selected inverse of the factor ----------------------------
int kh::spa::covariance_pass(kh_spa * s, kh_spa_cov_summary * summary, const std::vector<int32_t> & query_ids, kh_spa_cov_columns_summary * col_summary,
                             const char * caller)
{
  const std::string who = caller;
  settle(s);
  s->cov_valid = false; s->cov_on_host = false;
  s->col_ids.clear(); s->col_free.clear(); s->h_columns.clear();
  kh_spa_cov_summary sum;
  std::memset(&sum, 0, sizeof(sum));
  kh_spa_cov_columns_summary csum;
  std::memset(&csum, 0, sizeof(csum));
  auto finish = [&](int rc) {
    if (summary) {*summary = sum;}
    if (col_summary) {csum.cov = sum; *col_summary = csum;}
    return rc;
  };
  // preconditions: a graph, a usable loss, a problem, known queries, the level pipeline, every component tied to the gauge
  if (s->nodes.empty()) {set_error(who + ": the graph has no nodes"); return finish(KH_ERR_NOT_FOUND);}
  int rc = check_loss_scale(s);
  if (rc) {return finish(rc);}
  KS_HIP(hipSetDevice(s->device));
  const auto t_begin = std::chrono::steady_clock::now();
  SpaDev dev;
  std::memset(&dev, 0, sizeof(dev));
  bool has_work = false;
  rc = prepare_problem(s, dev, has_work);
  if (rc) {return finish(rc);}
  if (!has_work) {set_error(who + ": no constraint touches a free node: nothing is in the problem"); return finish(KH_ERR_NOT_FOUND);}
  const Symbolic & sym = s->sym;
  const int32_t n_queries = static_cast<int32_t>(query_ids.size());
  std::vector<int32_t> query_free(query_ids.size(), -1);
  for (int32_t k = 0; k < n_queries; ++k) {
    rc = covariance_index(s, query_ids[k], query_free[k]);
    if (rc) {return finish(rc);}
  }
  sum.n_free = dev.n_free; sum.levels = static_cast<int>(sym.levels.size());
  sum.analysis = analysis_kind(s);
  if (!select_factor_mode(s, dev)) {
    // (the downward pass needs W = L11^-T of every front, which only the level pipeline leaves behind)
    set_error(who + ": needs the level pipeline (a front exceeds its LDS budget, or factor kernels 1 / 2 are selected)");
    return finish(KH_ERR_SOLVER);
  }
  rc = check_tied_to_gauge(s, who);
  if (rc) {return finish(rc);}
  for (int32_t k = 0; k < sym.n_fronts; ++k) {
    const int64_t ns = sym.front_ns[k], nu = sym.front_m[k] - ns;
    sum.inverse_flops += nu * ns * ns + 2 * nu * nu * ns + 2 * ns * ns * nu;
  }
  if (s->d_zbuf.ensure(static_cast<size_t>(sym.fronts_size) + 16) || s->d_cov.ensure(static_cast<size_t>(s->n_slots) * 9 + 16)) {return finish(KH_ERR_HIP);}
  const int32_t R = (3 * n_queries + 15) & ~15;
  std::vector<int32_t> col_level_off;
  rc = plan_and_upload_columns(s, dev, who, query_free, R, col_level_off, csum);
  if (rc) {return finish(rc);}
  // the launches
  const std::pair<int32_t, int32_t> shard = set_loss_and_shard(s, dev);
  rc = linearize_normal_equations(s, dev, s->d_x.p, s->d_scal.p, shard.first, shard.second, nullptr); if (rc) {return finish(rc);}
  rc = make_scale(s, dev); if (rc) {return finish(rc);}
  KS_HIP(hipStreamSynchronize(s->stream));
  sum.linearize_ms = ms_since(t_begin);
  const auto t_factor = std::chrono::steady_clock::now();
  const bool events = (s->debug_flags & 2) != 0;
  rc = launch_pass(s, dev, n_queries, R, col_level_off, events);
  if (rc) {return finish(rc);}
  KS_HIP(hipStreamSynchronize(s->stream));
  rc = check_pass(s, dev, who);
  if (rc) {return finish(rc);}
  if (events) {fold_event_times(s, n_queries, sum, csum);}
  s->cov_valid = true;
  s->col_ids = query_ids; s->col_free = query_free; s->h_columns.assign(query_ids.size(), {});
  sum.factor_ms = ms_since(t_factor);
  sum.total_ms = ms_since(t_begin);
  csum.total_ms = sum.total_ms;
  return finish(KH_OK);
}

int kh::spa::covariance_index(kh_spa * s, int32_t id, int32_t & free_index)
{
  const auto it = s->index_of.find(id);
  if (it == s->index_of.end()) {set_error("kh_spa: no node with id " + std::to_string(id)); return KH_ERR_NOT_FOUND;}
  free_index = s->free_of_node[it->second];
  if (free_index < 0 && it->second != s->fixed_index) {
    set_error("kh_spa: node " + std::to_string(id) + " has no constraints: it is not in the problem");
    return KH_ERR_NOT_FOUND;
  }
  return KH_OK;
}

namespace
{
// the array and the pattern it is addressed by, on the host (first getter behind a computation)
int fetch_covariances(kh_spa * s)
{
  if (!s->cov_valid) {return stale("kh_spa_compute_covariances");}
  if (s->cov_on_host) {return KH_OK;}
  const size_t nf = s->node_of_free.size(), nslots = static_cast<size_t>(s->n_slots);
  s->h_cov.resize(nslots * 9); s->h_cov_row_ptr.resize(nf + 1); s->h_cov_col.resize(nslots); s->h_cov_diag.resize(nf);
  KS_HIP(hipSetDevice(s->device));
  KS_HIP(hipMemcpyAsync(s->h_cov.data(), s->d_cov.p, nslots * 9 * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  KS_HIP(hipMemcpyAsync(s->h_cov_row_ptr.data(), s->d_bsr_row_ptr.p, (nf + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
  KS_HIP(hipMemcpyAsync(s->h_cov_col.data(), s->d_bsr_col.p, nslots * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
  KS_HIP(hipMemcpyAsync(s->h_cov_diag.data(), s->d_bsr_diag.p, nf * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
  KS_HIP(hipStreamSynchronize(s->stream));
  s->cov_on_host = true;
  return KH_OK;
}

// position of `id` among the queries of the last column pass; KH_ERR_SOLVER when stale, KH_ERR_NOT_FOUND when the node was no query
int column_of_query(kh_spa * s, int32_t id, int32_t & k)
{
  if (!s->cov_valid) {return stale("kh_spa_compute_covariance_columns");}
  const auto it = std::find(s->col_ids.begin(), s->col_ids.end(), id);
  if (it == s->col_ids.end()) {
    set_error("kh_spa: node " + std::to_string(id) + " was not a query of the last kh_spa_compute_covariance_columns: its column is not resident");
    return KH_ERR_NOT_FOUND;
  }
  k = static_cast<int32_t>(it - s->col_ids.begin());
  return KH_OK;
}

// the column of query k on the host (the first getter that asks for it brings it)
int fetch_column(kh_spa * s, int32_t k)
{
  const size_t len = 9 * s->node_of_free.size();
  if (s->h_columns[k].size() == len) {return KH_OK;}
  s->h_columns[k].resize(len);
  KS_HIP(hipSetDevice(s->device));
  KS_HIP(hipMemcpyAsync(s->h_columns[k].data(), s->d_columns.p + len * static_cast<size_t>(k), len * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  KS_HIP(hipStreamSynchronize(s->stream));
  return KH_OK;
}

// The covariance of every listed node's pose relative to node id_ref (`relative`: in the reference's frame, which takes the poses
// up as well) or of the plain difference of the two poses in the world frame, nine doubles per node, from the resident column of id_ref.
int pair_covariances(kh_spa * s, const char * who, bool relative, int32_t id_ref, int32_t n, const int32_t * ids, double * out)
{
  int rc = enter(!(n < 0 || (n > 0 && !out)), s);
  if (rc) {return rc;}
  int32_t k = -1;
  rc = column_of_query(s, id_ref, k);
  if (rc) {return rc;}
  rc = check_listed(s, who, n, ids);
  if (rc) {return rc;}
  if (n == 0) {return KH_OK;}
  // [relative: poses of the listed nodes, then the reference's |] their free indices go up, nine doubles per node come back
  const size_t nn = static_cast<size_t>(n), pose_bytes = relative ? (3 * nn + 3) * sizeof(double) : 0;
  std::vector<char> in(pose_bytes + nn * sizeof(int32_t));
  double * poses = reinterpret_cast<double *>(in.data());
  int32_t * free_idx = reinterpret_cast<int32_t *>(in.data() + pose_bytes);
  for (int32_t t = 0; t < n; ++t) {
    const int32_t id = ids ? ids[t] : s->nodes[t].id;
    rc = covariance_index(s, id, free_idx[t]);
    if (rc) {return rc;}
    if (relative) {
      const double * pose = s->nodes[s->index_of[id]].pose;
      std::copy(pose, pose + 3, poses + 3 * static_cast<size_t>(t));
    }
  }
  if (relative) {
    const double * ref_pose = s->nodes[s->index_of[id_ref]].pose;
    std::copy(ref_pose, ref_pose + 3, poses + 3 * nn);
  }
  KS_HIP(hipSetDevice(s->device));
  if (s->d_rel_in.ensure(in.size()) || s->d_rel.ensure(9 * nn)) {return KH_ERR_HIP;}
  KS_HIP(hipMemcpyAsync(s->d_rel_in.p, in.data(), in.size(), hipMemcpyHostToDevice, s->stream));
  const SpaDev dev = resident_view(s);
  const double * column = s->d_columns.p + 9 * static_cast<size_t>(dev.n_free) * k;
  const double * d_poses = reinterpret_cast<const double *>(s->d_rel_in.p);
  const int32_t * d_free_idx = reinterpret_cast<const int32_t *>(s->d_rel_in.p + pose_bytes);
  if (relative) {
    spa_launch_cov_relative(dev, s->d_cov.p, column, s->col_free[k], d_poses + 3 * nn, d_free_idx, d_poses, n, s->d_rel.p, s->stream);
  } else {
    spa_launch_cov_difference(dev, s->d_cov.p, column, s->col_free[k], d_free_idx, n, s->d_rel.p, s->stream);
  }
  KS_HIP(hipGetLastError());
  KS_HIP(hipMemcpyAsync(out, s->d_rel.p, 9 * nn * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  KS_HIP(hipStreamSynchronize(s->stream));
  return KH_OK;
}
}  // namespace

extern "C" {

int kh_spa_compute_covariances(kh_spa * s, kh_spa_cov_summary * summary)
{
  const int rc = enter(true, s);
  if (rc) {return rc;}
  return covariance_pass(s, summary, {}, nullptr, "kh_spa_compute_covariances");
}

int kh_spa_compute_covariance_columns(kh_spa * s, int32_t n, const int32_t * ids, kh_spa_cov_columns_summary * summary)
{
  if (summary) {std::memset(summary, 0, sizeof(*summary));}
  if (n < 1 || n > KH_SPA_MAX_COV_COLUMNS || !ids) {
    set_error("kh_spa_compute_covariance_columns: between 1 and " + std::to_string(KH_SPA_MAX_COV_COLUMNS) + " query nodes are listed");
    return KH_ERR_INVALID_ARG;
  }
  std::vector<int32_t> query_ids(ids, ids + n);
  {
    std::vector<int32_t> sorted = query_ids;
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) {
      set_error("kh_spa_compute_covariance_columns: a query node is listed twice");
      return KH_ERR_INVALID_ARG;
    }
  }
  const int rc = enter(true, s);
  if (rc) {return rc;}
  return covariance_pass(s, nullptr, query_ids, summary, "kh_spa_compute_covariance_columns");
}

int kh_spa_get_covariances(kh_spa * s, int32_t n, const int32_t * ids, double * cov)
{
  int rc = enter(!(n < 0 || (n > 0 && !cov)), s);
  if (rc) {return rc;}
  rc = fetch_covariances(s);
  if (rc) {return rc;}
  rc = check_listed(s, "kh_spa_get_covariances", n, ids);
  if (rc) {return rc;}
  for (int32_t k = 0; k < n; ++k) {
    int32_t f = -1;
    rc = covariance_index(s, ids ? ids[k] : s->nodes[k].id, f);
    if (rc) {return rc;}
    if (f < 0) {
      std::fill(cov + 9 * static_cast<size_t>(k), cov + 9 * static_cast<size_t>(k) + 9, 0.0);
    } else {
      const double * b = s->h_cov.data() + 9 * static_cast<size_t>(s->h_cov_diag[f]);
      std::copy(b, b + 9, cov + 9 * static_cast<size_t>(k));
    }
  }
  return KH_OK;
}

int kh_spa_get_joint_covariance(kh_spa * s, int32_t id_a, int32_t id_b, double cov[36])
{
  int rc = enter(cov != nullptr, s);
  if (rc) {return rc;}
  rc = fetch_covariances(s);
  if (rc) {return rc;}
  int32_t f[2] = {-1, -1};
  rc = covariance_index(s, id_a, f[0]); if (rc) {return rc;}
  rc = covariance_index(s, id_b, f[1]); if (rc) {return rc;}
  if (s->first_constraint(id_a, id_b) < 0 && s->first_constraint(id_b, id_a) < 0) {
    set_error("kh_spa_get_joint_covariance: no constraint joins the two nodes: their cross block is not on the pattern of the factor");
    return KH_ERR_NOT_FOUND;
  }
  std::fill(cov, cov + 36, 0.0);
  for (int p = 0; p < 2; ++p) {
    for (int q = 0; q < 2; ++q) {
      if (f[p] < 0 || f[q] < 0) {continue;}                    // the gauge node: zeros
      const auto b = s->h_cov_col.begin() + s->h_cov_row_ptr[f[p]], e = s->h_cov_col.begin() + s->h_cov_row_ptr[f[p] + 1];
      const auto it = std::lower_bound(b, e, f[q]);
      if (it == e || *it != f[q]) {set_error("kh_spa_get_joint_covariance: block outside the pattern"); return KH_ERR_SOLVER;}
      place_block(cov, p, q, s->h_cov.data() + 9 * static_cast<size_t>(it - s->h_cov_col.begin()));
    }
  }
  return KH_OK;
}

int kh_spa_covariance_device(kh_spa * s, const double ** cov_bsr, int64_t * n_slots)
{
  const int rc = enter(cov_bsr && n_slots, s);
  if (rc) {return rc;}
  if (!s->cov_valid) {return stale("kh_spa_compute_covariances");}
  *cov_bsr = s->d_cov.p; *n_slots = s->n_slots;
  return KH_OK;
}

// ---- covariance columns: the getters --------------------------------------------------------------------------------------
int kh_spa_get_covariance_column(kh_spa * s, int32_t id_q, int32_t n, const int32_t * ids, double * out)
{
  int rc = enter(!(n < 0 || (n > 0 && !out)), s);
  if (rc) {return rc;}
  int32_t k = -1;
  rc = column_of_query(s, id_q, k);
  if (rc) {return rc;}
  rc = check_listed(s, "kh_spa_get_covariance_column", n, ids);
  if (rc) {return rc;}
  rc = fetch_column(s, k);
  if (rc) {return rc;}
  for (int32_t t = 0; t < n; ++t) {
    int32_t f = -1;
    rc = covariance_index(s, ids ? ids[t] : s->nodes[t].id, f);
    if (rc) {return rc;}
    double * o = out + 9 * static_cast<size_t>(t);
    if (f < 0 || s->col_free[k] < 0) {
      std::fill(o, o + 9, 0.0);                                    // the gauge node, as a row or as the query
    } else {
      std::copy(s->h_columns[k].begin() + 9 * static_cast<size_t>(f), s->h_columns[k].begin() + 9 * static_cast<size_t>(f) + 9, o);
    }
  }
  return KH_OK;
}

int kh_spa_get_joint_covariance_any(kh_spa * s, int32_t id_a, int32_t id_b, double cov[36])
{
  int rc = enter(cov != nullptr, s);
  if (rc) {return rc;}
  rc = fetch_covariances(s);
  if (rc) {return rc;}
  int32_t f[2] = {-1, -1};
  rc = covariance_index(s, id_a, f[0]); if (rc) {return rc;}
  rc = covariance_index(s, id_b, f[1]); if (rc) {return rc;}
  // the column of id_b where it is resident, else that of id_a; `row` is the other node: its block of the column is Sigma(row, query)
  int32_t k = -1, row = 0;
  if (std::find(s->col_ids.begin(), s->col_ids.end(), id_b) != s->col_ids.end()) {
    rc = column_of_query(s, id_b, k); row = 0;
  } else {
    rc = column_of_query(s, id_a, k); row = 1;
  }
  if (rc) {return rc;}
  rc = fetch_column(s, k);
  if (rc) {return rc;}
  std::fill(cov, cov + 36, 0.0);
  for (int p = 0; p < 2; ++p) {
    if (f[p] < 0) {continue;}                                       // the gauge node: zeros
    place_block(cov, p, p, s->h_cov.data() + 9 * static_cast<size_t>(s->h_cov_diag[f[p]]));
  }
  if (f[0] >= 0 && f[1] >= 0) {
    const double * blk = s->h_columns[k].data() + 9 * static_cast<size_t>(f[row]);
    const int q = 1 - row;                                          // block (row, q) of the 6 x 6, and its transpose at (q, row)
    place_block(cov, row, q, blk);
    place_block(cov, q, row, blk, true);
  }
  return KH_OK;
}

int kh_spa_get_relative_covariances(kh_spa * s, int32_t id_ref, int32_t n, const int32_t * ids, double * out)
{
  return pair_covariances(s, "kh_spa_get_relative_covariances", true, id_ref, n, ids, out);
}

int kh_spa_get_difference_covariances(kh_spa * s, int32_t id_ref, int32_t n, const int32_t * ids, double * out)
{
  return pair_covariances(s, "kh_spa_get_difference_covariances", false, id_ref, n, ids, out);
}

// ---- constraint audit: the leave-one-out test of every constraint from the resident selected inverse ----
int kh_spa_audit_constraints(kh_spa * s, double min_redundancy, kh_spa_audit_t * out, kh_spa_audit_summary * summary)
{
  if (summary) {std::memset(summary, 0, sizeof(*summary));}
  if (!std::isfinite(min_redundancy) || !(min_redundancy > 0.0) || !(min_redundancy < 1.0) || !out) {
    set_error("kh_spa_audit_constraints: min_redundancy must lie in (0, 1) and out must not be NULL");
    return KH_ERR_INVALID_ARG;
  }
  int rc = enter(true, s);
  if (rc) {return rc;}
  settle(s);
  const auto t_begin = std::chrono::steady_clock::now();
  kh_spa_audit_summary sum;
  std::memset(&sum, 0, sizeof(sum));
  auto finish = [&](int code) {
    sum.total_ms = ms_since(t_begin);
    if (summary) {*summary = sum;}
    return code;
  };
  const int32_t E = static_cast<int32_t>(s->cons.size());
  if (E == 0) {return finish(KH_OK);}
  if (!s->cov_valid) {
    rc = covariance_pass(s, &sum.cov, {}, nullptr, "kh_spa_audit_constraints");
    if (rc) {return finish(rc);}
  }
  KS_HIP(hipSetDevice(s->device));
  const size_t ne = static_cast<size_t>(E);
  if (s->d_audit_lin.ensure(21 * ne) || s->d_audit_cost.ensure(ne) || s->d_audit_out.ensure(4 * ne) || s->d_audit_flag.ensure(ne)) {return finish(KH_ERR_HIP);}
  // the audit's own linearisation of every edge: only what k_edge_lin and k_edge_audit read is filled in
  SpaDev dev = resident_view(s);
  dev.edge_lin = s->d_audit_lin.p; dev.edge_cost = s->d_audit_cost.p;
  (void)set_loss_and_shard(s, dev);          // the audit walks every edge: only the loss
  const bool events = (s->debug_flags & 2) != 0;
  if (events) {KS_HIP(hipEventRecord(s->ev_audit[0], s->stream));}
  spa_launch_edge_audit(dev, s->d_x.p, s->d_cov.p, min_redundancy, s->d_audit_out.p, s->d_audit_flag.p, s->stream);
  if (events) {KS_HIP(hipEventRecord(s->ev_audit[1], s->stream));}
  KS_HIP(hipGetLastError());
  std::vector<double> h_out(4 * ne);
  std::vector<int32_t> h_flag(ne);
  KS_HIP(hipMemcpyAsync(h_out.data(), s->d_audit_out.p, 4 * ne * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  KS_HIP(hipMemcpyAsync(h_flag.data(), s->d_audit_flag.p, ne * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
  KS_HIP(hipStreamSynchronize(s->stream));
  if (events) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, s->ev_audit[0], s->ev_audit[1]) == hipSuccess) {sum.kernel_ms = ms;}
  }
  for (int32_t e = 0; e < E; ++e) {
    kh_spa_audit_t & o = out[e];
    o.index = e; o.id_a = s->cons[e].a; o.id_b = s->cons[e].b; o.verifiable = h_flag[e];
    o.chi2 = h_out[4 * static_cast<size_t>(e)]; o.redundancy = h_out[4 * static_cast<size_t>(e) + 1];
    o.min_pivot = h_out[4 * static_cast<size_t>(e) + 2]; o.chi2_loo = h_out[4 * static_cast<size_t>(e) + 3];
    sum.n_verifiable += h_flag[e] ? 1 : 0;
  }
  sum.n_constraints = E;
  return finish(KH_OK);
}

}  // extern "C"

namespace kh
{
// whether the resident covariances still belong to the graph (the mapper recomputes lazily)
bool spa_covariances_valid(const kh_spa * s) {return s && s->cov_valid;}
// ... and whether the block column of node `id` is resident with them
bool spa_covariance_column_resident(const kh_spa * s, int32_t id)
{
  return s && s->cov_valid && std::find(s->col_ids.begin(), s->col_ids.end(), id) != s->col_ids.end();
}
// ... and whether node `id` is in the problem of the last covariance pass (the gauge node or a node with constraints): the
// nodes the covariance getters answer for
bool spa_covariance_has_node(const kh_spa * s, int32_t id)
{
  if (!s || !s->cov_valid) {return false;}
  const auto it = s->index_of.find(id);
  if (it == s->index_of.end() || static_cast<size_t>(it->second) >= s->free_of_node.size()) {return false;}
  return s->free_of_node[it->second] >= 0 || it->second == s->fixed_index;
}
}  // namespace kh
