// Compute() of the pose-graph SPA solver (hot path B): the Levenberg-Marquardt control loop on the host, all numeric work on the
// GPU (spa_linearize.hip, spa_potrf.hip + spa_update.hip, spa_factor_front.hip; spa_device.hpp lists the kernel files), and the linear-algebra pieces it shares with the covariance pass (spa_covariance.cpp).
//
// Reference: solvers/ceres_solver.cpp:214-269 (CeresSolver::Compute), solvers/ceres_utils.h (residual).  The minimiser restates
// Ceres 2.0's trust-region LM (trust_region_minimizer.cc, levenberg_marquardt_strategy.cc, trust_region_step_evaluator.cc); Ceres
// itself is a third-party dependency that is not in the reference tree ("parity unpinned").
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "host_wait.hpp"
#include "spa_private.hpp"

using namespace kh;
using namespace kh::spa;

// ---- pieces Compute() and the covariance pass share -------------------------------------------------------------------
namespace kh
{
namespace spa
{
int check_loss_scale(const kh_spa * s)
{
  if (s->opt.loss_function != KH_LOSS_NONE && !(s->opt.loss_scale > 0.0)) {
    set_error("kh_spa: loss_scale must be positive");
    return KH_ERR_INVALID_ARG;
  }
  return KH_OK;
}

int32_t analysis_kind(const kh_spa * s) {return s->last_symbolic_ms > 0.0 ? (s->last_analysis_incremental ? 2 : 1) : 0;}

int allreduce_normal_equations(kh_spa * s, const SpaDev & into)
{
  const int64_t hg_count = static_cast<int64_t>(s->n_slots) * 9 + static_cast<int64_t>(into.n_free) * 3;
  if (s->comm) {
    // on the solver's stream (RCCL over xGMI)
    const int arc = kh_comm_allreduce_sum_f64(s->comm, into.H, hg_count, s->stream);
    if (arc) {return arc;}
  } else if (s->shard_world > 1) {
    if (!s->allreduce) {set_error("kh_spa: sharding enabled without a communicator or an all-reduce callback"); return KH_ERR_INVALID_ARG;}
    if (s->allreduce(s->allreduce_user, into.H, hg_count, s->stream) != 0) {set_error("kh_spa: all-reduce callback failed"); return KH_ERR_SOLVER;}
  }
  return KH_OK;
}

int linearize_normal_equations(kh_spa * s, const SpaDev & into, const double * at, double * cost_slot, int32_t e_lo, int32_t e_hi, hipEvent_t * ev)
{
  if (ev) {KS_HIP(hipEventRecord(ev[0], s->stream));}
  spa_launch_linearize(into, at, cost_slot, e_lo, e_hi, s->stream);
  if (ev) {KS_HIP(hipEventRecord(ev[1], s->stream));}
  return allreduce_normal_equations(s, into);
}

// The fronts (and buffer B) start every factorisation as zeros: 2 x 190 MB on the 10k-node graph, 27 us each at the head of
// the critical stream.  In scatter mode the fronts are SELF-CLEANING instead: every entry has exactly one last reader in a
// factorisation (k_potrf the pivot block, k_trsm buffer B under L21, k_syrk the update block, k_backward3 L21 -- behind a covariance
// pass k_selinv_clean, which zeroes what the downward pass wrote over L21), and that reader
// stores a zero behind itself; only the update matrices that stay in place take a (small) kernel of their own.  (Zeroing on a
// second stream beside the step evaluation was tried first: the fill kernels take every compute unit, k_step_fused and the
// linearisation ran 2-3 x longer and the iteration gained 10 us of the 54.)
int zero_fronts(kh_spa * s, const SpaDev & dev)
{
  hipStream_t st = s->stream;
  if (dev.scatter && s->clean_a == dev.fronts && s->clean_b == dev.fronts_b) {s->clean_a = nullptr; return KH_OK;}
  s->clean_a = nullptr;
  // (the WHOLE allocation: a later analysis may lay larger fronts over the same buffers, and "clean" has to mean all of them)
  KS_HIP(hipMemsetAsync(dev.fronts, 0, sizeof(double) * (dev.scatter ? s->d_fronts.cap : static_cast<size_t>(dev.fronts_size)), st));
  if (dev.scatter) {KS_HIP(hipMemsetAsync(dev.fronts_b, 0, sizeof(double) * s->d_fronts_b.cap, st));}
  return KH_OK;
}

bool select_factor_mode(const kh_spa * s, SpaDev & dev)
{
  const int factor_mode = ((s->debug_flags >> 4) & 15) ? ((s->debug_flags >> 4) & 15) : 3;
  const bool pipeline = factor_mode >= 3 && spa_level_pipeline_fits(s->sym.max_m, s->sym.max_ns);
  dev.gather = pipeline && (s->debug_flags & 256) ? 1 : 0;
  dev.scatter = pipeline && !dev.gather && !(s->debug_flags & 512) ? 1 : 0;
  return pipeline;
}

int launch_factor_levels(kh_spa * s, const SpaDev & dev, bool pipeline)
{
  hipStream_t st = s->stream;
  const Symbolic & sym = s->sym;
  const int n_levels = static_cast<int>(sym.levels.size());
  constexpr int32_t kNarrowLevel = 128;      // levels of at most this many fronts take the chip-wide extend-add
  for (int l = 0; l < n_levels; ++l) {
    const int32_t n_level = s->level_offsets[l + 1] - s->level_offsets[l];
    const int32_t * lf = s->d_level_fronts.p + s->level_offsets[l];
    if (pipeline) {
      // (running the part of the extend-add that k_potrf does not read on a second stream beside the pivot chains was measured
      // slower on the 10k / 30k graph: 14.7 ms per solve against 13.2 -- the event records and stream waits on the critical
      // stream cost more than the overlap wins)
      if (l > 0 && !dev.gather && !dev.scatter) {spa_launch_extend_add(dev, lf, n_level, s->level_max_m[l], st);}
      spa_launch_potrf_level(dev, s->level_offsets[l], n_level, s->level_max_m[l], s->level_max_ns[l], s->d_fail.p, s->d_rhs.p, s->d_upd.p, st);
      // the update of the level: the fronts that fit one workgroup's LDS whole in k_front_update (when there are enough of them), the
      // larger ones -- the head of the level -- in k_trsm / k_syrk
      if (s->level_max_nu[l] == 0) {continue;}                   // (the root: nothing below the pivot block)
      const int32_t split = dev.gather ? n_level : s->level_split[l];
      spa_launch_update_level(dev, s->level_offsets[l], split, s->level_max_m[l], s->level_max_ns[l], s->d_rhs.p, s->d_upd.p, st);
      spa_launch_front_update(dev, s->level_offsets[l] + split, n_level - split, s->level_fused_lds[l], s->d_rhs.p, s->d_upd.p, st);
      continue;
    }
    // narrow levels: the extend-add runs chip-wide in its own launch instead of on each front's single CU
    const bool split = l > 0 && n_level <= kNarrowLevel;
    if (split) {spa_launch_extend_add(dev, lf, n_level, s->level_max_m[l], st);}
    spa_launch_factor_level(dev, lf, n_level, s->level_max_m[l], s->d_fail.p, s->d_rhs.p, s->d_upd.p, split ? 1 : 0, st);
  }
  return KH_OK;
}

std::pair<int32_t, int32_t> set_loss_and_shard(const kh_spa * s, SpaDev & dev)
{
  dev.loss_kind = s->opt.loss_function; dev.loss_b = s->opt.loss_scale * s->opt.loss_scale; dev.loss_a = s->opt.loss_scale;
  return {static_cast<int32_t>(static_cast<int64_t>(dev.n_edges) * s->shard_rank / s->shard_world),
          static_cast<int32_t>(static_cast<int64_t>(dev.n_edges) * (s->shard_rank + 1) / s->shard_world)};
}

int make_scale(kh_spa * s, const SpaDev & dev)
{
  if (s->opt.jacobi_scaling) {spa_launch_jacobi_scale(dev, s->d_scale.p, s->stream); return KH_OK;}
  std::vector<double> ones(static_cast<size_t>(dev.n_free) * 3, 1.0);
  KS_HIP(hipMemcpyAsync(s->d_scale.p, ones.data(), ones.size() * 8, hipMemcpyHostToDevice, s->stream));
  KS_HIP(hipStreamSynchronize(s->stream));
  return KH_OK;
}

int check_fronts_clean(kh_spa * s, const SpaDev & dev, const char * left_by)
{
  hipStream_t st = s->stream;
  KS_HIP(hipMemsetAsync(s->d_fail.p, 0, sizeof(int32_t), st));
  spa_launch_count_nonzero(dev.fronts, dev.fronts_size, s->d_fail.p, st);
  spa_launch_count_nonzero(dev.fronts_b, dev.fronts_size, s->d_fail.p, st);
  KS_HIP(hipMemcpyAsync(s->h_fail, s->d_fail.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));
  if (s->h_fail[0] != 0) {
    s->clean_a = nullptr;
    set_error("kh_spa: " + std::to_string(s->h_fail[0]) + " entries of the self-cleaning fronts were left behind by " + left_by);
    return KH_ERR_SOLVER;
  }
  return KH_OK;
}
}  // namespace spa
}  // namespace kh

// ---- one LM iteration on the device ------------------------------------------------------------------------------------------
namespace
{
// what stays the same over the iterations of one Compute(), and how many event pairs it has used
struct ComputeRun
{
  bool pipeline = false;           // the level pipeline factorises (select_factor_mode)
  // kh_spa_set_debug bit 1: HIP events around the phases of every LM iteration (kh_spa_summary.*_gpu_ms).  Off by default: an event
  // record between two kernels is a 5-6 us bubble on the stream, three of them per iteration were 0.15 ms of a 9 ms solve.
  bool phase_events = false;
  bool lin_check = false;          // kh_spa_set_debug bit 0: the residual of every linear solve
  bool direct = false;             // the iteration's scalars come through the host-coherent block instead of a copy
  int32_t e_lo = 0, e_hi = 0;      // this rank's edge block
  int n_lin = 0, n_timed = 0;

  hipEvent_t * next_lin_events(kh_spa * s) {return phase_events && n_lin < 2 * kh_spa::kMaxTimed + 2 ? s->ev_lin[n_lin++] : nullptr;}
};

// the scalars and the fail word by copy, behind a drain of the stream
int fetch_scalars(kh_spa * s)
{
  hipStream_t st = s->stream;
  KS_HIP(hipMemcpyAsync(s->h_scal, s->d_scal.p, sizeof(double) * 16, hipMemcpyDeviceToHost, st));
  KS_HIP(hipMemcpyAsync(s->h_fail, s->d_fail.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  KS_HIP(hipStreamSynchronize(st));
  return KH_OK;
}

// The launches of one iteration (ComputeTrustRegionStep and the evaluation of its candidate): the damped system of `dev` at
// 1 / radius factorised and solved, the step taken from x into cand, the candidate's cost and -- into `alt` -- its normal equations.
int launch_iteration(kh_spa * s, ComputeRun & run, const SpaDev & dev, const SpaDev & alt, const double * x, double * cand, double radius, bool new_diagonal)
{
  hipStream_t st = s->stream;
  const kh_spa_options & opt = s->opt;
  const int n_levels = static_cast<int>(s->sym.levels.size());
  const bool timed = run.phase_events && run.n_timed < kh_spa::kMaxTimed;
  if (timed) {KS_HIP(hipEventRecord(s->ev_phase[run.n_timed][0], st));}
  int rc = zero_fronts(s, dev); if (rc) {return rc;}
  // one launch: the scaled + damped matrix into the fronts (forming the LM diagonal on the way when a new one is due), the
  // right-hand side in elimination order (factorisation and forward solve are one kernel per level) and the fail word's reset
  spa_launch_assemble(dev, s->d_scale.p, s->d_diag.p, 1.0 / radius, new_diagonal, opt.min_lm_diagonal, opt.max_lm_diagonal, s->d_rhs.p, s->d_fail.p, st);
  rc = launch_factor_levels(s, dev, run.pipeline); if (rc) {return rc;}
  if (timed) {KS_HIP(hipEventRecord(s->ev_phase[run.n_timed][1], st));}
  for (int l = n_levels - 1; l >= 0; --l) {
    const int32_t n_level = s->level_offsets[l + 1] - s->level_offsets[l];
    const int32_t * lf = s->d_level_fronts.p + s->level_offsets[l];
    if (run.pipeline) {
      spa_launch_backward3_level(dev, s->level_offsets[l], n_level, s->level_max_m[l], s->level_max_ns[l], s->d_rhs.p, st);
    } else {
      spa_launch_backward_level(dev, lf, n_level, s->level_max_m[l], s->d_rhs.p, st);
    }
  }
  if (dev.scatter) {
    spa_launch_zero_update_blocks(dev, s->d_deferred.p, s->n_deferred_fronts, s->deferred_max_m, st);
    s->clean_a = dev.fronts; s->clean_b = dev.fronts_b;
  }
  // the candidate's cost AND its normal equations (speculative: a step is nearly always accepted) ride in the same batch
  hipEvent_t * ev_lin = run.next_lin_events(s);
  if (ev_lin) {KS_HIP(hipEventRecord(ev_lin[0], st));}
  spa_launch_step_and_linearize(dev, alt, s->d_scale.p, s->d_rhs.p, x, s->d_step.p, s->d_delta.p, cand, s->d_partial.p, run.e_lo, run.e_hi, st);
  if (ev_lin) {KS_HIP(hipEventRecord(ev_lin[1], st));}
  // a communicator (or a sharding callback) sums this rank's H || g with the others', also with one rank (identity)
  rc = allreduce_normal_equations(s, alt); if (rc) {return rc;}
  if (run.direct) {s->res_seq = s->res_seq == 0x7fffffff ? 1 : s->res_seq + 1;}
  spa_launch_step_scalars(alt, cand, s->d_partial.p, run.e_lo > 0 || run.e_hi < dev.n_edges, s->d_scal.p, st, run.direct ? s->h_res : nullptr, s->h_res_flag,
                          s->d_fail.p, s->res_seq);
  if (run.lin_check) {spa_launch_lin_check(dev, s->d_scale.p, s->d_diag.p, 1.0 / radius, s->d_step.p, s->d_scal.p + 12, st);}
  if (timed) {KS_HIP(hipEventRecord(s->ev_phase[run.n_timed][2], st)); ++run.n_timed;}
  KS_HIP(hipGetLastError());
  return KH_OK;
}

// the iteration's scalars in h_scal[3..] and its fail word in h_fail[0]
int read_iteration_scalars(kh_spa * s, const ComputeRun & run)
{
  if (!run.direct) {return fetch_scalars(s);}
  // the iteration's last kernel writes its scalars to host-coherent memory and raises the flag behind them; the stream is asked
  // now and then so that a failed launch cannot hang the caller
  hipError_t e = hipSuccess;
  const FlagWait w = wait_device_flag(s->h_res_flag, s->res_seq, s->stream, &e);
  if (w == FlagWait::kDrained) {set_error("kh_spa: the stream drained without the iteration's result flag"); return KH_ERR_HIP;}
  if (w == FlagWait::kFailed) {set_error(std::string("kh_spa: ") + hipGetErrorString(e)); return KH_ERR_HIP;}
  for (int q = 3; q <= 10; ++q) {s->h_scal[q] = s->h_res[q];}
  s->h_fail[0] = static_cast<int32_t>(s->h_res[11]);
  return KH_OK;
}

// the event times of the run into the summary (every recorded event has completed: each iteration ended with a stream
// synchronisation or its result flag)
void fold_event_times(kh_spa * s, const ComputeRun & run, kh_spa_summary & sum)
{
  float ms = 0.0f;
  for (int k = 0; k < run.n_timed; ++k) {
    if (hipEventElapsedTime(&ms, s->ev_phase[k][0], s->ev_phase[k][1]) == hipSuccess) {sum.factor_gpu_ms += ms;}
    if (hipEventElapsedTime(&ms, s->ev_phase[k][1], s->ev_phase[k][2]) == hipSuccess) {sum.backward_gpu_ms += ms;}
  }
  for (int k = 0; k < run.n_lin; ++k) {
    if (hipEventElapsedTime(&ms, s->ev_lin[k][0], s->ev_lin[k][1]) == hipSuccess) {sum.linearize_gpu_ms += ms;}
  }
}

void store_corrections(kh_spa * s)
{
  s->corr_ids.clear(); s->corr_poses.clear();
  for (const Node & n : s->nodes) {
    s->corr_ids.push_back(n.id);
    s->corr_poses.insert(s->corr_poses.end(), n.pose, n.pose + 3);
  }
}
}  // namespace

// CeresSolver::Compute, ceres_solver.cpp:214-269
extern "C" int kh_spa_compute(kh_spa * s, kh_spa_summary * summary)
{
  settle(s);
  if (!s) {return KH_ERR_INVALID_ARG;}
  s->cov_valid = false;
  kh_spa_summary sum;
  std::memset(&sum, 0, sizeof(sum));
  sum.usable = 1;
  auto finish = [&](int rc) {if (summary) {*summary = sum;} return rc;};
  if (s->nodes.empty()) {
    set_error("CeresSolver: Ceres was called when there are no nodes. This shouldn't happen.");
    return finish(KH_ERR_NOT_FOUND);
  }
  KS_HIP(hipSetDevice(s->device));
  const auto t_begin = std::chrono::steady_clock::now();
  SpaDev dev;
  std::memset(&dev, 0, sizeof(dev));
  bool has_work = false;
  int rc = prepare_problem(s, dev, has_work);
  if (rc) {return finish(rc);}
  if (!has_work) {          // nothing to optimise: Ceres returns the input, which is "usable"
    store_corrections(s);
    return finish(KH_OK);
  }
  const kh_spa_options & opt = s->opt;
  const Symbolic & sym = s->sym;
  hipStream_t st = s->stream;
  double * x = s->d_x.p; double * cand = s->d_cand.p;
  double * scal = s->d_scal.p;
  // the fused step kernel writes the candidate of the free nodes only: the gauge node and unused nodes carry their pose
  KS_HIP(hipMemcpyAsync(cand, x, sizeof(double) * 3 * static_cast<size_t>(dev.n_nodes), hipMemcpyDeviceToDevice, s->stream));
  sum.nnz_factor = sym.nnz_factor;
  double lin_ms = 0.0, solve_ms = 0.0;

  // ---- iteration zero ----
  const auto t0 = std::chrono::steady_clock::now();
  rc = check_loss_scale(s); if (rc) {return finish(rc);}
  ComputeRun run;
  const std::pair<int32_t, int32_t> shard = set_loss_and_shard(s, dev);
  run.e_lo = shard.first; run.e_hi = shard.second;
  run.phase_events = (s->debug_flags & 2) != 0;
  run.lin_check = (s->debug_flags & 1) != 0;
  run.direct = s->h_res != nullptr && !run.lin_check;
  // The normal equations at the CANDIDATE point are built speculatively, into a second H || g, in the same batch of
  // launches that evaluates the candidate's cost: a step is nearly always accepted, and the iteration then needs one
  // read-back of scalars instead of two (each was a stream drain plus ~90 us before the next launch reached the GPU).
  // A rejected step simply leaves the second buffer unused.
  SpaDev alt = dev;
  alt.H = s->d_Hg_alt.p; alt.g = s->d_Hg_alt.p + static_cast<size_t>(s->n_slots) * 9;
  run.pipeline = select_factor_mode(s, dev);
  rc = linearize_normal_equations(s, dev, x, scal + 0, run.e_lo, run.e_hi, run.next_lin_events(s)); if (rc) {return finish(rc);}
  rc = make_scale(s, dev); if (rc) {return finish(rc);}
  spa_launch_grad_norms(dev, x, scal + 1, st);
  KS_HIP(hipMemsetAsync(s->d_fail.p, 0, sizeof(int32_t), st));
  rc = fetch_scalars(s); if (rc) {return finish(rc);}
  lin_ms += ms_since(t0);
  double x_cost = s->h_scal[0], gmax = s->h_scal[1], x_norm = std::sqrt(s->h_scal[2]);
  sum.initial_cost = x_cost;
  double minimum_cost = x_cost;
  std::vector<double> best_x(static_cast<size_t>(dev.n_nodes) * 3);
  for (int32_t i = 0; i < dev.n_nodes; ++i) {std::copy(s->nodes[i].pose, s->nodes[i].pose + 3, best_x.begin() + 3 * i);}
  bool best_is_current = true;     // device x holds the minimum-cost iterate
  bool best_on_device = false;     // ... otherwise d_best does (best_x on the host until the first accepted step)
  // TrustRegionStepEvaluator
  const int max_nonmono = opt.use_nonmonotonic_steps ? opt.max_consecutive_nonmonotonic_steps : 0;
  double ev_min = x_cost, ev_cur = x_cost, ev_ref = x_cost, ev_cand = x_cost, ev_acc_ref = 0.0, ev_acc_cand = 0.0;
  int ev_nonmono = 0;
  // LevenbergMarquardtStrategy
  double radius = opt.initial_trust_region_radius, decrease_factor = 2.0;
  bool reuse_diagonal = false, have_diagonal = false;
  int num_invalid = 0, iteration = 0;
  bool step_successful = true;
  sum.successful_steps = 1;
  sum.termination = 1;
  if (!(x_cost == x_cost) || std::isinf(x_cost)) {   // initial evaluation failed
    sum.usable = 0; sum.termination = 2;
    set_error("CeresSolver: Ceres could not find a usable solution to optimize.");
    return finish(KH_ERR_SOLVER);
  }

  s->iter_log.clear();
  auto trace = [&](double cost, double cand_cost, double model_change, double radius_used, double radius_next, double step_norm, double verdict) {
    s->iter_log.push_back({static_cast<double>(iteration), cost, cand_cost, model_change, radius_used, radius_next, step_norm, verdict});
  };
  while (true) {
    if (iteration >= opt.max_num_iterations) {sum.termination = 1; break;}
    if (step_successful && gmax <= opt.gradient_tolerance) {sum.termination = 0; break;}
    if (radius < opt.min_trust_region_radius) {sum.termination = 0; break;}
    ++iteration;
    step_successful = false;

    // ---- ComputeTrustRegionStep ----
    const auto t1 = std::chrono::steady_clock::now();
    const bool new_diagonal = !reuse_diagonal || !have_diagonal;
    have_diagonal = true;
    rc = launch_iteration(s, run, dev, alt, x, cand, radius, new_diagonal); if (rc) {return finish(rc);}
    rc = read_iteration_scalars(s, run); if (rc) {return finish(rc);}
    solve_ms += ms_since(t1);
    if (run.lin_check) {
      std::fprintf(stderr, "[kh_spa] iteration %d: relative residual of the linear solve %.3e (fail flag %d)\n", iteration,
        std::sqrt(s->h_scal[12] / std::max(s->h_scal[13], 1e-300)), s->h_fail[0]);
      sum.worst_linear_residual = std::max(sum.worst_linear_residual, std::sqrt(s->h_scal[12] / std::max(s->h_scal[13], 1e-300)));
    }
    reuse_diagonal = true;
    const double step_dot_g = s->h_scal[3], step_H_step = s->h_scal[4], nonfinite = s->h_scal[5];
    const double step_norm = std::sqrt(s->h_scal[6]);
    const double cand_norm = std::sqrt(s->h_scal[7]);
    double cand_cost = s->h_scal[8];
    const double model_cost_change = -(step_dot_g + 0.5 * step_H_step);
    bool step_valid = s->h_fail[0] == 0 && nonfinite == 0.0 && std::isfinite(model_cost_change) && model_cost_change > 0.0;
    if (!step_valid) {
      ++num_invalid;
      if (num_invalid >= opt.max_num_consecutive_invalid_steps) {
        trace(x_cost, cand_cost, model_cost_change, radius, radius, step_norm, -1.0);     // (one log row per iteration, this one included)
        sum.termination = 2; sum.usable = 0; break;
      }
      trace(x_cost, cand_cost, model_cost_change, radius, radius / decrease_factor, step_norm, -1.0);
      radius = radius / decrease_factor;      // StepIsInvalid -> StepRejected(0)
      decrease_factor *= 2.0;
      continue;
    }
    num_invalid = 0;
    if (!std::isfinite(cand_cost)) {cand_cost = std::numeric_limits<double>::max();}

    if (step_norm <= opt.parameter_tolerance * (x_norm + opt.parameter_tolerance)) {
      trace(x_cost, cand_cost, model_cost_change, radius, radius, step_norm, 2.0); sum.termination = 0; break;
    }
    const double cost_change = x_cost - cand_cost;
    if (std::fabs(cost_change) <= opt.function_tolerance * x_cost) {
      trace(x_cost, cand_cost, model_cost_change, radius, radius, step_norm, 3.0); sum.termination = 0; break;
    }

    double quality;
    if (cand_cost >= std::numeric_limits<double>::max()) {
      quality = std::numeric_limits<double>::lowest();
    } else {
      const double rel = (ev_cur - cand_cost) / model_cost_change;
      const double hist = (ev_ref - cand_cost) / (ev_acc_ref + model_cost_change);
      quality = std::max(rel, hist);
    }
    if (quality > opt.min_relative_decrease) {
      // HandleSuccessfulStep
      if (best_is_current) {   // keep a copy of the best iterate before x moves on (device to device, no drain)
        KS_HIP(hipMemcpyAsync(s->d_best.p, x, best_x.size() * 8, hipMemcpyDeviceToDevice, st));
        best_on_device = true;
        best_is_current = false;
      }
      std::swap(x, cand);
      x_norm = cand_norm;
      std::swap(dev.H, alt.H); std::swap(dev.g, alt.g);          // the speculative linearisation is the current one now
      x_cost = s->h_scal[8]; gmax = s->h_scal[9];
      step_successful = true;
      ++sum.successful_steps;
      const double radius_used = radius;
      radius = radius / std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * quality - 1.0, 3));
      radius = std::min(opt.max_trust_region_radius, radius);
      trace(ev_cur, cand_cost, model_cost_change, radius_used, radius, step_norm, 1.0);
      decrease_factor = 2.0;
      reuse_diagonal = false;
      // TrustRegionStepEvaluator::StepAccepted
      ev_cur = cand_cost;
      ev_acc_cand += model_cost_change;
      ev_acc_ref += model_cost_change;
      if (ev_cur < ev_min) {
        ev_min = ev_cur; ev_nonmono = 0; ev_cand = ev_cur; ev_acc_cand = 0.0;
      } else {
        ++ev_nonmono;
        if (ev_cur > ev_cand) {ev_cand = ev_cur; ev_acc_cand = 0.0;}
      }
      if (ev_nonmono == max_nonmono) {ev_ref = ev_cand; ev_acc_ref = ev_acc_cand;}
      if (x_cost < minimum_cost) {minimum_cost = x_cost; best_is_current = true;}
    } else {
      trace(x_cost, cand_cost, model_cost_change, radius, radius / decrease_factor, step_norm, 0.0);
      radius = radius / decrease_factor;      // StepRejected
      decrease_factor *= 2.0;
      reuse_diagonal = true;
    }
  }

  if ((s->debug_flags & 1) && dev.scatter && s->clean_a == dev.fronts && iteration > 0) {
    rc = check_fronts_clean(s, dev, "the last factorisation"); if (rc) {return finish(rc);}
  }
  sum.iterations = iteration;
  sum.final_cost = minimum_cost;
  sum.linearize_ms = lin_ms; sum.solve_ms = solve_ms;
  sum.factor_flops = sym.factor_flops; sum.factorizations = iteration; sum.levels = static_cast<int>(sym.levels.size());
  sum.symbolic_ms = s->last_symbolic_ms;
  sum.analysis = analysis_kind(s);
  fold_event_times(s, run, sum);
  if (!sum.usable) {
    sum.total_ms = ms_since(t_begin);
    set_error("CeresSolver: Ceres could not find a usable solution to optimize.");
    return finish(KH_ERR_SOLVER);          // ceres_solver.cpp:249-254: state and corrections unchanged
  }
  if (best_is_current || best_on_device) {
    KS_HIP(hipMemcpyAsync(best_x.data(), best_is_current ? x : s->d_best.p, best_x.size() * 8, hipMemcpyDeviceToHost, st));
    KS_HIP(hipStreamSynchronize(st));
  }
  for (int32_t i = 0; i < dev.n_nodes; ++i) {std::copy(best_x.begin() + 3 * i, best_x.begin() + 3 * i + 3, s->nodes[i].pose);}
  store_corrections(s);
  sum.total_ms = ms_since(t_begin);
  return finish(KH_OK);
}
