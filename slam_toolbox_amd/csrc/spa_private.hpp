// Private definitions of the pose-graph SPA solver's host side (kh_spa_*, hot path B), shared by its source files:
//   spa_host.cpp         the handle's life, options, sharding, comm and debug; the graph store (add, remove, modify, tombstones,
//                        settle); the plain getters, kh_link_info and the exact host pieces; the session-state export and import
//   spa_graph_file.cpp   kh_spa_save / kh_spa_load, the text and binary parsers
//   spa_problem.cpp      prepare_problem: the problem of a Compute() or a covariance pass on the device, stage by stage
//                        (its device-free stages: spa_problem_plan.hpp)
//   spa_compute.cpp      the linear-algebra pieces Compute() and the covariance pass share, and kh_spa_compute
//   spa_covariance.cpp   the covariance pass, its getters, the constraint audit
//   spa_marginalize.cpp  the marginalizing removal
// Not part of the ABI (include/karto_hip.h); spa_internal.hpp stays the contract with the kernel files (spa_*.hip, listed in spa_device.hpp) and the mapper.  The shared
// names live in kh::spa; what one file alone uses stays in that file's anonymous namespace.
//
// Linear algebra design (MI355X): the normal matrix is factorised by a multifrontal block Cholesky.
// Ordering = geometric nested dissection on the node positions (a pose graph is a geometric graph:
// edges only link poses a few metres apart), which directly yields the supernodes (leaf clusters and
// separators); each supernode's frontal matrix is a small dense problem handled by one workgroup, and
// the elimination tree is processed level by level.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/karto_hip.h"
#include "covariance_columns_plan.hpp"
#include "host_common.hpp"
#include "marginalize.hpp"
#include "spa_internal.hpp"
#include "spa_symbolic.hpp"

#define KS_HIP(call)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      kh::set_error(std::string(#call) + ": " + hipGetErrorString(e_));                      \
      return KH_ERR_HIP;                                                                     \
    }                                                                                        \
  } while (0)

namespace kh
{
namespace spa
{
// `dead`: removed, waiting for settle() (RemoveNode / RemoveConstraint are O(1) / O(degree); a lifelong mapper removes a
// node every other scan, and erasing from the middle of 60 000 constraints + re-keying the maps each time cost ~1 ms per
// removed node)
struct Node {int32_t id; double pose[3]; uint8_t dead = 0;};
struct Constraint {int32_t a, b; double z[3]; double u[9]; double omega[6]; uint8_t dead = 0;};   // omega: upper triangle of the information

// A device array that owns its allocation (freed with the buffer) or names a slice of somebody else's (never freed).
template <class T>
struct DevBuf
{
  typedef T value_type;
  T * p = nullptr; size_t cap = 0;
  bool owned = true;                 // false: p is a slice of another allocation (alias)
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf & operator=(const DevBuf &) = delete;
  ~DevBuf() {release();}
  // the buffer becomes n elements of somebody else's allocation (the analysis' arrays: slices of ONE block, one copy)
  void alias(T * slice, size_t n)
  {
    if (owned && p) {(void)hipFree(p);}
    p = slice; cap = n; owned = false;
  }
  int ensure(size_t n)
  {
    if (!owned) {p = nullptr; cap = 0; owned = true;}
    if (n <= cap) {return KH_OK;}
    if (p) {KS_HIP(hipFree(p)); p = nullptr;}
    cap = std::max(n, cap + cap / 2);
    KS_HIP(hipMalloc(reinterpret_cast<void **>(&p), cap * sizeof(T)));
    // KH_SPA_POISON=1 (debugging aid): new buffers start as NaN / -1 patterns, so that a kernel that reads what nobody
    // wrote shows up as a failed solve instead of as a last-bit difference between two processes
    static const bool poison = std::getenv("KH_SPA_POISON") != nullptr;
    if (poison) {KS_HIP(hipMemset(p, 0xFF, cap * sizeof(T))); KS_HIP(hipDeviceSynchronize());}
    return KH_OK;
  }
  int upload(const std::vector<T> & v, hipStream_t s)
  {
    int rc = ensure(std::max<size_t>(v.size(), 1));
    if (rc) {return rc;}
    if (!v.empty()) {KS_HIP(hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));}
    return KH_OK;
  }
  void release() {if (p && owned) {(void)hipFree(p);} p = nullptr; cap = 0; owned = true;}
};
}  // namespace spa
}  // namespace kh

struct kh_spa
{
  template <class T> using DevBuf = kh::spa::DevBuf<T>;
  int32_t device = 0;
  hipStream_t stream = nullptr;
  // self-cleaning fronts (scatter mode): the buffers these pointers name are all zeros (every kernel of the last factorisation
  // and its backward sweep ran, each zeroing what it was the last to read)
  const double * clean_a = nullptr; const double * clean_b = nullptr;
  DevBuf<int32_t> d_deferred;                  // fronts whose update matrix stays in place (Symbolic::scatter_mode == 0, not a root)
  int32_t n_deferred_fronts = 0, deferred_max_m = 0;
  kh_spa_options opt;
  std::vector<kh::spa::Node> nodes;              // insertion order
  std::unordered_map<int32_t, int32_t> index_of; // id -> position in nodes
  std::vector<kh::spa::Constraint> cons;
  std::unordered_multimap<uint64_t, int32_t> con_of;             // edge_key(a, b) -> position in cons (hashed: settle() re-keys
                                                                 // tens of thousands of constraints before a Compute)
  static uint64_t edge_key(int32_t a, int32_t b) {return (static_cast<uint64_t>(static_cast<uint32_t>(a)) << 32) | static_cast<uint32_t>(b);}
  // the constraint between a and b (in that order) that was added first, -1 = none
  int32_t first_constraint(int32_t a, int32_t b) const
  {
    int32_t best = -1;
    auto range = con_of.equal_range(edge_key(a, b));
    for (auto it = range.first; it != range.second; ++it) {if (best < 0 || it->second < best) {best = it->second;}}
    return best;
  }
  std::unordered_map<int32_t, std::vector<int32_t>> incident;   // node id -> positions in cons of its constraints (dead ones included until settle())
  int32_t n_dead = 0;                            // tombstones in nodes + cons (settle() compacts, order preserved)
  int32_t n_dead_nodes = 0;                      // ... of which nodes
  int32_t first_id = 0; bool has_first = false; bool was_constant_set = false;
  std::vector<int32_t> corr_ids; std::vector<double> corr_poses;
  bool topology_dirty = true;
  // cached problem
  kh::Symbolic sym;
  std::vector<int32_t> free_of_node, node_of_free;
  int32_t fixed_index = -1;
  // signature of the topology the cached analysis belongs to (node count, edge endpoints in order, gauge): a graph that
  // is reset and re-added unchanged -- loadSerializedPoseGraph followed by Compute -- keeps its ordering, symbolic
  // factorisation and device index maps
  std::vector<int32_t> cached_ea, cached_eb; int32_t cached_n = -1, cached_fixed = -2;
  // supernodes of the last nested dissection by NODE ID (incremental re-analysis), the factorisation cost and size it had
  std::vector<std::vector<int32_t>> cached_sn_ids;
  int64_t cached_full_flops = 0; int32_t cached_full_nf = 0; int32_t reuse_count = 0; int32_t cached_full_levels = 0;
  int32_t last_analysis_incremental = 0;
  // device buffers
  DevBuf<int32_t> d_edge_a, d_edge_b, d_free_of_node, d_node_of_free, d_slot_contrib_ptr, d_slot_contrib,
    d_bsr_row_ptr, d_bsr_col, d_bsr_diag, d_node_contrib_ptr, d_node_contrib, d_front_m, d_front_ns,
    d_front_first, d_rows_ptr, d_rows, d_child_ptr, d_child_list, d_relpos_ptr, d_relpos, d_slot_ld,
    d_elim_of_free, d_free_of_elim, d_level_fronts, d_fail;
  DevBuf<int64_t> d_front_off, d_slot_dest, d_winv_off;
  DevBuf<double> d_winv;                       // L11^-T of every front (level pipeline, round 3)
  DevBuf<kh::FrontDesc> d_desc;
  uint8_t * h_upload = nullptr; size_t h_upload_cap = 0;     // pinned staging of an analysis' uploads (one block, ~30 copies out of it)
  DevBuf<int32_t> d_cinv;
  DevBuf<char> d_pack;                         // the analysis' arrays (the DevBufs the upload block of prepare_problem lists are its slices)
  DevBuf<double> d_fronts_b;                   // buffer B of the fronts (Symbolic::scatter_mode)
  DevBuf<double> d_edge_z, d_edge_u, d_edge_lin, d_edge_cost, d_Hg, d_fronts, d_x, d_cand, d_scale,
    d_diag, d_rhs, d_step, d_delta, d_scal;
  double * h_scal = nullptr; int32_t * h_fail = nullptr;
  // host-coherent block the last kernel of an iteration writes its scalars to, and the flag it raises behind them
  double * h_res = nullptr; int32_t * h_res_flag = nullptr; int32_t res_seq = 0;
  // trace of the last Compute(): one row per LM iteration, see kh_spa_iteration_log
  std::vector<std::array<double, 8>> iter_log;
  int32_t n_slots = 0;
  std::vector<int32_t> level_offsets, level_max_m, level_max_ns;
  // per level: the fronts behind the first level_split[l] of it go through k_front_update (they fit one workgroup's LDS), with
  // level_fused_lds[l] bytes of it; level_split[l] = the level's size: none
  std::vector<int32_t> level_split; std::vector<size_t> level_fused_lds;
  // per level: the most rows any of its fronts has below the pivot block (0: the root -- no update launches)
  std::vector<int32_t> level_max_nu;
  DevBuf<double> d_upd, d_partial;
  DevBuf<double> d_Hg_alt, d_best;          // normal equations at the candidate point (speculative); minimum-cost iterate
  // multi-GPU: edge-block sharded linearisation, H and g summed by the caller's collective
  int32_t shard_rank = 0, shard_world = 1;
  kh_allreduce_fn allreduce = nullptr; void * allreduce_user = nullptr;
  kh_comm * comm = nullptr;                    // RCCL communicator of kh_spa_set_comm: the all-reduce happens in the library
  // measurement: event pairs around the phases of an LM iteration (kMaxTimed iterations are timed, the rest only counted)
  static constexpr int kMaxTimed = 64;
  hipEvent_t ev_phase[kMaxTimed][4] = {};     // factor begin, factor end = backward begin, backward end, (spare)
  hipEvent_t ev_lin[2 * kMaxTimed + 2][2] = {};
  double last_symbolic_ms = 0.0;
  int32_t debug_flags = 0;                     // kh_spa_set_debug
  // covariances (kh_spa_compute_covariances): the selected inverse over the fronts' layout, allocated on first use, and the blocks
  // of the inverse on H's pattern; cov_valid falls with every change of the graph or of a pose.  The host copies (the array
  // and the pattern it is addressed by) are fetched by the first getter behind a computation.
  DevBuf<double> d_zbuf, d_cov;
  bool cov_valid = false, cov_on_host = false;
  std::vector<double> h_cov;
  std::vector<int32_t> h_cov_row_ptr, h_cov_col, h_cov_diag;
  hipEvent_t ev_cov[3] = {};
  // covariance columns (kh_spa_compute_covariance_columns): the right-hand sides of the sweeps, the block columns they leave
  // (n_queries x n_free blocks, valid with cov_valid), the plan's lists on the device, and who the queries of the last pass were
  // (free index -1: the gauge node).  A column comes to the host when a getter first asks for it.
  DevBuf<double> d_col_rhs, d_columns, d_rel;
  DevBuf<int32_t> d_col_lists;
  DevBuf<uint64_t> d_col_masks;
  DevBuf<char> d_rel_in;
  // constraint audit (kh_spa_audit_constraints): the audit's own linearisation of all edges and cost slots, what k_edge_audit
  // leaves (4 doubles and a flag per constraint)
  DevBuf<double> d_audit_lin, d_audit_cost, d_audit_out;
  DevBuf<int32_t> d_audit_flag;
  hipEvent_t ev_audit[2] = {};
  std::vector<int32_t> col_ids, col_free, h_col_lists;
  std::vector<std::vector<double>> h_columns;
  kh::CovColumnsPlan col_plan;
  hipEvent_t ev_col[3] = {};
  // marginalizing removal (kh_spa_marginalize_nodes): a round's upload and download, and what the last call did to the graph
  // (the mapper mirrors it: spa_marginalize_edits)
  DevBuf<char> d_marg_in, d_marg_out;
  std::vector<kh::MargEdit> marg_edits;
};

namespace kh
{
namespace spa
{
// ---- spa_host.cpp ----
// drops the tombstones; positions in `nodes` / `cons` and both maps are final again afterwards.  Every entry point that
// hands out positions, counts or the arrays themselves settles first.
void settle(kh_spa * s);
void bury_constraint(kh_spa * s, int32_t k);
int add_constraint_information(kh_spa * s, int32_t id_a, int32_t id_b, const double * z, const double * omega);
void remove_found_node(kh_spa * s, std::unordered_map<int32_t, int32_t>::iterator it);
// U = llt().matrixU() of the information whose upper triangle is omega (ceres_solver.cpp:364-376)
void sqrt_information(const double * omega, double * U);

// ---- spa_problem.cpp ----
// the problem of the graph as it stands on the device, and `dev` filled with it; has_work false: nothing is in the problem
int prepare_problem(kh_spa * s, SpaDev & dev, bool & has_work);

// ---- spa_compute.cpp: pieces Compute() and the covariance pass share ----
// KH_OK, or KH_ERR_INVALID_ARG and its text when a loss is selected whose scale is not positive
int check_loss_scale(const kh_spa * s);
// kh_spa_summary::analysis of the last prepare_problem: 0 cached, 1 full dissection, 2 incremental
int32_t analysis_kind(const kh_spa * s);
// H || g of this rank's edge block -> sums over all ranks; also with one rank of a communicator (identity)
int allreduce_normal_equations(kh_spa * s, const SpaDev & into);
// cost, H and g at the poses `at` (this rank's edge block [e_lo, e_hi), then the all-reduce); ev: an event pair around the
// kernels, or nullptr
int linearize_normal_equations(kh_spa * s, const SpaDev & into, const double * at, double * cost_slot, int32_t e_lo, int32_t e_hi, hipEvent_t * ev);
// the fronts (and buffer B) as zeros at the head of a factorisation: a memset, or nothing where they are known to be clean
int zero_fronts(kh_spa * s, const SpaDev & dev);
// how a front's update matrix reaches its parent (kh_spa_set_debug bits 8, 9): added in by k_syrk (default), read in place by the
// parent, or summed in by an extend-add launch per level (rounds 3-5); returns whether the level pipeline runs
bool select_factor_mode(const kh_spa * s, SpaDev & dev);
// numeric factorisation + forward solve of the assembled fronts, leaves to root
int launch_factor_levels(kh_spa * s, const SpaDev & dev, bool pipeline);
// the loss of the options into dev; returns the edge block [first, second) that this rank linearises (dev.n_edges is set)
std::pair<int32_t, int32_t> set_loss_and_shard(const kh_spa * s, SpaDev & dev);
// d_scale: the Jacobi scaling of the linearised H, or ones (a pageable upload: it has landed when this returns)
int make_scale(kh_spa * s, const SpaDev & dev);
// kh_spa_set_debug bit 0 (every test that checks its linear solves checks this): the self-cleaning fronts must be all zeros
// behind their last reader; `left_by` ends the message
int check_fronts_clean(kh_spa * s, const SpaDev & dev, const char * left_by);

// ---- spa_covariance.cpp ----
// The covariance pass.  query_ids (possibly none): the nodes whose block columns of Sigma are solved for while the factor is
// still in the fronts; without queries the launches are the selected inverse's alone, in their order.
int covariance_pass(kh_spa * s, kh_spa_cov_summary * summary, const std::vector<int32_t> & query_ids, kh_spa_cov_columns_summary * col_summary,
                    const char * caller);
// free index of node `id`: -1 the gauge node; KH_ERR_NOT_FOUND (through rc) for an unknown id or a node without constraints
int covariance_index(kh_spa * s, int32_t id, int32_t & free_index);
}  // namespace spa
}  // namespace kh
