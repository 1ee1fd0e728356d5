// Host side of the pose-graph SPA solver (hot path B): the plugin's handle and its graph store.  The other concerns have files of
// their own (spa_private.hpp lists them); all numeric work runs on the GPU (the spa_*.hip files, listed in spa_device.hpp).
//
// Reference: solvers/ceres_solver.cpp (state + options + gauge), lib/karto_sdk/include/karto_sdk/Mapper.h:954-1066
// (karto::ScanSolver), :174-188 (LinkInfo::Update), Karto.h:2533-2577 (Matrix3::Inverse).
#include <cmath>
#include <cstring>

#include "spa_private.hpp"

using namespace kh;
using namespace kh::spa;

// ---- the graph store's tombstones -----------------------------------------------------------------
void kh::spa::settle(kh_spa * s)
{
  if (!s || s->n_dead == 0) {return;}
  s->cons.erase(std::remove_if(s->cons.begin(), s->cons.end(), [](const Constraint & c) {return c.dead != 0;}), s->cons.end());
  s->nodes.erase(std::remove_if(s->nodes.begin(), s->nodes.end(), [](const Node & n) {return n.dead != 0;}), s->nodes.end());
  s->con_of.clear();
  s->con_of.reserve(s->cons.size());
  s->incident.clear();
  for (size_t k = 0; k < s->cons.size(); ++k) {
    s->con_of.insert({kh_spa::edge_key(s->cons[k].a, s->cons[k].b), static_cast<int32_t>(k)});
    s->incident[s->cons[k].a].push_back(static_cast<int32_t>(k));
    s->incident[s->cons[k].b].push_back(static_cast<int32_t>(k));
  }
  s->index_of.clear();
  for (size_t k = 0; k < s->nodes.size(); ++k) {s->index_of[s->nodes[k].id] = static_cast<int32_t>(k);}
  s->n_dead = 0;
  s->n_dead_nodes = 0;
}

void kh::spa::bury_constraint(kh_spa * s, int32_t k)
{
  Constraint & c = s->cons[k];
  if (c.dead) {return;}
  s->cov_valid = false;
  auto range = s->con_of.equal_range(kh_spa::edge_key(c.a, c.b));
  for (auto it = range.first; it != range.second; ++it) {
    if (it->second == k) {s->con_of.erase(it); break;}
  }
  c.dead = 1;
  ++s->n_dead;
  s->topology_dirty = true;
}

void kh::spa::remove_found_node(kh_spa * s, std::unordered_map<int32_t, int32_t>::iterator it)
{
  const int32_t id = it->first;
  s->cov_valid = false;
  auto inc = s->incident.find(id);                     // O(degree): the node's own constraint list
  if (inc != s->incident.end()) {
    for (int32_t k : inc->second) {bury_constraint(s, k);}
    s->incident.erase(inc);
  }
  s->nodes[it->second].dead = 1;
  ++s->n_dead;
  ++s->n_dead_nodes;
  // ceres_solver.cpp:395-427 erases the node and its parameter blocks; first_node_ keeps pointing at the erased entry
  // there (never dereferenced again once the blocks were set constant).  Here the gauge simply ends with the node: no
  // later node takes it over, and the pose-graph files stop naming it.
  if (s->has_first && id == s->first_id) {s->has_first = false;}
  s->index_of.erase(it);
  s->topology_dirty = true;
}

// ---- exact host pieces ------------------------------------------------------------------------
namespace
{
void matrix3_inverse(const double * m, double * inv)    // Karto.h:2533-2577 (row-major 3x3)
{
  inv[0] = m[4] * m[8] - m[5] * m[7];
  inv[1] = m[2] * m[7] - m[1] * m[8];
  inv[2] = m[1] * m[5] - m[2] * m[4];
  inv[3] = m[5] * m[6] - m[3] * m[8];
  inv[4] = m[0] * m[8] - m[2] * m[6];
  inv[5] = m[2] * m[3] - m[0] * m[5];
  inv[6] = m[3] * m[7] - m[4] * m[6];
  inv[7] = m[1] * m[6] - m[0] * m[7];
  inv[8] = m[0] * m[4] - m[1] * m[3];
  const double det = m[0] * inv[0] + m[1] * inv[3] + m[2] * inv[6];
  if (std::fabs(det) <= 1e-14) {return;}      // assert(false) is compiled out in Release
  const double inv_det = 1.0 / det;
  for (int i = 0; i < 9; ++i) {inv[i] *= inv_det;}
}

// AddConstraint, ceres_solver.cpp:364-376: information = symmetrised inverse (its upper triangle, row-major:
// 00 01 02 11 12 22); U = llt().matrixU()
void information_from_covariance(const double * cov, double * omega)
{
  double p[9];
  matrix3_inverse(cov, p);
  omega[0] = p[0]; omega[1] = p[1]; omega[2] = p[2]; omega[3] = p[4]; omega[4] = p[5]; omega[5] = p[8];
}

double karto_normalize_angle(double angle)   // Math.h:181-202
{
  const double pi = 3.14159265358979323846, two_pi = 6.28318530717958647692;
  while (angle < -pi) {
    if (angle < -two_pi) {angle += static_cast<uint32_t>(angle / -two_pi) * two_pi;} else {angle += two_pi;}
  }
  while (angle > pi) {
    if (angle > two_pi) {angle -= static_cast<uint32_t>(angle / two_pi) * two_pi;} else {angle -= two_pi;}
  }
  return angle;
}
}  // namespace

void kh::spa::sqrt_information(const double * omega, double * U)
{
  const double a00 = omega[0], a01 = omega[1], a02 = omega[2], a11 = omega[3], a12 = omega[4], a22 = omega[5];
  const double l00 = std::sqrt(a00);
  const double l10 = a01 / l00, l20 = a02 / l00;
  const double l11 = std::sqrt(a11 - l10 * l10);
  const double l21 = (a12 - l20 * l10) / l11;
  const double l22 = std::sqrt(a22 - l20 * l20 - l21 * l21);
  U[0] = l00; U[1] = l10; U[2] = l20;
  U[3] = 0.0; U[4] = l11; U[5] = l21;
  U[6] = 0.0; U[7] = 0.0; U[8] = l22;
}

int kh::spa::add_constraint_information(kh_spa * s, int32_t id_a, int32_t id_b, const double * z, const double * omega)
{
  if (!s->index_of.count(id_a) || !s->index_of.count(id_b) || id_a == id_b) {
    set_error("CeresSolver: Failed to add constraint, could not find nodes.");
    return KH_ERR_NOT_FOUND;
  }
  Constraint c; c.a = id_a; c.b = id_b;
  std::copy(z, z + 3, c.z);
  std::copy(omega, omega + 6, c.omega);
  sqrt_information(c.omega, c.u);
  if (!(c.u[0] > 0.0 && c.u[4] > 0.0 && c.u[8] > 0.0)) {     // also false for NaN: llt() of a matrix that is not positive definite
    set_error("CeresSolver: constraint information matrix is not positive definite");
    return KH_ERR_INVALID_ARG;
  }
  s->con_of.insert({kh_spa::edge_key(id_a, id_b), static_cast<int32_t>(s->cons.size())});
  s->incident[id_a].push_back(static_cast<int32_t>(s->cons.size()));
  s->incident[id_b].push_back(static_cast<int32_t>(s->cons.size()));
  s->cons.push_back(c);
  s->cov_valid = false;
  s->topology_dirty = true;
  return KH_OK;
}

// ---- the handle's life -------------------------------------------------------------------------
namespace
{
// the stream, the pinned blocks and the events of a new handle; what a failure leaves half made is kh_spa_destroy's
int create_resources(kh_spa * s)
{
  KS_HIP(hipSetDevice(s->device));
  KS_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  KS_HIP(hipHostMalloc(reinterpret_cast<void **>(&s->h_scal), sizeof(double) * 32, hipHostMallocDefault));
  KS_HIP(hipHostMalloc(reinterpret_cast<void **>(&s->h_fail), sizeof(int32_t) * 4, hipHostMallocDefault));
  // (a platform without host-coherent mappings keeps the copies + stream drain)
  if (hipHostMalloc(reinterpret_cast<void **>(&s->h_res), sizeof(double) * 16 + 64, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
    s->h_res_flag = reinterpret_cast<int32_t *>(s->h_res + 16);
    s->h_res_flag[0] = 0;
  } else {
    (void)hipGetLastError();
    s->h_res = nullptr;
  }
  for (auto & row : s->ev_phase) {for (auto & e : row) {KS_HIP(hipEventCreate(&e));}}
  for (auto & row : s->ev_lin) {for (auto & e : row) {KS_HIP(hipEventCreate(&e));}}
  for (auto & e : s->ev_cov) {KS_HIP(hipEventCreate(&e));}
  for (auto & e : s->ev_col) {KS_HIP(hipEventCreate(&e));}
  for (auto & e : s->ev_audit) {KS_HIP(hipEventCreate(&e));}
  return KH_OK;
}
}  // namespace

// =============================================================================================
extern "C" {

void kh_spa_options_default(kh_spa_options * o)
{
  // ceres_solver.cpp:157-186; max_num_iterations is left at the Ceres default
  o->max_num_iterations = 50;
  o->function_tolerance = 1e-3; o->gradient_tolerance = 1e-6; o->parameter_tolerance = 1e-3;
  o->min_relative_decrease = 1e-3;
  o->initial_trust_region_radius = 1e4; o->max_trust_region_radius = 1e8; o->min_trust_region_radius = 1e-16;
  o->min_lm_diagonal = 1e-6; o->max_lm_diagonal = 1e32;
  o->max_num_consecutive_invalid_steps = 3; o->use_nonmonotonic_steps = 1;
  o->max_consecutive_nonmonotonic_steps = 3; o->jacobi_scaling = 1;
  o->loss_function = KH_LOSS_NONE; o->loss_scale = 0.7;
}

int kh_spa_create(int32_t device, kh_spa ** out)
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    set_error("no usable HIP device (libkartohip has no CPU fallback)");
    return KH_ERR_NO_DEVICE;
  }
  kh_spa * s = new kh_spa();
  s->device = device;
  kh_spa_options_default(&s->opt);
  const int rc = create_resources(s);
  if (rc) {kh_spa_destroy(s); return rc;}
  *out = s;
  return KH_OK;
}

// (the device buffers free themselves with the handle: DevBuf owns its allocation)
void kh_spa_destroy(kh_spa * s)
{
  if (!s) {return;}
  (void)hipSetDevice(s->device);
  if (s->stream) {(void)hipStreamSynchronize(s->stream);}
  for (auto & row : s->ev_phase) {for (auto & e : row) {if (e) {(void)hipEventDestroy(e);}}}
  for (auto & row : s->ev_lin) {for (auto & e : row) {if (e) {(void)hipEventDestroy(e);}}}
  for (auto & e : s->ev_cov) {if (e) {(void)hipEventDestroy(e);}}
  for (auto & e : s->ev_col) {if (e) {(void)hipEventDestroy(e);}}
  for (auto & e : s->ev_audit) {if (e) {(void)hipEventDestroy(e);}}
  if (s->h_scal) {(void)hipHostFree(s->h_scal);}
  if (s->h_res) {(void)hipHostFree(s->h_res);}
  if (s->h_upload) {(void)hipHostFree(s->h_upload);}
  if (s->h_fail) {(void)hipHostFree(s->h_fail);}
  if (s->stream) {(void)hipStreamDestroy(s->stream);}
  delete s;
}

int kh_spa_set_options(kh_spa * s, const kh_spa_options * o)
{
  if (!s || !o) {return KH_ERR_INVALID_ARG;}
  s->opt = *o;
  return KH_OK;
}

int kh_spa_set_sharding(kh_spa * s, int32_t rank, int32_t world, kh_allreduce_fn fn, void * user)
{
  if (!s || world < 1 || rank < 0 || rank >= world || (world > 1 && !fn)) {return KH_ERR_INVALID_ARG;}
  s->shard_rank = rank; s->shard_world = world; s->allreduce = fn; s->allreduce_user = user; s->comm = nullptr;
  return KH_OK;
}

int kh_spa_set_comm(kh_spa * s, kh_comm * comm)
{
  if (!s) {return KH_ERR_INVALID_ARG;}
  if (comm && kh_comm_device(comm) != s->device) {
    set_error("kh_spa_set_comm: the communicator lives on another device than the solver");
    return KH_ERR_INVALID_ARG;
  }
  s->comm = comm; s->allreduce = nullptr; s->allreduce_user = nullptr;
  s->shard_rank = comm ? kh_comm_rank(comm) : 0;
  s->shard_world = comm ? kh_comm_world(comm) : 1;
  return KH_OK;
}

int kh_spa_set_debug(kh_spa * s, int32_t flags)
{
  if (!s) {return KH_ERR_INVALID_ARG;}
  s->debug_flags = flags;
  return KH_OK;
}

// ---- the graph store ---------------------------------------------------------------------------
int kh_spa_reset(kh_spa * s)     // ceres_solver.cpp:279-314
{
  if (!s) {return KH_ERR_INVALID_ARG;}
  s->cov_valid = false;
  if (s->d_col_rhs.p || s->d_columns.p) {
    // (the columns' buffers are the large ones of the handle: 46 MB at 10 000 nodes and 64 queries)
    (void)hipSetDevice(s->device);
    if (s->stream) {(void)hipStreamSynchronize(s->stream);}
    s->d_col_rhs.release(); s->d_columns.release();
  }
  s->col_ids.clear(); s->col_free.clear(); s->h_columns.clear();
  s->nodes.clear(); s->index_of.clear(); s->cons.clear(); s->con_of.clear(); s->incident.clear(); s->n_dead = 0; s->n_dead_nodes = 0;
  s->corr_ids.clear(); s->corr_poses.clear();
  s->has_first = false; s->was_constant_set = false; s->topology_dirty = true; s->fixed_index = -1;
  s->cached_sn_ids.clear(); s->reuse_count = 0;        // a rebuilt graph is dissected from scratch
  return KH_OK;
}

int kh_spa_clear(kh_spa * s)     // ceres_solver.cpp:272-276
{
  if (!s) {return KH_ERR_INVALID_ARG;}
  s->cov_valid = false;
  s->corr_ids.clear(); s->corr_poses.clear();
  return KH_OK;
}

int kh_spa_add_node(kh_spa * s, int32_t id, const double pose[3])    // ceres_solver.cpp:317-336
{
  if (!s || !pose) {return KH_ERR_INVALID_ARG;}
  if (s->index_of.count(id)) {return KH_OK;}       // unordered_map::insert keeps the existing entry
  s->cov_valid = false;
  Node n; n.id = id; std::copy(pose, pose + 3, n.pose);
  s->index_of[id] = static_cast<int32_t>(s->nodes.size());
  s->nodes.push_back(n);
  // the reference sets first_node_ whenever nodes_->size() == 1 after the insert (ceres_solver.cpp:331-334); tombstoned
  // nodes are already gone from its map, so they do not count here either
  if (static_cast<int32_t>(s->nodes.size()) - s->n_dead_nodes == 1) {s->first_id = id; s->has_first = true;}
  s->topology_dirty = true;
  return KH_OK;
}

int kh_spa_add_constraint(kh_spa * s, int32_t id_a, int32_t id_b, const double z[3], const double cov[9])   // :339-392
{
  if (!s || !z || !cov) {return KH_ERR_INVALID_ARG;}
  double omega[6];
  information_from_covariance(cov, omega);
  return add_constraint_information(s, id_a, id_b, z, omega);
}

int kh_spa_add_constraint_information(kh_spa * s, int32_t id_a, int32_t id_b, const double z[3], const double info_upper[6])
{
  if (!s || !z || !info_upper) {return KH_ERR_INVALID_ARG;}
  return add_constraint_information(s, id_a, id_b, z, info_upper);
}

int kh_spa_remove_node(kh_spa * s, int32_t id)     // ceres_solver.cpp:395-427 (RemoveParameterBlock drops its residuals)
{
  if (!s) {return KH_ERR_INVALID_ARG;}
  auto it = s->index_of.find(id);
  if (it == s->index_of.end()) {set_error("RemoveNode: Failed to find node matching id"); return KH_ERR_NOT_FOUND;}
  remove_found_node(s, it);
  return KH_OK;
}

int kh_spa_remove_constraint(kh_spa * s, int32_t id_a, int32_t id_b)    // ceres_solver.cpp:430-448
{
  if (!s) {return KH_ERR_INVALID_ARG;}
  int32_t k = s->first_constraint(id_a, id_b);
  if (k < 0) {k = s->first_constraint(id_b, id_a);}
  if (k < 0) {set_error("RemoveConstraint: Failed to find residual block"); return KH_ERR_NOT_FOUND;}
  bury_constraint(s, k);
  return KH_OK;
}

int kh_spa_modify_node(kh_spa * s, int32_t id, const double pose[3])    // ceres_solver.cpp:451-461
{
  if (!s || !pose) {return KH_ERR_INVALID_ARG;}
  auto it = s->index_of.find(id);
  if (it == s->index_of.end()) {return KH_ERR_NOT_FOUND;}
  Node & n = s->nodes[it->second];
  const double yaw_init = n.pose[2];
  s->cov_valid = false;
  n.pose[0] = pose[0]; n.pose[1] = pose[1]; n.pose[2] = pose[2];
  n.pose[2] += yaw_init;
  return KH_OK;
}

// ---- plain getters -----------------------------------------------------------------------------
int kh_spa_get_constraint(kh_spa * s, int32_t index, int32_t * id_a, int32_t * id_b, double z[3], double info_upper[6])
{
  settle(s);
  if (!s || index < 0) {return KH_ERR_INVALID_ARG;}
  if (index >= static_cast<int32_t>(s->cons.size())) {return KH_ERR_NOT_FOUND;}
  const Constraint & c = s->cons[index];
  if (id_a) {*id_a = c.a;}
  if (id_b) {*id_b = c.b;}
  if (z) {std::copy(c.z, c.z + 3, z);}
  if (info_upper) {std::copy(c.omega, c.omega + 6, info_upper);}
  return KH_OK;
}

int kh_spa_get_nodes(kh_spa * s, int32_t * ids, double * poses)
{
  settle(s);
  if (!s) {return KH_ERR_INVALID_ARG;}
  for (size_t k = 0; k < s->nodes.size(); ++k) {
    if (ids) {ids[k] = s->nodes[k].id;}
    if (poses) {std::copy(s->nodes[k].pose, s->nodes[k].pose + 3, poses + 3 * k);}
  }
  return KH_OK;
}

int kh_spa_get_node_at(kh_spa * s, int32_t index, int32_t * id, double pose[3])
{
  settle(s);
  if (!s || index < 0) {return KH_ERR_INVALID_ARG;}
  if (index >= static_cast<int32_t>(s->nodes.size())) {return KH_ERR_NOT_FOUND;}
  if (id) {*id = s->nodes[index].id;}
  if (pose) {std::copy(s->nodes[index].pose, s->nodes[index].pose + 3, pose);}
  return KH_OK;
}

int kh_spa_get_node(kh_spa * s, int32_t id, double pose[3])
{
  if (!s || !pose) {return KH_ERR_INVALID_ARG;}
  auto it = s->index_of.find(id);
  if (it == s->index_of.end()) {return KH_ERR_NOT_FOUND;}
  std::copy(s->nodes[it->second].pose, s->nodes[it->second].pose + 3, pose);
  return KH_OK;
}

int32_t kh_spa_num_nodes(kh_spa * s) {settle(s); return s ? static_cast<int32_t>(s->nodes.size()) : 0;}
int32_t kh_spa_num_constraints(kh_spa * s) {settle(s); return s ? static_cast<int32_t>(s->cons.size()) : 0;}

int kh_spa_iteration_log(kh_spa * s, int32_t capacity, double * rows, int32_t * n_rows)
{
  if (!s || !n_rows || capacity < 0 || (capacity > 0 && !rows)) {return KH_ERR_INVALID_ARG;}
  *n_rows = static_cast<int32_t>(s->iter_log.size());
  const int32_t n = std::min(capacity, *n_rows);
  for (int32_t i = 0; i < n; ++i) {std::copy(s->iter_log[i].begin(), s->iter_log[i].end(), rows + 8 * static_cast<size_t>(i));}
  return KH_OK;
}

int kh_spa_get_corrections(kh_spa * s, int32_t * n, int32_t * ids, double * poses)
{
  if (!s || !n) {return KH_ERR_INVALID_ARG;}
  *n = static_cast<int32_t>(s->corr_ids.size());
  if (ids) {std::copy(s->corr_ids.begin(), s->corr_ids.end(), ids);}
  if (poses) {std::copy(s->corr_poses.begin(), s->corr_poses.end(), poses);}
  return KH_OK;
}

int kh_link_info(const double pose1[3], const double pose2[3], const double cov[9], double diff[3], double cov_out[9])
{
  if (!pose1 || !pose2 || !cov || !diff || !cov_out) {return KH_ERR_INVALID_ARG;}
  // LinkInfo::Update, Mapper.h:174-188; Transform(rPose1, Pose2()), Karto.h:3003-3024
  const double x1 = pose1[0], y1 = pose1[1], t1 = pose1[2];
  double c = 1.0, sn = 0.0, tx = 0.0, ty = 0.0, tth = 0.0;
  if (!(x1 == 0.0 && y1 == 0.0 && t1 == 0.0)) {
    ::sincos(0.0 - t1, &sn, &c);             // one sincos like the reference's GCC build (see ref_sincos in matcher_host.cpp)
    if (x1 != 0.0 || y1 != 0.0) {
      tx = 0.0 - (c * x1 + (0.0 - sn) * y1 + 0.0 * t1);
      ty = 0.0 - (sn * x1 + c * y1 + 0.0 * t1);
    }
    tth = 0.0 - t1;
  }
  diff[0] = tx + (c * pose2[0] + (0.0 - sn) * pose2[1] + 0.0 * pose2[2]);
  diff[1] = ty + (sn * pose2[0] + c * pose2[1] + 0.0 * pose2[2]);
  diff[2] = karto_normalize_angle(pose2[2] + tth);
  // covariance rotated into the frame of pose1: R(-t1) * cov * R(-t1)^T (Matrix3 triple-loop products)
  double cr, sr;
  ::sincos(-t1, &sr, &cr);
  const double omc = 1.0 - cr;      // Matrix3::FromAxisAngle(0, 0, 1, -t1), Karto.h:2482-2511
  const double R[9] = {0.0 * omc + cr, 0.0 - sr, 0.0, 0.0 + sr, 0.0 * omc + cr, 0.0, 0.0, 0.0, 1.0 * omc + cr};
  double tmp[9], Rt[9];
  for (int r = 0; r < 3; ++r) {for (int q = 0; q < 3; ++q) {Rt[3 * r + q] = R[3 * q + r];}}
  for (int r = 0; r < 3; ++r) {
    for (int q = 0; q < 3; ++q) {
      tmp[3 * r + q] = R[3 * r] * cov[q] + R[3 * r + 1] * cov[3 + q] + R[3 * r + 2] * cov[6 + q];
    }
  }
  for (int r = 0; r < 3; ++r) {
    for (int q = 0; q < 3; ++q) {
      cov_out[3 * r + q] = tmp[3 * r] * Rt[q] + tmp[3 * r + 1] * Rt[3 + q] + tmp[3 * r + 2] * Rt[6 + q];
    }
  }
  return KH_OK;
}

}  // extern "C"

// ---- the part of the solver's state a mapping session file carries besides nodes and constraints (mapper_session.cpp) ----
// The gauge bookkeeping (first_node_ and whether it was set constant) and the analysis cache that makes the next Compute()
// history dependent: the supernodes of the last full dissection by node id, its cost and size, and how many incremental
// re-analyses have leaned on it since.  words: [0] has_first, [1] first_id, [2] was_constant_set, [3] cached_full_flops,
// [4] cached_full_nf, [5] reuse_count, [6] cached_full_levels; the supernodes as a CSR list of node ids.
namespace kh
{
void spa_export_session_state(kh_spa * s, int64_t words[7], std::vector<int32_t> & sn_ptr, std::vector<int32_t> & sn_ids)
{
  settle(s);
  words[0] = s->has_first ? 1 : 0; words[1] = s->first_id; words[2] = s->was_constant_set ? 1 : 0;
  words[3] = s->cached_full_flops; words[4] = s->cached_full_nf; words[5] = s->reuse_count; words[6] = s->cached_full_levels;
  sn_ptr.assign(1, 0); sn_ids.clear();
  for (const auto & ids : s->cached_sn_ids) {
    sn_ids.insert(sn_ids.end(), ids.begin(), ids.end());
    sn_ptr.push_back(static_cast<int32_t>(sn_ids.size()));
  }
}

// after kh_spa_reset + AddNode* + AddConstraint* of the stored graph (which leave a first node and an empty cache behind)
void spa_import_session_state(kh_spa * s, const int64_t words[7], const std::vector<int32_t> & sn_ptr, const std::vector<int32_t> & sn_ids)
{
  s->has_first = words[0] != 0; s->first_id = static_cast<int32_t>(words[1]); s->was_constant_set = words[2] != 0;
  s->cached_full_flops = words[3]; s->cached_full_nf = static_cast<int32_t>(words[4]);
  s->reuse_count = static_cast<int32_t>(words[5]); s->cached_full_levels = static_cast<int32_t>(words[6]);
  s->cached_sn_ids.assign(sn_ptr.empty() ? 0 : sn_ptr.size() - 1, {});
  for (size_t k = 0; k + 1 < sn_ptr.size(); ++k) {s->cached_sn_ids[k].assign(sn_ids.begin() + sn_ptr[k], sn_ids.begin() + sn_ptr[k + 1]);}
  s->topology_dirty = true;
}
}  // namespace kh
