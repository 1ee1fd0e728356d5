/*
 * karto_hip.h -- C ABI of libkartohip.so, the MI355X (gfx950) implementation of slam_toolbox's
 * data-parallel hot path:
 *   (A) karto correlative scan matcher   (reference: lib/karto_sdk/src/Mapper.cpp:477-1208,
 *                                          lib/karto_sdk/include/karto_sdk/Mapper.h:1074-1544,
 *                                          Karto.h:6603-6963)
 *   (B) pose-graph SPA solver plugin     (reference: solvers/ceres_solver.cpp, solvers/ceres_utils.h,
 *                                          karto::ScanSolver Mapper.h:954-1066)
 *
 * Everything is POD: plain pointers and sizes, caller-owned buffers, int status returns.  No C++
 * or torch types cross this boundary.  A handle is NOT re-entrant (like karto::ScanMatcher,
 * which keeps per-call state in members, Mapper.cpp:767-772); different handles may be used
 * from different threads.  The thin C++ adaptors that restore the reference's class surface
 * (karto::ScanMatcher / karto::ScanSolver look-alikes) live in include/karto_hip/ and are
 * header-only over this ABI; INTEGRATION.md shows the binding a slam_toolbox maintainer adds.
 *
 * All paths compute on the GPU.  There is no CPU fallback: every entry point that needs the
 * device returns KH_ERR_NO_DEVICE when no gfx950 device / HIP runtime is usable.
 */
#ifndef KARTO_HIP_H_
#define KARTO_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KH_API __attribute__((visibility("default")))

/* ---------------------------------------------------------------- status codes */
enum {
  KH_OK = 0,
  KH_ERR_INVALID_ARG = 1,   /* ScanMatcher::Create returns NULL (Mapper.cpp:481-493) / smear out of range throws (Mapper.h:1226-1235) */
  KH_ERR_NO_DEVICE = 2,     /* no HIP device: the product has no CPU fallback */
  KH_ERR_HIP = 3,           /* a HIP runtime call failed (kh_last_error() has the text) */
  KH_ERR_SEARCH = 4,        /* the reference throws std::runtime_error (Mapper.cpp:786-796, 828) */
  KH_ERR_NOT_FOUND = 5,     /* unknown node / constraint id (reference logs and returns) */
  KH_ERR_SOLVER = 6,        /* solution not usable (ceres_solver.cpp:249-254): state left unchanged */
  KH_ERR_IO = 7             /* a pose-graph or session file could not be read / written */
};

KH_API const char * kh_last_error(void);
KH_API int kh_device_count(void);           /* 0 when no GPU is visible */
KH_API const char * kh_version(void);

/* ---------------------------------------------------------------- scans */
/* What the matcher reads from a karto::LocalizedRangeScan (Karto.h:5380-5760):
 *   ranges       GetRangeReadings()                      n doubles (NaN / inf allowed)
 *   points_xy    GetPointReadings(false): the UNFILTERED world points of all n beams as left by
 *                the scan's last Update() (Karto.h:5644-5704), x0,y0,x1,y1,...
 *   sensor_pose  GetSensorPose()                         x, y, heading
 * Buffers are host memory owned by the caller and only read during the call. */
typedef struct kh_scan {
  int32_t n;
  const double * ranges;
  const double * points_xy;
  double sensor_pose[3];
  /* optional (NULL = not resident): the same 2 * n doubles as points_xy in DEVICE memory of the matcher's device
   * (kh_device_malloc / kh_device_upload).  A scan used as a BASE scan (AddScans / MatchScan) is then read where it
   * lies instead of being uploaded with every call -- the scan store of a mapper belongs in HBM (173 MB
   * for 10 k scans); the caller re-uploads when the scan's pose changes (LocalizedRangeScan::Update).  points_xy must
   * still be valid: the query side and the host half read it. */
  const double * device_points_xy;
} kh_scan;

/* helper restating LocalizedRangeScan::Update for callers without karto objects
 * (Karto.h:5644-5704): pt_i = pose + r_i * (cos, sin)(heading + min_angle + i * ang_res) */
KH_API int kh_scan_points(const double * ranges, int32_t n, const double sensor_pose[3],
                          double min_angle, double angular_resolution, double * out_points_xy);

/* ---------------------------------------------------------------- scan matcher (A) */
typedef struct kh_matcher kh_matcher;

/* The eight Mapper parameters ScanMatcher reads through friend access
 * (Mapper.cpp:590-591, 600, 626-627, 674-682), AS STORED by karto::Mapper -- i.e. the two
 * variance penalties are the already-squared values (setters square them, Mapper.cpp:2562-2570). */
typedef struct kh_match_params {
  double coarse_search_angle_offset;   /* m_pCoarseSearchAngleOffset */
  double coarse_angle_resolution;      /* m_pCoarseAngleResolution   */
  double fine_search_angle_offset;     /* m_pFineSearchAngleOffset   */
  int32_t use_response_expansion;      /* m_pUseResponseExpansion    */
  double distance_variance_penalty;    /* m_pDistanceVariancePenalty (squared) */
  double minimum_distance_penalty;     /* m_pMinimumDistancePenalty  */
  double angle_variance_penalty;       /* m_pAngleVariancePenalty (squared) */
  double minimum_angle_penalty;        /* m_pMinimumAnglePenalty     */
} kh_match_params;

/* karto defaults of Mapper::InitializeParameters (Mapper.cpp:2250-2293) */
KH_API void kh_match_params_default(kh_match_params * p);

/* ScanMatcher::Create (Mapper.cpp:477-522).  device = HIP device ordinal; max_batch = number of
 * independent matches one kh_matcher_match_batch call may carry (each owns a correlation grid in
 * HBM: (side + 2*ceil(range/res) + 2*border)^2 bytes). */
KH_API int kh_matcher_create(double search_size, double resolution, double smear_deviation,
                             double range_threshold, int32_t device, int32_t max_batch,
                             kh_matcher ** out);
KH_API void kh_matcher_destroy(kh_matcher * m);
KH_API int kh_matcher_set_params(kh_matcher * m, const kh_match_params * p);

/* ScanMatcher::MatchScan<LocalizedRangeScanVector> (Mapper.cpp:534-639); base scans in container
 * order.  mean = x, y, heading; cov = row-major 3x3; *response in [0, 1]. */
KH_API int kh_matcher_match(kh_matcher * m, const kh_scan * query, const kh_scan * base,
                            int32_t n_base, int32_t do_penalize, int32_t do_refine,
                            double mean[3], double cov[9], double * response);

/* n independent MatchScan calls in one pass (loop-closure candidate batches, BASELINE config 3).
 * base scans of all matches are concatenated; base_begin[i]..base_begin[i+1] delimits match i
 * (n+1 entries).  status[i] is the per-match status. */
KH_API int kh_matcher_match_batch(kh_matcher * m, int32_t n, const kh_scan * queries,
                                  const kh_scan * base, const int32_t * base_begin,
                                  int32_t do_penalize, int32_t do_refine,
                                  double * means /* 3n */, double * covs /* 9n */,
                                  double * responses /* n */, int32_t * status /* n */);

/* ---- the same batch over several devices of ONE process (loop-closure candidate batches shard
 * across the GPUs of a node; replaces nothing in the reference, which walks the candidates one at a time,
 * Mapper.cpp:1500-1561).  One matcher per entry of `devices` (the same device may be listed more than once: independent
 * members sharing a GPU), each driven by its own host thread; candidate i goes to member i % n_members, every member
 * works through its share in chunks of at most max_batch_per_member, and the results come back in candidate order -- what
 * TryCloseLoop's first-acceptance rule needs.  No collective: the matches are independent.
 * base_device_points: NULL, or n_members pointers per base scan, entry [t * n_members + k] = the copy of base[t]'s
 * points_xy in the memory of member k's device (NULL = not resident there: the member uploads the scan itself);
 * kh_scan.device_points_xy is only honoured by a one-member group without such a table. */
typedef struct kh_matcher_group kh_matcher_group;
KH_API int kh_matcher_group_create(double search_size, double resolution, double smear_deviation, double range_threshold,
                                   const int32_t * devices, int32_t n_devices, int32_t max_batch_per_member,
                                   kh_matcher_group ** out);
KH_API void kh_matcher_group_destroy(kh_matcher_group * g);
KH_API int kh_matcher_group_set_params(kh_matcher_group * g, const kh_match_params * p);
KH_API int32_t kh_matcher_group_size(const kh_matcher_group * g);
KH_API kh_matcher * kh_matcher_group_member(kh_matcher_group * g, int32_t index);     /* owned by the group */
KH_API int32_t kh_matcher_group_device(const kh_matcher_group * g, int32_t index);
KH_API int kh_matcher_group_match_batch(kh_matcher_group * g, int32_t n, const kh_scan * queries, const kh_scan * base,
                                        const int32_t * base_begin, const double * const * base_device_points,
                                        int32_t do_penalize, int32_t do_refine, double * means /* 3n */,
                                        double * covs /* 9n */, double * responses /* n */, int32_t * status /* n */);

/* MapperGraph::TryCloseLoop's pair of matches (Mapper.cpp:1515-1549) for n candidate chains at once: the coarse match of
 * queries[i] against base[base_begin[i] .. base_begin[i + 1]) on the loop matcher `coarse` (doPenalize false, doRefineMatch
 * false), the gate (response > minimum_response_coarse, cov(0,0) and cov(1,1) < maximum_variance_coarse: passed[i]), and for
 * the chains that pass the match of the temporary scan at the coarse pose (the same ranges, point readings recomputed with
 * kh_scan_points for min_angle / angular_resolution) on the sequential matcher `fine` (doPenalize false, refined).  The
 * batch is cut into `pieces` (1 = the two batches one after the other, which measures fastest on one GPU: 10.0 ms against
 * 10.4 ms with 4 pieces for 256 chains) and the two matchers work on neighbouring pieces at the same time.  fine_* entries of chains that did not pass are left untouched.  Both matchers need
 * max_batch >= ceil(n / pieces); their base scans' device_points_xy, if any, must live on BOTH matchers' device. */
KH_API int kh_loop_closure_batch(kh_matcher * coarse, kh_matcher * fine, int32_t n, const kh_scan * queries, const kh_scan * base,
                                 const int32_t * base_begin, double min_angle, double angular_resolution,
                                 double minimum_response_coarse, double maximum_variance_coarse, int32_t pieces,
                                 double * coarse_means, double * coarse_covs, double * coarse_responses, int32_t * passed,
                                 double * fine_means, double * fine_covs, double * fine_responses);

/* MatchScan steps 1-4 + AddScans only (Mapper.cpp:543-574): centre the grid of batch slot
 * `slot` on the query's sensor pose and rasterise the base scans into it. */
KH_API int kh_matcher_add_scans(kh_matcher * m, int32_t slot, const kh_scan * query,
                                const kh_scan * base, int32_t n_base);

/* ScanMatcher::CorrelateScan (Mapper.cpp:712-862) against the grid currently rasterised in
 * `slot`.  cov is in/out: the fine pass (doing_fine_match) only rewrites cov[8]. */
KH_API int kh_matcher_correlate(kh_matcher * m, int32_t slot, const kh_scan * query,
                                const double center[3], const double search_offset[2],
                                const double search_resolution[2], double angle_offset,
                                double angle_resolution, int32_t do_penalize,
                                int32_t doing_fine_match, double mean[3], double cov[9],
                                double * response);

/* The same CorrelateScan on n slots at once (one launch per kernel for the whole batch);
 * arrays are per-slot (slot i uses queries[i], centers[3i..], ...). */
KH_API int kh_matcher_correlate_batch(kh_matcher * m, int32_t n, const kh_scan * queries,
                                      const double * centers, const double search_offset[2],
                                      const double search_resolution[2], double angle_offset,
                                      double angle_resolution, int32_t do_penalize,
                                      int32_t doing_fine_match, double * means, double * covs,
                                      double * responses, int32_t * status);

/* ScanMatcher::ComputePositionalCovariance (Mapper.cpp:874-966): walks the search-space probabilities the last COARSE
 * CorrelateScan of `slot` left behind (the reference keeps them in m_pSearchSpaceProbs) with the caller's geometry. */
KH_API int kh_matcher_positional_covariance(kh_matcher * m, int32_t slot, const double best_pose[3], double best_response,
                                            const double center[3], const double search_offset[2],
                                            const double search_resolution[2], double angle_resolution, double cov[9]);
/* ScanMatcher::ComputeAngularCovariance (Mapper.cpp:977-1025) for `query` against the grid in `slot`: only cov[8] is
 * written.  (The reference reads the lookup table of its last CorrelateScan; here the scan is named.) */
KH_API int kh_matcher_angular_covariance(kh_matcher * m, int32_t slot, const kh_scan * query, const double best_pose[3],
                                         double best_response, const double center[3], double angle_offset,
                                         double angle_resolution, double cov[9]);

/* ---- introspection used by the parity tests and the bench (not needed by the adaptor) ---- */
typedef struct kh_grid_info {
  int32_t width, height, width_step, data_size;      /* Grid<kt_int8u> incl. border (Karto.h:4636-4664) */
  int32_t roi_x, roi_y, roi_w, roi_h;                /* CorrelationGrid ROI (Mapper.h:1204) */
  int32_t kernel_size;                               /* Mapper.h:1240 */
  int32_t search_side;                               /* side of the search-space-probs grid (Mapper.cpp:498) */
  double offset_x, offset_y, scale;                  /* CoordinateConverter of `slot` */
} kh_grid_info;
KH_API int kh_matcher_grid_info(kh_matcher * m, int32_t slot, kh_grid_info * out);
KH_API int kh_matcher_read_grid(kh_matcher * m, int32_t slot, uint8_t * out /* data_size */);
KH_API int kh_matcher_read_kernel(kh_matcher * m, uint8_t * out /* kernel_size^2 */);
/* last lookup table of `slot`: n_angles x n_points int32 (Karto.h:6797-6894); pass out=NULL to query sizes */
KH_API int kh_matcher_read_lookup(kh_matcher * m, int32_t slot, int32_t * n_angles,
                                  int32_t * n_points, int32_t * out);
/* last response volume of `slot` in the reference's order ((y*nX + x)*nAngles + a), Mapper.cpp:688:
 * raw integer sums (GetResponse numerator, Mapper.cpp:1200) and the penalised responses */
KH_API int kh_matcher_read_volume(kh_matcher * m, int32_t slot, int32_t * nx, int32_t * ny,
                                  int32_t * na, int32_t * out_sums, double * out_responses);
/* search-space probabilities (m_pSearchSpaceProbs, Mapper.cpp:781-799) of the last COARSE CorrelateScan of `slot`: for every
 * cell of its lattice the best response over the search angles, ny rows of nx doubles; pass out=NULL to query sizes.
 * KH_ERR_NOT_FOUND when the slot has run no coarse search.  Host-side state: no GPU work. */
KH_API int kh_matcher_read_search_probabilities(kh_matcher * m, int32_t slot, int32_t * nx, int32_t * ny, double * out);
/* bit 0: keep the penalised response volume of every CorrelateScan on the device so that
 * kh_matcher_read_volume can return it (parity tests); bit 1: score EVERY search the LDS-staged kernels can take through
 * them (by default only the large ones: windows of at most 61 bytes x 64 rows with >= 1e8 lookups per search, where they
 * were measured faster); bit 6: none (the windowed kernel scores everything); bit 2: dense scoring --
 * do not leave out the beams whose whole search window lies in grid blocks no scan point was stamped into
 * (they add 0 to every pose, so the results are identical either way; for measurements); bit 3: send every batch
 * of >= 128 searches through the chunked pipeline, which otherwise only large searches take (tests); bit 4: score from the
 * grid itself instead of its re-pitched copies (same results; for measurements); bit 7: kh_matcher_match takes the general
 * (batch) path instead of the fused path of one MatchScan (same results; the parity tests compare the two).  Results are
 * identical under every combination. */
KH_API int kh_matcher_set_debug(kh_matcher * m, int32_t flags);
/* Counters of the fused path ONE MatchScan takes (kh_matcher_match, Mapper.cpp:534-639; csrc/matcher_seq.cpp) since the handle
 * was made: [0] calls that took it, [1] fine passes finished on the device (the coarse pass had exactly one best pose),
 * [2] fine passes handed to the general path (several best poses, response expansion, an off-lattice best pose),
 * [3] fine passes of the device rejected by the host's check of their centre (must stay 0), [4] coarse passes redone by the
 * general path (degenerate searches: more ties than the result block holds), [5] coarse passes scored by the fused
 * table + scoring kernel (linear lattices), [6] calls that went the general way because the fused kernels' fixed-size tables
 * cannot take them, [7] the last such call's reason (1 profiling / kept volume, 2 query beams, 3 readings per base scan,
 * 4 no base readings, 5 scans / points / tiles, 6 LDS, 7 no host-coherent memory: the handle keeps the general path). */
KH_API int kh_matcher_seq_stats(kh_matcher * m, int64_t out[8]);
/* The handle's main HIP stream (hipStream_t as void*): every kernel of a call that is not a chunked batch is launched on it, so
 * the caller can bracket launches with HIP events there; chunked batches (>= 128 large searches) run their chunks on two
 * side streams of the handle that are joined to this stream before the call returns. */
KH_API void * kh_matcher_stream(kh_matcher * m);
/* accumulated GPU time of the scoring kernel (K3) since the last reset, measured with HIP events
 * on the handle's stream when profiling is enabled: total ms and launch count */
KH_API int kh_matcher_profile(kh_matcher * m, int32_t enable, double * score_ms, int64_t * score_launches,
                              double * raster_ms, int64_t * raster_launches);

/* GPU time of the kernels either side of the scoring kernel in the same launches (HIP events on their stream while profiling is
 * enabled): the table / list kernel (K2, K2') and the tie kernel (K4), total ms since the last call (which this one resets).
 * Call it BEFORE kh_matcher_profile(m, 0, ...) reads and resets the launch count. */
KH_API int kh_matcher_profile_side(kh_matcher * m, double * offsets_ms, double * ties_ms);

/* wave-level dword-load instructions (256 B each: 16 lanes x 4 B across, 4 grid rows down) the scoring kernel issued
 * for the searches run while profiling was enabled, tallied on the device by K2 from the beam lists it hands to K3
 * (slow-path beams, which need the per-pose range check, are not included).  This is the L1 (TCP) side of the
 * roofline: bytes = 256 * wave_loads.  reset != 0 zeroes the tally after reading it. */
KH_API int kh_matcher_score_loads(kh_matcher * m, int64_t * wave_loads, int32_t reset);

/* ---------------------------------------------------------------- SPA solver (B) */
typedef struct kh_spa kh_spa;

/* options hard-wired by CeresSolver::Configure (ceres_solver.cpp:157-186) + Ceres defaults */
typedef struct kh_spa_options {
  int32_t max_num_iterations;          /* Ceres default 50 */
  double function_tolerance;           /* 1e-3 */
  double gradient_tolerance;           /* 1e-6 */
  double parameter_tolerance;          /* 1e-3 */
  double min_relative_decrease;        /* 1e-3 */
  double initial_trust_region_radius;  /* 1e4 */
  double max_trust_region_radius;      /* 1e8 */
  double min_trust_region_radius;      /* 1e-16 */
  double min_lm_diagonal;              /* 1e-6 */
  double max_lm_diagonal;              /* 1e32 */
  int32_t max_num_consecutive_invalid_steps;   /* 3 */
  int32_t use_nonmonotonic_steps;              /* true */
  int32_t max_consecutive_nonmonotonic_steps;  /* 3 */
  int32_t jacobi_scaling;                      /* true */
  /* `ceres_loss_function` (ceres_solver.cpp:60-94): KH_LOSS_NONE (squared loss, the default), KH_LOSS_HUBER =
   * ceres::HuberLoss(loss_scale), KH_LOSS_CAUCHY = ceres::CauchyLoss(loss_scale); the reference hard-wires
   * the scale 0.7 for both */
  int32_t loss_function;
  double loss_scale;                           /* 0.7 */
} kh_spa_options;
enum { KH_LOSS_NONE = 0, KH_LOSS_HUBER = 1, KH_LOSS_CAUCHY = 2 };
KH_API void kh_spa_options_default(kh_spa_options * o);

typedef struct kh_spa_summary {
  int32_t iterations;           /* LM iterations executed (successful + unsuccessful) */
  int32_t successful_steps;
  int32_t termination;          /* 0 convergence, 1 no convergence (max iters), 2 failure */
  int32_t usable;               /* Summary::IsSolutionUsable() */
  double initial_cost, final_cost;
  double linearize_ms, solve_ms, total_ms;   /* GPU/host wall split of Compute() */
  int64_t nnz_factor;           /* scalar non-zeros of the Cholesky factor */
  /* measurement (HIP events on the solver's stream, summed over the LM iterations of this Compute()) */
  int64_t factor_flops;         /* floating-point operations of ONE numeric factorisation: sum over the fronts of
                                   sum_{j < ns} (m - j)^2 (partial dense Cholesky of ns pivots of an m x m front) */
  int32_t factorizations;       /* numeric factorisations executed (= LM iterations) */
  int32_t levels;               /* elimination-tree levels = dependent launches per factorisation */
  double factor_gpu_ms;         /* assemble + factor + forward sweeps */
  double backward_gpu_ms;       /* backward sweeps + step evaluation */
  double linearize_gpu_ms;      /* edge linearisation + gathers of H and g (every evaluation point) */
  double symbolic_ms;           /* host: pattern + ordering + symbolic factorisation + uploads (0 when the topology was cached) */
  double worst_linear_residual; /* kh_spa_set_debug bit 0 only (else 0): max over the iterations of |(Hs + D/radius) step + gs| / |gs|,
                                   evaluated from the block-sparse matrix, independent of the factorisation */
  int32_t analysis;             /* symbolic analysis of this Compute(): 0 none (topology unchanged), 1 full nested dissection,
                                   2 incremental (supernodes of the last dissection reused, new nodes as leading leaves) */
  int32_t analysis_pad;
} kh_spa_summary;

KH_API int kh_spa_create(int32_t device, kh_spa ** out);
/* Test / measurement switches, 0 = none.  Bit 0: every LM iteration also evaluates the residual of its linear solve from
 * the block-sparse matrix (kh_spa_summary.worst_linear_residual).  Bit 1: HIP events around the phases of every iteration
 * (kh_spa_summary.factor_gpu_ms, backward_gpu_ms, linearize_gpu_ms; 0 without it -- each event costs the stream 5-6 us).  Bits 4-7: numeric factorisation kernels -- 0 default
 * (3), 3 level pipeline potrf/trsm/syrk, 1 and 2 (the same) the any-size kernel k_factor, one workgroup per front, which
 * also takes the problems whose fronts do not fit the pipeline; all give the same factor.  How a front's
 * update matrix reaches its parent in the level pipeline: added into the parent front by the kernel that computes it
 * (default); bit 8: every front reads its children's update matrices in place; bit 9: an extend-add launch per level sums
 * them in (rounds 3-5). */
KH_API int kh_spa_set_debug(kh_spa * s, int32_t flags);
/* Multi-GPU (one process per GPU, every rank holds the same graph): rank r linearises the edge block
 * [E*r/world, E*(r+1)/world) into PARTIAL normal equations, and `allreduce` -- supplied by the host
 * framework, e.g. RCCL through torch.distributed -- must sum `count` doubles at `device_buf` (H followed
 * by g, one contiguous buffer) in place across the ranks, ordered after the work already queued on
 * `hip_stream` (a hipStream_t) and complete, as far as that stream is concerned, when it returns 0.  The
 * factorisation and the LM control stay replicated.  world = 1 (default) disables sharding. */
typedef int (*kh_allreduce_fn)(void * user, double * device_buf, int64_t count, void * hip_stream);
KH_API int kh_spa_set_sharding(kh_spa * s, int32_t rank, int32_t world, kh_allreduce_fn allreduce, void * user);
/* The same sharding with the collective INSIDE the library: ncclAllReduce(sum, f64) of RCCL on `comm` (see kh_comm_*
 * below), rank and world taken from the communicator, which must live on the solver's device and outlive the solver's
 * use of it.  comm = NULL returns to the unsharded solver.  With a one-rank communicator the (identity) all-reduce is
 * still issued, so a single-GPU box exercises the whole path. */
typedef struct kh_comm kh_comm;
KH_API int kh_spa_set_comm(kh_spa * s, kh_comm * comm);
KH_API void kh_spa_destroy(kh_spa * s);
KH_API int kh_spa_set_options(kh_spa * s, const kh_spa_options * o);
KH_API int kh_spa_reset(kh_spa * s);                                   /* ScanSolver::Reset  (ceres_solver.cpp:279-314) */
KH_API int kh_spa_clear(kh_spa * s);                                   /* ScanSolver::Clear  (ceres_solver.cpp:272-276) */
KH_API int kh_spa_add_node(kh_spa * s, int32_t id, const double pose[3]);   /* AddNode (ceres_solver.cpp:317-336) */
/* AddConstraint (ceres_solver.cpp:339-392): z = LinkInfo::GetPoseDifference, cov = LinkInfo::GetCovariance
 * (row-major 3x3); the inverse (Karto.h:2533-2577), symmetrisation and upper Cholesky happen inside */
KH_API int kh_spa_add_constraint(kh_spa * s, int32_t id_a, int32_t id_b, const double z[3],
                                 const double cov[9]);
KH_API int kh_spa_remove_node(kh_spa * s, int32_t id);                 /* ceres_solver.cpp:395-427 */
KH_API int kh_spa_remove_constraint(kh_spa * s, int32_t id_a, int32_t id_b);  /* :430-448 */
KH_API int kh_spa_modify_node(kh_spa * s, int32_t id, const double pose[3]);  /* :451-461 (adds old yaw) */
KH_API int kh_spa_get_node(kh_spa * s, int32_t id, double pose[3]);    /* getGraph()/GetNodeOrientation */
KH_API int32_t kh_spa_num_nodes(kh_spa * s);
KH_API int32_t kh_spa_num_constraints(kh_spa * s);
KH_API int kh_spa_compute(kh_spa * s, kh_spa_summary * summary);       /* Compute (ceres_solver.cpp:214-269) */
/* Trace of the last Compute(), one row of 8 doubles per trust-region iteration -- what ceres::IterationSummary holds for it, so
 * that a Ceres run of the same problem (oracle/ceres_driver.cpp, where Ceres is installed) can be laid beside it line by line:
 * [0] iteration (1-based), [1] cost of the iterate the step starts from, [2] cost of the candidate, [3] model cost change,
 * [4] trust-region radius the step was computed with, [5] radius after the iteration's update, [6] step norm (scaled space),
 * [7] verdict: 1 accepted, 0 rejected, -1 invalid step, 2 / 3 terminated on parameter / function tolerance.
 * Writes min(capacity, rows) rows, *n_rows = rows available. */
KH_API int kh_spa_iteration_log(kh_spa * s, int32_t capacity, double * rows, int32_t * n_rows);
/* ---- pose-graph covariances (no counterpart in the reference: it never asks Ceres for a Covariance).
 * Sigma = (J^T J)^-1 over the free nodes at the CURRENT poses, in the tangent (x, y, theta) of every node; J is the linearisation
 * Compute() itself uses, the loss function's reweighting included, undamped.  The gauge node (the first node, constant) has
 * covariance zero; a node no constraint touches is not in the problem.  kh_spa_compute_covariances linearises, factorises
 * (cached analysis where the topology is unchanged; legal before any Compute) and walks the factor back down the assembly tree --
 * the selected inverse, every block of the inverse on the pattern of the factor, at about the cost of one more factorisation --
 * and keeps the blocks on the pattern of H resident on the device: every node's 3 x 3 marginal and the cross block of every pair
 * of nodes joined by a constraint.  The cross block of a pair WITHOUT a constraint is not on the pattern and is not available.
 * The result is valid until the graph or a pose changes (add_* / remove_* / modify_node / compute / reset / clear / load); after
 * that the getters answer KH_ERR_SOLVER ("stale").  KH_ERR_SOLVER also where the level pipeline does not run (fronts beyond its
 * LDS budget, or factor kernels 1 / 2 selected by kh_spa_set_debug) and for a graph with a free component that is not tied to
 * the gauge (non-positive pivot); nothing stays resident then.  Arguments are checked first (KH_ERR_INVALID_ARG), then the device
 * (KH_ERR_NO_DEVICE), then the handle. */
typedef struct kh_spa_cov_summary {
  int32_t n_free, levels;
  int32_t analysis;             /* as kh_spa_summary.analysis: 0 cached, 1 full, 2 incremental */
  int32_t pad;
  double linearize_ms, factor_ms;   /* host wall time up to the end of the linearisation / of everything behind it */
  double inverse_ms, gather_ms;     /* GPU time of the downward pass / of the collecting kernel, from HIP events under kh_spa_set_debug bit 1, else 0 */
  double total_ms;
  int64_t inverse_flops;        /* sum over the fronts of the flops of G = L21 W^T, Z21 = -Z22 G and G^T Z21 */
} kh_spa_cov_summary;
KH_API int kh_spa_compute_covariances(kh_spa * s, kh_spa_cov_summary * summary /* may be NULL */);
/* cov[9 k ..]: row-major 3 x 3 of node ids[k]; ids = NULL: all nodes in insertion order (n = kh_spa_num_nodes).  The gauge node:
 * zeros.  An unknown id or a node without constraints: KH_ERR_NOT_FOUND. */
KH_API int kh_spa_get_covariances(kh_spa * s, int32_t n, const int32_t * ids, double * cov /* 9n */);
/* row-major 6 x 6 [[aa ab], [ba bb]] of two nodes joined by a constraint (either direction); KH_ERR_NOT_FOUND for an unknown id,
 * a node without constraints and a pair without a constraint between them (their cross block is not on the pattern).  Rows and
 * columns of the gauge node are zeros. */
KH_API int kh_spa_get_joint_covariance(kh_spa * s, int32_t id_a, int32_t id_b, double cov[36]);
/* the resident array for device consumers: n_slots blocks of 9 doubles (row-major), block-sparse rows over the free nodes on the
 * pattern of H; owned by the solver, valid like the getters' answers */
KH_API int kh_spa_covariance_device(kh_spa * s, const double ** cov_bsr, int64_t * n_slots);
/* ---- covariance columns: the cross-covariance of ANY two nodes, joined by a constraint or not (a loop-closure candidate, a pose
 * against the dock or the first scan).  kh_spa_compute_covariance_columns is kh_spa_compute_covariances -- the same pass, the same
 * marginals, the same refusals -- and, while the factor is still in the fronts, solves A X = E_q for the listed query nodes through
 * it (a forward sweep up the assembly tree over the fronts between a query and the root, a backward sweep over all of them): the
 * block column Sigma(:, q) of every query, every row at once, resident on the device as n_queries x n_free blocks of 9 doubles and
 * valid exactly as long as the marginals are.  At most KH_SPA_MAX_COV_COLUMNS queries per call; the gauge node is a legal query
 * (its column is zeros).  n < 1, n > KH_SPA_MAX_COV_COLUMNS, ids = NULL or an id listed twice: KH_ERR_INVALID_ARG, before a device
 * is looked for (then KH_ERR_NO_DEVICE, then the handle); an unknown id or a node without constraints: KH_ERR_NOT_FOUND.  A call
 * replaces the columns of the call before it; kh_spa_compute_covariances leaves none. */
#define KH_SPA_MAX_COV_COLUMNS 64
typedef struct kh_spa_cov_columns_summary {
  kh_spa_cov_summary cov;           /* the pass the columns rode on */
  int32_t n_queries;
  int32_t path_fronts;              /* fronts the forward sweep visited: the union of the paths from a query's front to its root */
  double forward_ms, backward_ms;   /* GPU time of the two sweeps, from HIP events under kh_spa_set_debug bit 1, else 0 */
  double total_ms;
  int64_t column_flops;             /* flops of the two sweeps over the padded right-hand sides */
} kh_spa_cov_columns_summary;
KH_API int kh_spa_compute_covariance_columns(kh_spa * s, int32_t n, const int32_t * ids, kh_spa_cov_columns_summary * summary /* may be NULL */);
/* out[9 k ..]: row-major 3 x 3 Sigma(ids[k], id_q); ids = NULL: all nodes in insertion order (n = kh_spa_num_nodes).  The gauge
 * node as a row or as the query: zeros.  id_q not among the queries of the last column pass: KH_ERR_NOT_FOUND; stale: KH_ERR_SOLVER. */
KH_API int kh_spa_get_covariance_column(kh_spa * s, int32_t id_q, int32_t n, const int32_t * ids, double * out /* 9n */);
/* kh_spa_get_joint_covariance for a pair with or without a constraint: one of the two must be a query of the last column pass
 * (id_b's column is used when both are).  The diagonal blocks are the marginals of kh_spa_get_covariances, the cross block comes
 * from the column and its transpose fills the other corner: the 6 x 6 is bit-wise symmetric. */
KH_API int kh_spa_get_joint_covariance_any(kh_spa * s, int32_t id_a, int32_t id_b, double cov[36]);
/* out[9 k ..]: first-order covariance of node ids[k]'s pose expressed in the frame of id_ref (a query of the last column pass),
 * d = R(-theta_ref) (t_k - t_ref), theta_k - theta_ref at the solver's current poses: J [[S_rr S_rk], [S_kr S_kk]] J^T with
 * J = [dd/dref dd/dk], one thread per listed node (k_cov_relative).  ids = NULL: all nodes in insertion order.  ids[k] = id_ref:
 * exact zeros. */
KH_API int kh_spa_get_relative_covariances(kh_spa * s, int32_t id_ref, int32_t n, const int32_t * ids, double * out /* 9n */);
/* out[9 k ..]: row-major covariance of x_k - x_ref in the WORLD frame, D = S_kk + S_rr - S_kr - S_kr^T (k_cov_difference, one
 * thread per listed node): no pose enters and nothing is rotated, which is what a gate over world positions wants (section 7h).
 * id_ref must be a query of the last column pass.  The upper triangle is computed and mirrored: bit-wise symmetric.  The gauge
 * node's blocks are zeros, as k or as the reference; ids[k] = id_ref: exact zeros.  Argument checks, ids = NULL and staleness as
 * kh_spa_get_relative_covariances. */
KH_API int kh_spa_get_difference_covariances(kh_spa * s, int32_t id_ref, int32_t n, const int32_t * ids, double * out /* 9n */);
/* ---- constraint audit (no counterpart in the reference, whose only remedy for a false loop closure is a person dragging nodes;
 * DESIGN.md section 7i): the leave-one-out test of every constraint that is already in the graph, from the resident selected
 * inverse.  For constraint e between a and b, with r (3) the whitened, loss-weighted residual and A = [Ja Jb] (3 x 6) of the
 * linearisation at the current poses, and Sigma(ab, ab) the joint covariance of the two poses (a gauge end: no Jacobian, zeros):
 *   chi2        r^T r: what the constraint costs now
 *   redundancy  trace(M), M = I - A Sigma(ab, ab) A^T, in [0, 3]: how much of the constraint the rest of the graph checks
 *   min_pivot   the smallest pivot of the lower Cholesky factorisation of M in the order 0, 1, 2, which stops at the first pivot
 *               that is not > min_redundancy (a NaN is not); the failing pivot is included
 *   verifiable  1 when all three pivots are > min_redundancy.  0: a bridge, or the only constraint that fixes some direction --
 *               nothing else in the graph has an opinion on it, and removing it would cut the graph or leave it underdetermined
 *   chi2_loo    r^T M^-1 r, chi-square (3 degrees of freedom) of the constraint against the graph WITHOUT it (the linear
 *               leave-one-out identity e_loo = M^-1 e, cov = M^-1); -1 when not verifiable
 * k_edge_audit, one thread per constraint; an edge's figures do not depend on which other edges are audited with it.  Under a
 * robust loss r and A carry the loss weights: a down-weighted outlier looks milder, which is the loss at work. */
typedef struct kh_spa_audit_t { int32_t index, id_a, id_b, verifiable; double chi2, redundancy, min_pivot, chi2_loo; } kh_spa_audit_t;
typedef struct kh_spa_audit_summary { kh_spa_cov_summary cov; /* the pass this call ran, zeros when it rode on a resident one */
  int32_t n_constraints, n_verifiable; double kernel_ms /* HIP events under debug bit 1, else 0 */, total_ms; } kh_spa_audit_summary;
/* out: kh_spa_num_constraints records in constraint insertion order (index = the index of kh_spa_get_constraint).  Runs
 * kh_spa_compute_covariances itself when no valid marginals are resident -- its refusals (KH_ERR_SOLVER) are this call's -- and
 * leaves them resident; otherwise it rides on them.  The linearisation of the audit covers all edges, on a sharded solver too,
 * in a buffer of its own: the call is bit-neutral for every kh_spa_compute and covariance getter around it.  min_redundancy
 * must be finite and in (0, 1) (1e-6 is a good value), out not NULL: KH_ERR_INVALID_ARG before a device is looked for; then
 * KH_ERR_NO_DEVICE, then the handle.  A graph without constraints: KH_OK and no records.  summary may be NULL. */
KH_API int kh_spa_audit_constraints(kh_spa * s, double min_redundancy, kh_spa_audit_t * out /* kh_spa_num_constraints */, kh_spa_audit_summary * summary);
/* ---- marginalizing node removal (no counterpart in the reference, whose RemoveNode drops the node's constraints and transfers
 * nothing: a lifelong graph falls apart).  Every listed node leaves like kh_spa_remove_node, but first its constraints are composed
 * through it into constraints among its neighbours: parallel constraints to one neighbour are fused; the
 * neighbour whose (fused) information has the largest determinant is the hub, ties to the lowest id; for every other neighbour n
 * the constraint hub -> n = inverse(v -> hub) (+) (v -> n) is formed, the hub's covariance weighted d - 1 (d neighbours), which
 * keeps the d - 1 new constraints together no more informative than the exact dense marginal (exact for d = 2); it is fused into
 * the first existing constraint between hub and n, which keeps its index and its direction, or appended.  Only constraints are
 * read: no poses, no linearisation point.  A node with fewer than two neighbours is simply removed.
 * The list is worked off in ROUNDS, formed greedily in list order: a node whose closed neighbourhood meets that of a listed node
 * before it which is in the round or still waiting, waits for the next round.  One launch marginalizes a round, one wave per node
 * and one lane per neighbour; the values equal those of the list processed one node after the other, and so does the order of the
 * constraints when no node of the list had to wait behind a node that is not its predecessor in the list (appended constraints
 * are in round order).  Arguments are checked first (n < 0, ids NULL: KH_ERR_INVALID_ARG), then the device (KH_ERR_NO_DEVICE),
 * then the handle.  Before anything changes: an unknown id is KH_ERR_NOT_FOUND; a duplicate id, the gauge node (the first node:
 * it cannot be handed on) and a node with more than 64 neighbours are KH_ERR_INVALID_ARG.  A node that only GROWS past 64
 * neighbours through the nodes listed before it stops the call at its round with KH_ERR_INVALID_ARG; the earlier rounds stay. */
typedef struct kh_marginalize_summary {
  int32_t n_marginalized, n_plain;   /* nodes whose constraints were handed on / that had fewer than two neighbours */
  int32_t n_rounds;
  int32_t n_added, n_fused;          /* new constraints appended / fused into an existing one */
  int32_t max_degree;
  double pack_ms, kernel_ms, apply_ms, total_ms;   /* host: rounds + packing; upload + launch + download; edits of the graph */
} kh_marginalize_summary;
KH_API int kh_spa_marginalize_nodes(kh_spa * s, int32_t n, const int32_t * ids, kh_marginalize_summary * summary /* may be NULL */);
/* GetCorrections (ceres_solver.cpp:272): pass ids=NULL to query the count */
KH_API int kh_spa_get_corrections(kh_spa * s, int32_t * n, int32_t * ids, double * poses /* 3n */);
/* ---- pose-graph files.  The reference persists a Boost binary archive of the whole
 * Mapper (Mapper.cpp:2635-2651, serialization.hpp:38-82; not readable without Boost) and rebuilds the solver from it
 * with Reset / AddNode* / AddConstraint* (slam_toolbox_common.cpp:959-1016).  Here the solver's own state is the file:
 *   text    g2o SE2 records   VERTEX_SE2 id x y theta            (AddNode order; the first one is the gauge)
 *                             FIX id                             (optional; must name the first vertex)
 *                             EDGE_SE2 a b dx dy dtheta  i00 i01 i02 i11 i12 i22   (upper triangle of the information)
 *           '#' comments and blank lines are skipped; numbers are written with 17 significant digits, so a
 *           save / load round trip is bit-exact;
 *   binary  "KHPG\1\0\0\0", int64 n, int64 m, int32 id[n], f64 pose[3n], int32 a[m], int32 b[m], f64 z[3m],
 *           f64 info[6m], little endian.
 * kh_spa_load parses and validates the whole file first (KH_ERR_IO / KH_ERR_INVALID_ARG leave the current graph in
 * place), then Reset + AddNode + AddConstraint in file order; the format is detected from the first 8 bytes. */
enum { KH_GRAPH_TEXT = 0, KH_GRAPH_BINARY = 1 };
KH_API int kh_spa_save(kh_spa * s, const char * path, int32_t format);
KH_API int kh_spa_load(kh_spa * s, const char * path);
/* AddConstraint for callers that hold the information matrix (upper triangle 00 01 02 11 12 22, what EDGE_SE2
 * carries) instead of LinkInfo's covariance: skips the inverse of ceres_solver.cpp:364-375, same llt() after it */
KH_API int kh_spa_add_constraint_information(kh_spa * s, int32_t id_a, int32_t id_b, const double z[3],
                                             const double info_upper[6]);
/* enumeration in insertion order (what the files hold); KH_ERR_NOT_FOUND past the end */
KH_API int kh_spa_get_node_at(kh_spa * s, int32_t index, int32_t * id, double pose[3]);
/* all nodes at once, insertion order: ids[kh_spa_num_nodes], poses[3 * kh_spa_num_nodes] (either may be NULL) */
KH_API int kh_spa_get_nodes(kh_spa * s, int32_t * ids, double * poses);
KH_API int kh_spa_get_constraint(kh_spa * s, int32_t index, int32_t * id_a, int32_t * id_b, double z[3],
                                 double info_upper[6]);
/* LinkInfo::Update (Mapper.h:174-188) for callers without karto objects */
KH_API int kh_link_info(const double pose1[3], const double pose2[3], const double cov[9],
                        double pose_difference[3], double cov_out[9]);

/* ---------------------------------------------------------------- multi-GPU communicator (RCCL over xGMI) */
/* One process per GPU.  Rank 0 makes an id with kh_comm_unique_id and hands the 128 bytes to the other ranks by whatever
 * the launcher offers (MPI, a torch.distributed store, a file); every rank then calls kh_comm_create with its device,
 * its rank and the world size (collective: returns when all ranks have joined, like ncclCommInitRank).  librccl is
 * bound at run time, so single-GPU users never load it; KH_ERR_NO_DEVICE when it cannot be found. */
#define KH_COMM_ID_BYTES 128
KH_API int kh_comm_unique_id(uint8_t id[KH_COMM_ID_BYTES]);
KH_API int kh_comm_create(int32_t device, int32_t rank, int32_t world, const uint8_t id[KH_COMM_ID_BYTES], kh_comm ** out);
KH_API void kh_comm_destroy(kh_comm * c);
KH_API int32_t kh_comm_rank(const kh_comm * c);
KH_API int32_t kh_comm_world(const kh_comm * c);
KH_API int32_t kh_comm_device(const kh_comm * c);     /* the device the communicator was created on; -1 for NULL */
/* in-place sum of `count` doubles at device_buf across the ranks, enqueued on hip_stream (a hipStream_t) */
KH_API int kh_comm_allreduce_sum_f64(kh_comm * c, double * device_buf, int64_t count, void * hip_stream);
/* every rank contributes count_per_rank doubles; device_recv (world * count_per_rank) holds them in rank order.  What the
 * sharded candidate matcher uses to collect the 13 result doubles of every pair */
KH_API int kh_comm_allgather_f64(kh_comm * c, const double * device_send, double * device_recv, int64_t count_per_rank,
                                 void * hip_stream);

/* device buffers for callers without a HIP binding of their own (the two collectives take device pointers); download
 * waits for all work queued on the device first */
KH_API int kh_device_malloc(int32_t device, int64_t bytes, void ** out);
KH_API void kh_device_free(void * p);
KH_API int kh_device_upload(void * device_dst, const void * host_src, int64_t bytes);
/* the upload queued on a HIP stream (hipStream_t as void *, e.g. kh_matcher_stream): ordered in front of whatever is launched there next */
KH_API int kh_device_upload_on(void * device_dst, const void * host_src, int64_t bytes, void * hip_stream);
KH_API int kh_device_download(void * host_dst, const void * device_src, int64_t bytes);
/* self-test of the once-per-device bookkeeping behind the kernels' dynamic-LDS attribute (csrc/lds_attr.hpp), run on made-up
 * device ids; 0 = every check holds.  Needs no device: the CPU test suite calls it. */
KH_API int kh_selftest_lds_attr(void);

/* ---------------------------------------------------------------- loop-candidate enumeration (next row f-1) */
/* GPU-resident copy of what karto::MapperGraph's candidate search reads: the reference position
 * GetReferencePose(use_scan_barycenter) of every scan of a sensor in scan-list order (NULL scans left out:
 * the reference skips them, Mapper.cpp:1980-1982) and the adjacency of the pose graph in CSR form with the
 * neighbours in Vertex::GetAdjacentVertices order (Mapper.h:338-361).  Indices are positions in that list. */
typedef struct kh_graph kh_graph;
KH_API int kh_graph_create(int32_t device, kh_graph ** out);
KH_API void kh_graph_destroy(kh_graph * g);
KH_API int kh_graph_set(kh_graph * g, int32_t n_scans, const double * ref_xy /* 2n */,
                        const int32_t * adj_ptr /* n+1 */, const int32_t * adj_idx);
KH_API int kh_graph_set_positions(kh_graph * g, int32_t n_scans, const double * ref_xy);   /* after CorrectPoses */
/* For every query scan: all the chains successive MapperGraph::FindPossibleLoopClosure calls return
 * (Mapper.cpp:1960-2010, enumerated like TryCloseLoop does, Mapper.cpp:1500-1560), FindNearLinkedScans
 * (Mapper.cpp:1795-1806) included, for the CURRENT graph state (speculative batch).
 * Chains are runs of consecutive scans: chains[2k], chains[2k+1] = first, last index; query i owns
 * chains chain_begin[i] .. chain_begin[i+1]-1 (n_queries+1 entries).  *n_chains is the total even when it
 * exceeds cap_chains (then only the first cap_chains are written). */
KH_API int kh_graph_find_loop_candidates(kh_graph * g, int32_t n_queries, const int32_t * query_scans,
                                         double loop_search_maximum_distance, int32_t loop_match_minimum_chain_size,
                                         int32_t * chain_begin, int32_t * chains, int32_t cap_chains,
                                         int32_t * n_chains);
/* The same with TryCloseLoop's resume index: query i enumerates as successive FindPossibleLoopClosure calls starting at
 * rStartNum = start_scans[i] do (Mapper.cpp:1963, 1976: the chain under construction is empty at the resume point, so a
 * run of candidate scans that straddles it counts from there).  What the speculative batch re-issues after a closure
 * moved the poses.  start_scans = NULL: all zero. */
KH_API int kh_graph_find_loop_candidates_from(kh_graph * g, int32_t n_queries, const int32_t * query_scans,
                                              const int32_t * start_scans, double loop_search_maximum_distance,
                                              int32_t loop_match_minimum_chain_size, int32_t * chain_begin, int32_t * chains,
                                              int32_t cap_chains, int32_t * n_chains);
/* kh_graph_find_loop_candidates_from with the distance test widened by the uncertainty of every scan's displacement from the
 * query: gate holds, per query, n_scans rows of 9 doubles in list order -- the row-major 3 x 3 world-frame
 * covariance D of x_i - x_query (kh_spa_get_difference_covariances), of which Dxx, Dxy, Dyy = [0], [1], [4] are read.  With
 * r = loop_search_maximum_distance and s = chi2 / (r * r), every operation rounded on its own:
 *   a = 1 + s Dxx, c = 1 + s Dyy, b = s Dxy, det = a c - b b, q = ((c (dx dx) - 2 b (dx dy)) + a (dy dy)) / det
 * -- q = delta^T (I + s D)^-1 delta, so q < r^2 is the ellipse delta^T (r^2 I + chi2 D)^-1 delta < 1 -- and q replaces the squared
 * distance in BOTH tests (candidate: q < r^2 + KT_TOLERANCE; visitable by the breadth-first "linked" walk: q <= r^2 - KT_TOLERANCE).
 * A row with det <= 0, a < 1, c < 1 or a quotient that is not finite is tested with the plain squared distance.  D = 0 or chi2 = 0
 * gives q = dx dx + dy dy exactly: the chains of kh_graph_find_loop_candidates_from, bit for bit.  gate = NULL, chi2 < 0 or NaN:
 * KH_ERR_INVALID_ARG; everything else as kh_graph_find_loop_candidates_from. */
KH_API int kh_graph_find_loop_candidates_gated(kh_graph * g, int32_t n_queries, const int32_t * query_scans,
                                               const int32_t * start_scans /* may be NULL */, double loop_search_maximum_distance,
                                               int32_t loop_match_minimum_chain_size, double chi2,
                                               const double * gate /* n_queries x 9 n_scans, host */, int32_t * chain_begin,
                                               int32_t * chains, int32_t cap_chains, int32_t * n_chains);
KH_API double kh_graph_last_kernel_ms(kh_graph * g);
/* After scans were removed (lifelong mode) the reference's candidate walks stop at the SIZE of its scan map, which has
 * fallen behind the largest scan id (Mapper.cpp:1974-1976, 1751-1756): only the first n_visit scans of the list are
 * visited as chain members (all of them still count for the breadth-first "linked" test).  kh_graph_set resets it to n. */
KH_API int kh_graph_set_scan_limit(kh_graph * g, int32_t n_visit);
/* Incremental edits of the store (what MapperGraph::AddVertex / AddEdge and a scan's SetSensorPose do to the reference's
 * graph): a mapper that appends a scan and links it a few times per processed scan does not rebuild the store with
 * kh_graph_set every time.  Positions are list positions as in kh_graph_set; an edge goes to the END of both
 * adjacency lists (Vertex::GetAdjacentVertices order).  Removing a scan renumbers the list: rebuild with kh_graph_set. */
KH_API int kh_graph_append_scan(kh_graph * g, const double ref_xy[2]);
KH_API int kh_graph_add_edge(kh_graph * g, int32_t scan_a, int32_t scan_b);
KH_API int kh_graph_set_position(kh_graph * g, int32_t scan, const double ref_xy[2]);
/* The store's second point per vertex: GetCorrectedPose() x, y of the scan, which is what the reference's KD-tree adaptor reads
 * (nanoflann_adaptors.h:44-49) -- not ref_xy, which is the sensor pose or the barycentre.  It follows the store's life cycle:
 * kh_graph_set drops the poses (kh_graph_set_poses gives all of them, also after CorrectPoses), kh_graph_append_scan_with_pose appends
 * vertex and pose (the pose-less kh_graph_append_scan leaves the store without poses), kh_graph_set_pose re-poses one vertex.
 * The near-by queries answer KH_ERR_INVALID_ARG on a non-empty store without poses. */
KH_API int kh_graph_set_poses(kh_graph * g, int32_t n_scans, const double * pose_xy /* 2n */);
KH_API int kh_graph_set_pose(kh_graph * g, int32_t scan, const double pose_xy[2]);
KH_API int kh_graph_append_scan_with_pose(kh_graph * g, const double ref_xy[2], const double pose_xy[2]);
/* MapperGraph::FindNearByScan (Mapper.cpp:1877-1912) for n_queries poses in ONE kernel launch: nearest[i] = the vertex whose pose
 * has the smallest squared distance (dx * dx) + (dy * dy) to query i -- nanoflann's L2_Simple_Adaptor sum (nanoflann.hpp:475-485),
 * each operation rounded on its own, so dist_sq[i] (may be NULL) has the bits of the host expression; between equal distances
 * the lower index (nanoflann's own answer to an exact tie depends on the shape of its tree).  An empty store answers
 * nearest = -1 (the reference returns NULL) and dist_sq = +inf. */
KH_API int kh_graph_find_near_by_scan(kh_graph * g, int32_t n_queries, const double * query_xy /* 2q */, int32_t * nearest /* q */,
                                      double * dist_sq /* q */);
/* MapperGraph::FindNearByVertices (Mapper.cpp:1837-1875), i.e. radiusSearch exactly as the reference calls it: max_distance is
 * handed to an L2 metric that compares it with the SQUARED distance (dist < radius, strict, nanoflann.hpp:274), and the hits come
 * back by ascending distance (SearchParams::sorted defaults to true, nanoflann.hpp:630, 1418; lower index first between equal
 * distances).  *n_found is the total even beyond cap; 0 for an empty store. */
KH_API int kh_graph_find_near_by_vertices(kh_graph * g, const double query_xy[2], double max_distance, int32_t * scans, int32_t cap,
                                          int32_t * n_found);
KH_API double kh_graph_last_near_by_kernel_ms(kh_graph * g);       /* device time of the last near-by kernel (HIP events) */
/* Where to try a scan that comes without a pose (global relocalization), over the store's poses:
 *   seeds   a lattice of side seed_spacing; the cell of a vertex is (floor(x / seed_spacing), floor(y / seed_spacing)) in FP64; the seed
 *           of a non-empty cell is its vertex with the lowest index; seeds come in ascending index.  With center_xy and radius > 0
 *           only the seeds with (dx * dx) + (dy * dy) < radius * radius + KT_TOLERANCE from the centre (radius <= 0 or center_xy
 *           NULL: the whole map).
 *   bases   seed k owns base_idx[base_begin[k] .. base_begin[k + 1]): every vertex with (dx * dx) + (dy * dy) <
 *           base_radius * base_radius + KT_TOLERANCE from the seed, ascending; of more than max_base, entries 0, s, 2s, ... of that
 *           list with s = ceil(count / max_base).
 * *n_seeds / *n_base are the totals even beyond cap_seeds / cap_base; seeds and base_idx take the first cap entries, base_begin
 * min(*n_seeds, cap_seeds) + 1.  An empty store answers zero seeds.  Needs the store's poses, like the near-by queries. */
KH_API int kh_graph_relocalize_candidates(kh_graph * g, double seed_spacing, double base_radius, int32_t max_base,
                                          const double * center_xy, double radius, int32_t * seeds, int32_t cap_seeds,
                                          int32_t * n_seeds, int32_t * base_begin, int32_t * base_idx, int32_t cap_base,
                                          int32_t * n_base);
KH_API double kh_graph_last_relocalize_kernel_ms(kh_graph * g);    /* device time of the last call's kernels (HIP events) */
/* MapperGraph::FindNearLinkedVertices (Mapper.cpp:1808-1819): the vertices a breadth-first traversal from the scan
 * reaches through vertices within max_distance of it, in visiting order (the scan itself first).  *n_found is the total. */
KH_API int kh_graph_find_near_linked(kh_graph * g, int32_t query_scan, double max_distance, int32_t * scans, int32_t cap,
                                     int32_t * n_found);
/* The rest of the row -- neighbourhood-sized, exact host arithmetic, no kernel:
 * MapperGraph::FindNearChains (Mapper.cpp:1683-1793) for one scan of the current graph: the maximal runs of
 * consecutive scans within link_scan_maximum_distance of it that hold a near linked scan (FindNearLinkedScans,
 * Mapper.cpp:1795-1806), in the order the breadth-first traversal meets them, without the run that contains the scan
 * itself.  chains[2k], chains[2k+1] = first, last index; *n_chains is the total even beyond cap_chains. */
KH_API int kh_graph_find_near_chains(kh_graph * g, int32_t query_scan, double link_scan_maximum_distance,
                                     int32_t * chains, int32_t cap_chains, int32_t * n_chains);
/* MapperGraph::GetClosestScanToPose (Mapper.cpp:1563-1582): first scan of the list with the smallest squared
 * distance of its reference position to pose_xy; -1 for an empty list */
KH_API int kh_graph_closest_scan_to_pose(kh_graph * g, const int32_t * scans, int32_t n, const double pose_xy[2],
                                         int32_t * closest);
/* MapperGraph::ComputeWeightedMean (Mapper.cpp:1914-1958): inverse-covariance weighted mean of n poses (means 3n,
 * covariances 9n row-major), heading = atan2 of the mean sine and cosine */
KH_API int kh_weighted_mean(int32_t n, const double * means, const double * covariances, double mean[3]);

/* ---------------------------------------------------------------- occupancy grid (next row f-2) */
/* karto::OccupancyGrid::CreateFromScans (Karto.h:5947-5962, 6118-6274).  Scans are handed over like to the
 * matcher (ranges + UNFILTERED point readings + sensor pose, GetPointReadings(false) at Karto.h:6157). */
typedef struct kh_occupancy kh_occupancy;
/* OccupancyGrid::ComputeDimensions (Karto.h:6086-6112) from the scans' bounding boxes (Karto.h:5694-5700) */
KH_API int kh_occupancy_compute_dimensions(int32_t n_scans, const kh_scan * scans, double min_range,
                                           double range_threshold, double resolution, int32_t * width,
                                           int32_t * height, double offset[2]);
KH_API int kh_occupancy_create(int32_t width, int32_t height, double offset_x, double offset_y, double resolution,
                               int32_t device, kh_occupancy ** out);
KH_API void kh_occupancy_destroy(kh_occupancy * g);
KH_API int kh_occupancy_clear(kh_occupancy * g);
/* AddScan for every scan (Karto.h:6148-6189): pass / hit counters only */
KH_API int kh_occupancy_add_scans(kh_occupancy * g, int32_t n_scans, const kh_scan * scans, double range_threshold,
                                  double min_range, double max_range);
/* Update (Karto.h:6257-6274); karto defaults: min_pass_through 2, occupancy_threshold 0.1 (Karto.h:5920-5921) */
KH_API int kh_occupancy_update(kh_occupancy * g, uint32_t min_pass_through, double occupancy_threshold);
/* cells: width_step * height bytes (0 unknown, 100 occupied, 255 free, Karto.h:4379-4381); pass / hits: the
 * counter grids (same layout, uint32); any pointer may be NULL */
KH_API int kh_occupancy_read(kh_occupancy * g, uint8_t * cells, uint32_t * pass, uint32_t * hits);
/* vis_utils::toNavMap (include/slam_toolbox/visualization_utils.hpp:108-146) of the cell states, on the device: out gets
 * width * height values WITHOUT row padding, row-major -- the data of a nav_msgs/OccupancyGrid: -1 unknown, 100 occupied,
 * 0 free.  For any kh_occupancy: kh_mapper_build_map's, kh_merge_build's, a hand-made one after kh_occupancy_update. */
KH_API int kh_occupancy_read_nav(kh_occupancy * g, int8_t * out);
KH_API int kh_occupancy_info(kh_occupancy * g, int32_t * width, int32_t * height, int32_t * width_step,
                             double * trace_ms, int64_t * beams_traced);
/* the grid's offset (world position of cell 0, 0) and 1 / scale; either pointer may be NULL */
KH_API int kh_occupancy_geometry(kh_occupancy * g, double offset[2], double * resolution);

/* A device view of a map: what the matcher's map entry points (kh_matcher_add_map / _match_map*, below) read.  The world point of
 * cell (i, j) is anchor + (o + i) / scale, in float64 with the integer sum first: CoordinateConverter::GridToWorld without flip,
 * and the inverse of the live map's round((x - ax) * scale).
 * A view is a BORROWED pointer: it is valid until its source is next updated, grown, cleared or destroyed (kh_occupancy_add_scans /
 * _update / _clear / _write_nav / _destroy; kh_live_map_update / _destroy), and the cells must not be written while a call that
 * was handed the view runs.  A caller may also fill a view by hand over any device buffer it owns (kh_device_malloc /
 * kh_device_upload). */
typedef struct kh_map_view {
  const uint8_t * device_cells;   /* karto cell states (0 unknown, 100 occupied, 255 free), row stride width_step */
  int32_t device;
  int32_t width, height, width_step;
  int32_t ox, oy;                 /* lattice index of column 0 / row 0 (0 for a kh_occupancy; the window origin of a live map) */
  double anchor[2];               /* kh_occupancy: its offset; live map: its anchor */
  double scale;                   /* the source's stored 1 / resolution, not recomputed */
} kh_map_view;
KH_API int kh_occupancy_view(kh_occupancy * g, kh_map_view * out);
/* The inverse of kh_occupancy_read_nav: nav holds width * height values without row padding, -1 -> 0 (unknown), 100 -> 100
 * (occupied), 0 -> 255 (free); any other value is refused with KH_ERR_INVALID_ARG and the grid stays as it was.  The row padding
 * of the cells is zeroed, and so are the pass / hit counters: a later kh_occupancy_update recomputes the cells from the counters,
 * i.e. wipes what was written here.  This is how a map that arrives as an image or a nav_msgs/OccupancyGrid gets onto the device. */
KH_API int kh_occupancy_write_nav(kh_occupancy * g, const int8_t * nav);

/* ---------------------------------------------------------------- lifelong node-decay scoring (next row f-4) */
/* LifelongSlamToolbox::computeScores (src/experimental/slam_toolbox_lifelong.cpp:295-329) with the metrics
 * of :373-478 and the objective of :199-250.  A kh_scan_box is what the scoring reads from a scan / vertex:
 * GetBarycenterPose(), GetBoundingBox().GetSize(), the FILTERED point readings GetPointReadings(true), the
 * unique id, the vertex's edge count and its current score. */
typedef struct kh_scan_box {
  double barycenter[2];
  double bbox_size[2];            /* width, height */
  int32_t unique_id;
  int32_t n_edges;                /* Vertex::GetEdges().size() */
  double score;                   /* Vertex::GetScore() */
  int32_t n_points;
  const double * points_xy;       /* filtered point readings, host memory */
} kh_scan_box;
typedef struct kh_decay_params {
  double iou_thresh;              /* lifelong_minimum_score          0.10 */
  double iou_match;               /* lifelong_iou_match              0.85 */
  double removal_score;           /* lifelong_node_removal_score     0.10 (used by the caller, :166) */
  double overlap_scale;           /* lifelong_overlap_score_scale    0.5  */
  double constraint_scale;        /* lifelong_constraint_multiplier  0.05 */
  double nearby_penalty;          /* lifelong_nearby_penalty         0.001 */
  double candidates_scale;        /* lifelong_candidates_scale       0.03 (computed but unused upstream, :231-240) */
  int32_t scan_buffer_size;       /* mapper scan_buffer_size */
} kh_decay_params;
KH_API void kh_decay_params_default(kh_decay_params * p);
/* kept[k] = 0 for candidates computeScores erases (IoU below iou_thresh or fewer than 2 edges); scores[k] is
 * computeScore's return for the kept ones.  Output pointers may be NULL. */
KH_API int kh_lifelong_scores(int32_t device, const kh_scan_box * reference, int32_t n, const kh_scan_box * candidates,
                              const kh_decay_params * params, int32_t * kept, double * iou, double * area_overlap,
                              double * reading_overlap, double * scores);
/* The same scoring in the form the mapper calls after every accepted scan (kh_mapper_set_lifelong), for a caller that holds the
 * readings on the host: candidate k has n_scan UNFILTERED point readings at points_xy[k] (2 * n_scan doubles; NULL = its
 * readings are not counted, reading overlap 0 / n_points) and (n_scan + 63) / 64 mask words at masks[k], bit i of word i / 64
 * set where reading i passed the range filter.  candidates[k].n_points is the number of readings that count (the denominator
 * of the reading overlap); candidates[k].points_xy is not read.  The readings are uploaded for the call.  1 <= n_scan <= 4096. */
KH_API int kh_lifelong_scores_resident(int32_t device, const kh_scan_box * reference, int32_t n, const kh_scan_box * candidates,
                                       const double * const * points_xy, const uint64_t * const * masks, int32_t n_scan,
                                       const kh_decay_params * params, int32_t * kept, double * iou, double * area_overlap,
                                       double * reading_overlap, double * scores);

/* ---------------------------------------------------------------- mapper front end (BASELINE configs 1 and 5) */
/* ROS-free restatement of what karto::Mapper::Process does around the scan matcher and the solver plugin
 * (lib/karto_sdk/src/Mapper.cpp:2679-2748 with MapperGraph::AddEdges / LinkNearChains / TryCloseLoop / CorrectPoses,
 * :1434-1561, 1641-1681, 2012-2030), for replaying a scan queue end to end on the GPU: sequential match against the running
 * scans, links to the previous scan, the running chain and the near chains (matched as one batch), loop closure as
 * speculative batches (all candidate chains enumerated by kh_graph_find_loop_candidates_from, coarse-matched in one
 * kh_matcher_match_batch, the ones passing the coarse gate fine-matched in a second, results consumed in the reference's
 * order up to the first accepted closure, then kh_spa_compute and re-enumeration behind it).  One laser.  Mapping mode is
 * kh_mapper_process; localization mode is the group of calls below it.  The values are AS STORED by karto::Mapper (loop_match_maximum_variance_coarse and the two
 * variance penalties of `match` are the squared values). */
typedef struct kh_mapper kh_mapper;
typedef struct kh_laser {                       /* karto::LaserRangeFinder (Karto.h:4060-4330) */
  int32_t n_beams;
  double minimum_angle, angular_resolution, minimum_range, maximum_range, range_threshold;
  double offset_x, offset_y, offset_heading;    /* LaserRangeFinder::GetOffsetPose: where the sensor sits on the robot (zeros = at
                                                   its centre); sensor pose = GetSensorAt(corrected pose), Karto.h:5566-5588 */
} kh_laser;
typedef struct kh_mapper_params {               /* Mapper::InitializeParameters (Mapper.cpp:2086-2297) */
  int32_t use_scan_matching, use_scan_barycenter;
  double minimum_time_interval, minimum_travel_distance, minimum_travel_heading;
  int32_t scan_buffer_size;
  double scan_buffer_maximum_scan_distance;
  double link_match_minimum_response_fine, link_scan_maximum_distance, loop_search_maximum_distance;
  int32_t do_loop_closing, loop_match_minimum_chain_size;
  double loop_match_maximum_variance_coarse, loop_match_minimum_response_coarse, loop_match_minimum_response_fine;
  double correlation_search_space_dimension, correlation_search_space_resolution, correlation_search_space_smear_deviation;
  double loop_search_space_dimension, loop_search_space_resolution, loop_search_space_smear_deviation;
  kh_match_params match;
} kh_mapper_params;
typedef struct kh_mapper_stats {
  int64_t scans_processed, matches, loop_candidates, loop_closures, speculation_discarded, nodes_removed;
  double process_ms, match_ms, solver_ms, update_ms, lifelong_ms;
  int64_t fused_declined, fused_declined_reason;   /* ... that went the general way, and why the last one did (kh_matcher_seq_stats [6], [7]) */
  int64_t fused_matches, fused_fine_passes;     /* sequential matches that took the fused path of one MatchScan / whose fine pass
                                                   the device finished (kh_matcher_seq_stats of the sequential matcher) */
  int64_t decay_calls_resident, decay_calls_packed;   /* node-decay calls scored from the resident readings + filter masks / sent
                                                   down the packed form because a candidate had no device copy */
  int64_t marginalize_fallbacks;                /* KH_REMOVE_MARGINALIZE: nodes node decay removed plainly because
                                                   kh_spa_marginalize_nodes would have refused them */
} kh_mapper_stats;
/* config/mapper_params_offline.yaml:31-66 */
KH_API void kh_mapper_params_default(kh_mapper_params * p);
/* max_candidates = capacity of one matcher batch (near chains / loop candidates beyond it go in further batches) */
KH_API int kh_mapper_create(const kh_mapper_params * params, const kh_laser * laser, int32_t device, int32_t max_candidates,
                            kh_mapper ** out);
/* The same mapper with its candidate batches (loop closure, near chains) dealt over one matcher pair per entry of `devices`
 * (kh_matcher_group); devices[0] also carries the sequential matches, the solver and the graph store.  The run is
 * identical to the one-device mapper's: the matches are independent and are consumed in candidate order. */
KH_API int kh_mapper_create_on_devices(const kh_mapper_params * params, const kh_laser * laser, const int32_t * devices,
                                       int32_t n_devices, int32_t max_candidates, kh_mapper ** out);
KH_API void kh_mapper_destroy(kh_mapper * m);
/* Mapper::Process for one scan: `ranges` = laser->n_beams readings, the odometric pose of the robot, the time stamp.
 * *accepted = 0 when the scan is dropped by HasMovedEnough (Mapper.cpp:3110-3142).  corrected_pose / covariance may be NULL. */
KH_API int kh_mapper_process(kh_mapper * m, const double * ranges, const double odometric_pose[3], double time,
                             int32_t * accepted, double corrected_pose[3], double covariance[9]);
/* ---- localization mode (slam_toolbox_localization.cpp) ----
 * Mapper::ProcessLocalization (Mapper.cpp:2831-2909) = Process + AddScanToLocalizationBuffer (:2911-2937): the accepted scan enters
 * a rolling buffer; once the buffer holds more than scan_buffer_size scans its oldest one leaves the graph, the solver and the scan
 * list like kh_mapper_remove_node (RemoveNodeFromGraph + RemoveScan).  Scans accepted by kh_mapper_process never enter the buffer:
 * a map built or loaded with it is permanent.  scan_buffer_size < 1 is KH_ERR_INVALID_ARG (the scan would evict itself). */
KH_API int kh_mapper_process_localization(kh_mapper * m, const double * ranges, const double odometric_pose[3], double time,
                                          int32_t * accepted, double corrected_pose[3], double covariance[9]);
/* Mapper::ProcessAgainstNode (Mapper.cpp:3023-3096; ProcessAtDock :3098-3102 is node_id 0): the running scans are cleared and
 * re-seeded with the node's scan, which becomes the last scan; the scan is matched against it WITHOUT the HasMovedEnough gate
 * (*accepted is always 1), its odometric pose is overwritten with the corrected pose (:3065), so the next scan's odometry
 * delta starts there; then vertex, edges, running scan and TryCloseLoop as in Process.  A removed or unknown node is
 * KH_ERR_NOT_FOUND (the reference dereferences NULL). */
KH_API int kh_mapper_process_against_node(kh_mapper * m, const double * ranges, const double odometric_pose[3], double time,
                                          int32_t node_id, int32_t * accepted, double corrected_pose[3], double covariance[9]);
/* Mapper::ProcessAgainstNodesNearBy (Mapper.cpp:2751-2829; "start near pose" / /initialpose, slam_toolbox_common.cpp:818-832,
 * slam_toolbox_localization.cpp:195-217): the node is kh_graph_find_near_by_scan of the odometric pose over the scans still in
 * the graph; with an empty graph there is no match and the scan becomes the first vertex.  add_to_localization_buffer != 0
 * puts the scan into the rolling buffer (what the localization node does). */
KH_API int kh_mapper_process_against_nodes_near_by(kh_mapper * m, const double * ranges, const double odometric_pose[3], double time,
                                                   int32_t add_to_localization_buffer, int32_t * accepted, double corrected_pose[3],
                                                   double covariance[9]);
/* Mapper::ClearLocalizationBuffer (Mapper.cpp:2939-2962): every buffered scan removed, oldest first; then the running scans and
 * the last scan are cleared, so the next scan is a first scan (no gate, no match). */
KH_API int kh_mapper_clear_localization_buffer(kh_mapper * m);
/* ids of the buffered scans, oldest first: *n = their number, `ids` (may be NULL) receives at most `cap` */
KH_API int kh_mapper_localization_buffer(const kh_mapper * m, int32_t * ids, int32_t cap, int32_t * n);
KH_API int32_t kh_mapper_num_scans(const kh_mapper * m);
KH_API int64_t kh_mapper_num_edges(const kh_mapper * m);
KH_API int kh_mapper_get_poses(const kh_mapper * m, double * corrected_poses /* 3 * num_scans */);
/* scan `index` as the matcher / occupancy grid / lifelong scoring read it (pointers stay valid until the next process) */
KH_API int kh_mapper_get_scan(const kh_mapper * m, int32_t index, kh_scan * scan, kh_scan_box * box);
KH_API int kh_mapper_get_stats(const kh_mapper * m, kh_mapper_stats * out);
/* Mapper::RemoveNodeFromGraph + MapperSensorManager::RemoveScan (Mapper.cpp:2964-3021, :208-218; what
 * LifelongSlamToolbox::removeFromSlamGraph does, slam_toolbox_lifelong.cpp:330-342): the scan's edges leave its
 * neighbours, the graph and the solver (RemoveConstraint), the node leaves the solver (RemoveNode) and the scan list. */
KH_API int kh_mapper_remove_node(kh_mapper * m, int32_t scan_id);
/* Vertex::GetAdjacentVertices of the scan's vertex, in the reference's order (Mapper.h:338-361): *n = their number,
 * `adjacent` (may be NULL) receives at most `capacity` scan ids.  Vertex::SetScore (Mapper.h:326-329), what
 * LifelongSlamToolbox::updateScoresSlamGraph does to a vertex that stays (slam_toolbox_lifelong.cpp:356-365).  Together
 * with kh_mapper_get_scan and kh_mapper_remove_node a host can run its own node-decay policy -- and the tests replay the
 * library's policy with an independent restatement. */
KH_API int kh_mapper_get_adjacency(const kh_mapper * m, int32_t scan_id, int32_t * adjacent, int32_t capacity, int32_t * n);
KH_API int kh_mapper_set_node_score(kh_mapper * m, int32_t scan_id, double score);
/* LifelongSlamToolbox::evaluateNodeDepreciation after every accepted scan (slam_toolbox_lifelong.cpp:149-178):
 * FindNearLinkedVertices within half the diagonal of the scan's bounding box, kh_lifelong_scores over them, removal of the
 * ones scoring below params->removal_score, the new score stored on the others.  params = NULL switches it off. */
KH_API int kh_mapper_set_lifelong(kh_mapper * m, const kh_decay_params * params);
/* kh_spa_marginalize_nodes on the mapper's solver, mirrored in the mapper: every listed scan leaves as in kh_mapper_remove_node
 * (adjacency, edge sources, localization buffer, device copies), every NEW constraint becomes an edge whose source is the hub, a
 * constraint fused into an existing one changes nothing in the topology.  The solver log gets the E / D lines of a removal and a
 * C line for every added or replaced constraint (its covariance column holds the inverse of the information).  Error codes as
 * kh_spa_marginalize_nodes; a removed or unknown scan is KH_ERR_NOT_FOUND. */
KH_API int kh_mapper_marginalize_nodes(kh_mapper * m, int32_t n, const int32_t * scan_ids);
/* How node decay (kh_mapper_set_lifelong) removes a scan.  KH_REMOVE_PLAIN (the default) is the reference's removal.  Under
 * KH_REMOVE_MARGINALIZE the scans of one decay step that score below removal_score are marginalized as one list, in the order
 * the step visits them; those the solver call would refuse (the gauge, more than 64 neighbours) are removed plainly and counted
 * in kh_mapper_stats.marginalize_fallbacks.  The localization buffer's evictions and kh_mapper_remove_node are plain in every
 * mode.  The mode is NOT part of a session file: a caller sets it again after kh_mapper_load. */
enum { KH_REMOVE_PLAIN = 0, KH_REMOVE_MARGINALIZE = 1 };
KH_API int kh_mapper_set_removal_mode(kh_mapper * m, int32_t mode);
/* ids of the scans still in the graph, ascending (ids[kh_mapper_num_alive]) */
KH_API int32_t kh_mapper_num_alive(const kh_mapper * m);
KH_API int kh_mapper_get_alive(const kh_mapper * m, int32_t * ids);
/* the solver plugin instance the mapper drives (RemoveNode / save / load ... ); owned by the mapper */
KH_API kh_spa * kh_mapper_solver(kh_mapper * m);
/* graph-aware covariances of scan poses (kh_spa_compute_covariances / kh_spa_get_covariances of the mapper's solver; a scan's
 * solver node carries the scan's id): computed on the first call after the graph or a pose has changed, answered from the
 * resident result otherwise.  scan_ids = NULL: all solver nodes in insertion order (n = kh_spa_num_nodes of the solver).
 * summary (may be NULL): the computation this call ran, all zeros when it ran none. */
KH_API int kh_mapper_get_covariances(kh_mapper * m, int32_t n, const int32_t * scan_ids, double * cov /* 9n */, kh_spa_cov_summary * summary);
/* kh_spa_get_relative_covariances of the mapper's solver, lazy in the same way: the column of ref_scan is computed
 * (kh_spa_compute_covariance_columns with that one query) only when it is not resident or is stale.  summary (may be NULL): the
 * computation this call ran, all zeros when it ran none. */
KH_API int kh_mapper_get_relative_covariances(kh_mapper * m, int32_t ref_scan, int32_t n, const int32_t * scan_ids, double * out /* 9n */,
                                              kh_spa_cov_columns_summary * summary);
/* kh_spa_get_difference_covariances of the mapper's solver (world-frame covariance of x_k - x_ref), lazy as above */
KH_API int kh_mapper_get_difference_covariances(kh_mapper * m, int32_t ref_scan, int32_t n, const int32_t * scan_ids, double * out /* 9n */,
                                                kh_spa_cov_columns_summary * summary);
/* ---- the covariance gate of the loop search (no counterpart in the reference, whose TryCloseLoop looks within a fixed radius;
 * DESIGN.md section 7h).  Enabled, TryCloseLoop enumerates with kh_graph_find_loop_candidates_gated: the search disk of
 * loop_search_maximum_distance widened, per scan, by the chi2_position ellipse of covariance_scale * D, D the world-frame covariance
 * of the scan's displacement from the current scan (kh_spa_get_difference_covariances).
 *   refresh  D is refreshed -- one column pass with the current scan as the query, then k_cov_difference over the scans alive --
 *            when refresh_scans TryCloseLoop calls have passed since the last refresh, and always after a closure moved the poses.
 *            In between the last D is reused; a scan appended since, and a scan the solver does not know, has D = 0.  A pass the
 *            solver refuses (KH_ERR_SOLVER: a component not tied to the gauge, fronts beyond the LDS budget) leaves that scan's
 *            search ungated and is counted; any other error is returned.
 *   reach    where s (Gxx + Gyy) > (max_reach / r)^2 - 1 (G = covariance_scale D, r the search distance, s = chi2_position / r^2)
 *            G is scaled down to meet it: no semi-axis of the widened ellipse exceeds max_reach.
 *   jump     (chi2_jump > 0) a chain whose fine match passes is still not accepted when the correction it asks for,
 *            e = fine mean - current sensor pose (angle normalised), has e^T (covariance_scale D3 + C_fine)^-1 e > chi2_jump or that
 *            3 x 3 is not positive definite; D3 = the full D of the chain's scan LinkChainToScan would link to, C_fine the fine
 *            match's covariance.  Consumption goes on to the next passing chain.
 * With enabled = 0 the mapper is the reference's; enabled with covariance_scale = 0, or with chi2_position = 0 and chi2_jump <= 0,
 * runs no column pass and is the same run bit for bit.  The gate is NOT part of a session file: after kh_mapper_load it is off.
 * Localization mode, kh_mapper_relocalize and sessions are untouched. */
typedef struct kh_loop_gate_params {
  int32_t enabled;
  int32_t refresh_scans;        /* >= 1 */
  double chi2_position;         /* >= 0; 5.991 = 95 % of chi-square, 2 degrees of freedom */
  double chi2_jump;             /* <= 0: no jump test; 7.815 = 95 %, 3 degrees of freedom */
  double covariance_scale;      /* >= 0: how far the solver's covariances are trusted */
  double max_reach;             /* > 0, metres; default loop_search_maximum_distance + loop_search_space_dimension / 2: the coarse
                                   matcher cannot pull a scan further than half its window */
} kh_loop_gate_params;
typedef struct kh_loop_gate_stats {
  int64_t column_passes;        /* refreshes that ran */
  int64_t ungated_searches;     /* scans whose search ran ungated because the solver refused the pass */
  int64_t jump_rejected;        /* chains the jump test kept from being accepted */
  double column_ms;             /* wall time of the refreshes (pass + k_cov_difference + download) */
  double max_semi_axis;         /* metres: the largest semi-axis sqrt(r^2 + chi2_position lambda_max(G)) of a prepared row */
} kh_loop_gate_stats;
/* params = NULL: kh_mapper_params_default's distances */
KH_API void kh_loop_gate_params_default(const kh_mapper_params * params, kh_loop_gate_params * gate);
/* refresh_scans < 1, chi2_position < 0, covariance_scale < 0, max_reach <= 0, a NaN or an infinite value (chi2_jump may be
 * infinite): KH_ERR_INVALID_ARG, before the device is looked for; then KH_ERR_NO_DEVICE, then the handle */
KH_API int kh_mapper_set_loop_gate(kh_mapper * m, const kh_loop_gate_params * gate);
KH_API int kh_mapper_get_loop_gate(const kh_mapper * m, kh_loop_gate_params * gate);
KH_API int kh_mapper_get_loop_gate_stats(const kh_mapper * m, kh_loop_gate_stats * out);
/* ---- single-edge edits, the constraint audit and outlier rejection (no counterpart in the reference).
 * kh_mapper_add_edge + kh_mapper_correct_poses are the interactive node's "manual loop closure".
 * kh_mapper_add_edge: MapperGraph::LinkScans made public.  mean_sensor_pose = the SENSOR pose of `to` the constraint asserts, as
 *   LinkChainToScan passes it, cov its covariance; the duplicate test of AddEdge (an edge from -> to exists: nothing is attached,
 *   KH_OK) and the `C` log line are LinkScans'.  correct != 0: kh_mapper_correct_poses afterwards.  A dead or unknown scan, or
 *   from == to: KH_ERR_NOT_FOUND; a NULL or non-finite mean or cov: KH_ERR_INVALID_ARG before the device is looked for.
 * kh_mapper_remove_edge: the edge with that source and target leaves the adjacency of both scans, the edge list and the solver
 *   (kh_spa_remove_constraint), with the `E from to` log line of a node removal.  KH_ERR_NOT_FOUND (nothing changed) when there is
 *   no such edge -- the direction counts.
 * kh_mapper_correct_poses: MapperGraph::CorrectPoses -- solve, every scan re-posed and re-projected.
 * kh_mapper_audit: kh_spa_audit_constraints on the mapper's solver (node ids are scan ids); *n = the number of constraints, which
 *   cap must hold (KH_ERR_INVALID_ARG otherwise, *n still set). */
KH_API int kh_mapper_add_edge(kh_mapper * m, int32_t from, int32_t to, const double mean_sensor_pose[3], const double cov[9], int32_t correct);
KH_API int kh_mapper_remove_edge(kh_mapper * m, int32_t from, int32_t to);
KH_API int kh_mapper_correct_poses(kh_mapper * m);
KH_API int kh_mapper_audit(kh_mapper * m, double min_redundancy, kh_spa_audit_t * out, int32_t cap, int32_t * n, kh_spa_audit_summary * summary);
/* Outlier rejection.  Each round: kh_mapper_correct_poses, then the audit; the candidates are the verifiable constraints with
 * |id_a - id_b| >= min_id_gap (odometry is exempt: on a cycle that only a false closure closes every edge of the cycle has the
 * same chi2_loo); top = their largest chi2_loo; top <= chi2 ends the loop; otherwise, among the candidates with
 * chi2_loo >= (1 - tie) top, the one with the highest constraint index -- the constraint added last is the one the graph was
 * consistent without -- leaves through kh_mapper_remove_edge, and the next round begins.  When the rounds run out behind a
 * removal a final kh_mapper_correct_poses follows, so the poses are always those of a solve after the last removal.  An
 * unverifiable constraint is never removed: the number of connected components cannot grow and the solver never loses a pinned
 * direction.  removed[k]: the record of the k-th removal as audited in the round that removed it; more removals than cap:
 * KH_ERR_INVALID_ARG (the graph keeps the removals made).  The loop gate, when on, refreshes at the next scan. */
typedef struct kh_reject_params {
  double chi2;                  /* >= 0; 16.266 = 99.9 % of chi-square, 3 degrees of freedom */
  double min_redundancy;        /* in (0, 1); 1e-6 */
  double tie;                   /* in [0, 1); 1e-6: candidates within this relative distance of the top are tied */
  int32_t min_id_gap;           /* >= 1; 2: consecutive scans (odometry) are no candidates */
  int32_t max_rounds;           /* >= 1; 8 */
} kh_reject_params;
typedef struct kh_reject_summary {
  int32_t rounds;               /* audits run */
  int32_t n_removed;
  double max_chi2_loo;          /* the largest chi2_loo among the candidates of the last audit (0: no candidate) */
  double solve_ms, audit_ms;    /* wall time of the kh_mapper_correct_poses calls / of the audits (covariance pass included) */
  double total_ms;
} kh_reject_summary;
KH_API void kh_reject_params_default(kh_reject_params * params);
/* params = NULL: the defaults.  min_id_gap < 1, max_rounds < 1, tie outside [0, 1), min_redundancy outside (0, 1), chi2 < 0, a
 * non-finite parameter, cap < 0 or removed = NULL with cap > 0: KH_ERR_INVALID_ARG before the device is looked for; then
 * KH_ERR_NO_DEVICE, then the handle. */
KH_API int kh_mapper_reject_outliers(kh_mapper * m, const kh_reject_params * params, kh_spa_audit_t * removed, int32_t cap, kh_reject_summary * summary);
/* every solver call the mapper makes, one line each, in the format oracle/ref_slam_driver.cpp logs the reference
 * Mapper's calls with (N id pose, C a b z cov, X n ms, P id pose, K): the two logs of one scan queue must agree */
KH_API int kh_mapper_set_log(kh_mapper * m, const char * path);

/* ---- mapping sessions: save, load, resume (slam_toolbox's serializePoseGraph / deserializePoseGraph + loadSerializedPoseGraph,
 * slam_toolbox_common.cpp:952-1017).  The reference writes a Boost binary archive of the Mapper; here the session file is the
 * library's own little-endian format "KHMS" (DESIGN.md section 7 lists it byte by byte): parameters, laser, the lifelong switch,
 * every scan still in the map (id, time, odometric and corrected pose, vertex score, ranges), the adjacency lists and edge
 * sources in insertion order, the running scans, the last scan, the localization buffer, and the solver -- nodes and
 * constraints in insertion order with the information matrices as stored, the gauge, and the analysis cache that decides
 * whether the next Compute() dissects from scratch or incrementally.  A mapper loaded from a file continues the run the
 * saved mapper would have made, call for call.  Point readings, masks, barycentres and boxes are not stored: load recomputes
 * them with LocalizedRangeScan::Update on the host.  The reference's post-load solver_->Compute() is NOT part of load.
 * kh_mapper_save refuses (KH_ERR_INVALID_ARG) a mapper whose earlier Process() failed.  kh_mapper_load and kh_session_info answer
 * KH_ERR_IO with a kh_last_error() text for a missing file, a wrong magic, an unknown version, a truncated file, a checksum
 * mismatch and counts that do not fit the file; kh_mapper_load validates the whole file BEFORE it touches a device, so a good
 * file on a machine without one is KH_ERR_NO_DEVICE.  devices / max_candidates as in kh_mapper_create_on_devices. */
typedef struct kh_session_info_t {
  int64_t version, file_bytes;
  int64_t n_beams;
  int64_t n_scan_slots;            /* kh_mapper_num_scans: ids handed out so far, removed ones included */
  int64_t n_alive;                 /* kh_mapper_num_alive */
  int64_t n_edges;                 /* kh_mapper_num_edges */
  int64_t n_running, last_scan;    /* running-scan window, id of the last scan (-1 none) */
  int64_t n_localization_buffer;
  int64_t lifelong;                /* 1: kh_mapper_set_lifelong was on */
  int64_t n_solver_nodes, n_solver_constraints, n_supernodes;
} kh_session_info_t;
KH_API int kh_mapper_save(const kh_mapper * m, const char * path);
KH_API int kh_mapper_load(const char * path, const int32_t * devices, int32_t n_devices, int32_t max_candidates, kh_mapper ** out);
KH_API int kh_session_info(const char * path, kh_session_info_t * out);     /* needs no device */
/* wall time of the pieces of the last successful kh_mapper_load of this process, ms: [0] read + validate, [1] create + Update of
 * every scan, [2] adjacency + solver rebuild, [3] graph store */
KH_API int kh_session_last_load_ms(double out[4]);
/* OccupancyGrid::CreateFromScans (Karto.h:5947-5962) over the scans still in the map, read where the mapper keeps them in HBM:
 * dimensions from the per-scan boxes (equal to kh_occupancy_compute_dimensions over the same scans with the laser's minimum
 * range and range threshold), one trace kernel over a table of (points, ranges, sensor position) per scan, then Update.  A
 * scan's ranges are uploaded once in its life, its point readings only when its pose has moved since the last upload, so a
 * rebuild after k new scans moves k scans.  *out is an ordinary kh_occupancy (kh_occupancy_read / _info / _destroy). */
KH_API int kh_mapper_build_map(kh_mapper * m, double resolution, uint32_t min_pass_through, double occupancy_threshold,
                               kh_occupancy ** out);
/* LocalizedRangeScan::SetCorrectedPose + Update (Karto.h:5644-5704) for one scan still in the map: its readings, box and
 * barycentre follow the new pose at once.  The solver's node is not touched, as in the reference: the next CorrectPoses (a loop
 * closure) puts the scan back where the solver has it.  For a caller that places scans itself -- a mapper created with
 * use_scan_matching 0, an interactive tool -- and for the live map's tests.  A removed or unknown id is KH_ERR_NOT_FOUND. */
KH_API int kh_mapper_set_scan_pose(kh_mapper * m, int32_t scan_id, const double corrected_pose[3]);
/* counters of kh_mapper_build_map: [0] calls, [1] scans traced by the last call, [2] point-reading uploads and [3] range uploads
 * the last call made, [4], [5] the same two since the mapper was made */
KH_API int kh_mapper_map_stats(const kh_mapper * m, int64_t out[6]);

/* ---- global relocalization: place one scan in the map without a pose guess.  Every hypothesis is
 * MapperGraph::TryCloseLoop's own test (Mapper.cpp:1515-1549, kh_loop_closure_batch) with the scan placed at a pose taken from the
 * map: hypothesis k * n_headings + h puts the robot at seed k's corrected position with heading -pi + h * (2 pi / n_headings) (the
 * sensor through the laser's offset, the readings with kh_scan_points) and matches against the seed's base
 * (kh_graph_relocalize_candidates with base_radius = loop_search_maximum_distance): coarse match on the loop matcher, the gate
 * (response > loop_match_minimum_response_coarse, cov(0,0) and cov(1,1) < loop_match_maximum_variance_coarse), fine match of the
 * temporary scan on the sequential matcher, accepted when fine response >= loop_match_minimum_response_fine.  The accepted ones come
 * back by fine response (descending), then coarse response (descending), then index. */
typedef struct kh_relocalize_params {
  double seed_spacing;      /* side of the seed lattice, > 0 (default: loop_search_maximum_distance / 2) */
  int32_t n_headings;       /* headings per seed; 0 = ceil(2 pi / (2 * coarse_search_angle_offset)), 10 for the shipped 0.349 rad */
  int32_t max_base;         /* most base scans per hypothesis, >= 1 (default 40) */
  int32_t top_k;            /* most hypotheses returned; 0 = as many as `cap` holds (default 8) */
  int32_t pad;
  double center_xy[2];      /* with radius > 0: only the seeds within radius of this point */
  double radius;            /* <= 0: the whole map (default) */
} kh_relocalize_params;
typedef struct kh_relocalize_hyp {
  int32_t index;            /* seed ordinal * n_headings + heading ordinal */
  int32_t seed_scan;        /* scan id of the seed */
  double heading;
  double coarse_mean[3], coarse_cov[9], coarse_response;      /* sensor pose of the coarse match */
  double fine_mean[3], fine_cov[9], fine_response;            /* sensor pose of the fine match */
  double robot_pose[3];     /* GetCorrectedAt(fine_mean): what goes to kh_mapper_process_against_nodes_near_by */
} kh_relocalize_hyp;
typedef struct kh_relocalize_summary {
  int32_t n_seeds, n_headings, n_hypotheses, n_passed /* the coarse gate */, n_accepted, n_returned;
  double kernel_ms;         /* device time of the seed and base kernels */
  double candidates_ms, scans_ms, batch_ms, total_ms;         /* wall: enumeration, query scans on the host, match batches, the call */
} kh_relocalize_summary;
/* the parameters the mapper was created (or loaded) with */
KH_API int kh_mapper_get_params(const kh_mapper * m, kh_mapper_params * out);
/* defaults for a mapper with parameters *mapper_params (NULL: kh_mapper_params_default's) */
KH_API void kh_relocalize_params_default(const kh_mapper_params * mapper_params, kh_relocalize_params * p);
/* out takes the first min(top_k, cap) accepted hypotheses (top_k 0: cap), the summary the totals.  NULL ranges / params / summary,
 * out NULL with cap > 0, seed_spacing <= 0, n_headings < 0, max_base < 1, top_k < 0, cap < 0 or a non-finite parameter are
 * KH_ERR_INVALID_ARG before the device is touched; without a device KH_ERR_NO_DEVICE; an empty map is KH_OK with zero everything.
 * The mapper is left as it was: no vertex, edge, running scan, last scan or solver state changes (scans the batches read become
 * resident on the device, as in any loop-closure batch), and a failure leaves it usable.  Like kh_mapper_build_map the call must not
 * run concurrently with a Process* call. */
KH_API int kh_mapper_relocalize(kh_mapper * m, const double * ranges, const kh_relocalize_params * params, kh_relocalize_hyp * out,
                                int32_t cap, kh_relocalize_summary * summary);

/* ---- merging sessions (slam_toolbox's merge_maps_kinematic, src/merge_maps_kinematic.cpp): several mappers -- live ones, or
 * sessions loaded from files -- each placed by a rigid correction T = (tx, ty, yaw), and ONE occupancy grid traced from all their
 * scans where they lie in HBM.  The reference moves a submap by dragging a marker (processInteractiveFeedback :313-352), rewrites
 * every scan with the correction (transformScan :195-248) and calls OccupancyGrid::CreateFromScans (mergeMapCallback :251-291).
 * Here a merge never modifies a session: the correction is applied to every point reading inside the trace kernel, so a re-merge
 * after a correction changed uploads two small tables and no reading.  The arithmetic is this library's own (DESIGN.md section
 * 7a; tf2 agrees with it to rounding): with c = cos(yaw), s = sin(yaw) taken once per submap,
 *   point   x' = (c x - s y) + tx,  y' = (s x + c y) + ty
 *   pose    position as a point, heading' = math::NormalizeAngle(heading + yaw)
 *   A . B = (A.x + (cA B.x - sA B.y), A.y + (sA B.x + cA B.y), NormalizeAngle(A.yaw + B.yaw))
 * The sensor position of a scan is GetSensorAt(transformed corrected pose) with the submap's laser; the box of a scan is the
 * min / max of the four transformed corners of its stored box (loose, like the reference's).  Submaps may have different lasers;
 * all are on the merger's device.  Submap ids are handed out ascending and never reused; the merged map takes the submaps in id
 * order, each one's scans in scan-id order. */
typedef struct kh_merge kh_merge;
KH_API int kh_merge_create(int32_t device, double resolution, kh_merge ** out);
KH_API void kh_merge_destroy(kh_merge * g);        /* destroys the mappers it loaded itself, never a borrowed one */
/* borrows a live mapper: the caller keeps it alive until kh_merge_remove_submap (or kh_merge_destroy) and may go on processing
 * scans with it between merges.  A mapper on another device is KH_ERR_INVALID_ARG. */
KH_API int kh_merge_add_mapper(kh_merge * g, kh_mapper * m, int32_t * submap_id);
/* kh_mapper_load of the file onto the merger's device (error codes as there); the merger owns the mapper */
KH_API int kh_merge_add_session(kh_merge * g, const char * path, int32_t * submap_id);
KH_API int kh_merge_remove_submap(kh_merge * g, int32_t submap_id);                     /* unknown id: KH_ERR_NOT_FOUND, as everywhere below */
KH_API int32_t kh_merge_num_submaps(const kh_merge * g);
/* out[0] = scans still in the submap's map, out[1] = beams of its laser */
KH_API int kh_merge_submap_info(const kh_merge * g, int32_t submap_id, int32_t out[2]);
/* the correction of a submap (the identity (0, 0, 0) when it is added).  A correction that is not finite (NaN, +-inf in any of the
 * three places) is KH_ERR_INVALID_ARG and leaves the correction as it was. */
KH_API int kh_merge_set_transform(kh_merge * g, int32_t submap_id, const double t[3]);
KH_API int kh_merge_get_transform(const kh_merge * g, int32_t submap_id, double t[3]);
/* the release of the marker at marker_pose = (x, y, yaw): correction <- correction . inverse(translation(previous location)) .
 * marker_pose, then location <- (x, y, location yaw + yaw).  The location starts at the centre of the submap's own grid at the
 * merger's resolution, (offset + width * resolution / 2, offset + height * resolution / 2, 0) (addSubmapCallback :115-122).
 * A marker pose that is not finite is KH_ERR_INVALID_ARG and leaves correction and location as they were. */
KH_API int kh_merge_move_submap(kh_merge * g, int32_t submap_id, const double marker_pose[3]);
KH_API int kh_merge_get_location(const kh_merge * g, int32_t submap_id, double location[3]);
/* what transformScan leaves on scan `index` (0 .. info[0] - 1, scan-id order) of the submap under its current correction:
 * corrected, odometric and barycenter pose (the barycenter's heading is 0 before the correction), box = min x, min y, max x,
 * max y, and the 2 * n_beams unfiltered point readings (computed on the host for this call).  Any output may be NULL. */
KH_API int kh_merge_get_scan(const kh_merge * g, int32_t submap_id, int32_t index, double corrected_pose[3], double odometric_pose[3],
                             double barycenter_pose[3], double box[4], double * points_xy);
/* the submap's own, untransformed grid: kh_mapper_build_map of its mapper at the merger's resolution */
KH_API int kh_merge_build_submap(kh_merge * g, int32_t submap_id, uint32_t min_pass_through, double occupancy_threshold,
                                 kh_occupancy ** out);
/* the merged map: dimensions from the transformed boxes of every scan (rounded like kh_occupancy_compute_dimensions), one trace
 * kernel over every submap's resident scans, Update.  *out is an ordinary kh_occupancy.  No submap, or no scan in any of them,
 * is KH_ERR_INVALID_ARG. */
KH_API int kh_merge_build(kh_merge * g, uint32_t min_pass_through, double occupancy_threshold, kh_occupancy ** out);
/* [0] merges made, [1] scans and [2] beams traced by the last merge, [3] point-reading and [4] range uploads of the last merge,
 * [5], [6] the same two since the merger was made, [7] bytes of the two tables the last merge uploaded */
KH_API int kh_merge_stats(const kh_merge * g, int64_t out[8]);

/* ---- how well a correction places a submap, and corrections found automatically ("Fit and alignment").
 * The REFERENCE GRID of a submap M is the merge of every OTHER submap under its current correction (kh_merge_build without M).
 * For a candidate correction C of M, M's scans are traced under C on that grid's geometry exactly as kh_merge_build would trace
 * them -- the same gate, roundings and TraceLine walk -- but every visit looks up the STATE of the cell it would have incremented
 * (0 unknown, 100 occupied, 255 free) and is counted by state; visits outside the grid are dropped.  pass_s counts all visits of
 * cells in state s, hits_s those that are the end point of a beam that counts as a hit.  The end cell of a hit beam is visited
 * twice (by the line, then as the hit), so pass_s - 2 hits_s is the number of visits that are not such an end cell:
 *   agree    = hits_occupied + (pass_free - 2 hits_free)        beam ends on walls the others saw, rays through what they saw free
 *   conflict = (pass_occupied - 2 hits_occupied) + hits_free    rays through walls the others saw, beam ends where they saw free
 *   known    = agree + conflict;  score = agree / known as one FP64 division, 0.0 when known is 0
 * All sums are integers, so the result does not depend on the order the device adds them in. */
typedef struct kh_merge_fit_t {
  uint64_t pass_unknown, pass_occupied, pass_free, hits_unknown, hits_occupied, hits_free;
  uint64_t agree, conflict, known;
  double score;
} kh_merge_fit_t;
/* n_candidates corrections (tx, ty, yaw) of ONE submap against the merge of all the others: the reference grid is built once, then
 * one kernel counts every candidate (one wave per candidate, scan and run of 64 beams; k_occ_fit_merged).  Nothing of the merger
 * changes: no correction, no location.  NULL corrections / out, n_candidates < 1, a non-finite correction or a non-finite
 * occupancy_threshold are KH_ERR_INVALID_ARG before a device is looked for; without a device KH_ERR_NO_DEVICE; then a NULL merger
 * is KH_ERR_INVALID_ARG (the handle is looked at after the device, as kh_mapper_relocalize looks at its mapper: a merger cannot
 * exist without one); an unknown id KH_ERR_NOT_FOUND; no other submap, or no scan in any other submap, KH_ERR_INVALID_ARG as for
 * kh_merge_build.  Every min_pass_through is valid (a cell is known when it was passed more often), as for kh_occupancy_update.
 * A candidate may put the submap anywhere, and a beam is walked cell by cell from the sensor to its end: once the reference grid
 * exists and before anything is launched, KH_ERR_INVALID_ARG (a) where the moving submap's laser has range_threshold / resolution +
 * 2 > 2^20 cells, a range_threshold that is not finite and positive, or a minimum or maximum range that is NaN, and (b) where
 * under some candidate the sensor of one of the submap's scans lies more than 2^30 cells from the reference grid's offset on either
 * axis, |(sensor - offset) / resolution| > 2^30; kh_last_error() names the first such candidate by its index.  (Far outside the
 * grid is no reason: such a candidate counts nothing.)  kh_merge_fit_stats is unchanged by a refusal.
 * A failure leaves the merger usable. */
KH_API int kh_merge_fit(kh_merge * g, int32_t submap_id, int32_t n_candidates, const double * corrections /* 3n */,
                        uint32_t min_pass_through, double occupancy_threshold, kh_merge_fit_t * out /* n */);
/* [0] fits made (kh_merge_align makes one), [1] candidates fitted since the merger was made, [2] beams x candidates and [3] kernel
 * microseconds (HIP events) of the last fit */
KH_API int kh_merge_fit_stats(const kh_merge * g, int64_t out[4]);

/* Automatic alignment of submap `moving` to submap `target`.  n_probes scans of the moving submap -- entry floor(j * n_alive /
 * n_probes), j = 0 .. n_probes - 1, of its scans in scan-id order, n_probes clipped to their number -- are relocalized in the
 * target's map (kh_mapper_relocalize on the target's mapper with the probe's ranges).  Each returned hypothesis implies the
 * correction C = (T_target . P) . inverse(Q): P the hypothesis' robot_pose, Q the probe's corrected pose in its own session, T_target
 * the target's correction, `.` and inverse as kh_merge_move_submap composes.  Candidate 0 is the moving submap's current
 * correction, then the probes in order, each one's hypotheses in rank order; nothing is de-duplicated.  One scan cannot tell two
 * identical aisles apart, so the candidates are ranked by how the WHOLE session fits (kh_merge_fit against
 * all other submaps): known >= min_known first, then score descending, agree descending, candidate index ascending. */
typedef struct kh_merge_align_params {
  int32_t n_probes;            /* probe scans of the moving submap, >= 1 (default 4) */
  int32_t top_k;               /* hypotheses kept per probe, >= 1 (default 4) */
  uint64_t min_known;          /* candidates with fewer known visits rank last (default 0) */
  uint32_t min_pass_through; uint32_t pad; double occupancy_threshold;        /* the reference grid's Update rule (defaults 2, 0.1) */
  kh_relocalize_params relocalize;   /* as for kh_mapper_relocalize on the target's mapper; its top_k is overridden by top_k above */
} kh_merge_align_params;
typedef struct kh_merge_align_cand {
  double correction[3];
  int32_t probe_scan;          /* scan id in the moving submap; -1 for candidate 0 */
  int32_t hypothesis;          /* rank of the hypothesis in the probe's relocalization; -1 for candidate 0 */
  double fine_response;        /* 0 for candidate 0 */
  int32_t index, enough;       /* candidate index before ranking; known >= min_known */
  kh_merge_fit_t fit;
} kh_merge_align_cand;
/* defaults; the relocalization parameters are those of the target's mapper (g NULL or an unknown id: of kh_mapper_params_default) */
KH_API void kh_merge_align_params_default(const kh_merge * g, int32_t target_submap, kh_merge_align_params * p);
/* out takes the first min(cap, n) ranked candidates, *n_candidates takes n.  times_ms (may be NULL): [0] the relocalizations, [1]
 * the fit's reference grid, [2] the fit kernel (HIP events), [3] the whole call.  The merger and both mappers are left as they
 * were (scans become resident on the device, as in any merge); the caller applies a result with kh_merge_set_transform.
 * KH_ERR_INVALID_ARG before a device is looked for: NULL params / n_candidates, out NULL with cap > 0, cap < 0, n_probes < 1,
 * top_k < 1, a non-finite occupancy_threshold, invalid relocalization parameters, moving == target (every min_pass_through and
 * min_known is valid).  Then: no device KH_ERR_NO_DEVICE, a NULL merger KH_ERR_INVALID_ARG, an unknown id KH_ERR_NOT_FOUND, lasers that differ in any field of kh_laser KH_ERR_INVALID_ARG (the probe's ranges are read by the target's
 * laser; kh_merge_fit has no such restriction).  The candidates are fitted as kh_merge_fit fits them: its refusals (a) and (b)
 * apply, under this call's name.  A failure leaves the merger usable. */
KH_API int kh_merge_align(kh_merge * g, int32_t moving_submap, int32_t target_submap, const kh_merge_align_params * params,
                          kh_merge_align_cand * out, int32_t cap, int32_t * n_candidates, double times_ms[4]);

/* ---- the live map: the occupancy map slam_toolbox republishes every map_update_interval, kept on the mapper's device and brought
 * up to date by the DIFFERENCE since the last update instead of a fresh kh_mapper_build_map over every scan.  After
 * kh_live_map_update the pass / hit / cell grids are, bit for bit, what a fresh trace of the mapper's scans at their current poses
 * gives on the same lattice; the work is proportional to the scans that entered, left or moved.
 *
 * Lattice: an anchor (ax, ay) and a resolution, fixed at creation.  The cell of a world point is
 * o_to_int(o_round((x - ax) * scale)), scale = 1 / resolution -- k_occ_trace's own operations -- and may be negative.
 * Window: the grids cover lattice cells [ox, ox + width) x [oy, oy + height), row stride width_step = (width + 7) & ~7.  With
 * reach = ceil(range_threshold / resolution) + 2, the window holds every cell within `reach` of the sensor cell of every scan in
 * the map, rounded outward to multiples of 64 cells of the lattice, so no beam is ever clipped; it grows when a scan does not fit
 * (the counters are copied to their new place) and never shrinks.  kh_occupancy_create's size cap applies: an update whose window
 * would have (width + 7) * height > 2^31 - 4096 returns KH_ERR_INVALID_ARG and leaves the live map exactly as it was.
 * anchor = NULL: the offset kh_mapper_build_map would choose at that moment (needs a scan in the map); right after creation the
 * live map then equals kh_mapper_build_map's grid on the whole of that grid's rectangle.
 *
 * Each update classifies the mapper's scans against the log of what the map has traced: NEW scans are traced in (+1), GONE scans
 * (kh_mapper_remove_node, the localization buffer, node decay) are walked out of the counters along the logged lines (-1), MOVED
 * scans (the bits of the sensor pose differ: a loop closure, kh_mapper_set_scan_pose) have each beam's new line compared with the
 * logged one and only the beams that differ re-walked.  When more than rebuild_fraction of the scans in the map are in the delta
 * the update clears the counters and traces everything instead: 0 = always, +inf = never, negative = the library's default.
 *
 * The live map BORROWS the mapper: destroy the live map first.  Like kh_mapper_build_map, an update must not run concurrently
 * with a Process call of its mapper.  A live map is not part of a session file: after kh_mapper_load make a new one, whose first
 * update is a full pass.  The grids are on the mapper's own device. */
typedef struct kh_live_map kh_live_map;
typedef struct kh_live_map_info_t {
  double anchor[2], resolution, rebuild_fraction;
  int32_t ox, oy, width, height, width_step;    /* all zero before the first scan */
  int32_t reach;
} kh_live_map_info_t;
typedef struct kh_live_map_counts {
  int64_t scans_added, scans_removed, scans_moved;    /* the classification, whichever path the update took */
  int64_t beams_traced;            /* lines walked, +1 or -1 */
  int64_t beams_skipped;           /* traced beams of moved scans whose line did not change: left alone */
  int64_t cells_updated;           /* cells given to the cell-state kernel */
  int64_t relayouts;               /* the window grew */
  int64_t rebuilds;                /* the update cleared the counters and traced every scan (last: 0 or 1) */
  double trace_ms;                 /* the trace kernel, by device events */
} kh_live_map_counts;
typedef struct kh_live_map_stats_t {
  kh_live_map_counts last, total;  /* the last update / all updates */
  int64_t updates, scans_in_map, log_bytes;
} kh_live_map_stats_t;
KH_API int kh_live_map_create(kh_mapper * m, double resolution, const double anchor[2], double rebuild_fraction, kh_live_map ** out);
KH_API void kh_live_map_destroy(kh_live_map * g);
/* min_pass_through / occupancy_threshold as kh_occupancy_update.  The cell states are recomputed over the rectangle the delta can
 * have touched; over the whole window on the first call, after the window grew, after a rebuild and when the two parameters
 * differ from the previous call's. */
KH_API int kh_live_map_update(kh_live_map * g, uint32_t min_pass_through, double occupancy_threshold);
KH_API int kh_live_map_info(const kh_live_map * g, kh_live_map_info_t * out);
/* layout of kh_occupancy_read over the window: width_step * height entries each; any pointer may be NULL */
KH_API int kh_live_map_read(kh_live_map * g, uint8_t * cells, uint32_t * pass, uint32_t * hits);
KH_API int kh_live_map_stats(const kh_live_map * g, kh_live_map_stats_t * out);
/* the window's cell states as a kh_map_view (borrowed: valid until the next kh_live_map_update); KH_ERR_NOT_FOUND before the
 * first scan gave the map a window */
KH_API int kh_live_map_view(kh_live_map * g, kh_map_view * out);

/* ---- the map feed: the live map's way out, for a costmap, a viewer, a map_msgs/OccupancyGridUpdate publisher.  A feed hands its
 * consumer, as nav_msgs/OccupancyGrid values (-1 unknown, 100 occupied, 0 free: vis_utils::toNavMap), the 16 x 16 TILES whose
 * values changed since the consumer last asked, and nothing else.  Several feeds may be bound to one live
 * map, one per consumer, each polled at its own pace.
 *
 * The feed owns the PUBLISHED GRID on the device: one int8 per lattice cell of the window the feed has seen, holding what the
 * consumer has been told so far.  Every cell the feed has never reported is -1, the cells outside every window it has seen
 * included: a consumer starts from an all -1 map and grows it with -1.
 * Tile (tx, ty) covers lattice cells [16 tx, 16 tx + 16) x [16 ty, 16 ty + 16); tx, ty are floor quotients, negative left of and
 * below the anchor.  The live window's origin and size are multiples of 64, so a tile never straddles its edge.
 *
 * kh_live_map_update adds the cells it handed to the cell-state kernel -- a rectangle, or the whole window -- to the PENDING
 * REGION of every feed attached; updates between two polls accumulate.  kh_map_feed_poll follows the live window (a new
 * published grid filled with -1, the old content copied to its place), rounds the pending region outward to whole tiles, compares
 * the nav values of those tiles with the published grid on the device, and downloads the number of tiles that differ, their
 * coordinates and their 256 bytes each.  The published grid takes the new values of exactly those tiles.  With nothing pending,
 * or before the live map has a window, a poll launches nothing and reports 0 tiles.
 *
 * The feed BORROWS the live map: destroy the feed first.  A poll must not run concurrently with an update of its live map or a
 * Process call of the mapper.  A poll that meets a HIP error marks the feed's whole window pending, so the next one compares
 * everything again.  Feeds are not part of a session file, and a merge (kh_merge_build) has none: kh_occupancy_read_nav gives its
 * values. */
#define KH_MAP_TILE 16
typedef struct kh_map_feed kh_map_feed;
typedef struct kh_map_feed_delta_t {
  int64_t n_tiles;                 /* tiles that changed: what kh_map_feed_tiles hands out */
  int64_t tiles_scanned;           /* tiles compared on the device */
  int64_t bytes_downloaded;        /* device-to-host bytes of this poll: the count, 8 bytes of coordinates and 256 of values per tile */
  int32_t ox, oy, width, height;   /* the feed's window in lattice cells (= the live map's after a poll) */
  int32_t x, y, w, h;              /* bounding rectangle of the changed tiles in lattice cells (an OccupancyGridUpdate's); zero without tiles */
  double kernel_ms;                /* the compare kernel, by device events */
} kh_map_feed_delta_t;
typedef struct kh_map_feed_stats_t {
  int64_t polls, n_tiles, tiles_scanned, bytes_downloaded;      /* totals over every poll */
  double kernel_ms;
} kh_map_feed_stats_t;
KH_API int kh_map_feed_create(kh_live_map * g, kh_map_feed ** out);
KH_API void kh_map_feed_destroy(kh_map_feed * f);
KH_API int kh_map_feed_poll(kh_map_feed * f, kh_map_feed_delta_t * out);
/* what the last poll fetched: n_tiles tiles in ascending (ty, tx) order; tile_xy gets tx, ty per tile, data 256 values per tile,
 * 16 rows of 16, row-major.  Either pointer may be NULL. */
KH_API int kh_map_feed_tiles(const kh_map_feed * f, int32_t * tile_xy, int8_t * data);
/* lattice cells [x, x + w) x [y, y + h) of the published grid, dense (w * h values, row-major): a late joiner's full map, or an
 * update rectangle.  Cells outside the feed's window read -1; any x, y and any w, h >= 0 whose product fits an int32 are legal. */
KH_API int kh_map_feed_read(kh_map_feed * f, int32_t x, int32_t y, int32_t w, int32_t h, int8_t * out);
KH_API int kh_map_feed_stats(const kh_map_feed * f, kh_map_feed_stats_t * out);

/* ---------------------------------------------------------------- matching a scan against a map
 * The correlation grid of a slot rasterised from a MAP instead of base scans: centred on the query's sensor pose (MatchScan steps
 * 1-4), cleared, then ScanMatcher::AddScan's point loop (Mapper.cpp:1082-1104: WorldToGrid, region-of-interest test, "cell
 * already 100 -> skip", SmearPoint) over the world points of the map's cells whose state is exactly 100, visited in row-major
 * order (row j outer, column i inner).  There is no FindValidPoints: a map has no viewpoint-facing side.  Everything behind the
 * rasterisation is what the scan-sourced entry points run.
 * KH_ERR_INVALID_ARG: a NULL or malformed view (non-positive sizes, width_step < width, a scale that is not finite or <= 0, NULL
 * cells), a view on another device than the matcher's, a bad slot, n > max_batch.  A map with no occupied cell in reach is not an
 * error: the grid is empty, and the match is what MatchScan gives on an empty grid. */
/* kh_matcher_add_scans with the map in the place of the base scans; kh_matcher_correlate*, _read_grid and the covariance calls
 * then work on the slot as usual */
KH_API int kh_matcher_add_map(kh_matcher * m, int32_t slot, const kh_scan * query, const kh_map_view * map);
/* kh_matcher_match_batch with the rasterisation swapped: n <= max_batch independent MatchScans against ONE map (empty queries,
 * response expansion, fine pass and per-match status as there); kh_matcher_match_map is the batch of one */
KH_API int kh_matcher_match_map(kh_matcher * m, const kh_scan * query, const kh_map_view * map,
                                int32_t do_penalize, int32_t do_refine, double mean[3], double cov[9], double * response);
KH_API int kh_matcher_match_map_batch(kh_matcher * m, int32_t n, const kh_scan * queries, const kh_map_view * map,
                                      int32_t do_penalize, int32_t do_refine, double * means, double * covs,
                                      double * responses, int32_t * status);
/* a profiling aid, like kh_matcher_profile_side: while kh_matcher_profile is on, the GPU ms (device events) of the map-collect
 * kernels -- count + scan, and fill; the download of the counts and the host's wait between them are NOT included -- and the number
 * of map rasterisations, since the last call; reading resets them */
KH_API int kh_matcher_profile_map(kh_matcher * m, double * collect_ms, int64_t * collects);

/* ---------------------------------------------------------------- localizing in a map alone
 * Place one scan in a map without a pose guess, and carry a pose from scan to scan, with a kh_map_view as the only map: no scans,
 * no pose graph.  The lattice cell of a world point v is round_half_away((v - anchor) * scale) (the trace kernels' WorldToGrid); the
 * window holds lattice cells [ox, ox + width) x [oy, oy + height); columns width .. width_step - 1 are never read. */

/* ---- where a robot can stand: one seed per block of `pitch` x `pitch` lattice cells, pitch = max(1, round(seed_spacing * scale)) | 1
 * (odd: the coarse search steps by two cells, and seeds an even number of cells apart would all miss the same lattice phase).  Block
 * (bx, by) covers lattice cells [bx pitch, (bx + 1) pitch) x [by pitch, (by + 1) pitch), floor quotients of the lattice index: a block
 * stays where it is when a live window grows.  Its seed is its FREE cell (state 255) inside the window nearest to the block's centre,
 * (2 i - (2 bx pitch + pitch - 1))^2 + (2 j - (2 by pitch + pitch - 1))^2 smallest, ties to the smaller j, then the smaller i; a block
 * without a free cell has none.  Seeds come in ascending (by, bx).  The world point of a seed is anchor + (lattice index) / scale.  With
 * center_xy and radius > 0 only the seeds with (dx * dx) + (dy * dy) < radius * radius + KT_TOLERANCE are kept.
 * cells takes 2 int32 per seed (lattice i, j), xy 2 doubles per seed, each for the first `cap` seeds (either may be NULL); *n_seeds
 * is the total, also beyond cap.  KH_ERR_INVALID_ARG: a malformed view, NULL n_seeds, cap < 0, a spacing that is not finite or <= 0
 * or gives a pitch above 4096 cells, a non-finite radius or centre. */
KH_API int kh_map_seeds(const kh_map_view * view, double seed_spacing, const double * center_xy, double radius,
                        int32_t * cells, double * xy, int32_t cap, int32_t * n_seeds);

/* ---- how well a scan at a pose agrees with the map: the ray-consistency counters of kh_merge_fit (above) for ONE scan's readings
 * at n_poses sensor poses.  The beams of pose k are the ranges, kh_scan_points at that pose, and its (x, y); they pass AddScan's gate
 * with the laser's range_threshold / minimum_range / maximum_range and are walked by TraceLine on the view's lattice; every visit is
 * counted by the state of the cell it lands on, visits outside the window are dropped, a hit end cell is visited twice.  The map is
 * only read.  KH_ERR_INVALID_ARG: a malformed view or laser, NULL ranges / sensor_poses / out, n_poses < 1, a non-finite pose, and any
 * pose or range_threshold * scale that could make one beam walk more than 2^20 cells or leave the int32 lattice (a sensor cell beyond
 * +-2^30). */
KH_API int kh_map_fit(const kh_map_view * view, const kh_laser * laser, const double * ranges, int32_t n_poses,
                      const double * sensor_poses /* 3n */, kh_merge_fit_t * out /* n */);

/* ---- the localizer: a loop-preset and a sequential-preset matcher built from the same fields of kh_mapper_params as kh_mapper's,
 * and a map view.  max_batch = hypotheses per kh_matcher_match_map_batch call. */
typedef struct kh_map_localizer kh_map_localizer;
KH_API int kh_map_localizer_create(const kh_mapper_params * params, const kh_laser * laser, int32_t device, int32_t max_batch,
                                   kh_map_localizer ** out);
KH_API void kh_map_localizer_destroy(kh_map_localizer * loc);
/* copies the view STRUCT; the cells stay borrowed under kh_map_view's validity rule (set the map again after its source was updated).
 * A malformed view or one on another device is KH_ERR_INVALID_ARG and the localizer keeps the map it had. */
KH_API int kh_map_localizer_set_map(kh_map_localizer * loc, const kh_map_view * view);

/* Global relocalization in the map: section 7d's scheme with kh_map_seeds in the place of the seed vertices and the map in the place
 * of the base scans.  Hypothesis k * n_headings + h puts the robot at seed k with heading -pi + h * (2 pi / n_headings) (the sensor
 * through the laser's offset, the readings with kh_scan_points): coarse match against the map on the loop matcher (no penalty, no
 * refinement), the gate (response > minimum_response_coarse, cov(0,0) and cov(1,1) < maximum_variance_coarse), fine match of the
 * readings re-posed at the coarse mean on the sequential matcher (no penalty, refined), accepted when the fine response >=
 * minimum_response_fine.  The accepted ones are ordered by fine response (descending), coarse response (descending), index; each is
 * fitted (kh_map_fit) at its fine mean; those with known > 0 and score < min_fit_score are dropped; then, in that order, one is
 * dropped as a duplicate when a kept one lies within merge_distance and merge_heading of it on the fine means
 * ((dx * dx) + (dy * dy) < merge_distance^2 and |NormalizeAngle(dh)| < merge_heading; merge_distance <= 0: no suppression). */
typedef struct kh_map_relocalize_params {
  double seed_spacing;      /* > 0 (default: loop_search_space_dimension / 4: a block's diagonal stays inside the half window) */
  int32_t n_headings;       /* headings per seed; 0 = ceil(2 pi / (2 * coarse_search_angle_offset)) */
  int32_t top_k;            /* most hypotheses returned; 0 = as many as `cap` holds (default 8) */
  double center_xy[2];      /* with radius > 0: only the seeds within radius of this point */
  double radius;            /* <= 0: the whole map (default) */
  double minimum_response_coarse, maximum_variance_coarse, minimum_response_fine;   /* defaults: loop_match_* of the mapper parameters, as stored */
  double min_fit_score;     /* default 0: drops nothing */
  double merge_distance;    /* default loop_search_space_resolution */
  double merge_heading;     /* default coarse_angle_resolution */
} kh_map_relocalize_params;
typedef struct kh_map_hyp {
  int32_t index;            /* seed ordinal * n_headings + heading ordinal */
  int32_t seed_cell[2];     /* lattice cell of the seed */
  int32_t pad;
  double heading;
  double coarse_mean[3], coarse_cov[9], coarse_response;      /* sensor pose of the coarse match */
  double fine_mean[3], fine_cov[9], fine_response;            /* sensor pose of the fine match */
  double robot_pose[3];     /* GetCorrectedAt(fine_mean): what goes to kh_map_localizer_set_pose */
  kh_merge_fit_t fit;       /* of the scan at fine_mean */
} kh_map_hyp;
typedef struct kh_map_relocalize_summary {
  int32_t n_seeds, n_headings, n_hypotheses, n_passed /* the coarse gate */, n_accepted, n_rejected_fit, n_duplicates, n_returned;
  double seed_kernel_ms, fit_kernel_ms;      /* device time of k_map_seeds and k_map_fit */
  double coarse_ms, fine_ms, total_ms;       /* wall: the coarse batches, the fine batches, the call */
} kh_map_relocalize_summary;
/* defaults for parameters *mapper_params (NULL: kh_mapper_params_default's) */
KH_API void kh_map_relocalize_params_default(const kh_mapper_params * mapper_params, kh_map_relocalize_params * p);
/* out takes the first min(top_k, cap) kept hypotheses (top_k 0: cap), the summary the totals.  NULL ranges / params / summary, out
 * NULL with cap > 0, cap < 0, seed_spacing not finite or <= 0, n_headings < 0 or > 4096, top_k < 0, a non-finite centre or radius or
 * a NaN among the other parameters are KH_ERR_INVALID_ARG before a device is looked for; without a device KH_ERR_NO_DEVICE; then a
 * NULL localizer KH_ERR_INVALID_ARG, no map set KH_ERR_NOT_FOUND, a seed pitch above 4096 cells KH_ERR_INVALID_ARG.  A map without a
 * free cell (or a region without a seed) is KH_OK with zero everything.  The map's cells and the tracked pose are left as they were. */
KH_API int kh_map_localizer_relocalize(kh_map_localizer * loc, const double * ranges, const kh_map_relocalize_params * params,
                                       kh_map_hyp * out, int32_t cap, kh_map_relocalize_summary * summary);

/* ---- tracking: the robot pose the localizer holds and the odometric pose it belongs to */
KH_API int kh_map_localizer_set_pose(kh_map_localizer * loc, const double robot_pose[3], const double odometric_pose[3]);
KH_API int kh_map_localizer_get_pose(const kh_map_localizer * loc, double robot_pose[3], double odometric_pose[3]);   /* KH_ERR_NOT_FOUND before a pose was set */
typedef struct kh_map_track_t {
  double predicted_pose[3]; /* robot: Transform(last odometric, last corrected).TransformPose(odometric), Mapper::Process' prediction */
  double robot_pose[3];     /* GetCorrectedAt(sensor_pose): the pose the localizer holds from now on */
  double sensor_pose[3];    /* MatchScan against the map on the sequential matcher, penalised and refined, from GetSensorAt(predicted) */
  double covariance[9];
  double response;
  kh_merge_fit_t fit;       /* of the scan at sensor_pose */
} kh_map_track_t;
/* One tracking step.  The match is always adopted, as Mapper::Process adopts its own: response and fit are the caller's health
 * signal.  NULL arguments or a non-finite odometric pose are KH_ERR_INVALID_ARG before a device is looked for; then
 * KH_ERR_NO_DEVICE; no map or no pose set KH_ERR_NOT_FOUND.  A failure leaves the held pose as it was. */
KH_API int kh_map_localizer_process(kh_map_localizer * loc, const double * ranges, const double odometric_pose[3], kh_map_track_t * out);
typedef struct kh_map_localizer_stats_t {
  int64_t relocalizations, hypotheses, steps, poses_fitted;
  double relocalize_ms, process_ms, match_ms /* of the steps */, seed_kernel_ms, fit_kernel_ms;
} kh_map_localizer_stats_t;
KH_API int kh_map_localizer_stats(const kh_map_localizer * loc, kh_map_localizer_stats_t * out);

/* ---------------------------------------------------------------- where scans contradict a map, and the patched map
 * A change layer on a map view: two uint32 grids `pass` and `hits` on the view's window, zero at creation.  The lattice is section
 * 7k's.  Observing a scan at a sensor pose walks every beam that passes AddScan's gate with TraceLine, adds 1 to `pass` of every
 * visited cell inside the window and, at a hit end cell inside it, 1 more to `pass` and 1 to `hits` -- what kh_occupancy_add_scans
 * counts.  The map's cells are only read. */
typedef struct kh_map_changes kh_map_changes;
/* what a beam says about the map, with a tolerance of t cells around its end cell: `blocked` = the visited window cells of its line
 * (the hit's second visit of the end cell apart) of map state 100 further than t from the end cell (Chebyshev); `near` = a window cell
 * of map state 100 within t of the end cell */
enum {
  KH_BEAM_DROPPED = 0,      /* the gate dropped the beam */
  KH_BEAM_EXPLAINED = 1,    /* hit, blocked == 0, near */
  KH_BEAM_NOVEL = 2,        /* hit, blocked == 0, not near, the end cell is free */
  KH_BEAM_UNKNOWN = 3,      /* hit, blocked == 0, not near, the end cell is unknown or outside the window */
  KH_BEAM_THROUGH = 4,      /* blocked > 0, hit or not */
  KH_BEAM_CLEAR = 5         /* not a hit, blocked == 0 */
};
/* what the observed state of a cell -- UpdateCell's rule on the layer: pass > min_pass_through ? (hits / pass > occupancy_threshold ?
 * 100 : 255) : 0 -- makes of the map's state (a map state that is none of 0 / 100 / 255 counts as unknown) */
enum {
  KH_CELL_UNOBSERVED = 0,           /* observed state 0 */
  KH_CELL_CONFIRMED = 1,            /* observed state = map state */
  KH_CELL_APPEARED = 2,             /* map 255 -> observed 100 */
  KH_CELL_VANISHED = 3,             /* map 100 -> observed 255 */
  KH_CELL_DISCOVERED_OCCUPIED = 4,  /* map 0 -> observed 100 */
  KH_CELL_DISCOVERED_FREE = 5       /* map 0 -> observed 255 */
};
/* copies the view STRUCT; the cells stay borrowed under kh_map_view's validity rule.  The window is fixed.  Allocates the layer, the
 * codes and the patched cells on the view's device.  A NULL or malformed view or a NULL out: KH_ERR_INVALID_ARG before a device is
 * looked for; then KH_ERR_NO_DEVICE. */
KH_API int kh_map_changes_create(const kh_map_view * view, kh_map_changes ** out);
KH_API void kh_map_changes_destroy(kh_map_changes * c);
/* zeroes the layer and its counters of scans and beams; the last diff's codes and patched cells stay */
KH_API int kh_map_changes_clear(kh_map_changes * c);
/* pass >>= shift, hits >>= shift on every cell, 1 <= shift <= 31: the only forgetting */
KH_API int kh_map_changes_decay(kh_map_changes * c, int32_t shift);
/* Observes n_scans scans of the laser's n_beams beams: scan k has ranges[k * n_beams ..] and the sensor pose sensor_poses[3 k ..]
 * (its points: kh_scan_points).  labels, where not NULL, takes 2 int32 per beam, scan-major: the KH_BEAM_ class and `blocked`, against
 * the MAP's cell states (not the layer), with end_tolerance cells of tolerance.  KH_ERR_INVALID_ARG, with nothing changed: everything
 * kh_map_fit refuses, n_scans < 1, end_tolerance outside 0 .. 4, and a call after which a cell could hold more than 2^32 - 1 (the
 * layer keeps a bound: + 2 * n_beams per scan, shifted by a decay, 0 after a clear).  Arguments that need no handle are checked before
 * a device is looked for; then KH_ERR_NO_DEVICE; then the handle and what depends on its view. */
KH_API int kh_map_changes_observe(kh_map_changes * c, const kh_laser * laser, int32_t n_scans, const double * ranges /* n_scans * n_beams */,
                                  const double * sensor_poses /* 3 n_scans */, int32_t end_tolerance, int32_t * labels /* 2 per beam, or NULL */);
typedef struct kh_map_changes_summary_t {
  int64_t n_unobserved, n_confirmed, n_appeared, n_vanished, n_discovered_occupied, n_discovered_free;   /* window cells by KH_CELL_ code */
  int64_t n_changed;        /* cells of code >= 2: the length of the whole list */
  int64_t n_listed;         /* min(n_changed, cap): the entries written */
  int64_t scans_observed, beams_observed;      /* since the last clear */
  double observe_kernel_ms; /* k_map_observe since the last clear, by events */
  double diff_kernel_ms, list_kernel_ms, download_ms;      /* this call, by events: k_map_diff; count, prefix and fill; the copies to the host */
} kh_map_changes_summary_t;
/* Sets the layer against the map: the code and the patched state (the observed state where it is known, else the map's) of every
 * window cell, the counts, and the cells of code >= 2 in row-major window order -- cells takes (lattice i, lattice j, code) for the
 * first `cap` of them, out->n_changed is the total.  NULL out, cap < 0, cells NULL with cap > 0 or a NaN threshold:
 * KH_ERR_INVALID_ARG before a device is looked for. */
KH_API int kh_map_changes_diff(kh_map_changes * c, uint32_t min_pass_through, double occupancy_threshold, int32_t * cells /* 3 per entry */,
                               int32_t cap, kh_map_changes_summary_t * out);
/* the layer, and the codes and patched cells of the last diff (zeros before one), row stride width_step; any pointer may be NULL */
KH_API int kh_map_changes_read(kh_map_changes * c, uint32_t * pass, uint32_t * hits, uint8_t * codes, uint8_t * patched);
/* the patched cells of the last diff as a view on the source view's lattice, for kh_map_localizer_set_map and the matcher's map entry
 * points: borrowed until the next diff or destroy.  KH_ERR_NOT_FOUND before a diff. */
KH_API int kh_map_changes_view(kh_map_changes * c, kh_map_view * out);
/* the patched cells of the last diff as width * height nav values, kh_occupancy_read_nav's mapping.  KH_ERR_NOT_FOUND before a diff. */
KH_API int kh_map_changes_read_nav(kh_map_changes * c, int8_t * out);

/* ---------------------------------------------------------------- the scan a map would produce; placing one map in another
 * Ray casting on the lattice of section 7k.  Beam b of sensor pose k runs from the lattice cell c0 of the sensor's (x, y) to the
 * lattice cell c1 of its far point: what kh_scan_points gives at that pose for a reading of range_threshold.  Its cells are exactly
 * the cells TraceLine(c0, c1) visits, ordered outward by s = |long-axis coordinate - c0's|, s = 0 .. L.  A window cell of state 100 is
 * occupied, of state 255 free; every other state, and a cell outside the window, is unknown.  In ascending s: an occupied cell ends
 * the beam (HIT); an unknown cell counts, and ends the beam (UNKNOWN) when max_unknown >= 0 and more than max_unknown were counted;
 * the end of the line is FREE, reported with c1 and s = L.  The sensor's own cell is treated like any other. */
enum {
  KH_RAY_FREE = 0,          /* the line ended: nothing within range_threshold */
  KH_RAY_HIT = 1,           /* an occupied cell */
  KH_RAY_UNKNOWN = 2        /* the budget of unknown cells ran out */
};
typedef struct kh_ray_t {
  double range;             /* HIT: from the sensor to the hit cell's centre anchor + cell / scale, sqrt((dx * dx) + (dy * dy)); else no_return */
  int32_t cell[2];          /* lattice cell the beam ended on */
  int32_t steps;            /* its s */
  int32_t code;             /* KH_RAY_ */
} kh_ray_t;
/* out takes n_poses * laser->n_beams answers, pose-major; *kernel_ms (may be NULL) the kernel's time by events.  no_return is any
 * double, NaN included; a reading the caller's laser drops (> range_threshold and, to be dropped by AddScan's gate, >= maximum_range)
 * keeps a cast scan from painting walls where the map ended.  The map is only read.  KH_ERR_INVALID_ARG before a device is looked
 * for: everything kh_map_fit refuses of a view, a laser and poses, NULL sensor_poses / out, n_poses < 1, max_unknown < -1. */
KH_API int kh_map_raycast(const kh_map_view * view, const kh_laser * laser, int32_t n_poses, const double * sensor_poses /* 3n */,
                          int32_t max_unknown, double no_return, kh_ray_t * out /* n_poses * n_beams */, double * kernel_ms);

/* ---- placing the map `moving` in the localizer's map, with no scan of either.  Seeds of the moving map (kh_map_seeds at
 * probe_spacing) are robot poses of heading 0; the scans the moving map would produce there are cast in ONE kh_map_raycast launch
 * (max_unknown; no_return = the next double above range_threshold where that is below maximum_range, else NaN).  The n_probes seeds
 * with the most HIT beams are the probes (ties to the lower seed index; a seed without a HIT is none).  Each probe's cast ranges are
 * relocalized in the localizer's map; a hypothesis implies the correction C = P . inverse(Q), P the hypothesis' robot pose, Q the
 * probe's, `.` and inverse as kh_merge_move_submap composes.  Candidate 0 is `initial`, then the probes in pick order, each one's
 * hypotheses in rank order; nothing is de-duplicated.  Every candidate is fitted with every probe -- kh_map_fit of the probe's cast
 * ranges at the sensor pose C . S, S the probe's sensor pose, against the localizer's map -- the six counters summed over the probes
 * and derived as kh_merge_fit_t; the ranking is kh_merge_align's: known >= min_known first, then score descending, agree
 * descending, candidate index ascending. */
typedef struct kh_map_align_params {
  double probe_spacing;        /* > 0 (default: the localizer's default seed_spacing) */
  int32_t n_probes;            /* >= 1 (default 3) */
  int32_t top_k;               /* hypotheses kept per probe, >= 1 (default 4) */
  int32_t max_unknown;         /* the cast's budget, >= -1 (default 20) */
  int32_t pad;
  uint64_t min_known;          /* candidates with fewer known visits rank last (default 0) */
  double initial[3];           /* candidate 0 (default 0, 0, 0) */
  kh_map_relocalize_params relocalize;   /* as for kh_map_localizer_relocalize; its top_k is overridden by top_k above */
} kh_map_align_params;
typedef struct kh_map_align_cand {
  double correction[3];        /* moving map -> the localizer's map */
  int32_t probe_seed;          /* seed index in the moving map; -1 for candidate 0 */
  int32_t hypothesis;          /* rank of the hypothesis in the probe's relocalization; -1 for candidate 0 */
  double fine_response;        /* 0 for candidate 0 */
  int32_t index, enough;       /* candidate index before ranking; known >= min_known */
  kh_merge_fit_t fit;
} kh_map_align_cand;
/* defaults; the relocalization parameters are those of the localizer's mapper parameters (loc NULL: of kh_mapper_params_default) */
KH_API void kh_map_align_params_default(const kh_map_localizer * loc, kh_map_align_params * p);
/* out takes the first min(cap, n) ranked candidates, *n_candidates takes n.  times_ms (may be NULL): [0] seeds and cast, [1] the
 * relocalizations, [2] the fits, [3] the whole call.  The localizer (its map, its tracked pose) and both maps are left as they were.
 * KH_ERR_INVALID_ARG before a device is looked for: NULL params / n_candidates, out NULL with cap > 0, cap < 0, a malformed moving
 * view, probe_spacing not finite or <= 0, n_probes < 1, top_k < 1, max_unknown < -1, a non-finite initial, invalid relocalization
 * parameters.  Then: no device KH_ERR_NO_DEVICE, a NULL localizer KH_ERR_INVALID_ARG, no map set KH_ERR_NOT_FOUND, a moving view on
 * another device than the localizer or a probe pitch above 4096 cells KH_ERR_INVALID_ARG.  A moving map without a probe is KH_OK
 * with candidate 0 alone. */
KH_API int kh_map_align(kh_map_localizer * loc, const kh_map_view * moving, const kh_map_align_params * params,
                        kh_map_align_cand * out, int32_t cap, int32_t * n_candidates, double times_ms[4]);

/* ---------------------------------------------------------------- two finished maps merged into one
 * The map `moving` is warped through a rigid correction onto the lattice of the map `target` and the two are composed cell by cell;
 * the result is a kh_map_view on the target's own lattice (the same anchor, the same stored scale) that the localizer, the matcher's
 * map entry points, the change layer, the ray cast and another merge take as it is.  `correction` carries moving-map coordinates
 * into the target's frame: what kh_map_align_cand.correction holds.
 *   warp     output cell (I, J) lies at w = anchor_t + (double)I / scale_t.  With footprint n it has n x n sample points (wx + d_a,
 *            wy + d_b), d_k = ((2 k + 1 - n) / (2.0 n)) / scale_t (exactly 0 for n = 1).  Each goes through inverse(correction) -- (c * x -
 *            s * y) + tx, (s * x + c * y) + ty, c and s the host's cos and sin of its yaw -- and is rounded to a cell of the moving
 *            lattice (section 7k); a cell outside the moving window or beyond the int32 lattice reads unknown.  M = 100 if any
 *            sample read 100, else 255 if any read 255, else unknown.  The default footprint min(4, max(1, ceil(scale_m / scale_t)))
 *            is 1 unless the moving map is finer than the target: a footprint above the resolution ratio thickens walls.
 *   compose  T = the target's state at (I, J): 100, 255, else (any other state, no such cell) unknown.  The code of the cell and
 *            the merged state are KH_MERGED_'s below; a conflict is settled by the KH_MERGE_CONFLICT_ policy.
 *   window   grow 0: the target's window.  grow 1: its union with the box of the moving map's cells of state != 0 -- the corner
 *            points of their inclusive lattice box, pushed outward by half a moving cell, carried by the correction, rounded to
 *            target-lattice cells, min / max over the four, one cell of padding on every side.  A moving map with no such cell adds
 *            nothing.  Row stride (width + 7) & ~7, the padding columns 0.
 * Neither input is written. */
enum {
  KH_MERGED_NEITHER = 0,           /* both unknown: 0 */
  KH_MERGED_TARGET_ONLY = 1,       /* M unknown: T */
  KH_MERGED_MOVING_ONLY = 2,       /* T unknown: M */
  KH_MERGED_AGREE = 3,             /* equal and known: T */
  KH_MERGED_MOVING_OCCUPIED = 4,   /* T free, M occupied: by policy */
  KH_MERGED_MOVING_FREE = 5        /* T occupied, M free: by policy */
};
enum {
  KH_MERGE_CONFLICT_TARGET = 0,    /* the target's state */
  KH_MERGE_CONFLICT_MOVING = 1,    /* the moving map's state */
  KH_MERGE_CONFLICT_OCCUPIED = 2,  /* 100 (the default: a planner must not lose a wall) */
  KH_MERGE_CONFLICT_UNKNOWN = 3    /* 0 */
};
typedef struct kh_map_merge kh_map_merge;
typedef struct kh_map_merge_params {
  double correction[3];        /* moving map -> target map; finite */
  int32_t footprint;           /* 1 .. 4, or 0 = the default */
  int32_t conflict;            /* KH_MERGE_CONFLICT_ (default KH_MERGE_CONFLICT_OCCUPIED) */
  int32_t grow;                /* 0 / 1 (default 1) */
  int32_t pad;
} kh_map_merge_params;
typedef struct kh_map_merge_stats {
  int32_t ox, oy, width, height, width_step, footprint;   /* the output window and the footprint used */
  int32_t known_box[4];        /* i0, j0, i1, j1 of the moving map's cells of state != 0, lattice indices; i1 < i0: none */
  uint64_t target_only, moving_only, agree_free, agree_occupied, conflict_moving_occupied, conflict_moving_free;   /* output cells */
  uint64_t overlap;            /* the sum of the last four */
  double agreement;            /* (agree_free + agree_occupied) / overlap; 0 without overlap */
  double times_ms[3];          /* the known box and the merge kernel by events, the whole call */
} kh_map_merge_stats;
/* correction 0, footprint 0, KH_MERGE_CONFLICT_OCCUPIED, grow 1; a NULL output is ignored */
KH_API void kh_map_merge_params_default(kh_map_merge_params * p);
/* Merges and keeps the result on the device of the views.  KH_ERR_INVALID_ARG before a device is looked for: a NULL target, moving,
 * params or out, a malformed view, a non-finite correction, a footprint outside 0 .. 4, a conflict outside 0 .. 3, a grow outside
 * 0 .. 1.  Then: no device KH_ERR_NO_DEVICE; views on two different devices KH_ERR_INVALID_ARG; a carried corner of the moving map's
 * box more than 2^30 cells from the target's anchor, an output side above 32768 cells or an output above 2^28 cells
 * KH_ERR_INVALID_ARG.  A warp alone is a merge into an all-unknown target of the wanted lattice; a third map is merged with the
 * first merge's view as its target. */
KH_API int kh_map_merge_create(const kh_map_view * target, const kh_map_view * moving, const kh_map_merge_params * params, kh_map_merge ** out);
KH_API void kh_map_merge_destroy(kh_map_merge * m);
KH_API int kh_map_merge_stats_get(kh_map_merge * m, kh_map_merge_stats * out);
/* the merged cells as a view on the target's lattice: owned by the handle, valid until kh_map_merge_destroy */
KH_API int kh_map_merge_view(kh_map_merge * m, kh_map_view * out);
/* the merged cells and the KH_MERGED_ codes, width_step * height bytes each; either may be NULL */
KH_API int kh_map_merge_read(kh_map_merge * m, uint8_t * cells, uint8_t * codes);
/* the merged cells as width * height nav values, kh_occupancy_read_nav's mapping, no row padding */
KH_API int kh_map_merge_read_nav(kh_map_merge * m, int8_t * out);

/* ---------------------------------------------------------------- the distance field of a map
 * How far every cell of a map lies from the nearest obstacle, and three readers of that: costmap values, clearance at world points,
 * a dense endpoint score of a scan at many poses with the pose refinement built on it.  Every quantity a kernel produces is an
 * INTEGER -- squared distances in cells, counts, sums of squared distances -- and every square root, division by scale and exp is
 * taken on the host from those integers.
 *   field    a SNAPSHOT of the view's window [ox, ox + width) x [oy, oy + height): the handle copies the cells, the view may go or
 *            change once kh_map_field_create returns.  Cells outside the window do not exist (an obstacle there is not seen);
 *            columns width .. width_step - 1 are never read.  An obstacle is a cell of state 100 (KH_FIELD_OBSTACLE_OCCUPIED) or of
 *            any state other than 255 (KH_FIELD_OBSTACLE_NOT_FREE).  R = ceil(max_distance * scale) cells; max_distance 0 gives
 *            R = 0: uncapped.  For window cell (i, j): d2 = min over obstacle cells (a, b) of (i - a)^2 + (j - b)^2; the stored value
 *            is d2 when R == 0 or d2 <= R * R, else KH_FIELD_FAR; without any obstacle every value is KH_FIELD_FAR.  With sides of at
 *            most 32768 cells d2 < 2^31: KH_FIELD_FAR is no value.  In metres: sqrt((double)d2) / scale, +inf for KH_FIELD_FAR. */
#define KH_FIELD_FAR 0xFFFFFFFFu
enum {
  KH_FIELD_OBSTACLE_OCCUPIED = 0,  /* state 100 (the default) */
  KH_FIELD_OBSTACLE_NOT_FREE = 1   /* every state other than 255: unknown space is an obstacle too */
};
typedef struct kh_map_field kh_map_field;
typedef struct kh_map_field_params {
  double max_distance;         /* metres, finite, >= 0; 0 = uncapped (default 2.0) */
  int32_t obstacles;           /* KH_FIELD_OBSTACLE_ (default KH_FIELD_OBSTACLE_OCCUPIED) */
  int32_t pad;
} kh_map_field_params;
typedef struct kh_map_field_stats {
  int32_t ox, oy, width, height;   /* the window */
  int32_t radius_cells;        /* R */
  uint32_t max_d2;             /* the largest value that is not KH_FIELD_FAR; 0 when there is none */
  uint64_t n_obstacles, n_far; /* cells of value 0, cells of value KH_FIELD_FAR */
  double times_ms[3];          /* the column and the row kernel by events, the whole call */
} kh_map_field_stats;
/* max_distance 2.0, KH_FIELD_OBSTACLE_OCCUPIED; a NULL output is ignored */
KH_API void kh_map_field_params_default(kh_map_field_params * p);
/* KH_ERR_INVALID_ARG before a device is looked for: a NULL view, params or out, a malformed view, a max_distance that is not finite
 * or < 0, R > 1024, obstacles outside 0 .. 1, a side above 32768 cells or more than 2^28 cells, R == 0 with a side above 4096 cells
 * (the uncapped row pass costs width x (largest distance) per row: a bound the arguments alone give).  Then KH_ERR_NO_DEVICE. */
KH_API int kh_map_field_create(const kh_map_view * view, const kh_map_field_params * params, kh_map_field ** out);
KH_API void kh_map_field_destroy(kh_map_field * f);
KH_API int kh_map_field_stats_get(kh_map_field * f, kh_map_field_stats * out);
/* the values and the distances in metres, width * height each, row-major with no row padding; either may be NULL */
KH_API int kh_map_field_read(kh_map_field * f, uint32_t * d2, double * metres);

/* ---- costmap values: the field through an inflation curve.  Rt = ceil(inflation_radius * scale); the table has n = Rt * Rt + 1
 * entries indexed by d2; with m = sqrt((double)d2) / scale: d2 == 0 -> 254; m <= inscribed_radius -> 253; m <= inflation_radius ->
 * (uint8_t)(252.0 * exp(-cost_scaling_factor * (m - inscribed_radius))), truncated toward zero; else 0.  (nav2's
 * InflationLayer::computeCost restated from its published source; nothing here is pinned to nav2.)  A cell: c = table[d2] when
 * d2 <= Rt * Rt, else 0; a cell of state 100 or 255 gets c; any other state (unknown) gets c with track_unknown == 0, and with
 * track_unknown == 1 it gets 255 -- unless c >= 253, or inflate_unknown is set and c > 0: then c. */
typedef struct kh_inflation_params {
  double inscribed_radius, inflation_radius, cost_scaling_factor;   /* metres, metres, 1 / metres: finite, >= 0, inscribed <= inflation */
  int32_t track_unknown, inflate_unknown;                           /* 0 / 1 */
} kh_inflation_params;
/* 0.22, 0.55, 10.0, 1, 0; a NULL output is ignored */
KH_API void kh_inflation_params_default(kh_inflation_params * p);
/* the table on the host, no device: *n = Rt * Rt + 1 (also when cap is too small), table takes the entries when cap >= *n (table may
 * be NULL with cap 0).  KH_ERR_INVALID_ARG: NULL params or n, parameters as above, a scale that is not finite or <= 0, Rt > 1024,
 * cap < 0, a table that cap says is there and is NULL, cap > 0 and < *n. */
KH_API int kh_inflation_table(const kh_inflation_params * p, double scale, uint8_t * table, int32_t cap, int32_t * n);
/* out takes width * height costs, no row padding.  KH_ERR_INVALID_ARG before a device is looked for: NULL params or out, the
 * parameters as above but Rt; then KH_ERR_NO_DEVICE, the handle, Rt > 1024 at the field's scale, and a field with 0 < R < Rt (it
 * does not reach as far as the costs ask). */
KH_API int kh_map_field_costs(kh_map_field * f, const kh_inflation_params * p, uint8_t * out);

/* ---- clearance at n world points (x, y): the lattice cell of a point is section 7k's round_half_away((v - anchor) * scale); a cell
 * outside the window, or a coordinate beyond +-2^30 cells, is KH_CLEAR_OUTSIDE and +inf; a KH_FIELD_FAR value KH_CLEAR_FAR and +inf;
 * anything else KH_CLEAR_OK and sqrt((double)d2) / scale.  Any output may be NULL.  n < 1, NULL xy, a non-finite point:
 * KH_ERR_INVALID_ARG before a device is looked for. */
enum { KH_CLEAR_OK = 0, KH_CLEAR_FAR = 1, KH_CLEAR_OUTSIDE = 2 };
KH_API int kh_map_field_clearance(kh_map_field * f, int32_t n, const double * xy /* 2n */, double * metres, int32_t * status, uint32_t * d2);

/* ---- the endpoint score of ONE scan's readings at n_poses sensor poses.  The beams of pose k are kh_map_fit's: kh_scan_points at
 * that pose through AddScan's gate; only beams with a valid end (r < range_threshold - 1e-6) are scored, at the reading itself: no
 * line is walked.  T = truncate_cells, or the field's R when it is 0; T2 = T * T.  n_kept: beams that pass the gate; n_hit: those with
 * a valid end; n_inside: hit beams whose end cell lies in the window; n_near: those of them with a value <= T2; sum_d2: the sum of
 * their values; cost = sum_d2 + (n_hit - n_near) * T2 -- the sum of min(d2, T2), a missing cell counted as T2; score = 1 - cost /
 * (n_hit * T2) in doubles, 0 without a hit beam.  KH_ERR_INVALID_ARG before a device is looked for: NULL laser / ranges / sensor_poses
 * / out, n_poses < 1, n_beams < 1, truncate_cells < 0 or > 1024.  Then KH_ERR_NO_DEVICE, the handle, and on the handle's lattice
 * what kh_map_fit refuses of a laser and of poses; truncate_cells and R both 0. */
typedef struct kh_field_score {
  int32_t n_kept, n_hit, n_inside, n_near;
  uint64_t sum_d2, cost;
  double score;
} kh_field_score;
KH_API int kh_map_field_score(kh_map_field * f, const kh_laser * laser, const double * ranges, int32_t n_poses,
                              const double * sensor_poses /* 3n */, int32_t truncate_cells, kh_field_score * out /* n */);

/* ---- pose refinement: a compass search on the integer cost, all n starts in lockstep.  Every start is scored once where it
 * stands (cost_start, n_hit); then, per round, one launch scores the 27 candidates of every start that still runs.  Candidate
 * c = 0 .. 26 of a start at (x, y, h) with steps (s, s, a) is (x + (c % 3 - 1) * s, y + (c / 3 % 3 - 1) * s, h + (c / 9 - 1) * a), in
 * exactly these double operations; the heading is not normalised.  The start moves to the candidate of least cost -- on a tie the
 * centre (c = 13) if it is among the least, else the smallest c.  n_hit is the same for all candidates of a start (the gate reads
 * only the range), so comparing cost alone compares the scores.  When the centre wins: with halvings == n_halvings the start is
 * KH_REFINE_CONVERGED, else both steps are multiplied by 0.5 and halvings goes up by one.  A start that has run max_rounds rounds
 * stops there with KH_REFINE_MAX_ROUNDS; a start one of whose candidates kh_map_field_score would refuse stops where it is, before
 * that round, with KH_REFINE_LEFT_LATTICE. */
typedef struct kh_field_refine_params {
  double step_xy, step_heading;    /* metres > 0, radians >= 0: finite */
  int32_t n_halvings, max_rounds;  /* 0 .. 32, 1 .. 4096 */
  int32_t truncate_cells, pad;     /* as kh_map_field_score's */
} kh_field_refine_params;
/* 2 / scale, 0.02 rad, 4, 64, 0; a NULL output is ignored */
KH_API void kh_field_refine_params_default(kh_field_refine_params * p, double scale);
typedef struct kh_field_refined {
  double pose[3];
  uint64_t cost_start, cost;   /* at the start, at `pose` */
  int32_t n_hit, rounds, halvings, status;
} kh_field_refined;
enum { KH_REFINE_CONVERGED = 0, KH_REFINE_MAX_ROUNDS = 1, KH_REFINE_LEFT_LATTICE = 2 };
/* times_ms (may be NULL): the kernels by events summed, the whole call.  KH_ERR_INVALID_ARG before a device is looked for: what
 * kh_map_field_score refuses there (the starts are its poses), NULL params, steps and counts outside the ranges above; after the
 * handle what kh_map_field_score refuses there. */
KH_API int kh_map_field_refine(kh_map_field * f, const kh_laser * laser, const double * ranges, int32_t n, const double * sensor_poses /* 3n */,
                               const kh_field_refine_params * params, kh_field_refined * out /* n */, double times_ms[2]);

/* ---------------------------------------------------------------- a field that follows its map
 * kh_map_field_update brings an existing field up to date with a view of the same lattice by the part of the map that changed, exact
 * to the bit: afterwards every value, every reader and the statistics are what kh_map_field_create on the same view gives.  A field
 * that has been updated keeps its column distances resident.  For a capped field (R > 0) a value can change only within R cells
 * (Chebyshev) of a cell whose OBSTACLE-NESS changed: the call compares the view with the field's copy of the cells over `rect`,
 * finds the box of those cells, and recomputes that box grown by R.  An uncapped field (R == 0) is always recomputed whole.
 *   cells_box    the bounding box of the cells whose state changed at all (costs depend on the state)
 *   values_box   the bounding box of the cells whose obstacle-ness changed, grown by R and clipped to the window: every value that
 *                changed lies inside; after a rebuild both boxes are the whole window
 * Boxes and rectangles are x, y, w, h in lattice cells (the units of ox, oy); all zero = none. */
typedef struct kh_field_update {
  int32_t cells_box[4], values_box[4];
  int32_t rebuilt, relayout;              /* the whole window was recomputed / the window differs from the previous one */
  int64_t cells_compared, cells_recomputed;  /* cells of `rect` compared with the copy (0 for a rebuild); the area of values_box */
  double times_ms[4];                     /* compare, columns, rows by device events (0 where none ran); the call by wall time */
} kh_field_update;
/* The caller promises that cells outside `rect` (NULL: the whole window) equal the field's copy; rect is clipped to the window, an
 * empty clip (w or h <= 0 among them) does nothing and is KH_OK.  `out` may be NULL.  KH_ERR_INVALID_ARG before a device is looked
 * for: a NULL or malformed view; with a handle, a view off the field's lattice -- anchor x, anchor y, scale (each compared by its
 * bits), device, in this order -- or a new window beyond kh_map_field_create's limits.  Then KH_ERR_NO_DEVICE and the handle.  A view
 * whose window (ox, oy, width, height) differs reallocates and rebuilds (relayout = rebuilt = 1); so does the first update of a
 * field made by kh_map_field_create (rebuilt = 1: it allocates the column distances), every update of an uncapped field, and the
 * update after one that failed with KH_ERR_HIP (the field stays usable; what it holds until then is undefined inside `rect` grown
 * by R). */
KH_API int kh_map_field_update(kh_map_field * f, const kh_map_view * view, const int32_t rect[4], kh_field_update * out);
/* debugging: the height in rows of the bands the column pass of an update is cut into; 0 = the library's choice (max(R, 8)).  The
 * result does not depend on it.  rows < 0: KH_ERR_INVALID_ARG. */
KH_API int kh_map_field_set_band_rows(kh_map_field * f, int32_t rows);
/* the values / the costs of lattice cells [x, x + w) x [y, y + h), dense and row-major.  KH_ERR_INVALID_ARG before a device is
 * looked for: a NULL output, w or h < 1, and for the costs what kh_map_field_costs refuses there; after the handle: a rectangle that
 * does not lie inside the window, and what kh_map_field_costs refuses there. */
KH_API int kh_map_field_read_rect(kh_map_field * f, int32_t x, int32_t y, int32_t w, int32_t h, uint32_t * d2);
KH_API int kh_map_field_costs_rect(kh_map_field * f, const kh_inflation_params * p, int32_t x, int32_t y, int32_t w, int32_t h, uint8_t * out);
/* A field of the live map's current window that follows it: kh_live_map_update adds the cells it handed to the cell-state kernel to
 * the field's pending region (as it does for a kh_map_feed), kh_live_map_field_sync is kh_map_field_update with the live map's
 * current view and that region, and clears it; with nothing pending it launches nothing and reports no box.  The field borrows the
 * live map: kh_map_field_destroy detaches it; a live map destroyed first leaves the field readable and its sync KH_ERR_INVALID_ARG,
 * as is the sync of a field that is not attached.  kh_live_map_field_create: KH_ERR_NOT_FOUND before the live map has a window. */
KH_API int kh_live_map_field_create(kh_live_map * g, const kh_map_field_params * params, kh_map_field ** out);
KH_API int kh_live_map_field_sync(kh_map_field * f, kh_field_update * out);

/* ---------------------------------------------------------------- map regions: connected free space by clearance, frontier clusters
 * (DESIGN.md section 7q).  An analysis is made from a kh_map_field: it reads the field's own snapshot of the cell states and its
 * d2 values over the field's window.  Cells outside the window do not exist; columns width .. width_step - 1 are never read and
 * never connect anything.  The handle never borrows the field: the field may change or go once a call returns.
 *   N            the 4 or the 8 neighbours of a cell (connectivity), for everything below
 *   Rc           ceil(min_clearance * scale) cells, the field's own rule for R
 *   traversable  a cell of state 255 with d2 >= Rc * Rc (KH_FIELD_FAR counts as beyond)
 *   unknown      a cell of state neither 100 nor 255 (what kh_map_field_costs calls unknown)
 *   frontier     a cell of state 255 with at least one unknown cell of N inside the window: on states alone, not on clearance
 *   regions      the connected components of the traversable mask under N; frontier clusters: those of the frontier mask
 *   label        the root of a component: the window index j * width + i of its smallest cell
 *   kept         a component of at least min_region_cells (min_frontier_cells) cells that stands among the first max_regions
 *                (max_frontiers) such components in root order.  Kept components are numbered 0, 1, ... in root order.
 *   id grid      per cell the kept id, KH_REGION_NONE outside the mask, KH_REGION_DROPPED for a cell of a component that was too
 *                small or past the cap
 * Every quantity a kernel produces is an integer that does not depend on the order in which anything ran. */
#define KH_REGION_NONE 0xFFFFFFFFu
#define KH_REGION_DROPPED 0xFFFFFFFEu
enum { KH_REGIONS = 0, KH_FRONTIERS = 1 };   /* `which`: the two sets */
typedef struct kh_map_regions kh_map_regions;
typedef struct kh_map_regions_params {
  double min_clearance;                          /* metres, finite, >= 0 (default 0: every free cell) */
  int32_t connectivity;                          /* 4 or 8 (default 8) */
  int32_t min_region_cells, max_regions;         /* >= 1 (default 1), 1 .. 2^20 (default 4096) */
  int32_t min_frontier_cells, max_frontiers;     /* >= 1 (default 1), 1 .. 2^20 (default 4096) */
  int32_t pad;
} kh_map_regions_params;
/* One component of either set.  The doubles are taken on the host, in exactly these operations:
 *   centroid[k]  = anchor[k] + ((double)o_k + (double)sum_k / (double)n_cells) / scale      (o_k: ox, oy; sum_k: sum_i, sum_j)
 *   anchor_xy[k] = anchor[k] + (double)(o_k + a_k) / scale, (a_0, a_1) = (anchor_cell % width, anchor_cell / width): the world
 *                  point of the anchor cell by the view's rule */
typedef struct kh_region {
  uint32_t root, n_cells;
  int32_t box[4];              /* x, y, w, h in lattice cells (the units of ox, oy) */
  uint64_t sum_i, sum_j;       /* window-relative sums of the members' columns and rows */
  uint32_t max_d2;             /* the largest field value over the members; KH_FIELD_FAR if any member is FAR */
  uint32_t n_other;            /* members that are set in the OTHER mask: a region's frontier cells (0: nothing is left to explore
                                  from it), a cluster's traversable cells */
  uint32_t link;               /* the smallest kept id of the other set among the members -- for a cluster the region it can be
                                  reached from -- KH_REGION_NONE when there is none */
  uint32_t anchor_cell;        /* the member nearest the centroid cell ((2 sum_i + n) / (2 n), (2 sum_j + n) / (2 n)), integer
                                  divisions, by squared cell distance; ties go to the smallest window index */
  double centroid[2], anchor_xy[2];
} kh_region;
typedef struct kh_map_regions_stats {
  int32_t ox, oy, width, height;               /* the window */
  int32_t clearance_cells, connectivity;       /* Rc, 4 or 8 */
  uint64_t n_traversable, n_frontier_cells;
  uint32_t n_total[2], n_kept[2];              /* by KH_REGIONS / KH_FRONTIERS: all components, the kept ones */
  int32_t truncated[2];                        /* more components passed the minimum than the maximum takes */
  double times_ms[7];          /* by device events: tiles, seams, flatten and count, compaction and ids, records, anchors; the call */
} kh_map_regions_stats;
/* 0.0, 8, 1, 4096, 1, 4096; a NULL output is ignored */
KH_API void kh_map_regions_params_default(kh_map_regions_params * p);
/* KH_ERR_INVALID_ARG before a device is looked for, in this order: a NULL field, params or out; a min_clearance that is not finite
 * or < 0; Rc > 1024; a connectivity other than 4 or 8; a minimum < 1; a maximum outside 1 .. 2^20.  Then KH_ERR_NO_DEVICE; then a
 * field with 0 < R < Rc (it does not reach as far as the threshold asks: kh_map_field_costs' refusal). */
KH_API int kh_map_regions_create(kh_map_field * field, const kh_map_regions_params * params, kh_map_regions ** out);
/* the whole analysis again, of `field` as it stands (after kh_map_field_update or kh_live_map_field_sync, or of another field of the
 * same lattice): the allocations are reused, or made anew where the window changed.  KH_ERR_INVALID_ARG before a device is looked
 * for: a NULL field; with a handle, a field on another device or lattice (anchor x, anchor y, scale by their bits, device).  After
 * the handle: a field with 0 < R < Rc.  After a failure the handle holds no analysis until a recompute succeeds. */
KH_API int kh_map_regions_recompute(kh_map_regions * r, kh_map_field * field);
KH_API void kh_map_regions_destroy(kh_map_regions * r);
KH_API int kh_map_regions_stats_get(kh_map_regions * r, kh_map_regions_stats * out);
/* the id grid of set `which`: width * height values, row-major with no row padding.  NULL ids, which outside 0 .. 1:
 * KH_ERR_INVALID_ARG before a device is looked for. */
KH_API int kh_map_regions_read(kh_map_regions * r, int32_t which, uint32_t * ids);
/* the records of the kept components of set `which` in id order: *n = n_kept (also when cap is smaller), records takes the first
 * min(cap, n_kept).  KH_ERR_INVALID_ARG before a device is looked for: which outside 0 .. 1, NULL n, cap < 0, cap > 0 with NULL
 * records. */
KH_API int kh_map_regions_get(kh_map_regions * r, int32_t which, kh_region * records, int32_t cap, int32_t * n);
/* the region at n world points (x, y), by kh_map_field_clearance's cell rule: KH_REGION_OUTSIDE off the window or beyond +-2^30
 * cells (id KH_REGION_NONE), KH_REGION_AT_NONE where the cell is not traversable (KH_REGION_NONE), KH_REGION_AT_DROPPED where its
 * region was dropped (KH_REGION_DROPPED), KH_REGION_AT_OK with the id.  Two points can reach each other iff both are
 * KH_REGION_AT_OK with the same id.  Either output may be NULL.  n < 1, NULL xy, a non-finite point: KH_ERR_INVALID_ARG before a
 * device is looked for. */
enum { KH_REGION_AT_OK = 0, KH_REGION_AT_NONE = 1, KH_REGION_AT_DROPPED = 2, KH_REGION_OUTSIDE = 3 };
KH_API int kh_map_regions_lookup(kh_map_regions * r, int32_t n, const double * xy /* 2n */, int32_t * status, uint32_t * id);

/* ---------------------------------------------------------------- travel costs on a map: cost-to-go field from goals, paths, lookups
 * (DESIGN.md section 7r).  A travel analysis is made from a kh_map_field, as a region analysis is: it reads the field's snapshot of
 * the cell states and its d2 values over the field's window and never borrows the field.  Cells outside the window do not exist;
 * columns width .. width_step - 1 are never read.
 *   Rc, Rt       ceil(min_clearance * scale), ceil(inflation.inflation_radius * scale) cells, the field's rule for R
 *   traversable  a cell of state 255 with d2 >= Rc * Rc (KH_FIELD_FAR counts as beyond): section 7q's mask
 *   weight       q(v) = neutral_cost + ((cost_weight * c(v)) >> 4) for a traversable cell, c(v) what kh_map_field_costs gives a cell of
 *                state 255 (table[d2] for d2 <= Rt * Rt, else 0); q = 0 for every other cell.  With cost_weight == 0 the table is not
 *                needed and Rt is not checked against the field.
 *   steps        directions n = 0 .. 7: (+1,0), (0,+1), (-1,0), (0,-1), (+1,+1), (-1,+1), (-1,-1), (+1,-1); connectivity 4 has 0 .. 3
 *                only.  L(n) = 5 for n < 4, else 7.  A step u -> v is allowed when v is a traversable window cell; a diagonal step
 *                (di, dj) from (i, j) only when cut_corners is set or both (i + di, j) and (i, j + dj) are traversable.  Allowedness
 *                is symmetric.  The step costs L(n) * q(u): a cell is paid for when it is left.
 *   values       V = 0 at every goal cell; elsewhere V(u) = min over allowed steps u -> v of V(v) + L * q(u); KH_TRAVEL_FAR where no
 *                goal is reached and at every cell that is not traversable.  Shortest-path costs over positive integer weights are
 *                unique: no execution order shows in them.
 *   goal         the lattice cell of a goal point is kh_map_field_clearance's; the goal cell is the traversable window cell within
 *                Chebyshev distance goal_snap_cells of it with the smallest key dist2 << 32 | window index (dist2: the squared cell
 *                distance to the point's cell).  KH_TRAVEL_GOAL_BLOCKED: no such cell; KH_TRAVEL_GOAL_OUTSIDE: the point's own cell
 *                is off the window or beyond +-2^30 cells.  A solve without a usable goal is KH_OK with every value KH_TRAVEL_FAR.
 *   lookup       among the window cells within Chebyshev distance snap_cells of the point's cell whose value is not KH_TRAVEL_FAR,
 *                the one with the smallest key V << 32 | window index: KH_TRAVEL_AT_OK with its value and lattice cell;
 *                KH_TRAVEL_AT_UNREACHED where there is none, KH_TRAVEL_AT_OUTSIDE by the goal's rule: value KH_TRAVEL_FAR, cell (0, 0)
 *   path         the start cell is the lookup's; emit it; while V(cur) != 0 go to the allowed neighbour v of the smallest direction
 *                index with V(v) + L * q(cur) == V(cur).  V strictly decreases, so the walk ends.  KH_TRAVEL_PATH_TRUNCATED: max_cells
 *                cells were emitted and the last is no goal cell. */
#define KH_TRAVEL_FAR 0xFFFFFFFFu
enum { KH_TRAVEL_GOAL_OK = 0, KH_TRAVEL_GOAL_BLOCKED = 1, KH_TRAVEL_GOAL_OUTSIDE = 2 };
enum { KH_TRAVEL_AT_OK = 0, KH_TRAVEL_AT_UNREACHED = 1, KH_TRAVEL_AT_OUTSIDE = 2 };
enum { KH_TRAVEL_PATH_OK = 0, KH_TRAVEL_PATH_TRUNCATED = 1, KH_TRAVEL_PATH_UNREACHED = 2, KH_TRAVEL_PATH_OUTSIDE = 3 };
typedef struct kh_map_travel kh_map_travel;
typedef struct kh_map_travel_params {
  double min_clearance;                          /* metres, finite, >= 0 (default 0: every free cell) */
  kh_inflation_params inflation;                 /* c(v)'s curve (default kh_inflation_params_default); the unknown policy is not read */
  int32_t connectivity, cut_corners;             /* 4 or 8 (default 8); 0 / 1 (default 0) */
  int32_t neutral_cost, cost_weight;             /* 1 .. 255 (default 50); 0 .. 255 in sixteenths (default 13) */
  int32_t goal_snap_cells, pad;                  /* 0 .. 16 (default 0) */
} kh_map_travel_params;
typedef struct kh_map_travel_stats {
  int32_t ox, oy, width, height;                 /* the window */
  int32_t clearance_cells, inflation_cells;      /* Rc, Rt */
  int32_t connectivity, pad;
  uint64_t n_traversable, n_reached;             /* cells of weight > 0; cells of a value other than KH_TRAVEL_FAR (0 before a solve) */
  uint32_t max_value;                            /* the largest value that is not KH_TRAVEL_FAR; 0 when there is none */
  uint32_t rounds, launches;                     /* of the last solve: launches in which a tile ran; launches of k_travel_relax */
  uint32_t pad2;
  uint64_t tile_runs;                            /* tiles relaxed over all rounds (depends on what a tile saw of its neighbours in flight) */
  double times_ms[4];          /* by device events: the weights, the goals, the relaxation (summed); the last call by wall time */
} kh_map_travel_stats;
typedef struct kh_travel_path {
  int32_t status, n_cells;     /* KH_TRAVEL_PATH_; cells emitted */
  uint32_t cost, start_cell;   /* the value at the first cell; its window index (both KH_TRAVEL_FAR without a start cell) */
} kh_travel_path;
/* 0.0, kh_inflation_params_default, 8, 0, 50, 13, 0; a NULL output is ignored */
KH_API void kh_map_travel_params_default(kh_map_travel_params * p);
/* Snapshots the weights (uint16 per cell, dense) and the traversable count.  KH_ERR_INVALID_ARG before a device is looked for, in
 * this order: a NULL field, params or out; a connectivity other than 4 or 8; cut_corners outside 0 .. 1; neutral_cost outside
 * 1 .. 255; cost_weight outside 0 .. 255; goal_snap_cells outside 0 .. 16; a min_clearance that is not finite or < 0; Rc > 1024; what
 * kh_inflation_table refuses of the inflation parameters at the field's scale.  Then KH_ERR_NO_DEVICE; then, in this order: a field
 * with 0 < R < Rc; with cost_weight > 0 a field with 0 < R < Rt; a window with width * height * Lmax * q_max > 0xFFFFFFFE, Lmax = 7
 * under connectivity 8, else 5, q_max = neutral_cost + ((cost_weight * 253) >> 4): a bound the arguments alone give. */
KH_API int kh_map_travel_create(kh_map_field * field, const kh_map_travel_params * params, kh_map_travel ** out);
/* the snapshot again, of `field` as it stands (after kh_map_field_update or kh_live_map_field_sync, or of another field of the same
 * lattice); the solution is dropped.  Refusals and the reuse of allocations are kh_map_regions_recompute's, then the three above. */
KH_API int kh_map_travel_recompute(kh_map_travel * t, kh_map_field * field);
KH_API void kh_map_travel_destroy(kh_map_travel * t);
/* n_goals 1 .. 4096 world points (x, y); goal_status (may be NULL) takes a KH_TRAVEL_GOAL_ code each.  n_goals out of range, NULL
 * goals_xy, a non-finite point: KH_ERR_INVALID_ARG before a device is looked for.  A watchdog that ended the relaxation:
 * KH_ERR_HIP, and the handle holds no solution. */
KH_API int kh_map_travel_solve(kh_map_travel * t, int32_t n_goals, const double * goals_xy /* 2n */, int32_t * goal_status);
KH_API int kh_map_travel_stats_get(kh_map_travel * t, kh_map_travel_stats * out);
/* the values (uint32) and the weights (uint16), width * height each, row-major with no padding; either may be NULL.  This and the
 * two readers below: KH_ERR_NOT_FOUND before the first successful solve and after a recompute. */
KH_API int kh_map_travel_read(kh_map_travel * t, uint32_t * values, uint16_t * weights);
/* any output may be NULL.  n < 1, NULL xy, a non-finite point, snap_cells outside 0 .. 16: KH_ERR_INVALID_ARG before a device is
 * looked for. */
KH_API int kh_map_travel_lookup(kh_map_travel * t, int32_t n, const double * xy /* 2n */, int32_t snap_cells, int32_t * status, uint32_t * value,
                                int32_t * cell /* 2n: lattice x, y */);
/* heads takes n records; cells (may be NULL) 2 * n * max_cells int32 -- lattice x, y of cell s of path k at 2 * (k * max_cells + s) --
 * zeros past a path's n_cells.  KH_ERR_INVALID_ARG before a device is looked for: what kh_map_travel_lookup refuses, NULL heads,
 * max_cells outside 1 .. 65536, n * max_cells > 2^24.  A walk that finds no neighbour to go to (it cannot happen in a solved field)
 * ends there, and the call returns KH_ERR_HIP. */
KH_API int kh_map_travel_paths(kh_map_travel * t, int32_t n, const double * starts_xy /* 2n */, int32_t snap_cells, int32_t max_cells,
                               kh_travel_path * heads /* n */, int32_t * cells);
/* debugging: the launches of k_travel_relax between two reads of the "anything flagged" word; 0 = the library's choice, at most 64.
 * The result does not depend on it.  k < 0 or > 64: KH_ERR_INVALID_ARG. */
KH_API int kh_map_travel_set_rounds_per_check(kh_map_travel * t, int32_t k);

/* ---------------------------------------------------------------- visibility on a map: the cells a pose would see, gain, greedy views
 * (DESIGN.md section 7s).  The rays are kh_map_raycast's, with the same max_unknown; what is kept is every cell they visit.
 *   beam cells   beam b of sensor pose p walks TraceLine(c0, c1) outward as kh_map_raycast does and leaves at step s_end (kh_ray_t.steps):
 *                its visited cells are those of s = 0 .. s_end, the leaving cell included -- the HIT cell, the unknown cell that
 *                exceeded the budget, or c1 on FREE
 *   Seen(p)      the WINDOW cells among the visited cells of all beams of p, each once.  A cell outside the window is never counted;
 *                a window cell of state 100 is occupied, of state 255 free, of any other state unknown.  The sensor's own cell is
 *                treated like any other
 *   covered      the handle's mask over the view's window, one bit per cell: cleared by create and _clear, _commit(poses) ORs Seen(p)
 *                of every given pose into it
 *   record       seen_*: the cells of Seen(p) by state; new_*: the same over Seen(p) minus the covered mask as it stands at the call;
 *                gain = w_unknown * new_unknown + w_free * new_free + w_occupied * new_occupied; beams_*: the beams by KH_RAY_ code
 *   reach        floor(range_threshold * scale) + 2 cells bounds the Chebyshev distance from c0 to any c1 (both cells are rounded);
 *                a laser of reach > 511 is refused: the per-pose bitmap of side 2 * reach + 1 <= 1023 fits one workgroup's LDS, and
 *                gain <= 1023^2 * 765 stays below 2^32
 *   select       rounds r = 0 .. k - 1: among the candidates not yet picked, the largest gain against the mask as it stands, ties to
 *                the smallest index; below min_gain the selection ends with r picks; else (index, gain) is recorded and the pose
 *                committed.  The mask is not cleared first and is left holding the picks.
 * Every result is an integer no execution order shows in. */
typedef struct kh_map_visibility kh_map_visibility;
typedef struct kh_visibility_params {
  int32_t max_unknown;                           /* kh_map_raycast's budget, -1: none (default 20) */
  int32_t w_unknown, w_free, w_occupied;         /* 0 .. 255 each, not all zero (default 1, 0, 0) */
} kh_visibility_params;
typedef struct kh_visibility_t {
  uint32_t seen_free, seen_occupied, seen_unknown;
  uint32_t new_free, new_occupied, new_unknown;
  uint32_t gain;
  uint32_t beams_free, beams_hit, beams_unknown;
} kh_visibility_t;
typedef struct kh_map_visibility_stats {
  int32_t ox, oy, width, height;                 /* the window */
  int32_t reach, bitmap_bytes;                   /* cells; the bytes of one pose's bitmap in LDS */
  int32_t n_poses, pad;                          /* of the last gain, commit or select */
  uint32_t rounds, launches;                     /* of the last call: a select's rounds that picked (else 0); its kernel launches */
  double kernel_ms, call_ms;                     /* the last call's kernels by device events, the call by wall time */
} kh_map_visibility_stats;
/* 20, 1, 0, 0; a NULL output is ignored */
KH_API void kh_map_visibility_params_default(kh_visibility_params * p);
/* The handle copies the view struct; the cells stay borrowed under kh_map_view's validity rule.  KH_ERR_INVALID_ARG before a device
 * is looked for, in this order: a NULL view, laser, params or out; what kh_map_raycast refuses of a view; laser->n_beams < 1 and what
 * kh_map_raycast refuses of a laser; max_unknown < -1; a weight outside 0 .. 255, or all three zero; reach > 511. */
KH_API int kh_map_visibility_create(const kh_map_view * view, const kh_laser * laser, const kh_visibility_params * params,
                                    kh_map_visibility ** out);
KH_API void kh_map_visibility_destroy(kh_map_visibility * v);
/* another view of the same window (ox, oy, width, height), lattice (anchor, scale) and device: a map that changed in place or a
 * patched copy.  Anything else, and what kh_map_raycast refuses of a view: KH_ERR_INVALID_ARG.  The mask is kept. */
KH_API int kh_map_visibility_set_map(kh_map_visibility * v, const kh_map_view * view);
KH_API int kh_map_visibility_clear(kh_map_visibility * v);
/* The calls below take n sensor poses (x, y, heading).  KH_ERR_INVALID_ARG before a device is looked for, in this order: NULL
 * sensor_poses or a NULL required output; n outside 1 .. 65536; a pose kh_map_raycast refuses; (select) k outside 1 .. min(n, 4096);
 * (select) min_gain < 1; n * n_beams above 2^24 (the far points of a call are one table). */
KH_API int kh_map_visibility_commit(kh_map_visibility * v, int32_t n, const double * sensor_poses /* 3n */);
/* out takes n records; *kernel_ms (may be NULL) the kernel's time by events.  The mask is read, not written. */
KH_API int kh_map_visibility_gain(kh_map_visibility * v, int32_t n, const double * sensor_poses /* 3n */, kh_visibility_t * out /* n */,
                                  double * kernel_ms);
/* picks and pick_gains take k entries each, the first *n_picked of them set and the rest 0.  The rounds run on the device with no
 * host read between them. */
KH_API int kh_map_visibility_select(kh_map_visibility * v, int32_t n, const double * sensor_poses /* 3n */, int32_t k, uint32_t min_gain,
                                    int32_t * picks /* k */, uint32_t * pick_gains /* k */, int32_t * n_picked);
/* the covered mask as width * height bytes of 0 / 1, row-major with no padding */
KH_API int kh_map_visibility_read_mask(kh_map_visibility * v, uint8_t * out);
KH_API int kh_map_visibility_stats_get(kh_map_visibility * v, kh_map_visibility_stats * out);
/* debugging and measuring: 1 (the default) reads a bitmap word before the OR and leaves the OR out where the bit is set, 0 always ORs.
 * The result does not depend on it.  Any other value: KH_ERR_INVALID_ARG. */
KH_API int kh_map_visibility_set_skip(kh_map_visibility * v, int32_t skip);

/* ---------------------------------------------------------------- footprints on a map: an oriented convex polygon checked at poses and
 * by heading.  A footprint analysis is made from a kh_map_field, as a travel analysis is: it snapshots the
 * field's copy of the cell states and its d2 values over the field's window and never borrows the field.  A cell of state 100 is
 * occupied, of state 255 free, of any other state unknown.  Cells outside the window do not exist; columns width .. width_step - 1
 * are never read.
 *   footprint    3 .. 16 vertices (vx, vy) in metres in the robot frame, finite and strictly convex in either winding: the cross
 *                products of consecutive edges all have one sign, none is 0, and the polygon goes round once.  r_max = max_k
 *                sqrt(vx^2 + vy^2); reach = ceil(r_max * scale) + 1 cells, at most 255
 *   vertex cells of pose (x, y, theta), on the host: c = cos(theta), s = sin(theta); wx_k = x + (c vx_k - s vy_k), wy_k = y + (s vx_k +
 *                c vy_k); V_k = (round_half_away((wx_k - anchor_x) * scale), round_half_away((wy_k - anchor_y) * scale)),
 *                kh_map_field_clearance's cell of a point.  A coordinate of a vertex cell or of the pose's own cell beyond +-2^30
 *                cells: KH_FOOTPRINT_LATTICE, the record all zeros but the status and min_d2 = KH_FIELD_FAR.  Every V_k lies within
 *                Chebyshev distance reach of the pose's own cell
 *   covered      edge k is the cells of the outward TraceLine walk (kh_map_raycast's) from V_k to V_(k + 1) mod n, in the order the
 *                vertices were given; the outline is the union of the edges; for every row j from the smallest to the largest V_k.y,
 *                lo_j and hi_j are the smallest and the largest column of an outline cell of that row; Covered(p) = {(i, j): lo_j <= i
 *                <= hi_j}.  The outline is a closed 8-connected loop: no row of that range is empty
 *   record       the counts over Covered(p) by state, n_outside the covered cells off the window, n_cells their sum; min_d2 the
 *                smallest field value under the covered window cells, KH_FIELD_FAR without one; status the largest code that applies
 *   layer        theta_h = (2.0 * pi * h) / H; O_hk = (round_half_away((c vx_k - s vy_k) * scale), round_half_away((s vx_k + c vy_k) *
 *                scale)); for window cell (i, j) the vertex cells are (i, j) + O_hk, covered cells and status as above; bit h of the
 *                cell's mask is set when that status is <= max_status.  Defined through the offsets: it is not promised to equal a
 *                pose check at the cell's centre (a sum of roundings is not the rounding of a sum).  reach > 64 is refused: the
 *                kernel's tile plus a halo of reach cells lies in LDS
 * Every result is a set, a count, a minimum or an OR of integers: no execution order shows in it. */
enum { KH_FOOTPRINT_FREE = 0, KH_FOOTPRINT_UNKNOWN = 1, KH_FOOTPRINT_OUTSIDE = 2, KH_FOOTPRINT_COLLISION = 3, KH_FOOTPRINT_LATTICE = 4 };
#define KH_FOOTPRINT_LAYER_REACH 64
typedef struct kh_map_footprint kh_map_footprint;
typedef struct kh_footprint_t {
  int32_t status;              /* KH_FOOTPRINT_: FREE, or the largest of UNKNOWN (n_unknown > 0), OUTSIDE (n_outside > 0), COLLISION
                                * (n_occupied > 0), LATTICE */
  uint32_t n_cells, n_free, n_occupied, n_unknown, n_outside;
  uint32_t min_d2, pad;
} kh_footprint_t;
typedef struct kh_footprint_layer_t {
  uint64_t n_fit[32];          /* cells whose bit h is set; 0 from n_headings on */
  uint64_t n_any, n_all;       /* cells with a bit set; cells with all n_headings bits set */
} kh_footprint_layer_t;
typedef struct kh_map_footprint_stats {
  int32_t ox, oy, width, height;                 /* the window */
  int32_t n_vertices, reach;
  int32_t layer_rows, pad;                       /* the rows of the last layer's stencils, all headings together (0 before one) */
  double times_ms[3];          /* the last pose kernel and the last layer kernel by device events; the last call by wall time */
} kh_map_footprint_stats;
/* vertices_xy holds 2 * n_vertices doubles.  KH_ERR_INVALID_ARG before a device is looked for, in this order: a NULL argument;
 * n_vertices outside 3 .. 16; a vertex that is not finite; a polygon that is not strictly convex; reach > 255 at the field's scale.
 * Then KH_ERR_NO_DEVICE; then a field without a window. */
KH_API int kh_map_footprint_create(kh_map_field * field, int32_t n_vertices, const double * vertices_xy, kh_map_footprint ** out);
/* the snapshot again, of `field` as it stands; refusals and the reuse of allocations are kh_map_travel_recompute's */
KH_API int kh_map_footprint_recompute(kh_map_footprint * fp, kh_map_field * field);
KH_API void kh_map_footprint_destroy(kh_map_footprint * fp);
KH_API int kh_map_footprint_stats_get(kh_map_footprint * fp, kh_map_footprint_stats * out);
/* n poses (x, y, theta) -> n records.  KH_ERR_INVALID_ARG before a device is looked for, in this order: n outside 1 .. 65536; NULL
 * poses or out; a pose that is not finite.  A vertex cell beyond the reach (it cannot happen) is KH_ERR_HIP. */
KH_API int kh_map_footprint_check(kh_map_footprint * fp, int32_t n, const double * poses /* 3n */, kh_footprint_t * out /* n */);
/* masks (may be NULL) takes width * height words, row-major with no padding; summary may be NULL.  KH_ERR_INVALID_ARG before a
 * device is looked for, in this order: n_headings outside 1 .. 32; max_status outside 0 .. 2; reach > KH_FOOTPRINT_LAYER_REACH. */
KH_API int kh_map_footprint_layer(kh_map_footprint * fp, int32_t n_headings, int32_t max_status, uint32_t * masks, kh_footprint_layer_t * summary);

#ifdef __cplusplus
}
#endif
#endif  /* KARTO_HIP_H_ */
