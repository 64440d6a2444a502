/*
 * o3dslam_reg.h -- C ABI of the MI355X-native scan-to-map registration path.
 *
 * Drop-in boundary for the ONE hot path of leggedrobotics/open3d_slam_private:
 *   B2  PointMatcher<float>::ICP::initReference / compute
 *         libpointmatcher/pointmatcher/PointMatcher.h:1036-1042, ICP.cpp:813-898,902-1349
 *         called from open3d_slam/src/Mapper.cpp:343,372-373
 *   B1  o3d_slam::CloudRegistration::registerClouds (GICP operator)
 *         open3d_slam/include/open3d_slam/CloudRegistration.hpp:19-73, src/CloudRegistration.cpp:16-21
 * (paths relative to the reference tree).  Plain pointers and sizes only; no C++,
 * torch or Eigen types cross this boundary; no exception crosses it -- every throw
 * site of the reference maps to a reg_status code.
 *
 * LAYOUT CONTRACT
 *  - points:  `xyz` + `xyz_stride` (in floats).  stride 4 == libpointmatcher's
 *    DataPoints::features (Eigen column-major (dim+1) x N float => {x,y,z,1} per point,
 *    PointMatcher.h:176,375); stride 3 == packed xyz.  The 4th component is ignored
 *    (assumed 1).
 *  - normals: `nrm` + `nrm_stride` (3 == the `normals` descriptor rows, packed).
 *  - covariances (GICP): 6 floats per point, (xx, xy, xz, yy, yz, zz).
 *  - 4x4 transforms are COLUMN-major float[16] (T[c*4+r]) == Eigen::Matrix4f::data()
 *    of PointMatcher<float>::TransformationParameters; reading -> reference.
 *  - `on_device` != 0: the pointers are HIP device pointers on the handle's device
 *    (no PCIe copy); == 0: host pointers (copied with hipMemcpyAsync).
 *
 * THREADING: one handle == one non-re-entrant registration context (like the single
 * `icp_` member of o3d_slam::Mapper, Mapper.hpp:72, serialised by mapManipulationMutex_).
 * Independent handles may be used concurrently, each on its own HIP stream.
 */
#ifndef O3DSLAM_REG_H
#define O3DSLAM_REG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REG_API __attribute__((visibility("default")))

typedef struct reg_handle reg_handle;

/* Status codes; each names the reference behaviour it replaces. */
typedef enum {
    REG_OK = 0,
    REG_EMPTY_TARGET = 1,        /* initReference() returns false            ICP.cpp:850-855 */
    REG_EMPTY_SOURCE = 2,        /* runtime_error "reading point cloud is empty" ICP.cpp:958-960 */
    REG_NO_CORRESPONDENCES = 3,  /* ConvergenceError  ErrorMinimizer.cpp:75-77, Matches.cpp:76-80 */
    REG_BAD_TRANSFORM = 4,       /* runtime_error / TransformationError      ICP.cpp:910-918 */
    REG_NOT_CONFIGURED = 5,      /* "You must setup a matcher ..."           ICP.cpp:819-824; no target/source set */
    REG_BAD_ARGUMENT = 6,        /* InvalidParameter                         Registrar.h:103-109 */
    REG_MISSING_FIELD = 7,       /* InvalidField: no `normals` descriptor    DataPoints.cpp:1112 */
    REG_DEVICE_ERROR = 8,        /* HIP runtime failure (no reference analogue); the product never falls back to CPU */
    REG_UNSUPPORTED = 9,
    REG_OUT_OF_BOUNDS = 10       /* ConvergenceError "limit out of bounds" of BoundTransformationChecker
                                    TransformationCheckersImpl.cpp:217-224; nothing in ICP::compute catches it */
} reg_status;

typedef enum {
    REG_COST_P2PL = 0, /* PointToPlaneErrorMinimizer   ICP.cpp:1512-1566 + ErrorMinimizers/PointToPlane.cpp:274-400 */
    REG_COST_GICP = 1, /* plane-to-plane GICP factor (north star; arithmetic not in the reference tree) */
    /* The two other operators of o3d_slam::cloudRegistrationFactory (open3d_slam/src/CloudRegistration.cpp:54-119; config
       strings PointToPlaneIcp / PointToPointIcp, parameter_structure_definitions.lua:77,112):
       REG_COST_O3D_P2PL  open3d::pipelines::registration::RegistrationICP with TransformationEstimationPointToPlane and
                          the L2 loss (RegistrationIcpPointToPlane): per pair r = (p - q).n, J = [p x n, n] with p the
                          transformed reading point, q / n the matched reference point / normal; the update solves
                          J^T J x = -J^T r (fp64) and is x -> Rz(x2) Ry(x1) Rx(x0), t = x3..5 (TransformVector6dToMatrix4d).
       REG_COST_O3D_P2P   RegistrationICP with TransformationEstimationPointToPoint(with_scaling = false)
                          (RegistrationIcpPointToPoint): the update is Umeyama's closed form without scaling,
                          S = cov(q, p) = U D V^T, R = U diag(1, 1, sign(det U det V)) V^T, t = mean(q) - R mean(p).
       Rules of both: the input frame (no centring, as GICP); the update is LEFT-multiplied, T <- U T, in fp64; the loop
       always stops by Open3D's ICPConvergenceCriteria exactly as gicp_stop_rule = 1 does (evaluate, update, evaluate
       again; the last evaluation is reported), with gicp_rel_fitness / gicp_rel_rmse -- gicp_stop_rule itself is
       ignored; fixed_iters > 0 runs that many updates as for GICP.  A pair is a match when d^2 <= max_dist^2.
       Inputs: O3D_P2PL needs reference normals (reg_set_target: REG_MISSING_FIELD without), O3D_P2P only xyz; neither
       reads reading normals or covariances.  The outlier-filter flags are ignored; use_xicp is REG_BAD_ARGUMENT.
       reg_result: error = sum r^2 (O3D_P2PL) / sum |T p - q|^2 (O3D_P2P); H_last / b_last = J^T J / J^T r (O3D_P2PL),
       zero (O3D_P2P); rank_last = rank of the 6x6 system (O3D_P2PL) / of the 3x3 cross-covariance (O3D_P2P).
       reg_linearize returns J^T J / J^T r for O3D_P2PL and REG_UNSUPPORTED for O3D_P2P (Umeyama has no normal
       equations); the distributed entry points (reg_dist_*, reg_match_local, reg_reduce_local, reg_solve_update, ...)
       return REG_UNSUPPORTED for both.  Open3D 0.15.1 is an un-vendored dependency: restated, PARITY UNPINNED. */
    REG_COST_O3D_P2PL = 2,
    REG_COST_O3D_P2P = 3
} reg_cost;

/* Configuration == the hot-path subset of param/icp.yaml (open3d_slam_ros/param/icp.yaml:11-27,86-92). */
typedef struct {
    int32_t struct_size;        /* = sizeof(reg_params); checked */
    int32_t cost;               /* reg_cost */
    /* matcher: KDTreeMatcher (MatchersImpl.h:80-88) */
    int32_t knn;                /* must be 1 */
    float   max_dist;           /* maxDist; INFINITY allowed (default of the reference) */
    float   epsilon;            /* accepted for config compatibility; the search is always exact (epsilon = 0) */
    /* outlierFilters (OutlierFiltersImpl.cpp); chain = product of 0/1 weights */
    int32_t use_trimmed;        /* TrimmedDistOutlierFilter */
    float   trim_ratio;
    int32_t use_surface_normal; /* SurfaceNormalOutlierFilter */
    float   max_normal_angle;   /* rad */
    int32_t use_max_dist_filter;/* MaxDistOutlierFilter */
    float   outlier_max_dist;
    /* transformationCheckers (TransformationCheckersImpl.cpp:57-158) */
    int32_t max_iter;           /* CounterTransformationChecker.maxIterationCount */
    float   min_diff_rot;       /* DifferentialTransformationChecker */
    float   min_diff_trans;
    int32_t smooth_len;         /* smoothLength, at most 15: reg_create returns REG_BAD_ARGUMENT above (the device
                                   checkers keep the last 16 poses); <= 0 turns the differential checker off */
    int32_t fixed_iters;        /* >0: run exactly this many iterations, checkers ignored (throughput runs) */
    /* GICP termination, rule 0 (Gauss-Newton, rotation-first tangent); rule 1: gicp_stop_rule below */
    float   gicp_rot_eps;       /* rad */
    float   gicp_trans_eps;     /* m */
    /* device-side search structure */
    float   cell_size;          /* voxel-bin edge in metres; 0 = choose from target density */
    int32_t device;             /* HIP device ordinal */
    int32_t sort_source;        /* 1: Morton-order the reading on upload (speed only; results in input order) */
    /* degeneracyAwareness: OptimizedEqualityConstraints (icp.yaml:50-55; ICP.cpp:629-672, 2187-2444;
       PointToPlane.cpp:459-505): on the FIRST iteration the eigen-directions of the rotation / translation blocks of A
       are tested for information content (sums of |alignment| over the matched pairs above two cosine thresholds);
       every iteration then solves with the update constrained to zero along the non-localizable directions.
       Point-to-plane only.  Inert when every direction is localizable. */
    int32_t use_xicp;
    float   xicp_enough;        /* enoughInformationThreshold (250 shipped): sum over alignment > cos(min angle) */
    float   xicp_insufficient;  /* insufficientInformationThreshold (180 shipped): sum over alignment > cos(strong angle) */
    float   xicp_min_angle_deg; /* point2NormalMinimalAlignmentAngleThreshold (80 shipped) */
    float   xicp_strong_angle_deg; /* point2NormalStrongAlignmentAngleThreshold (45 shipped) */
    /* GICP stop rule.  0: |d_rot| < gicp_rot_eps && |d_trans| < gicp_trans_eps after an update (small_gicp's
       TerminationCriteria), or max_iter updates.  1: open3d::pipelines::registration::ICPConvergenceCriteria as
       RegistrationIcpGeneralized uses it (open3d_slam/src/CloudRegistration.cpp:16-21,45-52: only max_iteration_ is
       configured, relative_fitness_ = relative_rmse_ = 1e-6 by default): after every update the correspondences are
       re-evaluated at the new pose and the loop stops when |fitness - previous fitness| < gicp_rel_fitness AND
       |inlier_rmse - previous inlier_rmse| < gicp_rel_rmse (fitness = matched / N, inlier_rmse = sqrt(sum d2 / matched)),
       else after max_iter updates (+ the final evaluation, whose fitness / rmse are reported).  Open3D 0.15.1 is an
       un-vendored dependency: restated from its published RegistrationICP loop, PARITY UNPINNED. */
    int32_t gicp_stop_rule;
    float   gicp_rel_fitness;   /* relative_fitness_ (1e-6) */
    float   gicp_rel_rmse;      /* relative_rmse_ (1e-6) */
    int32_t reserved;
} reg_params;

typedef struct {
    int32_t iterations;
    int32_t converged;          /* DifferentialTransformationChecker said stop */
    int32_t max_iter_reached;   /* CounterTransformationChecker threw MaxNumIterationsReached (ICP.cpp:1294-1298) */
    int32_t rank_last;          /* numerical rank of the last 6x6 system (6 = invertible) */
    int64_t n_inliers;          /* pairs with non-zero weight in the last iteration */
    int64_t n_matched;          /* pairs with a neighbour inside max_dist in the last iteration */
    double  error;              /* P2PL: sum w r^2;  GICP: sum 0.5 r^T M r;  O3D_*: see reg_cost  (last iteration) */
    double  fitness;            /* n_inliers / N   (open3d RegistrationResult::fitness_ analogue); N = points of the
                                   WHOLE reading.  reg_dist_finish: N is known after reg_dist_register or
                                   reg_dist_prepare; a handle prepared only through reg_prepare_centroid reports NaN */
    double  inlier_rmse;        /* sqrt(sum_inliers d^2 / n_inliers) */
    float   H_last[36];         /* last normal matrix, row-major (symmetric) */
    float   b_last[6];
    float   target_build_ms;    /* last reg_set_target: upload + voxel-bin build */
    float   loop_ms;            /* iteration loop of the last reg_register (device time, HIP events) */
    float   T_iter_last[16];    /* final T_iter (column-major): P2PL in the centred frames, GICP == T_out */
    int32_t n_band_stalls;      /* fused path: iterations whose trimmed-band prediction failed and were re-run on the generic path */
    int32_t n_constraints;      /* use_xicp: number of non-localizable directions (0 = plain solve) */
    float   prof_ms[4];         /* loop profiling (o3dslam_reg_debug.h: profile_loop): summed device time of [0] k_match, [1] k_iter_fused launches;
                                   [2] a chain with with_cov: device time of the covariance evaluation after the loop (not in loop_ms) */
    int32_t prof_launches[4];   /* ... and how many launches that was */
    /* use_xicp: [0..2] rotation eigen-directions (descending eigenvalue), [3..5] translation; 1 = localizable
       (LocalizabilityCategory, PointMatcher.h:603-607); all 1 when the analysis is off */
    int32_t localizable[6];
    double  xicp_combined[6];   /* the two information sums per direction (ICP.cpp:2128-2155) */
    double  xicp_high[6];
    float   source_prep_ms;     /* last reg_set_source: upload + Morton order of the reading (device time, HIP events) */
    int32_t rotation_corrected; /* 1: |1 - det R| > 1e-3 in the pre-transform -> points moved with the re-orthogonalised copy
                                   (RigidTransformation::correctParameters, TransformationsImpl.cpp:73-76,105-166) */
    float   T_iter_prev[16];    /* the T_iter the LAST iteration ran at (column-major, same frames as T_iter_last): the
                                   correspondences / weights reg_get_correspondences reports belong to this pose */
    int32_t n_tail_launches;    /* launches of the persistent settled-tail kernel in this registration (0: three-launch path) */
    int32_t n_tail_iterations;  /* iterations those launches ran */
} reg_result;

/* ICPChainBase::setDefault (ICP.cpp:100-113): knn 1, eps 0, maxDist inf, Trimmed 0.85,
   Counter 40, Differential 0.001/0.001/3, point-to-plane. */
REG_API void reg_default_params(reg_params* p);
/* open3d_slam_ros/param/icp.yaml as shipped (maxDist 0.5, Trimmed 0.9, SurfaceNormal 1.57,
   Differential 0.001/0.008/3, Counter 30, degeneracyAwareness OptimizedEqualityConstraints 250 / 180 / 80 / 45 ->
   use_xicp = 1); epsilon is forced to 0 (exact search). */
REG_API void reg_shipped_params(reg_params* p);

REG_API reg_status reg_create(const reg_params* p, reg_handle** out);
REG_API void       reg_destroy(reg_handle* h);
REG_API const char* reg_last_error(const reg_handle* h);

/* All device work of the handle is enqueued on this hipStream_t (default: a stream the handle owns).  Work already
   queued on the previous stream is waited for before the switch (the handle's buffers are shared between them). */
REG_API reg_status reg_set_stream(reg_handle* h, void* hip_stream);

/* == ICP::initReference (ICP.cpp:847-898): copy, subtract centroid, build the search structure
   (voxel-bin table replaces KDTreeMatcher::init, MatchersImpl.cpp:78-83).
   P2PL and O3D_P2PL need `nrm`; GICP needs `cov`; O3D_P2P only `xyz`. */
REG_API reg_status reg_set_target(reg_handle* h, const float* xyz, int64_t xyz_stride, const float* nrm,
                                  int64_t nrm_stride, const float* cov, int64_t m, int on_device);

/* Reading cloud of the next reg_register / reg_prepare (ICP.cpp:952).  `nrm` is required when
   use_surface_normal is set (else REG_MISSING_FIELD); `cov` is required for GICP.
   BUFFER LIFETIME (reg_set_target, reg_set_source and their _f64 forms): host buffers are consumed before the call
   returns.  DEVICE buffers (on_device != 0) are read by copies / kernels enqueued on the handle's stream and the call
   may return before they have run: keep them valid and unmodified until a later blocking call on the handle
   (reg_register, reg_linearize, reg_get_correspondences, reg_dist_finish, ...) has returned or the stream has been
   synchronised.  reg_set_target itself blocks until the table is built.
   Time of the last reg_set_source (upload + Morton order) is reported as reg_result.source_prep_ms. */
REG_API reg_status reg_set_source(reg_handle* h, const float* xyz, int64_t xyz_stride, const float* nrm,
                                  int64_t nrm_stride, const float* cov, int64_t n, int on_device);

/* R11, reading side: Open3D's fp64 AoS arrays as Mapper::addRangeMeasurement holds them (points_ / normals_ n x 3
   doubles, covariances_ n x 9 doubles or NULL), cast to fp32 on the device exactly as open3dToPointmatcher does
   (open3d_conversions.cpp:57-118, static_cast<float> per coordinate; Mapper.cpp:288-289), then reg_set_source. */
REG_API reg_status reg_set_source_f64(reg_handle* h, const double* xyz, const double* normals, const double* covs,
                                      int64_t n, int on_device);

/* == ICP::compute(reading, -, T_init, false) (ICP.cpp:813-844 -> 902-1349) on the reading given to
   reg_set_source: R2 reading prep, the while(iterate) loop (R3-R9) on the device, R10 composition. */
REG_API reg_status reg_register(reg_handle* h, const float T_init[16], float T_out[16], reg_result* res);

/* Convenience == reg_set_source + reg_register. */
REG_API reg_status reg_compute(reg_handle* h, const float* xyz, int64_t xyz_stride, const float* nrm,
                               int64_t nrm_stride, const float* cov, int64_t n, int on_device,
                               const float T_init[16], float T_out[16], reg_result* res);

/* Factor-level hook (one pass of R3-R7, "Factor::linearize + reduction").
   reg_prepare does R2 for T_init (P2PL: centre + pre-transform the reading; GICP: no-op besides upload).
   reg_linearize evaluates the cost at T_iter (P2PL: transform in the centred frames, identity at
   iteration 0; GICP: full reading->reference transform) and returns the reduced system:
   P2PL: H = A, b as in ICP.cpp:1543,1565 (x = [rx ry rz tx ty tz]);  GICP: H = sum J^T M J, b = sum J^T M r. */
REG_API reg_status reg_prepare(reg_handle* h, const float T_init[16]);
REG_API reg_status reg_linearize(reg_handle* h, const float T_iter[16], float H[36], float b[6], double* err,
                                 int64_t* n_inliers);

/* Correspondences of the most recent iteration / linearize, in the reading's input order:
   ids = index into the target as given to reg_set_target (-1 = none within max_dist), d2 = squared
   distance (+inf = none) (PointMatcher.h:416-436), w = outlier weight (0/1).  Any pointer may be NULL. */
REG_API reg_status reg_get_correspondences(reg_handle* h, int32_t* ids, float* d2, float* w);

/* Distributed (point-partitioned reading) support: the per-iteration reduction is exposed in two
   halves so the caller can sum the partial systems of all ranks (RCCL all-reduce over xGMI) in between.
   reg_match_local     : R3+R4 on this rank's slice; fills hist[2048] with the level-`level` radix histogram
                         of finite d2 (level 0..2; prefix = bits fixed by previous levels).
   reg_reduce_local    : R5-R7 given the global trim limit -> 32 doubles {21 upper-tri H, 6 b, err, n_in, n_matched, sum d2 inliers, pad}.
   reg_apply_update    : R8+R9 from the globally summed 32 doubles (identical on every rank). */
REG_API reg_status reg_source_centroid_sums(reg_handle* h, int64_t sums[3]);   /* sum llrint(x*2^16): exact, order-free */
REG_API reg_status reg_prepare_centroid(reg_handle* h, const float T_init[16], const float c_read[3]); /* R2 with the GLOBAL reading centroid */
REG_API reg_status reg_compose(reg_handle* h, const float T_iter[16], float T_out[16]);              /* R10 */
REG_API reg_status reg_match_local(reg_handle* h, const float T_iter[16]);
REG_API reg_status reg_trim_histogram(reg_handle* h, int level, uint32_t prefix, uint32_t hist[2048]);
REG_API reg_status reg_reduce_local(reg_handle* h, const float T_iter[16], float trim_limit, double sums[32]);
REG_API reg_status reg_solve_update(const reg_params* p, const double sums[32], const float T_iter[16],
                                    float T_next[16], int32_t* rank);

/* Stream-ordered variant of the same exchange (no host round trip per iteration): each phase only ENQUEUES
   kernels on the handle's stream; between phases the caller all-reduces -- on the SAME stream (RCCL) -- the device
   buffers returned by reg_dist_buffers (hist: 3 x 2048 int32 counts, sums: 32 doubles).  Phases:
   0 match + level-0 histogram | 1, 2 radix levels of the exact global trimmed quantile | 3 weights + normal
   equations (local sums) | 4 solve + pose update + checkers on the device from the GLOBAL sums. */
REG_API reg_status reg_dist_begin(reg_handle* h, const float T_start[16] /* NULL: identity (P2PL) / T_init (GICP) */);
REG_API reg_status reg_dist_buffers(reg_handle* h, void** hist, void** sums);
REG_API reg_status reg_dist_phase(reg_handle* h, int phase);
REG_API reg_status reg_dist_finish(reg_handle* h, float T_out[16], reg_result* res);

/* Fused multi-GPU iteration (2 launches + ONE all-gather per iteration instead of 6 launches + 4 all-reduces), usable
   once the trimmed limit has settled -- same prediction / exact verification as the single-GPU fused iteration:
   phase 5: fused search + weights + normal equations on this rank's slice; its certain sums, band count and band
            records (<= 512) go into a fixed-size contribution block            -> all-gather(contrib -> gathered)
   phase 6: every rank reduces the SAME gathered blocks in rank order (identical results, no broadcast), verifies the
            band with the global counts, selects the exact global quantile, solves and updates on the device.
   A failed verification (or an overflowing block) sets `stall` on every rank alike; the caller then runs that
   iteration through phases 0-4. */
typedef struct {
    int64_t sequences_done;      /* update kernels that have reported since reg_dist_begin */
    int64_t sequences_enqueued;
    int32_t iterations;          /* completed Gauss-Newton iterations */
    int32_t done, stall, stream_idle;
    float   limit_last, limit_prev;
} reg_dist_status;
REG_API reg_status reg_dist_fused_buffers(reg_handle* h, int n_ranks, int rank, void** contrib, void** gathered,
                                          int64_t* contrib_bytes);
REG_API reg_status reg_dist_poll(reg_handle* h, reg_dist_status* out);
/* What the update kernel of ONE specific sequence reported (seq_rel = 1 for the first iteration enqueued after
   reg_dist_begin): sequences_done == seq_rel when available, 0 otherwise; stream_idle (sampled first) tells that it will
   never come (update kernels that find the loop done or stalled do not report).  Multi-GPU drivers must steer by these
   records only: they are identical on every rank, whereas "the latest state seen" depends on timing. */
REG_API reg_status reg_dist_record(reg_handle* h, int64_t seq_rel, reg_dist_status* out);
/* Reading preparation without a host round trip: reg_dist_centroid_sums enqueues this rank's integer centroid sums
   (numeric contract NC1) and returns their device address (3 x int64); the caller all-reduces (sum) them on the handle's
   stream; reg_dist_prepare then centres and pre-transforms the slice with the centroid of all n_global reading points. */
REG_API reg_status reg_dist_centroid_sums(reg_handle* h, void** sums_dev);
REG_API reg_status reg_dist_prepare(reg_handle* h, const float T_init[16], int64_t n_global);
/* Select-by-gather form of the trimmed iteration (fewer dependent collectives): phase 10 (match), all-gather the
   n_max floats at *d2_local of every rank into *d2_all (n_ranks x n_max), phase 11 (exact 3-level select on the
   gathered distances, redundantly on every rank; linearize of the local slice; partial sums), all-reduce the 32 sums,
   phase 4.  n_max >= every rank's reading size (the tail is padded with +inf).  Call after reg_set_source. */
REG_API reg_status reg_dist_gather_buffers(reg_handle* h, int n_ranks, int64_t n_max, void** d2_local, void** d2_all);
/* use_xicp on the distributed path: on the FIRST iteration, after phase 4, run phase 7, all-reduce (sum) the 4 doubles at
   *center, phase 8, all-reduce the 12 doubles at *sums, phase 9 (reports with the sequence number of phase 4). */
REG_API reg_status reg_dist_xicp_buffers(reg_handle* h, void** center, void** sums);

/* ---- multi-GPU registration behind the C ABI (BASELINE config C4) ---------------------------------
   One process per GPU.  The reading is point-partitioned: every rank gives ITS slice to reg_set_source; the reference
   (reg_set_target) and its tables are replicated.  reg_dist_register is ICP::compute (ICP.cpp:813-844, called from
   the C++ mapper, Mapper.cpp:343,372-373) for that layout: all kernels and collectives are enqueued on the handle's
   stream, nothing synchronises inside an iteration, and every rank returns the same T_out.  Per iteration the ranks
   exchange, over RCCL (xGMI): unsettled iterations -- one all-gather of the squared match distances (exact global
   trimmed quantile, selected redundantly on every rank) + one all-reduce of the 32-double (H, b, e, counts) record;
   settled iterations -- ONE all-gather of a fixed-size block {32 sums, band records} per rank.
   Group set-up: rank 0 calls reg_dist_get_unique_id and hands the 128 bytes to the other ranks by any means (MPI,
   a file, torch.distributed ...); every rank then calls reg_dist_init (ncclCommInitRank on the handle's device).
   COLLECTIVE CONTRACT: all ranks call reg_dist_init / reg_dist_register / reg_dist_shutdown in the same order, and a
   new reading is set on ALL ranks or on none between two registrations.  Every wait inside reg_dist_register has a
   deadline (O3D_DIST_TIMEOUT_S, default 30 s): a dead peer or a collective that never completes returns
   REG_DEVICE_ERROR on the survivors instead of hanging them -- the caller should then exit non-zero. */
#define REG_DIST_ID_BYTES 128
REG_API reg_status reg_dist_get_unique_id(char id[REG_DIST_ID_BYTES]);
REG_API reg_status reg_dist_init(reg_handle* h, const char id[REG_DIST_ID_BYTES], int rank, int n_ranks);
REG_API reg_status reg_dist_register(reg_handle* h, const float T_init[16], float T_out[16], reg_result* res);
REG_API reg_status reg_dist_shutdown(reg_handle* h);
/* after reg_dist_register: size of the whole reading and how the loop went (any pointer may be NULL) */
REG_API reg_status reg_dist_info(reg_handle* h, int64_t* n_global, int32_t* n_generic, int32_t* n_fused, int32_t* n_stalls);
/* A transport other than RCCL (tests on one GPU, other launchers): both callbacks ENQUEUE on `stream` (or complete
   before returning), operate in place on DEVICE memory and return 0 on success. */
enum { REG_DT_I32 = 0, REG_DT_I64 = 1, REG_DT_F64 = 2 };
typedef struct {
    void* ctx;
    int (*all_reduce_sum)(void* ctx, void* buf, int64_t count, int dtype, void* stream);
    int (*all_gather)(void* ctx, const void* send, void* recv, int64_t bytes_per_rank, void* stream);
} reg_collectives;
REG_API reg_status reg_dist_init_custom(reg_handle* h, const reg_collectives* c, int rank, int n_ranks);

/* The steering of reg_dist_register as a pure host-side state machine (no device, no collectives), exported so that
   the decision logic every rank must agree on can be exercised without a GPU (world_size-2 gloo tests on CPU):
   step() consumes the reply to its previous action and returns the next one.
     REG_STEER_RECORD  wait for the record of sequence `seq` (reg_dist_record); reply.available = 0 when the stream
                       drained without it (an earlier sequence ended or stalled the loop)
     REG_STEER_GENERIC enqueue one select-based iteration (no reply)
     REG_STEER_FUSED   enqueue `count` fused iterations (no reply)
     REG_STEER_DRAIN   wait until the stream is idle, reply with the latest state (reg_dist_poll)
     REG_STEER_DONE    the registration is complete */
enum { REG_STEER_RECORD = 0, REG_STEER_GENERIC = 1, REG_STEER_FUSED = 2, REG_STEER_DRAIN = 3, REG_STEER_DONE = 4 };
typedef struct { int32_t kind, count; int64_t seq; } reg_dist_action;
typedef struct { int32_t available, iterations, done, stall; float limit_last, limit_prev; } reg_dist_reply;
typedef struct reg_dist_steer reg_dist_steer;
REG_API reg_dist_steer* reg_dist_steer_create(int trimming, int fixed_iters, int max_iter, float settle_tol, int can_fuse);
REG_API void reg_dist_steer_destroy(reg_dist_steer* s);
REG_API reg_dist_action reg_dist_steer_step(reg_dist_steer* s, const reg_dist_reply* reply /* NULL on the first call */);
REG_API void reg_dist_steer_counts(const reg_dist_steer* s, int32_t* n_generic, int32_t* n_fused, int32_t* n_stalls);

/* Host-side pieces of the path, exported so they can be checked without a GPU
   (PointToPlane.cpp:112-265 solve, :327-381 x -> 4x4; column-major 4x4). */
REG_API int  reg_host_solve6(const float A[36], const float b[6], float x[6]);
REG_API void reg_host_x_to_T(const float x[6], float T[16]);
/* R8x equality-constrained solve (PointToPlane.cpp:459-505, null-space form): flags[k] = 1 keeps eigen-direction k
   (0-2 rotation block, 3-5 translation block, descending eigenvalue), 0 forbids any update along it.
   Returns the rank of the reduced system. */
REG_API int  reg_host_solve6_xicp(const float A[36], const float b[6], const int32_t flags[6], float x[6]);
REG_API void reg_host_centroid(const float* xyz, int64_t stride, int64_t n, float out[3]);
/* Update of the two Open3D costs from the reduced 32-double record of one iteration (the same code the update kernel
   runs): cost REG_COST_O3D_P2PL -- {0..20: J^T J packed upper triangle, 21..26: J^T r, 27: sum r^2, 28: pairs, 29: pairs,
   30: sum d^2}; REG_COST_O3D_P2P -- {0..2: sum (p - o), 3..5: sum (q - o), 6..14: sum (q - o)(p - o)^T row-major (row =
   q component), 15..17: sum o, 27: sum |p - q|^2, 28..30 as above} about an origin o near the data.  T_update: the
   column-major 4x4 U of T <- U T; *rank (may be NULL) as reg_result.rank_last.  REG_BAD_ARGUMENT for any other cost,
   REG_NO_CORRESPONDENCES when sums[28] == 0. */
REG_API reg_status reg_host_o3d_update(int cost, const double sums[32], double T_update[16], int32_t* rank);
/* ---- libpointmatcher chain extension: k-NN matching, RobustOutlierFilter, PointToPointErrorMinimizer -------------
   An opt-in extension of the REG_COST_P2PL loop (reg_params keeps its layout; reg_params.knn stays 1).  Set on a handle
   with reg_set_pm_chain; every registration of that handle then runs the generic iteration k-NN search -> exact selects
   -> weights + reduction -> update on the device (never the fused, tail or distributed forms).
     KDTreeMatcher.knn (MatchersImpl.cpp)          1..16 exact nearest reference points within reg_params.max_dist
                                                    (+inf allowed), ascending (d2, index); missing slots: id -1, d2 +inf
     filters (OutlierFiltersImpl.cpp)              product of the weights of TrimmedDist (quantile over ALL N*knn
                                                    finite d2, Matches.cpp:60-87), SurfaceNormal, MaxDist (reg_params),
                                                    RobustOutlierFilter (:397-598) when use_robust != 0, and MinDist /
                                                    MedianDist / VarTrimmedDist (below)
     minimizer                                     REG_PM_POINT_TO_PLANE: A = sum w F F^T, b = -sum w F r (ICP.cpp:1527-1565);
                                                    REG_PM_POINT_TO_POINT: weighted Kabsch (ErrorMinimizers/PointToPoint.cpp:62-100)
                                                    in fp64, composed T_iter <- dT T_iter in the centred frames
   Rules: only cost REG_COST_P2PL (else REG_BAD_ARGUMENT); use_xicp with knn > 1, robust weights or point-to-point is
   REG_UNSUPPORTED (see the Bound checker / covariance below for the one chain that runs with it); the "std" scale estimator is REG_UNSUPPORTED (getStandardDeviation, Matches.cpp:124-129, is an fp32
   Eigen sum in Eigen's order over every entry including the +inf ones: it cannot be restated to a stated tolerance).
   Robust state: the filter's `iteration` and `scale` persist across registrations of the handle as in the reference
   (ICP::compute never resets them, OutlierFiltersImpl.cpp:408-409,510-543); reg_set_pm_chain resets them.
   reg_result with a chain: n_inliers = pairs with w != 0, n_matched = pairs with finite d2, fitness = n_inliers /
   (N knn) (pointUsedRatio, ErrorMinimizer.cpp:139), inlier_rmse unweighted over the inliers, error = sum w r^2
   (point-to-plane) / sum w |p - q|^2 (point-to-point); point-to-point: H_last = b_last = 0 and rank_last is the rank
   of the 3x3 cross-covariance.  reg_get_correspondences returns REG_UNSUPPORTED with knn > 1, reg_linearize always
   with a chain; the distributed entry points return REG_UNSUPPORTED while a chain is set.

   MinDist, MedianDist and VarTrimmedDist outlier filters (OutlierFiltersImpl.cpp:86-220).  All three act on
   Matches.dists, the N x knn squared distances (+inf = no match), and multiply into the chain's weight like the others;
   a chain that sets one of them is not the default chain and runs the generic chain iteration.
     MinDist        w = [d2 >= minDist^2], minDist^2 an fp32 product; minDist in [1e-7, inf).  +inf passes, as in the
                    reference (the pair has no id and its weight is zero anyway).
     MedianDist     limit = factor * getDistsQuantile(0.5) in fp32, the quantile over the finite distances at index
                    (size_t)(n_finite * 0.5f) (the float-index form, as berg); w = [d2 <= limit]; factor in [1e-7, inf);
                    no finite distance: REG_NO_CORRESPONDENCES.
     VarTrimmedDist (Phillips 2007) n = N knn counts EVERY entry; v = ascending sort of the entries that are finite and
                    > 0, m = |v|; minEl = floor(minRatio n), maxEl = floor(maxRatio n) as fp32 products;
                    FRMS(j) = S(j) / (j + 1) / ((j + 1) / n)^(2 lambda) with S(j) = v[0] + ... + v[j]; k = the first j that
                    minimises FRMS; optRatio = (float)k / (float)n; limit = getDistsQuantile(optRatio) over the finite
                    distances, zeros included; w = [d2 <= limit].  Ratios in [1e-7, 1], minRatio >= maxRatio is
                    REG_BAD_ARGUMENT; m = 0 is REG_NO_CORRESPONDENCES.
                    Two documented deviations from the reference: (1) S and FRMS are fp64 with a fixed summation order
                    (deterministic from run to run), where the reference keeps an fp32 sequential running sum and
                    evaluates FRMS in fp32; near a flat minimum the two may pick ranks a few places apart.  (2) When
                    m < maxEl (entries that are +inf or 0) the reference maps n elements over a buffer that holds m and
                    reads uninitialised memory; here the candidates are j in [minEl, min(maxEl, m)), and k = m - 1
                    when that range is empty.
   Any of the three with use_xicp is REG_UNSUPPORTED.  struct_size: sizeof(reg_pm_chain), REG_PM_CHAIN_SIZE_V2 (the struct
   up to var_lambda) or REG_PM_CHAIN_SIZE_V1 (the struct up to reserved[2]), as callers built before the later fields pass
   it: the fields they do not hold are then off.

   Pose covariance, minimizer statistics, BoundTransformationChecker and SolutionRemapping.  A chain that
   sets with_cov, use_bound or degeneracy_method is not the default chain and runs the generic chain iteration: never the
   fused, tail or distributed forms.  use_xicp: a chain that is the plain loop plus with_cov and / or use_bound (knn 1,
   point-to-plane, none of the chain's filters) runs the first-iteration localizability analysis and the constrained
   solve inside the chain iteration, with the plain loop's kernels and arithmetic; together with any other chain field it
   stays REG_UNSUPPORTED, and SolutionRemapping with use_xicp is REG_BAD_ARGUMENT (two degeneracy methods at once).
     with_cov       PointToPlaneWithCovErrorMinimizer (ErrorMinimizers/PointToPlaneWithCov.cpp:61-162): Censi's closed form
                    cov = sensorStdDev^2 H^-1 M H^-1, read with reg_get_covariance.  The reference evaluates the estimate in
                    every iteration and keeps the last; here it is evaluated once, after the loop, on the state of the last
                    iteration (unobservable).  Point-to-plane only (with REG_PM_POINT_TO_POINT: REG_UNSUPPORTED --
                    PointToPointWithCov.cpp:77 sets normal = (1,1,1), so the first three components of every v are equal, H is
                    singular by construction and the reference's result is whatever PartialPivLU returns for it).
                    Pairs: every (i, k) of the last iteration with w != 0 and a finite d2, at T_iter_prev; the weight VALUES
                    are not used (the reference's `if (outlierWeights > 0)` is commented out).  p = the reading point moved by
                    T_iter_prev in the centred frames (the loop's fp32 arithmetic), q / n = the matched reference point /
                    normal; both clouds are then centred on their own mean over the kept pairs (compute_in_place,
                    PointToPlane.cpp:281-284).  Deviation: the mean is an fp64 sum in a fixed order rounded to fp32 (Eigen's
                    fp32 rowwise().mean() order is unspecified).  The last update dT gives beta = -asin(dT(2,0)), alpha =
                    atan2(dT(2,1), dT(2,2)), gamma = atan2(dT(1,0) / cos beta, dT(0,0) / cos beta), t = dT(0..2,3).  Per pair,
                    in fp32 and the reference's expression order (lines 116-146): ranges and directions of the centred
                    points, n_alpha / n_beta / n_gamma, E, N_reading, N_reference and the 6-vectors v, a, b;
                    H = sum v v^T, M = sum (a a^T + b b^T): 21 + 21 fp64 sums, per-workgroup partial rows and one fixed-order
                    final sum (no float atomics: two calls return identical bits).  cov = sigma^2 H^-1 M H^-1 in fp64,
                    stored as fp32, row-major in the reference's order [x y z alpha beta gamma].  rank = rank of H by the rank
                    rule of the solver (eigenvalues above 6 eps_fp32 of the largest); with rank < 6 the reference inverts a
                    singular matrix and returns whatever comes out: here cov is all NaN and the status REG_OK.  A kept pair
                    whose centred point has zero norm makes the result NaN, as in the reference.  Without reference normals:
                    REG_MISSING_FIELD (the reference returns FLT_MAX * I, PointToPlaneWithCov.cpp:91-92).
     use_bound      BoundTransformationChecker (TransformationCheckersImpl.cpp:166-225), evaluated in the update step on the
                    device after every update, in fp32: rotation = quaternion angular distance between T_iter and the identity
                    the checkers were initialised with (ICP.cpp:993-997), translation = |t_iter| in the centred frames;
                    strict `>` against max_rotation_norm / max_translation_norm.  A violation ends the registration with
                    REG_OUT_OF_BOUNDS: T_out = T_init, reg_result is filled and T_iter_last holds the offending pose.
                    Checkers run in YAML order and an exception ends the pass: with bound_after_counter != 0 a Counter that
                    fires in the same iteration hides the violation (the registration ends with max_iter_reached).
                    fixed_iters > 0 ignores this checker like the others.
     degeneracy_method  REG_DEGENERACY_SOLUTION_REMAPPING (ICP.cpp:2446-2501, 1621-1666; PointToPlane.cpp:301-309).
                    Point-to-plane only (REG_UNSUPPORTED with point-to-point: the reference warns and skips the detection).
                    Per iteration, on the fp32 normal matrix A: eigenvalues (descending) / eigenvectors u_j; direction j is
                    degenerate when lambda_j < sr_threshold -- with sr_use2019 the threshold is the condition number
                    lambda_max / lambda_min, as the code passes it (ICP.cpp:2473-2481).  If any direction is degenerate
                    P = sum over the kept j of u_j u_j^T (for orthonormal U the reference's eigenvectors^-T * copy^T);
                    otherwise P KEEPS ITS VALUE OF THE PREVIOUS ITERATION (the reference's behaviour: a stale projector
                    stays in force).  P is the identity at the start of every registration (PointMatcher.h:645).
                    x = P solve(A, b).  A all zero or P all zero: the loop stops before the update, T_out = T_init bit for
                    bit, status REG_OK, reg_minimizer_stats.returned_prior = 1 (ICP.cpp:1175-1179, 1335-1341).
                    Deviation: the fp64 Jacobi eigen-solver stands in for Eigen's fp32 JacobiSVD; decisions can differ only
                    when an eigenvalue lies within fp32 round-off of the threshold. */
enum { REG_PM_POINT_TO_PLANE = 0, REG_PM_POINT_TO_POINT = 1 };
enum {   /* robustFct (OutlierFiltersImpl.cpp:385-394) */
    REG_ROBUST_CAUCHY = 0, REG_ROBUST_WELSCH = 1, REG_ROBUST_SC = 2, REG_ROBUST_GM = 3, REG_ROBUST_TUKEY = 4,
    REG_ROBUST_HUBER = 5, REG_ROBUST_L1 = 6, REG_ROBUST_STUDENT = 7
};
enum { REG_SCALE_NONE = 0, REG_SCALE_MAD = 1, REG_SCALE_BERG = 2, REG_SCALE_STD = 3 /* REG_UNSUPPORTED */ };
enum { REG_DIST_POINT2POINT = 0, REG_DIST_POINT2PLANE = 1 /* needs reference normals */ };
typedef struct {
    int32_t struct_size;         /* = sizeof(reg_pm_chain); checked */
    int32_t knn;                 /* KDTreeMatcher knn, 1..16 (reg_params.knn stays 1) */
    int32_t minimizer;           /* REG_PM_POINT_TO_PLANE (the loop as today) | REG_PM_POINT_TO_POINT */
    int32_t use_robust;          /* RobustOutlierFilter in the chain */
    int32_t robust_fct;          /* REG_ROBUST_* */
    float   tuning;              /* "tuning" (> 0); with berg: the target scale */
    int32_t scale_estimator;     /* REG_SCALE_NONE | MAD | BERG */
    int32_t nb_iter_for_scale;   /* "nbIterationForScale" (0 = every iteration), 0..100 */
    int32_t distance_type;       /* REG_DIST_POINT2POINT | REG_DIST_POINT2PLANE */
    float   approximation;       /* "approximation" (INFINITY = off); w = 0 where e^2 >= (float)(approximation^2 in double) */
    int32_t reserved[2];
    /* -- fields after REG_PM_CHAIN_SIZE_V1 -- */
    int32_t use_min_dist_filter; /* MinDistOutlierFilter */
    float   outlier_min_dist;    /* "minDist" (1) */
    int32_t use_median_dist;     /* MedianDistOutlierFilter */
    float   median_factor;       /* "factor" (3) */
    int32_t use_var_trimmed;     /* VarTrimmedDistOutlierFilter */
    float   var_min_ratio;       /* "minRatio" (0.05) */
    float   var_max_ratio;       /* "maxRatio" (0.99) */
    float   var_lambda;          /* "lambda" (2.35) */
    /* -- fields after REG_PM_CHAIN_SIZE_V2 (pose covariance, BoundTransformationChecker, SolutionRemapping; below) -- */
    int32_t with_cov;            /* PointToPlaneWithCovErrorMinimizer: reg_get_covariance after the registration */
    float   sensor_std_dev;      /* "sensorStdDev" (0.01), [0, inf) */
    int32_t use_bound;           /* BoundTransformationChecker */
    float   max_rotation_norm;   /* "maxRotationNorm" (1), >= 0, rad */
    float   max_translation_norm;/* "maxTranslationNorm" (1), >= 0 */
    int32_t bound_after_counter; /* 1: the Counter checker is listed before the Bound checker (YAML order) */
    int32_t degeneracy_method;   /* REG_DEGENERACY_NONE | REG_DEGENERACY_SOLUTION_REMAPPING */
    float   sr_threshold;        /* SolutionRemapping "threshold" */
    int32_t sr_use2019;          /* SolutionRemapping "use2019" */
    int32_t reserved2;
} reg_pm_chain;
#define REG_PM_CHAIN_SIZE_V1 48
#define REG_PM_CHAIN_SIZE_V2 80
enum { REG_DEGENERACY_NONE = 0, REG_DEGENERACY_SOLUTION_REMAPPING = 1 };

/* knn 1, point-to-plane, robust / MinDist / MedianDist / VarTrimmedDist / covariance / Bound / SolutionRemapping off: the
   loop as without a chain (parameter defaults as OutlierFiltersImpl.h, PointToPlaneWithCov.h:75,
   TransformationCheckersImpl.h). */
REG_API void       reg_default_pm_chain(reg_pm_chain* c);
/* Pure check of a chain against the parameters it would run with (no device). */
REG_API reg_status reg_check_pm_chain(const reg_params* p, const reg_pm_chain* c);
/* c == NULL or the default chain: back to the plain loop.  Resets the robust state. */
REG_API reg_status reg_set_pm_chain(reg_handle* h, const reg_pm_chain* c);
/* Robust filter state as the next registration starts with it: scale and the filter's iteration counter (1 = fresh). */
REG_API reg_status reg_get_robust_state(const reg_handle* h, float* scale, int32_t* iteration);
/* VarTrimmedDist of the last iteration (taken at T_iter_prev, like the correspondences): the optimised ratio (the
   reference logs it as "Optimized ratio"), the rank k it came from and n = N knn.  REG_NOT_CONFIGURED without a chain
   registration with use_var_trimmed on the current reading.  Any pointer may be NULL. */
REG_API reg_status reg_get_var_trim(const reg_handle* h, float* ratio, int64_t* index, int64_t* n_total);
/* Pose covariance of the last registration (with_cov; contract above): cov row-major 6x6 [x y z alpha beta gamma], *rank
   the rank of H (cov is all NaN when rank < 6).  REG_NOT_CONFIGURED unless the last registration on the current reading
   ran with with_cov.  Two calls return identical bits.  Any output pointer may be NULL. */
REG_API reg_status reg_get_covariance(const reg_handle* h, float cov[36], int32_t* rank);
/* The 42 fp64 sums the covariance came from: the packed upper triangles (row by row) of H and M.  Same validity. */
REG_API reg_status reg_get_covariance_sums(const reg_handle* h, double H[21], double M[21]);
/* cov = sigma^2 H^-1 M H^-1 from the packed sums, the same code as the device, without a device. */
REG_API reg_status reg_host_censi_covariance(const double H[21], const double M[21], float sigma, float cov[36],
                                             int32_t* rank);
/* ErrorMinimizer quality getters (ErrorMinimizer.cpp:249-277, PointToPlane.cpp:780-930) of the last chain registration,
   valid whenever reg_get_correspondences[_k] is (REG_NOT_CONFIGURED otherwise); taken at T_iter_prev.
   The reference adds the weights in an fp32 running sum; here the sum is fp64 in a fixed order, rounded once. */
typedef struct {
    int32_t struct_size;               /* = sizeof(reg_minimizer_stats); checked */
    int32_t returned_prior;            /* SolutionRemapping left the loop and T_out = T_init */
    double  point_used_ratio;          /* pairs with w != 0 / (N knn)                    getPointUsedRatio */
    double  weighted_point_used_ratio; /* sum w / (N knn)                                 getWeightedPointUsedRatio */
    double  overlap;                   /* = weighted_point_used_ratio: what getOverlap returns for clouds without
                                          simpleSensorNoise / densities descriptors (PointToPlane.cpp:886-890) */
    double  residual_error;            /* sum w ((p - q) . n)^2 (PointToPlane.cpp:780-816) / sum w |p - q|^2
                                          (PointToPoint.cpp:103-116) = reg_result.error */
    int64_t n_rejected_matches;        /* pairs with w == 0 */
    int64_t n_rejected_points;         /* reading points all of whose knn pairs have w == 0 */
} reg_minimizer_stats;
REG_API reg_status reg_get_minimizer_stats(reg_handle* h, reg_minimizer_stats* out);
/* SolutionRemapping of the last iteration: categories (1 = kept, 0 = degenerate; solRemapCategories), the eigenvalues
   descending (optimizationEigenvalues) and lambda_max / lambda_min (optimizationConditionNumber_).  REG_NOT_CONFIGURED
   without a SolutionRemapping registration on the current reading.  Any pointer may be NULL. */
REG_API reg_status reg_get_degeneracy(const reg_handle* h, int32_t categories[6], float eigenvalues[6],
                                      float* condition_number);
/* BoundTransformationChecker's condition variables after the last update (rotation [rad], translation).
   REG_NOT_CONFIGURED without a use_bound registration on the current reading. */
REG_API reg_status reg_get_bound(const reg_handle* h, float* rotation, float* translation);
/* One SolutionRemapping step on the host, the same code as the device: A row-major fp32, P_in the projector in force
   (the identity for the first iteration), P_out the projector after this step (== P_in when nothing is degenerate).
   Returns REG_OK, or REG_NO_CORRESPONDENCES when the reference would return the prior (A or P_out all zero). */
REG_API reg_status reg_host_solution_remap(const float A[36], float threshold, int use2019, const double P_in[36],
                                           double P_out[36], int32_t categories[6], float eigenvalues[6]);
/* The VarTrimmedDist contract above on the host (no device): d2[n] may hold +inf and zeros.  *index = k, *ratio =
   optRatio, *limit = the quantile the weights compare against.  The device evaluates the same objective (fp64) with
   another, fixed, summation order.  REG_BAD_ARGUMENT for ratios outside [1e-7, 1] or minRatio >= maxRatio,
   REG_NO_CORRESPONDENCES when no entry is finite and > 0.  Any output pointer may be NULL. */
REG_API reg_status reg_host_var_trim(const float* d2, int64_t n, float minRatio, float maxRatio, float lambda,
                                     int64_t* index, float* ratio, float* limit);
/* Correspondences of the last iteration (taken at T_iter_prev), reading input order, N x knn entries each, ascending
   (d2, id); ids -1 / d2 +inf where fewer than knn reference points lie within max_dist.  knn must equal the chain's
   knn.  Any pointer may be NULL. */
REG_API reg_status reg_get_correspondences_k(reg_handle* h, int32_t knn, int32_t* ids, float* d2, float* w);
/* The robust weight of the chain's kernels on the host: w[i] for squared distances d2_or_e[i] (the filter's `dists`),
   scale and tuning as the filter holds them.  The same code as the device. */
REG_API reg_status reg_host_robust_weights(int32_t fct, float tuning, float scale, float approximation,
                                           const float* d2_or_e, int64_t n, float* w);
/* Point-to-point update of the chain from its 32 reduced doubles ({0..2: sum w p, 3..5: sum w q, 6..14: sum w q p^T
   row-major, 15..17: 0 (origin), 28: sum w}; the frames' origin): the column-major 4x4 dT of T_iter <- dT T_iter;
   *rank = rank of the cross-covariance.  REG_NO_CORRESPONDENCES when sums[28] == 0. */
REG_API reg_status reg_host_pm_p2p_update(const double sums[32], double T_update[16], int32_t* rank);

/* ---- degeneracyAwareness: EqualityConstraints (X-ICP, ternary; icp.yaml:56-67) -----------------------------------
   A companion of the chain (the layout of reg_pm_chain and the meaning of degeneracy_method do not change).  With it on
   the handle registers on the chain's generic iteration, also under the default chain, and EVERY iteration, after A, b
   and the deltas are known and before the solve:
     1. eigenvectors of the two 3x3 blocks of A, the data frame, the centre of the matched pairs and both alignment
        vectors exactly as the first-iteration analysis of use_xicp (translation: the matched normal; rotation:
        (p - centre) x n, normalised unless its norm is < 1), fp32 with one rounding per operation;
     2. per eigen-direction k (rotation 0-2, translation 3-5) with a = |alignment . v_k|:  high = sum a over a >
        cos(strong) (n_high pairs), combined = sum a over a >= cos(minimal) (n_combined pairs), fp64 sums over ALL pairs
        (the reference stops adding once a direction is localizable: the terms are non-negative, so no decision changes,
        only the reported sums of localizable directions are larger);
     3. category, tested in this order:  combined >= high_information || high >= enough_information -> LOCALIZABLE;
        combined >= enough_information -> PARTIAL_MIXED (sample: the n_combined pairs);  high >= insufficient_information
        -> PARTIAL_HIGH (sample: the n_high pairs);  otherwise NONE (constraint value 0).  Every category but LOCALIZABLE
        clears reg_result.localizable[k];
     4. a partial direction's constraint value is v_k . x3, x3 the solution of the 3x3 problem over its sample in the
        optimisation frame (translation: A3 = sum n n^T, b3 = -sum n r; rotation: A3 = sum c c^T, b3 = -sum c r with
        c = p x n, r = n . (p - q); no weights; nine fp64 sums of fp32 products rounded once to fp32), solved by the
        reference's sequence (partial-pivot LU in fp32, L^T L y = L^T P b3 in fp64, x3 = U^-1 y in fp32);
     5. the solve is the KKT system of PointToPlane.cpp:484-503 with the constraint values as right-hand side (plain
        solve when every direction is localizable).
   The prior is returned (REG_OK, T_out = T_init, reg_minimizer_stats.returned_prior = 1) when a sample holds fewer pairs
   than insufficient_information or more than there are pairs (ICP.cpp:1956-1967; with unit reference normals a <= 1 and
   the ordered thresholds rule this out, normals longer than 1 -- nothing normalises them -- do not), and -- a deviation -- when a constraint
   value is not finite (a singular U, e.g. exactly axis-aligned sample normals).  Further deviations: DESIGN.md 5l.
   PARITY UNPINNED against the reference itself (its localizability unit tests are empty); pinned: device == restatement.
   Runs with: point-to-plane, knn 1, the 0/1-weight outlier filters, the Bound checker, fixed_iters.  REG_UNSUPPORTED:
   knn > 1, RobustOutlierFilter, point-to-point, with_cov, a cost other than REG_COST_P2PL; reg_dist_* refuse a handle
   with it on.  REG_BAD_ARGUMENT: together with use_xicp or SolutionRemapping (two methods at once), thresholds that are
   not finite or not ordered insufficient <= enough <= high, angles outside (0, 90], a wrong struct_size. */
typedef enum {
    REG_TERNARY_LOCALIZABLE = 0,
    REG_TERNARY_PARTIAL_MIXED = 1,
    REG_TERNARY_PARTIAL_HIGH = 2,
    REG_TERNARY_NONE = 3
} reg_ternary_category;
typedef struct {
    int32_t struct_size;               /* sizeof(reg_ternary_xicp) */
    int32_t enabled;
    float high_information;            /* highInformationThreshold (250 shipped) */
    float enough_information;          /* enoughInformationThreshold (180) */
    float insufficient_information;    /* insufficientInformationThreshold (35) */
    float min_alignment_angle_deg;     /* point2NormalMinimalAlignmentAngleThreshold (80) */
    float strong_alignment_angle_deg;  /* point2NormalStrongAlignmentAngleThreshold (45) */
    int32_t reserved;
} reg_ternary_xicp;
typedef struct {
    int32_t struct_size;               /* sizeof(reg_ternary_xicp_result), set by the caller */
    int32_t iteration;                 /* 1-based number of the iteration the values belong to (taken at T_iter_prev) */
    int32_t category[6];               /* reg_ternary_category */
    int32_t sane;                      /* 0: the sanity rule failed (the prior was returned) */
    int32_t reserved;
    double combined[6], high[6];
    int64_t n_combined[6], n_high[6];
    int64_t n_pairs;
    float constraint[6];               /* 0 unless partial */
    double partial_sums[6][9];         /* 0-5 upper triangle of A3 row by row, 6-8 = -b3; zero unless partial */
    float eigenvectors[2][9];          /* optimisation frame, [0] rotation, [1] translation; [3 * k + r] = component r of k */
} reg_ternary_xicp_result;
/* enabled = 0 and the shipped yaml's commented values (250, 180, 35, 80, 45) */
REG_API void       reg_default_ternary_xicp(reg_ternary_xicp* t);
/* A pure check (no device) of the method against the parameters and a chain (NULL: the default chain). */
REG_API reg_status reg_check_ternary_xicp(const reg_params* p, const reg_pm_chain* c, const reg_ternary_xicp* t);
/* Turn the method on (or off: NULL or enabled = 0).  A call that would leave an invalid pair (method, chain) fails and
   leaves the handle unchanged; so does a later reg_set_pm_chain. */
REG_API reg_status reg_set_ternary_xicp(reg_handle* h, const reg_ternary_xicp* t);
/* The analysis of the last iteration.  REG_NOT_CONFIGURED unless the last registration on the current reading ran with
   the method on and analysed at least one iteration. */
REG_API reg_status reg_get_ternary_xicp(reg_handle* h, reg_ternary_xicp_result* out);
/* Step 3 on the host, the same code as the device; *sane = 0 when the sanity rule fails.  Returns REG_BAD_ARGUMENT for a
   params struct reg_check_ternary_xicp would refuse for its ranges. */
REG_API reg_status reg_host_ternary_decide(const double combined[6], const double high[6], const int64_t n_combined[6],
                                           const int64_t n_high[6], int64_t n_pairs, const reg_ternary_xicp* params,
                                           int32_t category[6], int32_t* sane);
/* Step 4 on the host, the same code as the device: sums9 as partial_sums above, v the eigenvector in the optimisation
   frame.  Returns REG_NO_CORRESPONDENCES (and stores the value all the same) when the value is not finite. */
REG_API reg_status reg_host_partial_constraint(const double sums9[9], const float v[3], float* value);
/* reg_host_solve6_xicp with right-hand sides rhs[k] on the constraint rows of the directions with flags[k] == 0; all of
   them zero gives reg_host_solve6_xicp's bits.  Returns the rank of the reduced system. */
REG_API int  reg_host_solve6_xicp_rhs(const float A[36], const float b[6], const int32_t flags[6], const float rhs[6],
                                      float x[6]);

/* Launch plan of the persistent tail kernel (csrc/kernels_tail.hpp) for a reading of n points on a device with `cus`
   compute units: plan = {usable (0/1), workgroups, workgroups per XCD class, reading points per XCD class}.  Octet
   oc = (s >> 3) * plan[2] + (b >> 3) of XCD class x = b & 7 is, with tile == 0, octet oc of the class's contiguous share
   (reading point x * plan[3] + 8 * oc + (s & 7)); with tile > 0 the classes take turns in tiles of `tile` octets: reading point
   8 * (((oc / tile) * 8 + x) * tile + oc % tile) + (s & 7).  Valid when 8 * oc + (s & 7) < plan[3] and the point lies below n
   (1024 slots per workgroup).  Host-only: lets the slot <-> point mapping be checked on CPU. */
REG_API void reg_host_tail_plan(int64_t n, int32_t cus, int32_t tile, int32_t plan[4]);

/* Measurement hook (bench.py roofline object): average device time in ms, by HIP events on the handle's
   stream, of [0] the match kernel, [1] the trimmed-quantile select passes, [2] linearize + final reduce. */
REG_API reg_status reg_profile_kernels(reg_handle* h, const float T_iter[16], int reps, float ms[3]);

/* ---- next row: surface normals / covariances by exact k-NN + PCA ------------------------------
   Replaces the CPU producers of the attributes the registration consumes:
     libpointmatcher/pointmatcher/DataPointsFilters/SurfaceNormal.cpp:152-252  (SurfaceNormalDataPointsFilter:
       self k-NN including the point itself, mean, C = NN NN^T, eigenvector of the smallest eigenvalue, clamped to
       [-1,1]; a neighbourhood of rank < 2 yields the zero vector),
     open3d_slam/src/CloudRegistration.cpp:25-43  (estimateNormals(KDTreeSearchParamKNN) +
       OrientNormalsTowardsCameraLocation before every point-to-plane registration),
     open3d_slam/src/helpers.cpp:153-165           (the same with a radius cap).
   xyz: n points, stride in floats.  k in [1,32] neighbours (the point itself counts), max_dist > 0 (may be +inf).
   viewpoint: NULL -> sign such that the largest component is positive; else normals face the viewpoint.
   Outputs (host pointers, or device pointers when on_device != 0), indexed like the input; every member but `normals`
   may be NULL (the names in brackets are the filter's keep* switches / descriptor names, SurfaceNormal.h:71-77):
     normals    n x 3                                                   [keepNormals, "normals"]
     eigvals    n x 3 ascending                                          [keepEigenValues + sortEigen, "eigValues"]
     eigvecs    n x 9: eigenvector k (ascending eigenvalue) at [9 i + 3 k + r]   [keepEigenVectors, "eigVectors"]
     covs       n x 6 {xx xy xz yy yz zz}: C/m, or with regularise != 0 the plane-like GICP covariance
                V diag(1e-3,1,1) V^T (small_gicp / Open3D GICP convention)
     densities  n: m / (4/3 pi r^3), r = largest distance of a neighbour from the neighbourhood mean (utils.h:106-128);
                0 for a degenerate neighbourhood                        [keepDensities, "densities"]
     mean_dists n: |p - mean| (SurfaceNormal.cpp:243-252); (float)SIZE_MAX when degenerate   [keepMeanDist, "meanDists"]
     ids        n x k neighbour indices ascending by (d2, index), -1 padded   [keepMatchedIds, "matchedIds"]
   n_rescanned (may be NULL): points whose candidate list exceeded the on-chip list (statistics; results are exact). */
typedef struct {
    float*   normals;
    float*   eigvals;
    float*   eigvecs;
    float*   covs;
    float*   densities;
    float*   mean_dists;
    int32_t* ids;
} reg_normals_out;
REG_API reg_status reg_estimate_normals(reg_handle* h, const float* xyz, int64_t xyz_stride, int64_t n, int on_device,
                                        int k, float max_dist, const float viewpoint[3], int regularise,
                                        const reg_normals_out* out, int64_t* n_rescanned);


/* SurfaceNormalDataPointsFilter's `smoothNormals` option (SurfaceNormal.cpp:259-283): every normal becomes the mean of its
   neighbours' normals (those pointing away from it flipped), IN PLACE in index order as the reference does it -- point i
   reads the already smoothed normals of its lower-indexed neighbours.  normals: n x 3 in / out; ids: n x k as
   reg_estimate_normals reports them (-1 = no neighbour).  Evaluated on the device as a level-synchronous sweep over the
   dependency DAG, bit-identical to the sequential loop; n_passes (may be NULL): sweeps launched. */
REG_API reg_status reg_smooth_normals(reg_handle* h, float* normals, const int32_t* ids, int64_t n, int k, int on_device,
                                      int32_t* n_passes);

/* ---- next row: target-side preparation on the device ------------------------------------------
   Replaces, in front of reg_set_target, what the mapper does on the host every referenceCloudSettingPeriod_:
     open3d_slam/src/ScanToMapRegistration.cpp:90-96   cropSubmap: scanMatcherCropper_->setPose(mapToRangeSensor); crop(map)
     open3d_slam/src/croppers.cpp:76-106               CroppingVolume::crop: order-preserving copy of the points (+ normals,
                                                       covariances) with isWithinVolume(p)
     open3d_slam/src/croppers.cpp:118-170              the volumes: MaxRadius |p-t| <= r; MinRadius |p-t| >= r; MinMaxRadius;
                                                       Cylinder z in [minZ,maxZ] (absolute) and |(p-t).xy| <= r; all in double
     open3d_utils/open3d_conversions/src/open3d_conversions.cpp:57-118  open3dToPointmatcher: fp64 AoS -> fp32 features / normals
       ("This is time consuming", Mapper.cpp:336)
   xyz / normals: m x 3 doubles (std::vector<Eigen::Vector3d>::data()); covs: m x 9 doubles (Matrix3d, symmetric) or NULL.
   The kept points keep their order; correspondence ids reported later index the CROPPED cloud (as in the reference,
   whose matcher only ever sees the patch); reg_get_target_source_indices maps them back. */
typedef enum {
    REG_CROP_NONE = 0, REG_CROP_MAX_RADIUS = 1, REG_CROP_MIN_RADIUS = 2, REG_CROP_MIN_MAX_RADIUS = 3, REG_CROP_CYLINDER = 4
} reg_crop_type;
typedef struct {
    int32_t type;          /* reg_crop_type */
    int32_t reserved;
    double  center[3];     /* pose_.translation() of the cropper (mapToRangeSensor) */
    double  radius_min;    /* MinRadius / MinMaxRadius */
    double  radius_max;    /* MaxRadius / MinMaxRadius / Cylinder radius */
    double  min_z, max_z;  /* Cylinder */
} reg_crop;
REG_API reg_status reg_set_target_f64(reg_handle* h, const double* xyz, const double* normals, const double* covs,
                                      int64_t m, int on_device, const reg_crop* crop, int64_t* n_kept);
/* idx[n_kept]: position of every kept point in the cloud given to reg_set_target_f64 */
REG_API reg_status reg_get_target_source_indices(reg_handle* h, int32_t* idx);

/* Map maintenance half of the same row: voxelizeWithinCroppingVolume (open3d_slam/src/helpers.cpp:117-192), which
   Submap::insertScan runs on the whole map after every inserted scan (Submap.cpp:39-96).  Points outside `volume` are
   copied through in their order; points inside are bucketed by voxel index floor(p * (1/voxel_size)) per axis
   (VoxelHashMap.hpp:48-51) and replaced by one averaged point per occupied voxel: sums in double in index order
   (AccumulatedPoint, helpers.cpp:30-72: NaN normals are skipped, the averaged normal is re-normalised, covariances are
   averaged).  The reference emits the voxels in std::unordered_map order (unspecified); here they follow the outside
   points in ascending (z, y, x) voxel index.  Inputs / outputs: m x 3 (x 9 for covs) doubles, host or device
   (on_device); the output arrays must hold m points.  voxel_size <= 0 copies the cloud through. */
REG_API reg_status reg_voxelize_within_volume(reg_handle* h, const double* xyz, const double* normals, const double* covs,
                                              int64_t m, int on_device, const reg_crop* volume, double voxel_size,
                                              double* out_xyz, double* out_normals, double* out_covs, int64_t* n_out,
                                              int64_t* n_outside);

/* Space carving (open3d_slam/src/Submap.cpp:130-143 -> helpers.cpp:238-283, getIdxsOfCarvedPoints): every scan point
   (already in the map frame) casts a ray from the sensor; the ray is sampled every `voxel_size` up to
   max(voxel_size, min(|p - sensor| - truncation, max_ray)); map points that share a voxel (floor(p * (1/voxel_size)),
   VoxelHashMap.hpp:43-51) with a sample are removed when |direction . normalized(normal)| > min_dot (always, without
   normals).  Only map points inside `subset` (the map builder's cropper, may be NULL = all) take part.  All in double,
   one rounding per operation.  removed[]: ascending map indices (the reference returns them in std::unordered_set
   order), capacity m.  Rays of zero length are skipped (the reference divides by zero there). */
REG_API reg_status reg_carve_indices(reg_handle* h, const double* map_xyz, const double* map_normals, int64_t m,
                                     const double* scan_xyz, int64_t n_scan, int on_device, const double sensor[3],
                                     const reg_crop* subset, double voxel_size, double max_ray, double truncation,
                                     double min_dot, int32_t* removed, int64_t* n_removed);

/* B1 result extra: the 6x6 information matrix of a registered pair, as the loop-closure and odometry
   constraint builders obtain it from open3d::pipelines::registration::GetInformationMatrixFromPointClouds
   (open3d_slam/src/constraint_builders.cpp:69-73, PlaceRecognition.cpp:148; arithmetic in un-vendored Open3D 0.15.1:
   PARITY UNPINNED, restated): for every reading point whose nearest reference point q (reference frame) lies within
   max_dist after applying T, G = [[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]] with (x, y, z) = q and
   info = sum G^T G (rotation-first ordering, row-major 6x6, float64).  max_dist must not exceed the handle's max_dist
   (the reach of the search structure).  Uses the reference and reading currently set; a prepared reading is
   re-prepared at T. */
REG_API reg_status reg_information_matrix(reg_handle* h, const float T[16], float max_dist, double info[36],
                                         int64_t* n_pairs);

/* ---- voxel-overlap selection and the submap-pair front of the constraint builders -----
   Every pose-graph constraint between two submaps starts with the same chain (open3d_slam/src/constraint_builders.cpp:43-90,
   PlaceRecognition.cpp:97-149): computeIndicesOfOverlappingPoints (helpers.cpp:320-345), SelectByIndex on both clouds,
   one registration, GetInformationMatrixFromPointClouds on the reduced clouds.  These entry points are the first two
   steps; reg_register and reg_information_matrix are the other two.

   Numeric contract: fp64, one rounding per operation (the build forbids contraction).
     transformed source point, T with rows r0..r3 (helpers.cpp:302-303: T * (x, y, z, 1), head<3>() / w):
         w  = ((T30*x + T31*y) + T32*z) + T33
         x' = (((T00*x + T01*y) + T02*z) + T03) / w          (y', z' alike)
       The reference transforms with Open3D's own PointCloud::Transform, which is not in the reference tree: PARITY of this
       line is UNPINNED; the formula above is that of the tree's own transform helper.  T_src_to_tgt == NULL is identity
       and runs no transform pass; identity through the formula reproduces finite inputs exactly, so the two agree.
       T_src_to_tgt: const double[16], column-major (Eigen::Matrix4d::data()).
     voxel key, per axis: floor(p * (1.0 / voxel_size)) (VoxelHashMap.hpp:43-51), the key of reg_voxelize_within_volume and
       reg_carve_indices; 21 bits per axis, offset binary.
     invalid keys: a non-finite coordinate or a voxel index outside +-2^20, in the target or in the transformed source,
       returns REG_BAD_ARGUMENT (the reference casts to int there: undefined behaviour).
     selected voxels: at least min_points_per_voxel points of the target AND of the transformed source;
       min_points_per_voxel >= 1 or REG_BAD_ARGUMENT (assert_ge, helpers.cpp:323).
     result: every point of either cloud that lies in a selected voxel.  Source indices refer to the untransformed source.
       Both lists ascend (the reference emits them in std::unordered_map order, which is unspecified; as reg_carve_indices).
   Common rules: on_device covers all cloud arrays of a call (and the index outputs of reg_overlap_indices);
   n, m <= 2^31 - 1; voxel_size <= 0 or non-finite returns REG_BAD_ARGUMENT.

   reg_overlap_indices: the index query.  n == 0 or m == 0, or clouds that share no voxel, return REG_OK with both counts 0. */
REG_API reg_status reg_overlap_indices(reg_handle* h, const double* src_xyz, int64_t n, const double* tgt_xyz, int64_t m,
                                       int on_device, const double T_src_to_tgt[16] /* NULL: identity */, double voxel_size,
                                       int32_t min_points_per_voxel, int32_t* src_idx /* capacity n */, int64_t* n_src,
                                       int32_t* tgt_idx /* capacity m */, int64_t* n_tgt);
/* reg_set_pair_overlap_f64: the whole front of buildConstraint in one call, both clouds on the device throughout: overlap
   flags, order-preserving compaction with the fp64 -> fp32 cast of reg_set_target_f64 (normals m x 3, covs m x 9 doubles,
   may be NULL), the search table on the selected target (as reg_set_target), the selected source as the reading (as
   reg_set_source).  Field requirements are those of reg_set_target / reg_set_source for the handle's cost
   (REG_MISSING_FIELD).  An empty overlap -- an empty cloud included -- returns REG_EMPTY_TARGET, as an empty crop does, and
   leaves the handle without reference and reading.  reg_get_target_source_indices maps reference ids back to tgt_xyz,
   reg_get_source_source_indices reading indices to src_xyz (idx[n_src_kept]); after a plain reg_set_source* the latter
   fails with REG_NOT_CONFIGURED, as the former does after a plain reg_set_target. */
REG_API reg_status reg_set_pair_overlap_f64(reg_handle* h, const double* src_xyz, const double* src_normals,
                                            const double* src_covs, int64_t n, const double* tgt_xyz, const double* tgt_normals,
                                            const double* tgt_covs, int64_t m, int on_device, const double T_src_to_tgt[16],
                                            double voxel_size, int32_t min_points_per_voxel, int64_t* n_src_kept,
                                            int64_t* n_tgt_kept);
REG_API reg_status reg_get_source_source_indices(reg_handle* h, int32_t* idx);

/* ---- FPFH features and mutual feature matching: the front of place recognition ---------------------
   open3d_slam/src/Submap.cpp:255-275 (Submap::computeFeatures: ComputeFPFHFeature(sparseMapCloud_,
   KDTreeSearchParamHybrid(featureRadius_, featureKnn_))) and the first step of
   RegistrationRANSACBasedOnFeatureMatching(..., mutual_filter = true, ...) (PlaceRecognition.cpp:71-85).  Open3D 0.15.1
   is not in the reference tree: PARITY UNPINNED; the contract below is this project's own.

   reg_compute_fpfh.  xyz / normals: n points, strides in floats (>= 3); host pointers, or device pointers with
   on_device != 0 (which covers fpfh, spfh and n_neighbours too).  2 <= max_nn <= 128, radius finite and > 0,
   n <= 2^31 - 1 (else REG_BAD_ARGUMENT); n <= 0 is REG_EMPTY_SOURCE; a non-finite coordinate or normal component is
   REG_BAD_ARGUMENT.  Outputs are fp64 (Feature::data_ is a double matrix; row i here is its column i): fpfh n x 33,
   spfh n x 33 (may be NULL), n_neighbours n (m_i below, may be NULL); n_rescanned (may be NULL): points whose candidate
   list exceeded the on-chip list (statistics; results are exact).

   Numeric contract: one rounding per operation (the build forbids contraction).
     neighbourhood of point i: the up to max_nn nearest points within radius, point i included in the count (FLANN's
       hybrid search), formed on the fp32 coordinates with d2 = (dx*dx + dy*dy) + dz*dz, the test d2 <= fl(radius*radius)
       and ascending (d2, index) order -- the order reg_estimate_normals reports.  Point i is then dropped BY INDEX
       (deviation: Open3D drops whatever comes first, with duplicated points possibly the twin); m_i neighbours remain.
     pair feature of (i, j), fp64 on the promoted fp32 values; a.b = (a.x*b.x + a.y*b.y) + a.z*b.z,
       (a x b).x = a.y*b.z - a.z*b.y etc.:
         d = p_j - p_i, L = sqrt(d.d); L == 0: (f0, f1, f2) = (0, 0, 0)
         a1 = (n_i.d)/L, a2 = (n_j.d)/L
         |a1| < |a2|: n1 = n_j, n2 = n_i, d = -d, f2 = -a2; otherwise (a tie included) n1 = n_i, n2 = n_j, f2 = a1
           (deviation: Open3D tests acos(|a1|) > acos(|a2|), which agrees except within acos' own rounding)
         v = d x n1, vn = sqrt(v.v); vn == 0: (0, 0, 0); v = v/vn
         w = n1 x v, f1 = v.n2, f0 = atan2(w.n2, n1.n2)
       Normals are used as given (FPFH does not normalise them).
     bins: floor((11*(f0 + pi))/(2*pi)), floor((11*(f1 + 1))*0.5), floor((11*(f2 + 1))*0.5), each clamped to [0, 10],
       counted in rows 0-10, 11-21, 22-32.
     spfh[i][b] = count_i[b] * (100.0 / m_i) (integer counts, one multiplication); all zero when m_i == 0.
     fpfh: acc[b] = sum over the neighbours j in ascending (d2, index) order of spfh[j][b] / d2_ij, d2_ij the fp64 d.d
       above (the SQUARED distance, Open3D's own weight), neighbours with d2_ij == 0 skipped; s_t = the eleven acc of
       sub-histogram t added in bin order; scale_t = 100.0 / s_t (0 when s_t == 0);
       fpfh[i][b] = acc[b] * scale_t + spfh[i][b]. */
REG_API reg_status reg_compute_fpfh(reg_handle* h, const float* xyz, int64_t xyz_stride, const float* normals,
                                    int64_t nrm_stride, int64_t n, int on_device, int max_nn, float radius,
                                    double* fpfh /* n x 33 */, double* spfh /* n x 33, may be NULL */,
                                    int32_t* n_neighbours /* n, may be NULL */, int64_t* n_rescanned /* may be NULL */);

/* reg_match_features: nearest neighbours between two sets of feature rows (na x dim, nb x dim doubles, 1 <= dim <= 64;
   on_device covers fa, fb, nn_ab, nn_ba and mutual).  D(a, b) = sum_j (fa[a][j] - fb[b][j])^2 in fp64, j ascending, one
   rounding per operation.  nn_ab[a] is the b of the smallest D, ties to the lowest b; nn_ba alike (may be NULL).
   mutual (may be NULL; interleaved (a, b) pairs, capacity na pairs): the pairs (a, nn_ab[a]) with nn_ba[nn_ab[a]] == a,
   ascending in a -- corres_mutual of Open3D's feature-matching front, the input of
   RegistrationRANSACBasedOnCorrespondence; *n_mutual their number (required with mutual).  With nn_ba and mutual both
   NULL only the forward search runs.  na <= 0: REG_EMPTY_SOURCE, nb <= 0: REG_EMPTY_TARGET. */
REG_API reg_status reg_match_features(reg_handle* h, const double* fa, int64_t na, const double* fb, int64_t nb, int dim,
                                      int on_device, int32_t* nn_ab /* na */, int32_t* nn_ba /* nb, may be NULL */,
                                      int32_t* mutual /* 2 x capacity na: (a, b) pairs */, int64_t* n_mutual);

/* ---- RANSAC registration on correspondences: the hypothesis loop of place recognition ----------------
   RegistrationRANSACBasedOnCorrespondence, the second half of RegistrationRANSACBasedOnFeatureMatching
   (PlaceRecognition.cpp:78-91), between reg_match_features and reg_set_pair_overlap_f64.  Open3D 0.15.1 is not in the
   reference tree: PARITY UNPINNED; the contract below is this project's own.

   src_xyz n x 3, tgt_xyz m x 3 doubles; corres: k interleaved int32 pairs (a, b); on_device covers the clouds, corres,
   inliers and iter_status.  params and result are host structs with struct_size set by the caller.
   Returns: REG_BAD_ARGUMENT for a NULL params / result or a wrong struct_size, ransac_n outside [3, 8], max_iteration < 1,
   confidence outside [0, 1], max_correspondence_distance not finite or <= 0, a NaN threshold, batch outside [0, 2^20],
   n, m or k > 2^31 - 1; then REG_EMPTY_SOURCE for k <= 0; then REG_BAD_ARGUMENT for a NULL src_xyz, tgt_xyz, corres or
   inliers or an empty cloud; then REG_OK with the default result (identity, zeros, best_iteration -1) for k < ransac_n,
   as Open3D (the indices are not looked at); then REG_BAD_ARGUMENT for an index outside [0, n) / [0, m) (checked on
   the device).  A valid run returns REG_OK even if nothing qualified.

   Numeric contract: fp64, one rounding per operation (the build forbids contraction); |d|^2 = (dx*dx + dy*dy) + dz*dz.
     sampling, with replacement as Open3D, counter based: slot j of iteration i draws, all mod 2^64,
         ctr = i*ransac_n + j;  z = seed + (ctr + 1)*0x9E3779B97F4A7C15;  z = (z ^ z>>30)*0xBF58476D1CE4E5B9;
         z = (z ^ z>>27)*0x94D049BB133111EB;  z ^= z>>31;  index = ((z >> 32)*k) >> 32
       and s_j / t_j are the source / target point of correspondence `index`.
     status of iteration i, the first rule that fails:
       -1  two slots drew the same correspondence (deviation: Open3D goes on with a rank-deficient sample)
       -2  edge-length checker (edge_similarity > 0): for some slots u < v, ds = |s_u - s_v|, dt = |t_u - t_v| (sqrt of the
           form above): ds < dt*sim or dt < ds*sim.  It needs no transform and runs before the fit; the outcome is that
           of Open3D's order.
       -3  degenerate fit: sigma_2 <= 1e-12*sigma_1.  The fit is TransformationEstimationPointToPoint(false) (umeyama
           without scale): sm, tm = (slot sums in slot order)/ransac_n, H = sum_j (s_j - sm)(t_j - tm)^T = U S V^T,
           R = V diag(1, 1, det(V U^T)) U^T, t = tm - R sm.  The SVD method is not part of the contract.
       -4  distance checker (distance_threshold > 0): some slot has |R s_j + t - t_j|^2 > fl(threshold*threshold), with
           (R s + t).x = ((R00*s.x + R01*s.y) + R02*s.z) + t.x (y, z alike).
       >= 0  the inlier count over all k correspondences (EvaluateRANSACBasedOnCorrespondence): correspondence (a, b) is
           an inlier iff d2 = |R s_a + t - t_b|^2 < fl(maxd*maxd) (deviation: Open3D tests sqrt(d2) < maxd).
           err2 = sum of d2 over the inliers: ascending k inside chunks of REG_RANSAC_CHUNK correspondences, each from 0,
           then the chunk sums added in ascending chunk order.
     best hypothesis, sequential semantics (deviation: Open3D's OpenMP loop is not deterministic), i = 0, 1, ...:
       a hypothesis with count > 0 replaces the best iff count > best.count, or count == best.count and err2 < best.err2
       (a tie keeps the earlier one); after each replacement
           x = log(1 - confidence) / log(1 - pow(count/k, ransac_n));   est_k = min(est_k, trunc(x)) when x >= 0
       on the host in libm (reg_host_ransac_est_k), est_k = max_iteration at the start.  An x that is not >= 0 changes
       nothing: NaN (-inf / -inf: confidence 1 with count == k) and -inf (pow(count/k, ransac_n) < 2^-53, so that the
       denominator is log(1) = +0; deviation from the IEEE quotient, which would end the loop where it knows least).  So
       confidence 1 never stops early and count == k gives est_k = 0.  The loop ends at the first i >= est_k: the stop
       index, max_iteration at the latest.  The device evaluates iterations in batches (params.batch, 0: the default);
       iterations past the stop index are wasted work and change nothing: the result does not depend on batch.
     result: T column-major (identity when nothing qualified), fitness = count/k, inlier_rmse = sqrt(err2/count),
       n_inliers and the inlier pairs of T in ascending k, n_iterations = the stop index, n_validated = iterations before
       it with status >= 0, best_iteration (-1: none), batch = the batch size that was used.  iter_status (may be NULL;
       max_iteration words): the status of every i < stop index; untouched beyond. */
#define REG_RANSAC_CHUNK 1024
typedef struct {
    int32_t  struct_size;                   /* sizeof(reg_ransac_params) */
    int32_t  ransac_n;                      /* 3 .. 8 */
    int64_t  max_iteration;                 /* >= 1 */
    double   confidence;                    /* 0 .. 1 */
    double   max_correspondence_distance;   /* finite, > 0 */
    double   distance_threshold;            /* CorrespondenceCheckerBasedOnDistance; <= 0: off */
    double   edge_similarity;               /* CorrespondenceCheckerBasedOnEdgeLength; <= 0: off */
    uint64_t seed;
    int32_t  batch;                         /* iterations per device batch; 0: the default */
    int32_t  reserved;
} reg_ransac_params;
typedef struct {
    int32_t struct_size;                    /* sizeof(reg_ransac_result), set by the caller */
    int32_t batch;                          /* iterations per device batch that were used (statistics; 0: no batch ran) */
    double  T[16];                          /* column-major */
    double  fitness;
    double  inlier_rmse;
    int64_t n_inliers;
    int64_t n_iterations;
    int64_t n_validated;
    int64_t best_iteration;
} reg_ransac_result;
REG_API reg_status reg_ransac_correspondences(reg_handle* h, const double* src_xyz, int64_t n, const double* tgt_xyz, int64_t m,
                                              const int32_t* corres /* 2 x k */, int64_t k, int on_device,
                                              const reg_ransac_params* params, reg_ransac_result* result,
                                              int32_t* inliers /* 2 x capacity k */,
                                              int32_t* iter_status /* max_iteration, may be NULL */);
/* The stop rule above, host-only: est_k after a replacement by a hypothesis with `count` inliers of k. */
REG_API double reg_host_ransac_est_k(double est_k, double confidence, int64_t count, int64_t k, int32_t ransac_n);

/* ---- the scan front end: VoxelDownSample, RandomDownSample, processForScanMatchingAndMerging ----------
   ScanToMapIcp::processForScanMatchingAndMerging (open3d_slam/src/ScanToMapRegistration.cpp:36-69, called at
   Mapper.cpp:186,287; LidarOdometry::preprocess, Odometry.cpp:22-27, runs the same chain): wide crop, VoxelDownSample,
   estimateNormalsOrCovariancesIfNeeded, RandomDownSample, narrow crop, open3dToPointmatcher.  Open3D 0.15.1 is not in the
   reference tree: PARITY UNPINNED; the contracts below are this project's own, restated from Open3D's published semantics
   and the tree's own copy of the accumulator (helpers.cpp:30-72).
   Clouds are Open3D's fp64 arrays: points_ / normals_ n x 3, covariances_ n x 9 doubles; normals and covs may be NULL;
   on_device covers every array of a call, outputs included.  fp64, one rounding per operation, no contraction.

   reg_voxel_down_sample == PointCloud::VoxelDownSample(voxel_size).
     origin, per axis: min_bound - 0.5*voxel_size, min_bound the exact fp64 minimum over the points.
     voxel index, per axis: floor((p - origin) / voxel_size) -- a true division -- non-negative, 21 bits per axis.
     one output point per occupied voxel, sums in double in ascending input index: points averaged; a normal with a NaN
       component is skipped while its point still counts, the averaged normal is sum / count and NOT re-normalised
       (Open3D's GetAverageNormal; reg_voxelize_within_volume re-normalises, as voxelizeWithinCroppingVolume does);
       covariances averaged.
     output order: ascending (z, y, x) voxel index (Open3D emits std::unordered_map order; as reg_voxelize_within_volume).
     voxel_size <= 0 or non-finite: REG_BAD_ARGUMENT (Open3D raises); a non-finite coordinate or an index >= 2^21:
     REG_BAD_ARGUMENT; n == 0: REG_OK with *n_out = 0.  The output arrays hold n rows. */
REG_API reg_status reg_voxel_down_sample(reg_handle* h, const double* xyz, const double* normals, const double* covs,
                                         int64_t n, int on_device, double voxel_size, double* out_xyz, double* out_normals,
                                         double* out_covs, int64_t* n_out);
/* reg_random_down_sample == PointCloud::RandomDownSample(ratio) under a determinism contract (Open3D shuffles with an
   mt19937 seeded from std::random_device and keeps the first (int)(ratio n) indices; deviation: counter based, as
   reg_ransac_correspondences).
     count = (int64)(ratio * (double)n): the fp64 product, truncated.
     key(i) = the 64-bit z of the sampler of reg_ransac_correspondences for ctr = i and `seed`, before its range reduction
       (reg_host_scan_key).
     kept: the count smallest (key, index) pairs, emitted in ascending index order with their normals and covariances.
   The result is a function of (n, ratio, seed) only.  ratio == 1 copies through; ratio outside [0, 1] or non-finite:
   REG_BAD_ARGUMENT.  out_idx (int32, ascending, may be NULL) and the out arrays hold count rows; xyz may be NULL when
   only the indices are wanted. */
REG_API reg_status reg_random_down_sample(reg_handle* h, const double* xyz, const double* normals, const double* covs,
                                          int64_t n, int on_device, double ratio, uint64_t seed, int32_t* out_idx,
                                          double* out_xyz, double* out_normals, double* out_covs, int64_t* n_out);
/* key(i) above, on the host: the same code as the device. */
REG_API uint64_t reg_host_scan_key(uint64_t seed, uint64_t index);

/* reg_process_scan: the whole front end in one call, on the device throughout, in the reference's order:
     1. wide crop (mapBuilderCropper_), order-preserving;
     2. reg_voxel_down_sample (voxel_size <= 0 skips the stage, helpers.cpp:108-111);
     3. a cloud without normals and normal_knn > 0: reg_estimate_normals on the fp32 cast of the voxelised cloud with
        k = normal_knn, max_dist = (float)normal_radius, the viewpoint at the origin; the normals are widened to fp64; a
        REG_COST_GICP handle also takes the regularise = 1 covariances of the same pass (unless the cloud brings its own).
        A cloud that arrives with normals skips the stage (CloudRegistration.cpp:27,64);
     4. reg_random_down_sample with `seed` (skipped when down_sampling_ratio >= 1, helpers.cpp:100-103);
     5. the result is the merge cloud (merge_): written to merge_xyz / merge_normals / merge_covs (n rows each; the two
        latter may be NULL), so that reg_carve_indices and reg_voxelize_within_volume can take device pointers directly;
     6. narrow crop (scanMatcherCropper_ at the identity pose) of the merge cloud, cast per coordinate as
        reg_set_source_f64 casts, installed as the handle's reading (match_ + open3dToPointmatcher);
        reg_get_source_source_indices then maps reading rows to merge-cloud rows.
   Statuses: REG_BAD_ARGUMENT for a bad struct_size, crop type, non-finite voxel_size, ratio < 0 or non-finite, normal_knn
   outside [0, 32], normal_radius <= 0 with normal_knn > 0; REG_EMPTY_SOURCE for an empty cloud or one that is empty after
   the wide or the narrow crop (the reference asserts, ScanToMapRegistration.cpp:66-67) -- no reading is set;
   REG_MISSING_FIELD when the handle's cost needs normals / covariances that the cloud neither brings nor gets estimated
   (normal_knn == 0), GICP with given normals and no covariances included.  Every failure leaves the handle without reading. */
typedef struct {
    int32_t  struct_size;          /* = sizeof(reg_scan_params); checked */
    int32_t  reserved;
    reg_crop wide;                 /* mapBuilderCropper_ */
    reg_crop narrow;               /* scanMatcherCropper_ at the identity pose */
    double   voxel_size;           /* scanProcessing_.voxelSize_; <= 0 skips the stage */
    double   down_sampling_ratio;  /* scanProcessing_.downSamplingRatio_; >= 1 skips the stage */
    uint64_t seed;
    int32_t  normal_knn;           /* icp_.knn_; 0: no estimation */
    int32_t  reserved2;
    double   normal_radius;        /* icp_.maxDistanceKnn_ */
} reg_scan_params;
typedef struct {
    int32_t struct_size;           /* = sizeof(reg_scan_result), set by the caller */
    int32_t has_normals;           /* the merge cloud carries normals (given or estimated) */
    int32_t has_covs;
    float   scan_prep_ms;          /* the whole call on the handle's stream (HIP events), uploads and read-backs included */
    int64_t n_wide;                /* points after the wide crop */
    int64_t n_voxels;              /* ... after the voxel grid */
    int64_t n_merge;               /* ... after the random selection: rows of the merge cloud */
    int64_t n_match;               /* rows of the reading */
} reg_scan_result;
/* param/default/parameter_structure_definitions.lua as shipped: MinMaxRadius 2 / 100 for both croppers, voxel 0.01,
   ratio 1, knn 20 within 1 m; seed 0. */
REG_API void reg_default_scan_params(reg_scan_params* p);
REG_API reg_status reg_process_scan(reg_handle* h, const double* xyz, const double* normals, const double* covs, int64_t n,
                                    int on_device, const reg_scan_params* params, double* merge_xyz, double* merge_normals,
                                    double* merge_covs, reg_scan_result* result);

/* Introspection of the search structure (tests, DESIGN.md numbers). */
typedef struct {
    int64_t n_points;
    int64_t n_bricks;
    int64_t n_cells_occupied;
    int64_t table_bytes;
    float   cell_size;
    float   origin[3];
    float   centroid[3];
    int32_t dims[3];
} reg_target_info;
REG_API reg_status reg_get_target_info(const reg_handle* h, reg_target_info* info);

/* ---- data-point filters on the device ----------------------------------------------------------
   SamplingSurfaceNormalDataPointsFilter (libpointmatcher DataPointsFilters/SamplingSurfaceNormal.cpp buildNew /
   fuseRange; parameter names and defaults of SamplingSurfaceNormal.h).  The cloud is split recursively: on the first
   strict argmax of the PROPAGATED box extents (utils.h argMax), by count (the left child gets count - count/2 points),
   the cut value (first point of the right half) bounding both children on that axis; a range of count <= knn is a leaf.
   A leaf whose actual extent exceeds max_box_dim is dropped; with keep_normals / keep_eigen_values / keep_eigen_vectors
   a leaf with rank(C) + 1 < 3 is dropped as well (rank rule of reg_estimate_normals).  Dropped points count in n_unfit.
   Determinism contract (libstdc++'s nth_element leaves ties and in-leaf order implementation-defined; these are the
   documented choices):
     - within a segment points are ordered by (coordinate on the cut axis, original index); -0.0 == +0.0;
       non-finite input is REG_BAD_ARGUMENT;
     - a leaf keeps the order the last split left; mean = sequential fp32 sum in that order / float(count);
       C = sum (q - mean)(q - mean)^T sequentially in fp32;
     - the kept index of a leaf is its SMALLEST original index; output rows are ascending by kept index;
     - eigenvalues ascending, normal = eigenvector of the smallest, sign as reg_estimate_normals with viewpoint NULL
       (largest component positive); densities = utils.h computeDensity.
   sampling_method 1: one row per fitted leaf holding the leaf mean.  sampling_method 0 with ratio >= 1: every point of
   every fitted leaf (its own xyz, the leaf's attributes).  sampling_method 0 with ratio < 1 draws from std::rand in
   the reference, a stream that cannot be reproduced: REG_UNSUPPORTED.  average_existing_descriptors is accepted and
   has no effect (the input carries no descriptors).  knn in [3, 64] (above: REG_UNSUPPORTED); n == 0 is
   REG_EMPTY_SOURCE. */
typedef struct {
    int32_t struct_size;                    /* sizeof(reg_ssn_params) */
    int32_t knn;                            /* 7 */
    int32_t sampling_method;                /* 0 */
    float   ratio;                          /* 0.5 */
    float   max_box_dim;                    /* +inf */
    int32_t average_existing_descriptors;   /* 1 (no effect) */
    int32_t keep_normals;                   /* 1 */
    int32_t keep_densities;                 /* 0 */
    int32_t keep_eigen_values;              /* 0 */
    int32_t keep_eigen_vectors;             /* 0 */
} reg_ssn_params;
REG_API void reg_default_ssn_params(reg_ssn_params* p);
/* Outputs (host pointers, or device pointers when on_device != 0), n rows of capacity each; only xyz is required.
     xyz        n_out x 3      normals  n_out x 3     densities n_out     eigvals n_out x 3 ascending
     eigvecs    n_out x 9      (eigenvector k at [9 i + 3 k + r], as reg_estimate_normals)
     src_idx    n_out          the kept input index of each row
     leaf_id    n (per INPUT point): index of its leaf in depth-first order, -1 for the points of dropped leaves */
typedef struct {
    float*   xyz;
    float*   normals;
    float*   densities;
    float*   eigvals;
    float*   eigvecs;
    int32_t* src_idx;
    int32_t* leaf_id;
} reg_ssn_out;
REG_API reg_status reg_sampling_surface_normal(reg_handle* h, const float* xyz, int64_t xyz_stride, int64_t n,
                                               int on_device, const reg_ssn_params* p, const reg_ssn_out* out,
                                               int64_t* n_out, int64_t* n_unfit);

/* Reading-side point filters, run as an ordered chain in one call (each filter's inPlaceFilter; defaults of its .h).
   Every filter is a predicate over the current cloud followed by an order-preserving compaction.  The norm is
   sqrtf((x*x + y*y) + z*z) in fp32 without contraction (Eigen's norm() may differ in the last ulp at a threshold).
     MAX_DIST        dim -1: |p| < |value|, else p[dim] < value              (MaxDist.cpp)
     MIN_DIST        dim -1: |p| > |value|, else p[dim] > value              (MinDist.cpp)
     BOUNDING_BOX    strict on all six bounds; remove_inside                 (BoundingBox.cpp)
     DISTANCE_LIMIT  remove_inside ? d > value : d < value, d as MAX_DIST    (DistanceLimit.cpp)
     REMOVE_NAN      drops points with a NaN coordinate; inf is kept        (RemoveNaN.cpp)
     MAX_QUANTILE_ON_AXIS  limit = exact order statistic int(float(m) * value) of p[dim] over the current m points;
                     keeps p[dim] < limit.  A NaN on that axis is REG_BAD_ARGUMENT (run REMOVE_NAN first).
     FIX_STEP_SAMPLING keeps positions phase, phase + step, ... of the current cloud; step = startStep (init() resets
                     it on every compute); the reference draws phase = rand() % step, here it is an argument (0..step-1)
     IDENTITY
   Inputs: xyz (stride in floats), nrm n x 3 and cov n x 6 (may be NULL) are carried along.  Outputs (capacity n rows):
   out_xyz m x 3, out_nrm / out_cov (when the input has them, may be NULL), out_idx m source indices (may be NULL). */
enum { REG_DPF_IDENTITY = 0, REG_DPF_MAX_DIST = 1, REG_DPF_MIN_DIST = 2, REG_DPF_BOUNDING_BOX = 3,
       REG_DPF_DISTANCE_LIMIT = 4, REG_DPF_REMOVE_NAN = 5, REG_DPF_MAX_QUANTILE_ON_AXIS = 6, REG_DPF_FIX_STEP_SAMPLING = 7 };
typedef struct {
    int32_t type;            /* REG_DPF_* */
    int32_t dim;             /* -1 (norm) or 0..2; MAX_QUANTILE_ON_AXIS: 0..2 */
    float   value;           /* maxDist / minDist / dist / ratio */
    int32_t remove_inside;   /* BOUNDING_BOX, DISTANCE_LIMIT */
    float   box[6];          /* xMin xMax yMin yMax zMin zMax */
    int32_t step;            /* FIX_STEP_SAMPLING: startStep >= 1 */
    int32_t phase;           /* FIX_STEP_SAMPLING: 0 <= phase < step */
} reg_point_filter;
REG_API reg_status reg_filter_points(reg_handle* h, const float* xyz, int64_t xyz_stride, const float* nrm,
                                     const float* cov, int64_t n, int on_device, const reg_point_filter* filters,
                                     int n_filters, float* out_xyz, float* out_nrm, float* out_cov, int32_t* out_idx,
                                     int64_t* n_out);

/* Descriptor-carrying filter chain (reg_filter_cloud): the cloud is xyz plus up to REG_MAX_FIELDS named descriptor
   fields, one n x span fp32 array each (the caller keeps the names; `normals` is a field of span 3, `covariances` of
   span 6, and so on).  A field with in == NULL does not exist until a filter of the chain creates it; a field with
   out == NULL is carried but not returned.  Every compaction carries every field; a field that never came to exist
   leaves its `out` untouched.  filters[] embeds reg_point_filter (`base`), so the eight filters above run unchanged in
   the same call; base.type also takes the descriptor filters below.  field_a / field_b / field_out index fields[]
   (-1: none).  A filter that reads a field which does not exist at its place in the chain returns REG_MISSING_FIELD
   (the reference throws InvalidField); an index outside [-1, n_fields) or a span that does not fit is REG_BAD_ARGUMENT.
   All arithmetic in fp32 without contraction: norm(v) = sqrtf((x*x + y*y) + z*z), dot(a, b) = (a0*b0 + a1*b1) + a2*b2,
   normalized(v) = v / norm(v) per component when norm(v) > 0, else v (Eigen's normalized()).
     OBSERVATION_DIRECTION  field_out (span 3) = v - p, v = the sensor centre {x, y, z}     (ObservationDirection.cpp:61-88)
     ORIENT_NORMALS         field_a (normals, span 3) is negated where dot(field_b, field_a) < 0 (flag = towardCenter 1)
                            or > 0 (flag 0); field_b = observationDirections (span 3)       (OrientNormals.cpp:60-96)
     SHADOW                 keeps |dot(normalized(field_a), normalized(p))| > v[0]; v[0] is sin(eps), computed by the
                            caller; field_a = normals (span 3)                              (Shadow.cpp:62-94)
     SIMPLE_SENSOR_NOISE    field_out (span 1); flag = sensorType: 0, 1, 2, 4: max(minRadius, beamAngle * norm(p) +
                            beamConst) with the fp32 constants of SimpleSensorNoise.cpp:87-113; 3: (norm(p) * norm(p)) *
                            float(0.5 * 0.00285).  v[0] = gain is accepted and unused, as in the reference.  flag outside
                            0..4 is REG_BAD_ARGUMENT                                        (SimpleSensorNoise.cpp:80-136)
     INCIDENCE_ANGLE        field_out (span 1) = acosf(dot(normalized(field_b), field_a)); field_a = normals, field_b =
                            observationDirections (both span 3)                             (IncidenceAngle.cpp:50-74)
     CUT_AT_DESCRIPTOR_THRESHOLD  keeps column 0 of field_a <= v[0] (flag = useLargerThan 1) or >= v[0] (flag 0)
                                                                                            (CutAtDescriptorThreshold.cpp:62-101)
     MAX_DENSITY            field_a = densities (column 0 of a field of any span), v[0] = maxDensity > 0.  last = the largest density of the
                            current cloud, nSat = how many points equal it.  A point with density <= maxDensity is kept.
                            Any other point consumes one draw r = float(rand()) / float(RAND_MAX), in cloud order, and is
                            kept when r < a, a = maxDensity / density, multiplied by float(1 - nSat / nPoints) (integer
                            division, as written there) when density == last.  Deviation: the reference continues the
                            process-wide std::rand stream; here every call replays glibc's rand() after srand(seed)
                            (seed 1 by default in the bindings)                              (MaxDensity.cpp:59-105) */
enum { REG_MAX_FIELDS = 16 };
enum { REG_DPF_OBSERVATION_DIRECTION = 8, REG_DPF_ORIENT_NORMALS = 9, REG_DPF_SHADOW = 10,
       REG_DPF_SIMPLE_SENSOR_NOISE = 11, REG_DPF_INCIDENCE_ANGLE = 12, REG_DPF_CUT_AT_DESCRIPTOR_THRESHOLD = 13,
       REG_DPF_MAX_DENSITY = 14 };
typedef struct {
    const float* in;         /* n x span, NULL: created by a filter of the chain */
    float*       out;        /* capacity n x span, NULL: not returned */
    int32_t      span;       /* 1..16 */
    int32_t      reserved;   /* must be 0 */
} reg_field;
typedef struct {
    int32_t  struct_size;    /* sizeof(reg_cloud_filter) */
    reg_point_filter base;   /* base.type: any REG_DPF_*; the other members only for the types 0..7 */
    int32_t  field_a;        /* see the table above; -1: none */
    int32_t  field_b;
    int32_t  field_out;
    float    v[3];           /* centre / sin(eps) / gain / threshold / maxDensity */
    int32_t  flag;           /* towardCenter / sensorType / useLargerThan */
    uint32_t seed;           /* MAX_DENSITY */
    int32_t  reserved[3];    /* must be 0 */
} reg_cloud_filter;
/* xyz, fields[].in / .out, out_xyz (m x 3, capacity n rows) and out_idx (m source indices, may be NULL) are host pointers,
   or device pointers when on_device != 0.  MAX_DENSITY reads two counters back per call, the other new filters none. */
REG_API reg_status reg_filter_cloud(reg_handle* h, const float* xyz, int64_t xyz_stride, int64_t n, int on_device,
                                    const reg_field* fields, int n_fields, const reg_cloud_filter* filters,
                                    int n_filters, float* out_xyz, int32_t* out_idx, int64_t* n_out);
/* The first `count` values of glibc's rand() after srand(seed) (TYPE_3 random_r), the stream MAX_DENSITY and the
   octree's random sampler replay. */
REG_API reg_status reg_host_glibc_rand(uint32_t seed, int64_t count, int32_t* out);

/* VoxelGridDataPointsFilter, useCentroid 1 (libpointmatcher DataPointsFilters/VoxelGrid.cpp:71-344; parameter names and
   defaults of VoxelGrid.h).  All fp32 without contraction, per axis a with v = v_size[a]:
     minBound = min / v;  numDiv = unsigned((1.0f + max / v) - minBound);  cell = unsigned(floorf(x / v - minBound));
     linear id = i + j * nx + k * nx * ny (64-bit).
   By rounding a cell index can reach numDiv on its axis; the linear id then aliases the neighbouring row's first cell
   (i = 0, j + 1), exactly as the reference's linear index does, and the two cells are one voxel.
   A voxel's output point is the sequential fp32 sum of its members in input order, starting from its first member,
   divided by float(count).  With average_existing_descriptors every field is averaged the same way (normals are not
   renormalised), otherwise the first member's descriptors are kept.  Output rows are ascending by first-member index;
   out_idx is that index.  The dense voxel array of the reference is never allocated (64-bit keys, a stable radix sort,
   one thread per voxel and column for the ordered sums: a crowded voxel is summed by one thread).
   use_centroid 0 is REG_UNSUPPORTED: that branch of this fork writes the cell centre into feature rows 1..3 -- y, z and
   the homogeneous pad (VoxelGrid.cpp:289-304) -- and the reference's own test never runs it (DataFilters.cpp:638-672).
   nx * ny * nz >= 2^32 (the reference wraps or fails to allocate), non-finite input, v_size not finite or <= 0, or a
   field with in == NULL is REG_BAD_ARGUMENT.  fields[] as for reg_filter_cloud (every field must exist). */
typedef struct {
    int32_t struct_size;                    /* sizeof(reg_voxel_grid_params) */
    float   v_size[3];                      /* vSizeX vSizeY vSizeZ: 1 1 1 */
    int32_t use_centroid;                   /* 1 */
    int32_t average_existing_descriptors;   /* 1 */
    int32_t reserved[2];                    /* must be 0 */
} reg_voxel_grid_params;
REG_API void reg_default_voxel_grid_params(reg_voxel_grid_params* p);
REG_API reg_status reg_voxel_grid(reg_handle* h, const float* xyz, int64_t xyz_stride, int64_t n, int on_device,
                                  const reg_field* fields, int n_fields, const reg_voxel_grid_params* p, float* out_xyz,
                                  int32_t* out_idx, int64_t* n_out);

/* OctreeGridDataPointsFilter (libpointmatcher DataPointsFilters/OctreeGrid.cpp, utils/octree/Octree.tpp build / idx /
   visit, OctreeSamplers.tpp; parameter names and defaults of OctreeGrid.h).  Everything in fp32 without
   FMA contraction:
     - root box: min / max per axis; radii = max - min; centre 0 when center_at_origin, else min + radii * 0.5f;
       radius = float(pow(2, ceil(log(x) / log(2)))) with x = double(max(radii)) * 0.5 in double with libm (x == 0
       gives radius 0, a single leaf).  With center_at_origin points may lie outside the root box.
     - a node is a leaf when double(radius) * 2.0 <= max_size_by_node or count <= max_point_by_node; otherwise a point
       goes to child (x > cx) | (y > cy) << 1 | (z > cz) << 2 (strict: a point on a centre goes low), the child centre
       is c + (+-0.5f * r) and the child radius r * 0.5f.  Members keep their input order; empty children are skipped.
       Coincident points with max_size_by_node 0 split until the radius underflows to 0 (about 280 levels at most).
     - non-empty leaves are visited depth-first, children 0..7; leaf k emits output row k:
         FIRST    (0) its first member;
         RAND     (1) member size_t(float(size - 1) * (float(rand()) / float(RAND_MAX))), one glibc rand() per
                      non-empty leaf after srand(1) (RandomPtsSampler seeds 1 on every call), clamped to size - 1;
         CENTROID (2) sequential fp32 sum in member order starting from the first member, / float(count); normals and
                      covariances are averaged the same way (not renormalised); src_idx is the first member;
         MEDOID   (3) the first member (member order) with the smallest sqrtf(dx*dx + (dy*dy + dz*dz)) (Eigen's norm of
                      a 3-vector) to the leaf mean (sequential fp32 sum from 0.0f, / float(count)), strict < from
                      FLT_MAX; when no distance is below FLT_MAX the first member.
   Deviation: the reference samplers move rows with swapCols(idx, j) and look a displaced row up one level deep only
   (indexVector[d]), so a row displaced twice before its leaf is visited emits the wrong point and drops the leaf's own
   one.  Here row k is the sample of the k-th non-empty leaf, which is the evident intent; the tree (leaf membership
   and depth-first order) matches exactly.
   Non-finite input, or an extent whose radius is not finite, is REG_BAD_ARGUMENT; n == 0 is REG_EMPTY_SOURCE.
   max_point_by_node >= 1, max_size_by_node >= 0 (not NaN), sampling_method 0..3, else REG_BAD_ARGUMENT.
   build_parallel is accepted and has no effect (the reference's tree does not depend on it). */
enum { REG_OCTREE_FIRST = 0, REG_OCTREE_RAND = 1, REG_OCTREE_CENTROID = 2, REG_OCTREE_MEDOID = 3 };
typedef struct {
    int32_t struct_size;          /* sizeof(reg_octree_params) */
    int32_t build_parallel;       /* 1 (no effect) */
    int64_t max_point_by_node;    /* 1 */
    float   max_size_by_node;     /* 0 */
    int32_t sampling_method;      /* 0 (REG_OCTREE_*) */
    int32_t center_at_origin;     /* 1 */
    int32_t reserved[5];
} reg_octree_params;
REG_API void reg_default_octree_params(reg_octree_params* p);
/* Outputs (host pointers, or device pointers when on_device != 0); only xyz is required.
     xyz        n_out x 3 (capacity n rows)   normals n_out x 3 and covs n_out x 6 when the input carries them
     src_idx    n_out: the chosen input index of each row (CENTROID: the leaf's first member)
     leaf_id    n (per INPUT point): the depth-first index of its non-empty leaf (== its output row)
     leaf_depth n (per INPUT point): the depth of its leaf (root 0) */
typedef struct {
    float*   xyz;
    float*   normals;
    float*   covs;
    int32_t* src_idx;
    int32_t* leaf_id;
    int32_t* leaf_depth;
} reg_octree_out;
REG_API reg_status reg_octree_grid(reg_handle* h, const float* xyz, int64_t xyz_stride, const float* nrm,
                                   const float* cov, int64_t n, int on_device, const reg_octree_params* p,
                                   const reg_octree_out* out, int64_t* n_out);
/* Host helpers of the contract: the root box from per-axis min / max, and RandomPtsSampler's member position of each of
   n_leaves leaves of the given sizes (glibc TYPE_3 rand() stream after srand(1)). */
REG_API void reg_host_octree_root(const float min[3], const float max[3], int center_at_origin, float center[3],
                                  float* radius);
REG_API reg_status reg_host_octree_random_picks(const int64_t* sizes, int64_t n_leaves, int64_t* picks);

/* ---- the dense map: VoxelizedPointCloud insert, carve, export -----------------------------------------
   The reference keeps a second, dense map per submap (o3d_slam::VoxelizedPointCloud, open3d_slam/src/Voxel.cpp:38-114),
   filled from every raw scan by its own worker (SlamWrapper.cpp:963-986 -> Submap::insertScanDenseMap, Submap.cpp:98-113).
   reg_dense_map is that object, resident on the device across calls.  It is created from a handle, uses that handle's
   stream and working storage, is as non-re-entrant as the handle, and MUST BE DESTROYED BEFORE THE HANDLE.  Several maps
   may live on one handle (one per submap); they are independent.

   Storage: structure-of-arrays, sorted by ascending key: uint64 key (offset binary, z<<42 | y<<21 | x, the packing of
   reg_voxelize_within_volume), int32 count, fp64 position / normal / colour sums (the two latter allocated when a cloud
   first brings the field).  Every column is double-buffered: a mutating call builds its result in the spare buffers and
   swaps at the end, so a call that fails -- on a bad point or a failed allocation -- leaves the map exactly as it was.
   Buffers grow geometrically; at most 2^31 - 1 voxels.

   Numeric contract: fp64, one rounding per operation (the build forbids contraction).
     map key, per axis: floor(p * (1.0 / voxel_size)) (VoxelHashMap.hpp:48-51,127).  Departure: a non-finite coordinate or an
       index outside +-(2^20 - 1) anywhere in the (transformed) input returns REG_BAD_ARGUMENT and leaves the map unchanged
       (the reference casts to int there).
     insert (VoxelizedPointCloud::insert, Voxel.cpp:66-88): a voxel's position, normal and colour sums are running sums in
       the order the points arrived; onto an existing voxel the new points are added one by one, ((S + p1) + p2) ..., not
       S + (p1 + p2 + ...).  count counts every point; a cloud without normals / colours adds nothing to those sums but still
       counts; has_normals / has_colors are sticky once a cloud brought the field; NaN normals are added as they are.
     transform before the insert (T == NULL: identity, no transform pass): the formula of reg_overlap_indices,
         w  = ((T30*x + T31*y) + T32*z) + T33,   x' = (((T00*x + T01*y) + T02*z) + T03) / w   (y', z' alike);
       normals (T (n, 0)).head<3>(): nx' = (T00*nx + T01*ny) + T02*nz; colours pass through (helpers.cpp:283-318).
       Departure: the identity shortcut of helpers.cpp:285-288, which appends the cloud to a copy of itself, is not reproduced.
     export (toPointCloud, Voxel.cpp:90-114): position, normal, colour = sum / count; normals are not re-normalised.
       Departure: voxels come in ascending key order, i.e. ascending (z, y, x) (the reference: std::unordered_map order).
     carve (getKeysOfCarvedPoints, helpers.cpp:360-390): per scan point, length, direction and the skip of zero-length or
       non-finite rays as reg_carve_indices; step = 2 r; reach = max(step, min(length - truncation, max_ray)); distance is
       the running sum 0, +step, +step ... while distance < reach; sample = distance*dir + sensor.  Per sample the
       neighbourhood of VoxelHashMap.cpp:13-45: per-axis offsets are the running sum -r, +v, +v ... while <= r
       (reg_host_dense_offsets); for each test point t = sample + offset the lookup key is floor(t / v) per axis -- a
       DIVISION, unlike the map key -- the centre k*v + v*0.5, and t is accepted if sqrt((d0^2 + d1^2) + d2^2) <= r.  The
       sample's own floor(sample / v) key is always looked up too.  Every key found in the map is erased; lookup keys
       outside +-(2^20 - 1) cannot be in the map and are skipped.  Departure (loop bounds): r and max_ray finite and > 0
       (the reference loops forever at r <= 0), truncation finite, at most 16 offsets per axis, max_ray / step <= 65536,
       else REG_BAD_ARGUMENT.  Result: the number of erased voxels and, optionally, their keys in ascending key order.
     de-duplication (removeDuplicatePointsWithinSameVoxels, Voxel.cpp:162-191): the lowest-index point of every voxel,
       map-key formula; ascending indices.
     transform of the map (VoxelizedPointCloud::transform, Voxel.cpp:49-64), REPRODUCED LITERALLY: keys stay; position sum
       and normal sum each become R S + t, per row ((R0*x + R1*y) + R2*z) + t; colour sum and count untouched.  This is the
       reference's behaviour and it is wrong for any t != 0 (a sum of k points should move by k t, a normal by none, and
       the keys should follow).
     centre (computeCenter, helpers.cpp:392-402): the sum of the averaged positions in key order, divided by (n + 1e-6).
   Matrices: const double[16], column-major.  Clouds: n x 3 doubles each (points, normals, colours); on_device covers every
   cloud array and every array output of a call.  n == 0 is REG_OK and a no-op; an empty map carves to 0.  Plain argument
   checks come before any device work (REG_BAD_ARGUMENT even on a handle without a device); then REG_DEVICE_ERROR. */
typedef struct reg_dense_map reg_dense_map;
typedef struct {
    int32_t  struct_size;          /* = sizeof(reg_dense_scan_params); checked */
    int32_t  reserved;
    reg_crop crop;                 /* denseMapCropper_; its centre is the caller's (the reference sets the identity pose) */
    double   rgb_min[3];           /* ColorRangeCropper (croppers.cpp:178-239): rgb_min <= c <= rgb_max on every channel; */
    double   rgb_max[3];           /*   a cloud without colours passes whole */
} reg_dense_scan_params;
typedef struct {
    int32_t struct_size;           /* = sizeof(reg_dense_carve_params); checked */
    int32_t reserved;
    double  neighborhood_radius;   /* neighborhoodRadiusDenseMap_ */
    double  max_ray;               /* maxRaytracingLength_ */
    double  truncation;            /* truncationDistance_ */
} reg_dense_carve_params;
typedef struct {
    int32_t struct_size;           /* = sizeof(reg_dense_map_info), set by the caller */
    int32_t has_normals;
    int32_t has_colors;
    int32_t reserved;
    int64_t n_voxels;
    int64_t capacity;              /* rows the current buffers hold */
    double  voxel_size;
} reg_dense_map_info;
REG_API reg_status reg_dense_map_create(reg_handle* h, double voxel_size, reg_dense_map** out);
REG_API void reg_dense_map_destroy(reg_dense_map* m);   /* before reg_destroy of its handle */
REG_API reg_status reg_dense_map_clear(reg_dense_map* m);   /* drops the voxels; the has-field flags stay, as the reference's */
REG_API reg_status reg_dense_map_insert(reg_dense_map* m, const double* xyz, const double* normals, const double* colors,
                                        int64_t n, int on_device, const double T[16] /* NULL: identity */, int64_t* n_voxels,
                                        int64_t* n_new);
/* no crop, colours within [0, 1] */
REG_API void reg_default_dense_scan_params(reg_dense_scan_params* p);
/* Submap.cpp:99-106 in one call: crop, ColorRangeCropper, transform, insert; the intermediate clouds never leave the device.
   *n_inserted: points that passed both croppers. */
REG_API reg_status reg_dense_map_insert_scan(reg_dense_map* m, const double* xyz, const double* normals, const double* colors,
                                             int64_t n, int on_device, const reg_dense_scan_params* params,
                                             const double T_map_to_sensor[16] /* NULL: identity */, int64_t* n_inserted,
                                             int64_t* n_voxels);
/* SpaceCarvingParameters as shipped (Parameters.hpp:88-95): radius 0.1, max ray 20, truncation 0.1 */
REG_API void reg_default_dense_carve_params(reg_dense_carve_params* p);
REG_API reg_status reg_dense_map_carve(reg_dense_map* m, const double* scan_xyz, int64_t n_scan, int on_device,
                                       const double sensor[3], const reg_dense_carve_params* params,
                                       int32_t* removed_keys /* may be NULL; n_voxels x 3: (x, y, z) per row */,
                                       int64_t* n_removed);
/* The body of Submap::carve for the dense map (Submap.cpp:146-157) in one call, without a host round trip:
     1. T == NULL: the scan as given (the reference's oddity: the raw sensor-frame scan against a map-frame sensor); with T
        the scan is transformed first, with the point formula above (carveInMapFrame of icp.DenseMapBuilder);
     2. removeDuplicatePointsWithinSameVoxels at the map's voxel size, with the contract and the refusals of
        reg_dedup_voxels: the lowest-index point of every voxel, in ascending index order; a non-finite coordinate or an index
        outside +-(2^20 - 1) in the (transformed) scan returns REG_BAD_ARGUMENT and leaves the map as it was;
     3. getKeysOfCarvedPoints on the kept points with the numeric contract of reg_dense_map_carve, word for word.  The
        lookups go through a coarse level built per call (the bricks of 8 x 8 x 8 voxels the map occupies, with a 512-bit
        mask each), which only skips keys it has proven absent;
     4. erase, swap, and the erased keys in ascending key order: a failing call leaves the map as it was.
   *n_removed, removed_keys and the map afterwards are identical to reg_dedup_voxels, a gather of the kept rows and
   reg_dense_map_carve on the same inputs.  The gate of Submap::carve (every N scans, a non-empty map) is the caller's:
   reg_submaps_insert_scan_dense_map applies it.  on_device covers scan_xyz and removed_keys. */
REG_API reg_status reg_dense_map_carve_scan(reg_dense_map* m, const double* scan_xyz, int64_t n_scan, int on_device,
                                            const double sensor[3], const reg_dense_carve_params* params,
                                            const double T[16] /* NULL: the scan as given */,
                                            int32_t* removed_keys /* may be NULL; n_voxels x 3 */, int64_t* n_removed);
REG_API reg_status reg_dense_map_transform(reg_dense_map* m, const double T[16]);
REG_API reg_status reg_dense_map_center(reg_dense_map* m, double center[3]);
REG_API reg_status reg_dense_map_get_info(const reg_dense_map* m, reg_dense_map_info* info);
/* Any output may be NULL; normals / colors are written only when the map has met the field (reg_dense_map_get_info);
   keys: n x 3 int32 (x, y, z); capacity_rows < n_voxels returns REG_BAD_ARGUMENT. */
REG_API reg_status reg_dense_map_export(reg_dense_map* m, int on_device, double* xyz, double* normals, double* colors,
                                        int32_t* keys, int32_t* counts, int64_t capacity_rows, int64_t* n_out);
REG_API reg_status reg_dedup_voxels(reg_handle* h, const double* xyz, int64_t n, int on_device, double voxel_size,
                                    int32_t* kept_idx /* capacity n */, int64_t* n_kept);
/* The per-axis neighbourhood offsets of the carve, on the host: returns their number (offsets may be NULL; capacity 16),
   or -1 for arguments reg_dense_map_carve refuses. */
REG_API int32_t reg_host_dense_offsets(double neighborhood_radius, double voxel_size, double* offsets);

/* ---- the map cloud: Submap::mapCloud_ resident on the device -- insertScan, carve, set as target ----------
   The scan-matching map of a submap (open3d_slam/src/Submap.cpp:39-144) and the per-scan cycle around it:
   Submap::insertScan (transform, carve, operator+=, setPose, voxelizeInsideCroppingVolume) and cropSubmap + initReference
   (ScanToMapRegistration.cpp:90-96).  reg_map_cloud is that object, resident on the device across calls.  It is created
   from a handle, uses that handle's stream and working storage, is as non-re-entrant as the handle, and MUST BE DESTROYED
   BEFORE THE HANDLE.  Several maps may live on one handle (one per submap); they are independent.

   Storage: fp64 structure-of-arrays in the reference's point order: points n x 3, optional normals n x 3, optional
   covariances n x 9 (Eigen's Matrix3d: element (r, c) at 3 c + r).  Every column is double-buffered: a mutating call builds
   its result in the spare side and swaps at the end, so a call that fails -- a refused point, a failed allocation, a bad
   argument found on the device -- leaves the points, the stored cropper centre and the scan counter exactly as they were.
   Buffers grow geometrically; at most 2^31 - 1 rows, map + scan during an insert included.

   Fields: the field set is fixed at creation (has_normals / has_covariances).  A cloud that brings other fields -- more or
   fewer -- is refused with REG_BAD_ARGUMENT.  Departure: Open3D's operator+= silently drops a field that one side lacks.
   Colours are not carried (as reg_voxelize_within_volume).

   Numeric contract: fp64, one rounding per operation (the build forbids contraction).
     transform (o3d_slam::transform, helpers.cpp:283-318; PointCloud::Transform for reg_map_cloud_transform), the formula of
       reg_overlap_indices and the dense map:
         w  = ((T30*x + T31*y) + T32*z) + T33,   x' = (((T00*x + T01*y) + T02*z) + T03) / w   (y', z' alike);
       normals (T (n, 0)).head<3>(): nx' = (T00*nx + T01*ny) + T02*nz;
       covariances R C R^T in this order: M = R C with M(r, c) = (R(r,0)*C(0,c) + R(r,1)*C(1,c)) + R(r,2)*C(2,c), then
       C'(r, c) = (M(r,0)*R(c,0) + M(r,1)*R(c,1)) + M(r,2)*R(c,2).  The result is as symmetric as that arithmetic leaves it.
       Departure: the identity shortcut of helpers.cpp:285-288, which appends the cloud to a copy of itself, is not reproduced.
     reg_map_cloud_insert_scan, in the reference's order (Submap.cpp:54-95):
       1. carve (Submap.cpp:130-144) runs only when all three hold: perform_carving, the map is non-empty, and
          scans_inserted % carve_every_n_scans == 1.  Two consequences of that rule, followed: it never runs with
          carve_every_n_scans == 1 (x % 1 is never 1), and it never runs on the first insert (the counter is 0).  The rays are
          the whole transformed raw scan, not de-duplicated, from the sensor at the translation of T.  The subset of the map
          that takes part is the map builder's volume at the pose stored by the PREVIOUS insert (at first: the centre given
          at creation), because setPose comes after the carve (Submap.cpp:85) -- an oddity of the reference, followed.
          Everything else is as reg_carve_indices, its refusal of a map point beyond the key range inside the volume included.
          The survivors are compacted in their order (removeByIds).  An empty raw scan carves nothing.
       2. append: the transformed scan rows follow the map rows (operator+=); then the stored cropper centre becomes the
          translation of T (setPose).
       3. voxelise: voxelizeWithinCroppingVolume with the contract of reg_voxelize_within_volume at the new centre: the
          outside rows first, in order; then one row per occupied voxel in ascending (z, y, x); sums in row order, so
          resident rows come before scan rows; NaN normals are skipped, the averaged normal is re-normalised, covariances
          are averaged.  map_voxel_size <= 0 leaves the concatenation as it is (n_outside = n_rows, n_voxels = 0).  A voxel
          index beyond +-(2^20 - 1), or a non-finite coordinate, inside the volume returns REG_BAD_ARGUMENT, map unchanged.
       4. the scan counter goes up by one.
       n_scan == 0 is REG_OK and a no-op (Submap.cpp:41-43): no carve, no counter, no pose.
     reg_map_cloud_set: the isUseInitialMap_ branch (Submap.cpp:47-52): the map becomes the cloud, voxel-down-sampled as
       reg_voxel_down_sample when voxel_size > 0 (and refused as there); it is not transformed and the counter and the
       cropper centre are untouched.  n == 0 empties the map.
     reg_map_cloud_set_target: exactly reg_set_target_f64 of the resident arrays as device pointers with that crop, its
       statuses included (REG_EMPTY_TARGET for an empty map or an empty patch; the previous reference is gone either way).
       reg_get_target_source_indices then indexes map rows, valid until the next mutating call on the map.
     centre (GetCenter): the sequential sum of the rows in order, divided by n; an empty map gives zero.
   Parity: PointCloud::Transform, GetCenter and operator+= live in un-vendored Open3D 0.15.1: PARITY UNPINNED, restated.
   Matrices: const double[16], column-major.  on_device covers every cloud array and every array output of a call.  Plain
   argument checks come before any device work (REG_BAD_ARGUMENT even on a handle without a device); then REG_DEVICE_ERROR. */
typedef struct reg_map_cloud reg_map_cloud;
typedef struct {
    int32_t  struct_size;          /* = sizeof(reg_map_cloud_params); checked */
    int32_t  has_normals;          /* the field set, fixed at creation */
    int32_t  has_covariances;
    int32_t  carve_every_n_scans;  /* carving_.carveSpaceEveryNscans_; >= 1 */
    double   map_voxel_size;       /* mapBuilder_.mapVoxelSize_; <= 0: no voxelisation */
    reg_crop crop;                 /* mapBuilderCropper_; its centre is owned by the map from then on */
    double   carve_voxel_size;     /* carving_.voxelSize_; finite and > 0 */
    double   carve_max_ray;        /* carving_.maxRaytracingLength_ */
    double   carve_truncation;     /* carving_.truncationDistance_ */
    double   carve_min_dot;        /* carving_.minDotProductWithNormal_ */
} reg_map_cloud_params;
typedef struct {
    int32_t struct_size;           /* = sizeof(reg_map_cloud_info), set by the caller */
    int32_t has_normals;
    int32_t has_covariances;
    int32_t reserved;
    int64_t n_rows;
    int64_t capacity;              /* rows the current buffers hold */
    int64_t scans_inserted;        /* nScansInsertedMap_ */
    double  crop_center[3];        /* the cropper centre the next carve uses */
} reg_map_cloud_info;
typedef struct {
    int32_t struct_size;           /* = sizeof(reg_map_cloud_insert_result), set by the caller */
    int32_t carved;                /* the carve rule held for this insert */
    int64_t n_carved;              /* rows the carve removed */
    int64_t n_outside;             /* rows outside the volume, passed through */
    int64_t n_voxels;              /* rows that stand for one voxel each */
    int64_t n_rows;                /* rows of the map after the call = n_outside + n_voxels */
} reg_map_cloud_insert_result;
/* Parameters.hpp:51-57,88-101 as shipped: map voxel 0.03, MaxRadius 20 at the origin, carve voxel 0.1, ray 20, truncation
   0.1, min dot 0.5, every 10 scans; normals, no covariances. */
REG_API void reg_default_map_cloud_params(reg_map_cloud_params* p);
REG_API reg_status reg_map_cloud_create(reg_handle* h, const reg_map_cloud_params* params, reg_map_cloud** out);
REG_API void reg_map_cloud_destroy(reg_map_cloud* m);   /* before reg_destroy of its handle */
REG_API reg_status reg_map_cloud_clear(reg_map_cloud* m);   /* drops the points; cropper centre and scan counter stay */
REG_API reg_status reg_map_cloud_get_info(const reg_map_cloud* m, reg_map_cloud_info* info);
REG_API reg_status reg_map_cloud_set(reg_map_cloud* m, const double* xyz, const double* normals, const double* covs, int64_t n,
                                     int on_device, double voxel_size);
/* Submap::insertScan (Submap.cpp:54-95) in one call; no intermediate cloud or index list leaves the device.
   raw_xyz: the raw scan in the sensor frame (the carve's rays; may be NULL with n_raw == 0); scan_*: the pre-processed scan
   (the merge cloud of reg_process_scan) in the sensor frame; result may be NULL. */
REG_API reg_status reg_map_cloud_insert_scan(reg_map_cloud* m, const double* raw_xyz, int64_t n_raw, const double* scan_xyz,
                                             const double* scan_normals, const double* scan_covs, int64_t n_scan,
                                             int on_device, const double T_map_to_sensor[16], int perform_carving,
                                             reg_map_cloud_insert_result* result);
REG_API reg_status reg_map_cloud_set_target(reg_map_cloud* m, const reg_crop* crop, int64_t* n_kept);
REG_API reg_status reg_map_cloud_transform(reg_map_cloud* m, const double T[16]);
REG_API reg_status reg_map_cloud_center(reg_map_cloud* m, double center[3]);
/* Any output may be NULL; normals / covs are written only when the map has the field; capacity_rows < n_rows returns
   REG_BAD_ARGUMENT. */
REG_API reg_status reg_map_cloud_export(reg_map_cloud* m, int on_device, double* xyz, double* normals, double* covs,
                                        int64_t capacity_rows, int64_t* n_out);

/* ---- motion compensation of a raw scan: the first step of both workers of the reference ------------------
   ConstantVelocityMotionCompensation::undistortInputPointCloud (MotionCompensation.cpp:64-139; called at
   SlamWrapper.cpp:730,890) for GIVEN velocities.  fp64 with one rounding per operation (the build forbids contraction); every
   sum of three products is (a0 b0 + a1 b1) + a2 b2.  on_device covers both arrays.  Plain argument checks come before any
   device work (they answer even on a handle without a device); then n == 0 returns REG_OK; then REG_DEVICE_ERROR.
     Finding: the reference's own velocity estimate is dead code.  buffer_ is a const reference, the const overload of
     latest_measurement(int) ignores its offset (TransformInterpolationBuffer.cpp:66-84), so start == finish, dt == 0 and
     assert_gt(dt, 0.0) throws (MotionCompensation.cpp:41-47).  The device side therefore takes the two velocities as
     arguments; the estimate as evidently intended lives in the Python and C++ mirrors (a departure).
     Per point p = (x, y, z), one thread each, in this order (MotionCompensation.cpp:82-139, math.cpp:32-37):
       a = atan2(y, x);  aw = a < 0 ? a + 2pi : a, with 2pi = 2.0 * M_PI;
       phase = 0 when aw == 0; clockwise: 1 - aw / 2pi; otherwise aw / 2pi;
       s = phase * scan_duration;  t = s * linear_velocity;  (roll, pitch, yaw) = s * angular_velocity_rpy;
       q = qz(yaw) qy(pitch) qx(roll), each factor (cos(0.5 angle), sin(0.5 angle) axis), two Hamilton products
         (qz qy) qx, every component summed left to right in Eigen's term order
           w = a.w b.w - a.x b.x - a.y b.y - a.z b.z     x = a.w b.x + a.x b.w + a.y b.z - a.z b.y
           y = a.w b.y + a.y b.w + a.z b.x - a.x b.z     z = a.w b.z + a.z b.w + a.x b.y - a.y b.x
         (the zero components take part); then q / sqrt(((w w + x x) + y y) + z z), each component divided;
       R = Eigen's toRotationMatrix: tx = 2x, ty = 2y, tz = 2z, twx = tx w, twy = ty w, twz = tz w, txx = tx x, txy = ty x,
         txz = tz x, tyy = ty y, tyz = tz y, tzz = tz z;  R00 = 1 - (tyy + tzz), R01 = txy - twz, R02 = txz + twy,
         R10 = txy + twz, R11 = 1 - (txx + tzz), R12 = tyz - twx, R20 = txz - twy, R21 = tyz + twx, R22 = 1 - (txx + tyy);
       p' = ((Rr0 x + Rr1 y) + Rr2 z) + t_r.
     Departure: when the three components of t and the three angles all compare equal to zero the motion is the identity
     and p' = p, copied (the arithmetic would only turn a -0.0 coordinate into +0.0).  So zero velocities, and the points
     of phase 0 (y = +-0, x > 0), come back bit for bit.
     atan2, sin, cos are the platform's (libm on the host, the device math library on the GPU); everything else is exact
     to the formula.  Normals and colours of a cloud pass through untouched (the reference rewrites points_ only), so the
     call takes points only.  out_xyz may be xyz itself.
     scan_duration <= 0 or non-finite, a non-finite velocity or a bad struct_size: REG_BAD_ARGUMENT (setParameters asserts
     scan_duration > 0); n == 0: REG_OK.
   reg_host_undistort_point: the same code for one point on the host. */
typedef struct {
    int32_t struct_size;              /* = sizeof(reg_undistort_params); checked */
    int32_t spinning_clockwise;       /* isSpinningClockwise_ */
    double  scan_duration;            /* scanDuration_ [s]; finite and > 0 */
    double  linear_velocity[3];       /* of the sensor, in its own frame [m/s] */
    double  angular_velocity_rpy[3];  /* roll, pitch, yaw rates [rad/s] */
} reg_undistort_params;
REG_API reg_status reg_undistort_scan(reg_handle* h, const double* xyz, int64_t n, int on_device,
                                      const reg_undistort_params* params, double* out_xyz);
REG_API reg_status reg_host_undistort_point(const double p[3], const reg_undistort_params* params, double out[3]);

/* ---- rows of the reading the handle holds -----------------------------------------------------------------
   The number of rows reg_get_correspondences / reg_get_correspondences_k write per array: the reading as it stands,
   whoever installed it (reg_set_source*, reg_process_scan, reg_set_pair_overlap_f64, reg_odometry_add_scan); 0 when there
   is none.  A binding sizes its arrays from this, never from a count of its own. */
REG_API reg_status reg_get_source_count(const reg_handle* h, int64_t* n_rows);

/* ---- GICP covariances from normals ------------------------------------------------------------------------
   What Open3D 0.15.1's RegistrationGeneralizedICP derives for a cloud that has normals and no covariances
   (InitializePointCloudForGeneralizedICP, GetRotationFromE1ToX), restated: Open3D is not vendored, PARITY UNPINNED.
   fp64, one rounding per operation (the build forbids contraction); every sum of three products is (a0 b0 + a1 b1) + a2 b2.
   Per normal x = (x0, x1, x2), NOT normalised first, in this order:
     v = e1 x x as Eigen's cross: v0 = 0 x2 - 0 x1, v1 = 0 x0 - 1 x2, v2 = 1 x1 - 0 x0;  c = (1 x0 + 0 x1) + 0 x2;
     c < -0.99: Rx = I.  (Oddity reproduced: Open3D's comment says "x and e1 are in the same direction"; they are opposite,
       and the identity does not rotate e1 onto x.  So the normal -e1 gets diag(epsilon, 1, 1), which happens to be right.)
     otherwise S = [v]x = [0 -v2 v1; v2 0 -v0; -v1 v0 0], f = 1 / (1 + c),
       S2(i,j) = (S(i,0) S(0,j) + S(i,1) S(1,j)) + S(i,2) S(2,j),  Rx(i,j) = (I(i,j) + S(i,j)) + S2(i,j) f;
     M(i,0) = Rx(i,0) epsilon, M(i,1) = Rx(i,1) 1, M(i,2) = Rx(i,2) 1;
     cov(i,j) = (M(i,0) Rx(j,0) + M(i,1) Rx(j,1)) + M(i,2) Rx(j,2), stored row-major: the covariances_ layout of reg_set_*_f64.
   A non-finite component yields whatever this arithmetic yields.  normals: n x 3 doubles, out_covs: n x 9 doubles, both host
   or both device pointers.  epsilon non-finite or <= 0, n < 0 or n > 2^31 - 1, a missing array for n > 0: REG_BAD_ARGUMENT,
   decided before any device work; then n == 0: REG_OK, with or without a device; then REG_DEVICE_ERROR.
   reg_host_covariance_from_normal: the same code for one normal on the host. */
REG_API reg_status reg_covariances_from_normals(reg_handle* h, const double* normals, int64_t n, int on_device, double epsilon,
                                                double* out_covs);
REG_API reg_status reg_host_covariance_from_normal(const double normal[3], double epsilon, double out_cov[9]);

/* ---- LidarOdometry resident on the device (Odometry.cpp:22-141) ---------------------------------------------
   One object per handle use: it keeps cloudPrev_ (fp64 points, optional normals and covariances) in two sides on the device
   and the cumulative pose, the pending initial transform and the last stamp on the host.  It works on the handle's stream
   and working storage and installs its own reference and reading on the handle; destroy it before the handle.
   The handle's cost selects the operator of cloudRegistrationFactory: REG_COST_GICP, REG_COST_O3D_P2PL or REG_COST_O3D_P2P
   (REG_COST_P2PL: REG_BAD_ARGUMENT, the factory has no libpointmatcher operator).  Configure the handle as the Open3D
   operators are configured: use_trimmed = 0, and gicp_stop_rule = 1 for GICP.
   reg_odometry_add_scan, in this order (flags in the result):
     first scan (no previous cloud): preprocess, keep as the previous cloud, record the stamp; accepted = pose_updated = 1
       (the caller pushes the unchanged cumulative pose, Odometry.cpp:33);
     timestamp < last stamp: accepted = 0, nothing changes (an equal stamp goes on: the reference tests <);
     use_odometry_topic: accepted = 1, pose_updated = 0, nothing else happens;
     preprocess (Odometry.cpp:22-27): crop, reg_voxel_down_sample (voxel_size <= 0 skips it), normals as reg_process_scan
       estimates them (viewpoint at the origin) when the scan brings none and the operator is GICP or O3D_P2PL,
       reg_random_down_sample (ratio >= 1 skips it).  There is no narrow crop.  A scan that brings normals keeps them;
     GICP: covariances of the NEW cloud from its normals, reg_covariances_from_normals with gicp_epsilon (the previous cloud
       keeps those it got when it was new);
     register: reading = the PREVIOUS cloud, reference = the NEW cloud (reg_set_target_f64 then reg_set_source_f64 of the
       resident arrays, no crop), T_init = identity (registerClouds(cloudPrev_, *preProcessed, I), Odometry.cpp:53);
     fitness > min_fitness fails: accepted = 0, the new cloud replaces the previous one, pose and stamp stay;
     otherwise: a pending initial transform BECOMES the cumulative pose and the registration result is discarded (oddity
       reproduced, Odometry.cpp:73-75); else cumulative = cumulative * T^-1 (reg_host_odometry_accumulate); the new cloud
       becomes the previous one, the stamp is recorded, pose_updated = 1.
   The hand-over is a swap of the two sides.  A call that returns an error status leaves cloud, pose and stamp as they were.
   Departure: a scan that is empty after preprocessing is REG_EMPTY_SOURCE with the state unchanged (the reference would run
   Open3D on an empty cloud).  GICP or O3D_P2PL with neither normals nor normal_knn > 0: REG_MISSING_FIELD.
   Every entry point that writes a caller array takes its capacity in rows and returns REG_BAD_ARGUMENT, writing nothing,
   when it is too small. */
typedef struct reg_odometry reg_odometry;
typedef struct {
    int32_t  struct_size;          /* = sizeof(reg_odometry_params); checked */
    int32_t  use_odometry_topic;   /* useOdometryTopic_ (true as shipped) */
    reg_crop crop;                 /* scanProcessing_.cropper_ */
    double   voxel_size;           /* scanProcessing_.voxelSize_; finite; <= 0: no voxel grid */
    double   down_sampling_ratio;  /* scanProcessing_.downSamplingRatio_; in [0, 1] */
    uint64_t seed;                 /* of reg_random_down_sample */
    int32_t  normal_knn;           /* 0 .. 32; 0: never estimate */
    int32_t  reserved;
    double   normal_radius;        /* > 0 when normal_knn > 0 */
    double   gicp_epsilon;         /* Open3D's epsilon (1e-3); finite and > 0 */
    double   min_fitness;          /* the fitness gate (0.1, "todo magic", Odometry.cpp:56); finite */
} reg_odometry_params;
typedef struct {
    int32_t struct_size;           /* = sizeof(reg_odometry_result), set by the caller */
    int32_t accepted;              /* addRangeScan's return value */
    int32_t pose_updated;          /* the caller pushes (timestamp, cumulative) into its buffer */
    int32_t registered;            /* a registration ran in this call */
    int32_t iterations;
    int32_t reserved;
    int64_t n_crop, n_voxels, n_selected;   /* rows after crop / voxel grid / random selection */
    int64_t n_source, n_target;    /* rows of the registration: previous cloud, new cloud */
    double  fitness, inlier_rmse;
    double  cumulative[16];        /* column-major, after the call */
    float   T[16];                 /* the registration result, column-major (identity when none ran) */
    float   prep_ms, register_ms;  /* device time of preprocess (+ covariances) and of target + source + loop (HIP events) */
} reg_odometry_result;
typedef struct {
    int32_t struct_size;           /* = sizeof(reg_odometry_info), set by the caller */
    int32_t has_cloud;             /* a previous cloud is held */
    int32_t has_normals, has_covariances;
    int32_t has_stamp;             /* a stamp has been recorded */
    int32_t initial_pending;       /* an initial transform waits for the next accepted registration */
    int64_t n_rows;
    int64_t last_stamp_ns;
    double  cumulative[16];
} reg_odometry_info;
/* Parameters.hpp:59-86 and the shipped Lua: the scan croppper and processing of reg_default_scan_params (MinMaxRadius 2 ..
   100, z -50 .. 50, voxel 0.01, ratio 1, knn 20 within 1 m), gicp_epsilon 1e-3, min_fitness 0.1, use_odometry_topic 1. */
REG_API void reg_default_odometry_params(reg_odometry_params* p);
/* The validation reg_odometry_create runs, without a device: REG_BAD_ARGUMENT for a wrong struct_size of either struct,
   cost P2PL, an unknown crop type, a non-finite voxel_size, a ratio outside [0, 1], normal_knn outside [0, 32],
   normal_radius <= 0 with normal_knn > 0, gicp_epsilon non-finite or <= 0, a non-finite min_fitness. */
REG_API reg_status reg_check_odometry_params(const reg_params* p, const reg_odometry_params* o);
/* sizeof of reg_odometry_params, reg_odometry_result, reg_odometry_info, for a binding to compare its mirrors with */
REG_API void reg_odometry_struct_sizes(int32_t sizes[3]);
REG_API reg_status reg_odometry_create(reg_handle* h, const reg_odometry_params* params, reg_odometry** out);
REG_API void reg_odometry_destroy(reg_odometry* o);   /* before reg_destroy of its handle */
REG_API reg_status reg_odometry_clear(reg_odometry* o);   /* a fresh LidarOdometry: no cloud, no stamp, identity pose */
REG_API reg_status reg_odometry_get_info(const reg_odometry* o, reg_odometry_info* info);
/* setInitialTransform (Odometry.cpp:110-126): *applied = 0 and nothing changes while an earlier one is pending (the reference
   prints and skips); otherwise the cumulative pose is set at once and the transform stays pending.  T: column-major. */
REG_API reg_status reg_odometry_set_initial_transform(reg_odometry* o, const double T[16], int32_t* applied);
/* xyz: n x 3 doubles, normals: n x 3 or NULL, both host or both device pointers; timestamp in nanoseconds. */
REG_API reg_status reg_odometry_add_scan(reg_odometry* o, const double* xyz, const double* normals, int64_t n, int on_device,
                                         int64_t timestamp_ns, reg_odometry_result* result);
/* getPreProcessedCloud: the previous cloud.  Any output may be NULL; normals / covs are written only when held. */
REG_API reg_status reg_odometry_export_cloud(reg_odometry* o, int on_device, double* xyz, double* normals, double* covs,
                                             int64_t capacity_rows, int64_t* n_out);
/* Correspondences of the last registration of this object (host arrays; rows = its n_source; ids index the new cloud, -1:
   none).  REG_NOT_CONFIGURED when the handle's reading is no longer the one this object installed. */
REG_API reg_status reg_odometry_get_correspondences(reg_odometry* o, int64_t capacity_rows, int32_t* ids, float* d2);

/* The branch logic of addRangeScan as one host function (no device).  Inputs: has_previous, the two stamps,
   use_odometry_topic, the rows of the preprocessed scan, the fitness, min_fitness, initial_pending.  Returns the bits that
   apply.  rows and fitness matter only where REG_ODOM_REGISTER is set: the object calls it once to learn whether to
   preprocess and register, and again with the outcome. */
enum {
    REG_ODOM_ACCEPTED = 1, REG_ODOM_POSE_UPDATED = 2, REG_ODOM_REPLACE_CLOUD = 4, REG_ODOM_POSE_FROM_INITIAL = 8,
    REG_ODOM_ACCUMULATE = 16, REG_ODOM_RECORD_STAMP = 32, REG_ODOM_PREPROCESS = 64, REG_ODOM_REGISTER = 128
};
REG_API int32_t reg_host_odometry_decide(int32_t has_previous, int64_t timestamp_ns, int64_t last_stamp_ns,
                                         int32_t use_odometry_topic, int64_t n_rows, double fitness, double min_fitness,
                                         int32_t initial_pending);
/* cumulative = cumulative * T^-1 in fp64, both column-major; T is the float result widened exactly.  One rounding per
   operation.  The inverse is the GENERAL cofactor inverse (no rigidity assumed, as Matrix4d::inverse() assumes none; bit
   parity with Eigen's vectorised inverse is unpinned).  With a(r,c) = T(r,c):
     s0 = a00 a11 - a10 a01, s1 = a00 a12 - a10 a02, s2 = a00 a13 - a10 a03, s3 = a01 a12 - a11 a02, s4 = a01 a13 - a11 a03,
     s5 = a02 a13 - a12 a03, c5 = a22 a33 - a32 a23, c4 = a21 a33 - a31 a23, c3 = a21 a32 - a31 a22, c2 = a20 a33 - a30 a23,
     c1 = a20 a32 - a30 a22, c0 = a20 a31 - a30 a21 (each product rounded, then the difference);
     det = ((((s0 c5 - s1 c4) + s2 c3) + s3 c2) - s4 c1) + s5 c0;  id = 1 / det;  with t(x,p,y,q,z,r) = (x p - y q) + z r:
     b00 =  t(a11,c5,a12,c4,a13,c3) id   b01 = -t(a01,c5,a02,c4,a03,c3) id   b02 =  t(a31,s5,a32,s4,a33,s3) id
     b03 = -t(a21,s5,a22,s4,a23,s3) id   b10 = -t(a10,c5,a12,c2,a13,c1) id   b11 =  t(a00,c5,a02,c2,a03,c1) id
     b12 = -t(a30,s5,a32,s2,a33,s1) id   b13 =  t(a20,s5,a22,s2,a23,s1) id   b20 =  t(a10,c4,a11,c2,a13,c0) id
     b21 = -t(a00,c4,a01,c2,a03,c0) id   b22 =  t(a30,s4,a31,s2,a33,s0) id   b23 = -t(a20,s4,a21,s2,a23,s0) id
     b30 = -t(a10,c3,a11,c1,a12,c0) id   b31 =  t(a00,c3,a01,c1,a02,c0) id   b32 = -t(a30,s3,a31,s1,a32,s0) id
     b33 =  t(a20,s3,a21,s1,a22,s0) id   (the sign applied to t, then the product with id);
     out(i,j) = ((cum(i,0) b0j + cum(i,1) b1j) + cum(i,2) b2j) + cum(i,3) b3j. */
REG_API reg_status reg_host_odometry_accumulate(double cumulative[16], const float T[16]);

/* ---- Pose-graph optimisation: o3d_slam::OptimizationProblem::solve (OptimizationProblem.cpp:25-44) ----
   What Open3D's GlobalOptimization does to the pose graph the mapper builds from its constraints: Levenberg-Marquardt with
   line processes on the uncertain (loop-closure) edges, a prune, a second pass, the compensation of the reference node.
   Open3D 0.15.1 is not vendored: the text below is the contract, its oracle is tests/pose_graph_restatement.py, and parity
   with Open3D 0.15.1 is unpinned.  fp64 throughout; every 4 x 4 matrix of this section is ROW-major, every 6 x 6 too.
   Graph: n_nodes poses; n_edges edges {source, target, X, info, uncertain, confidence}.
   Products and sums, in this order (one rounding per operation; the build forbids contraction):
     (A B)(i,j) = ((A(i,0) B(0,j) + A(i,1) B(1,j)) + A(i,2) B(2,j)) + A(i,3) B(3,j), all four rows and columns;
     rigid inverse of [R | t]: [R^T | t'], t'_i = -((R(0,i) t0 + R(1,i) t1) + R(2,i) t2) (DEPARTURE: Open3D takes Eigen's
       general 4 x 4 inverse);
     lin6(M) = [(M21 - M12) 0.5, (M02 - M20) 0.5, (M10 - M01) 0.5, M03, M13, M23];
     generators G0..G2: rotations about x, y, z (G0(1,2) = -1, G0(2,1) = 1; G1(0,2) = 1, G1(2,0) = -1; G2(0,1) = -1,
       G2(1,0) = 1), G3..G5: the unit translations in column 3;
     per edge A = X^-1 Tt^-1; zeta = lin6(A Ts); column k of Js = lin6((A Gk) Ts); column k of Jt = lin6((A (-Gk)) Ts);
     W = L J with L = info: W(i,c) = sum over j = 0..5 left to right of L(i,j) J(j,c); (J^T W)(a,c) = sum over i left to right
       of J(i,a) W(i,c); v = L zeta likewise; J^T v likewise; e^T L e = sum over i left to right of zeta_i v_i;
     H(s,s) += l Js^T L Js, H(s,t) += l Js^T L Jt, H(t,s) += l Jt^T L Js, H(t,t) += l Jt^T L Jt, b(s) -= l Js^T L e,
       b(t) -= l Jt^T L e with l = confidence, every element summed IN EDGE ORDER from zero, without atomics;
     line-process weight w = (preference (d d)) (sum of info(5,5) in edge order / n_edges), d = max_correspondence_distance;
       0 without edges; confidence of an uncertain edge = (w / (w + e^T L e))^2;
     residual = sum in edge order of l e^T L e + w (sqrt(l) - 1)^2;
     pose step: pose <- V(d) pose, V(al, be, ga, a, b, c) = [Rz(ga) Ry(be) Rx(al) | (a, b, c)] with
       V00 = cg cb, V01 = (cg sb) sa - sg ca, V02 = (cg sb) ca + sg sa, V10 = sg cb, V11 = (sg sb) sa + cg ca,
       V12 = (sg sb) ca - cg sa, V20 = -sb, V21 = cb sa, V22 = cb ca;
     pose vector (read by the increment test only): sy = sqrt(R00 R00 + R10 R10); sy >= 1e-6: (atan2(R21, R22),
       atan2(-R20, sy), atan2(R10, R00)), else (atan2(-R12, R11), atan2(-R20, sy), 0); then the translation.
   One LM pass (reg_pose_graph_optimize): zeta; current = new = residual; confidences; (H, b); lambda = 1e-5 max diag H;
   nu = 2; stop at once if max b < min_right_term.  Outer iteration iter = 0, 1, ...: lm_count = 0; inner loop: solve
   (H + lambda I) d = b; stop if |d| < min_relative_increment (|x| + min_relative_increment); trial poses, zeta and residual
   with the CURRENT confidences; rho = (current - new) / (d . (lambda d + b) + 1e-3); rho > 0: stop if current - new <
   min_relative_residual_increment current, else lambda *= max(lower, min(upper, 1 - (2 rho - 1)^3)), nu = 2, the trial
   becomes the state, then x, confidences, (H, b), and stop if the right-term test fires; rho <= 0: lambda *= nu, nu *= 2;
   lm_count++, stop if lm_count >= max_iteration_lm; repeat until rho > 0 or stop.  After the inner loop: stop if current <
   min_residual or iter >= max_iteration.
   reg_pose_graph_global_optimize: pass 1; prune (every certain edge stays, an uncertain one stays when its confidence is
   above edge_prune_threshold); pass 2 on the pruned graph (the edges keep their confidences); prune; C = pose_before(ref)
   pose_after(ref)^-1 (rigid inverse), pose <- C pose for every node (skipped when reference_node is out of range).
   The solver is a dense blocked Cholesky of H + lambda I on the device: its contract is a backward-error bar,
   and run-to-run bit equality.  A pivot that is not positive and finite: REG_BAD_TRANSFORM, reg_last_error names the row,
   the graph is left as it was.  Known open point: Open3D is believed to refuse certain edges between non-consecutive
   nodes; that is not reproduced. */
#define REG_POSE_GRAPH_MAX_NODES 2048
typedef struct reg_pose_graph reg_pose_graph;
typedef struct {
    int32_t struct_size;                       /* = sizeof(reg_pose_graph_params); checked */
    int32_t reference_node;                    /* 0 (Parameters.hpp:146); out of range: no compensation */
    double  max_correspondence_distance;       /* 10.0 (Parameters.hpp:143); finite, >= 0 */
    double  preference_loop_closure;           /* 2.0 (:144); finite, >= 0 */
    double  edge_prune_threshold;              /* 0.2 (:145); finite */
    int32_t max_iteration;                     /* 100; >= 0 */
    int32_t max_iteration_lm;                  /* 20; >= 1 */
    double  min_relative_increment;            /* 1e-6 */
    double  min_relative_residual_increment;   /* 1e-6 */
    double  min_right_term;                    /* 1e-6 */
    double  min_residual;                      /* 1e-6 */
    double  upper_scale_factor;                /* 2/3 */
    double  lower_scale_factor;                /* 1/3 */
} reg_pose_graph_params;
typedef enum {
    REG_PG_STOP_NONE = 0,
    REG_PG_STOP_RIGHT_TERM = 1,          /* max b < min_right_term */
    REG_PG_STOP_INCREMENT = 2,           /* |d| < min_relative_increment (|x| + min_relative_increment) */
    REG_PG_STOP_RESIDUAL_INCREMENT = 3,  /* current - new < min_relative_residual_increment current */
    REG_PG_STOP_MAX_ITERATION_LM = 4,    /* lm_count >= max_iteration_lm */
    REG_PG_STOP_MIN_RESIDUAL = 5,        /* current < min_residual */
    REG_PG_STOP_MAX_ITERATION = 6        /* iter >= max_iteration */
} reg_pose_graph_stop;
typedef struct {
    int32_t struct_size;       /* = sizeof(reg_pose_graph_result), set by the caller */
    int32_t outer_iterations;  /* outer iterations entered */
    int32_t lm_solves;         /* solves of (H + lambda I) d = b */
    int32_t accepted_steps;    /* steps with rho > 0 that became the state */
    int32_t stop_reason;       /* reg_pose_graph_stop */
    int32_t valid_edges;       /* edges with confidence above edge_prune_threshold after the pass */
    double  first_residual, last_residual, last_lambda, weight;
} reg_pose_graph_result;
typedef struct {
    int32_t struct_size;       /* = sizeof(reg_pose_graph_info), set by the caller */
    int32_t n_nodes, n_edges, n_uncertain;
    int64_t solver_rows;       /* rows of the padded factor buffer held (0: none yet) */
    int64_t device_bytes;      /* device memory the object holds */
} reg_pose_graph_info;
REG_API void reg_default_pose_graph_params(reg_pose_graph_params* p);
/* The validation reg_pose_graph_create runs, without a device. */
REG_API reg_status reg_check_pose_graph_params(const reg_pose_graph_params* p);
/* sizeof of reg_pose_graph_params, reg_pose_graph_result, reg_pose_graph_info */
REG_API void reg_pose_graph_struct_sizes(int32_t sizes[3]);
REG_API reg_status reg_pose_graph_create(reg_handle* h, const reg_pose_graph_params* params, reg_pose_graph** out);
REG_API void reg_pose_graph_destroy(reg_pose_graph* g);   /* before reg_destroy of its handle */
REG_API reg_status reg_pose_graph_clear(reg_pose_graph* g);   /* no nodes, no edges; the device buffers stay */
/* Replaces the graph (host arrays): poses n_nodes x 16, src / tgt / uncertain n_edges int32, X n_edges x 16, info n_edges x
   36, confidence n_edges (NULL: all 1).  REG_BAD_ARGUMENT before any device work for 1 <= n_nodes <=
   REG_POSE_GRAPH_MAX_NODES or n_edges >= 0 violated, an id out of range, source == target, a confidence outside [0, 1],
   a non-finite entry. */
REG_API reg_status reg_pose_graph_set(reg_pose_graph* g, const double* poses, int64_t n_nodes, const int32_t* src,
                                      const int32_t* tgt, const double* X, const double* info, const int32_t* uncertain,
                                      const double* confidence, int64_t n_edges);
/* The factor-level hook (as reg_linearize): H (6 n x 6 n, may be NULL), b (6 n), zeta (n_edges x 6), the residual and the
   line-process weight at the current poses and confidences.  Any output may be NULL. */
REG_API reg_status reg_pose_graph_linearize(reg_pose_graph* g, double* H, double* b, double* zeta, double* residual,
                                            double* weight);
REG_API reg_status reg_pose_graph_optimize(reg_pose_graph* g, reg_pose_graph_result* result);             /* one LM pass */
REG_API reg_status reg_pose_graph_global_optimize(reg_pose_graph* g, reg_pose_graph_result result[2]);   /* GlobalOptimization */
/* The graph as it stands: poses (capacity_nodes x 16), src / tgt / confidence (capacity_edges each); any may be NULL.
   REG_BAD_ARGUMENT, writing nothing, when a capacity is below the rows. */
REG_API reg_status reg_pose_graph_get(reg_pose_graph* g, int64_t capacity_nodes, double* poses, int64_t capacity_edges,
                                      int32_t* src, int32_t* tgt, double* confidence, int64_t* n_edges);
/* For every edge of the graph as it stands its index in the list reg_pose_graph_set received (which edges a prune kept). */
REG_API reg_status reg_pose_graph_get_edge_ids(reg_pose_graph* g, int64_t capacity_edges, int32_t* ids);
REG_API reg_status reg_pose_graph_get_info(const reg_pose_graph* g, reg_pose_graph_info* info);
/* Host-only (no device): one edge's zeta (6), Js, Jt (6 x 6 row-major, either may be NULL); the pose vector; the pose step;
   the line-process weight of n_edges information matrices (n_edges x 36). */
REG_API reg_status reg_host_pose_graph_edge(const double Ts[16], const double Tt[16], const double X[16], double zeta[6],
                                            double Js[36], double Jt[36]);
REG_API reg_status reg_host_pose_vector(const double T[16], double x[6]);
REG_API reg_status reg_host_pose_step(const double delta[6], const double pose[16], double out[16]);
REG_API reg_status reg_host_line_process_weight(const double* info, int64_t n_edges, double preference,
                                                double max_correspondence_distance, double* weight);

/* ---- the submap collection, resident on the device: o3d_slam::SubmapCollection ----------------------------
   SubmapCollection (SubmapCollection.cpp) with its AdjacencyMatrix (AdjacencyMatrix.cpp), the candidate rule of
   PlaceRecognition::getLoopClosureCandidatesIdxs (PlaceRecognition.cpp:231-284) and the pair selection of
   computeOdometryConstraints (constraint_builders.cpp:92-118).  reg_submaps is that object on a handle: it owns up to
   max_submaps map clouds (each a reg_map_cloud with the contract of that section, created from `map`), per submap the
   occupancy set of Submap::voxelMap_ as ascending unique 64-bit voxel keys (8 bytes per voxel), and the overlap buffer as a
   ring of num_scans_overlap device copies of pre-processed scans (points, optional normals / covariances, pose, stamp).  It
   works on the handle's stream and working storage, is as non-re-entrant as the handle and MUST BE DESTROYED BEFORE IT.
   Submap index == submap id (the reference never removes a submap).  Matrices: double[16], column-major.

   Occupancy set and revisiting fitness (Submap.cpp:239-240,260-264; SubmapCollection.cpp:390-402):
     key of a point: floor(p * inv) per axis with inv = 1.0 / (voxel_expansion_factor * map.map_voxel_size) -- a multiplication
       by the inverse (VoxelHashMap.hpp:48-51), not a division -- packed as the map voxel key of the other sections;
     DEPARTURE (the dense map's refused-keys rule): a row with a NaN or infinite coordinate or an index beyond
       +-(2^20 - 1) gets NO key (the reference hashes any int triple); a scan point without a key counts as not contained;
     the scan point is p' = R p + t with each row ((R0 x + R1 y) + R2 z) + t (no division by w: Isometry * point);
     count = scan points whose key is in the candidate's set (an integer; the same on every run);
     fitness = (double)count / (double)n_scan; n_scan == 0 gives NaN, and NaN is not > revisit_min_fitness: the check fails.
     Oddities reproduced: the set is rebuilt ONLY by reg_submaps_compute_features; reg_submaps_transform leaves it where it
       was (Submap::transform does not touch voxelMap_, Submap.cpp:115-128); a submap whose features were never computed
       has an empty set, so every revisit of it fails the check.

   reg_submaps_create: the constructor's first submap: id 0, parent 0, origin identity (SubmapCollection.cpp:28-32);
     num_scans_overlap == 0 is refused (:253).
   reg_submaps_insert_scan is SubmapCollection::insertScan (:189-245) with updateActiveSubmap (:94-148) inside, in this order:
     1. mapToRangeSensor_ and timestamp_ become the call's; the pre-processed scan is copied into the ring (the oldest entry
        leaves when the ring is full) BEFORE the decision;
     2. the decision is reg_host_submaps_decide on: the force flag; the scans merged into the active submap against
        min_num_range_data; is_use_initial_map; the closest submap over getMapToSubmapCenter() -- the translation of the origin
        until a centre has been computed -- where the FIRST minimum wins on ties; the rows of the active map against
        max_num_points, which only SETS the force flag: it takes effect at the NEXT call (reproduced); the distance to the
        closest centre against radius (strictly less); adjacency; the fitness verdict, computed only when it is reached;
        the distance to the active centre against radius (strictly greater).  Distances are sqrt((dx dx + dy dy) + dz dz).
     3. unchanged active submap: it receives the scan as reg_map_cloud_insert_scan with carving.
        changed (switched or created; a created submap has the next id, parent = the previous active index, origin = T):
        the PREVIOUS submap receives the scan with carving; its centre is computed (GetCenter) and marked computed; it is
        pushed to the finished queue with the stamp; the scans-merged counter returns to 0; the edge previous -- active is
        added (both loop-closure marks are cleared: AdjacencyMatrix::addEdge writes false, reproduced); the ring is drained,
        oldest first, into the now active submap with rawScan = scan and no carving (:87-92).
     4. the scans-merged counter goes up by one.
     A non-empty scan sets the receiving submap's own mapToRangeSensor_ (Submap.cpp:45).  is_carving_enabled == 0 never
     carves.  is_use_initial_map with an empty receiving map: the map becomes the scan as reg_map_cloud_set with
     map.map_voxel_size (Submap.cpp:47-52).  An empty scan inserts nothing but still enters the ring and the decision.
     Departure: the reference's assert "submap should not be empty after switching" is not raised.
   reg_submaps_force_new_submap (:180-187): the force flag, an insert of an EMPTY scan at the stored pose and stamp, flag off.
   reg_submaps_compute_features: the device half of Submap::computeFeatures (Submap.cpp:255-275), in this order:
     the gate `features computed before && now_seconds - last < min_seconds_between_features` (then *computed = 0 and nothing
     is written); with feature params: the sparse cloud = reg_voxel_down_sample of the map's points at feature_voxel_size,
     cast to fp32; its normals = reg_estimate_normals (normal_knn within normal_radius, oriented towards the origin, unit
     length); its features = reg_compute_fpfh (feature_knn within feature_radius), each with the contract of that operator
     and all on device pointers of this handle -- the map is not copied back; then the occupancy set is rebuilt from the
     current map cloud and the clock value is stored.  The outputs (n_sparse x 3 floats, x 3 floats, x 33 doubles, host or
     device pointers by on_device, any may be NULL) are written last; capacity_rows below the sparse rows is
     REG_BAD_ARGUMENT with nothing changed (the rows of the map are always enough).  params == NULL: the occupancy set only.
     An empty map gives n_sparse = 0.  The finished entry is then pushed to the loop-closure candidate queue by
     reg_submaps_push_loop_closure_candidate (SubmapCollection.cpp:268).
   reg_submaps_transform is SubmapCollection::transform (:322-373): every listed submap gets its own increment; every other
     submap walks up its parents to the first listed one (the plan is reg_host_submaps_transform_plan); "Stuck in a loop"
     becomes REG_BAD_TRANSFORM with nothing changed; the ring is flushed.  Per submap as Submap::transform: the map cloud
     (PointCloud::Transform), mapToRangeSensor_ = mapToRangeSensor_ * T, centre = T * centre (rows ((T0 x + T1 y) + T2 z) + T3);
     the origin mapToSubmap_ and the occupancy set stay (oddities reproduced).  Oddity reproduced: an unlisted submap reads
     transformIncrements.at(parent), the parent's POSITION in the list, not the entry whose id is the parent; a position
     beyond the list throws in the reference and is REG_BAD_TRANSFORM here.  An id >= the number of submaps is skipped.  An
     empty list only flushes the ring.
   Failure contract.  Bad arguments, unknown indices and an exhausted max_submaps (REG_BAD_ARGUMENT) are detected before
     anything changes.  Each device step commits by its map cloud's buffer swap; host state -- active index, queues,
     adjacency, counters, poses, the ring -- is committed only after the last device step of a call succeeded.  If a device
     step fails in the middle of a switch, the map clouds the earlier steps completed keep their new content (the previous
     submap already holds the scan; some ring scans may already be in the target submap) while every piece of host state
     is as before the call: repeating the call would insert those scans twice.  A REG_BAD_ARGUMENT of a map cloud step
     (a refused voxel key) behaves the same way.  In reg_submaps_transform the same holds per submap.
   Dense maps: reg_submaps_enable_dense_maps gives every submap, existing and future (created inside
     reg_submaps_insert_scan or reg_submaps_force_new_submap), a reg_dense_map of voxel_size with the contract of that section;
     they are destroyed with the collection.  A second enable is REG_BAD_ARGUMENT; every dense call on a collection without
     dense maps is REG_NOT_CONFIGURED.  A collection on which they were never enabled behaves exactly as before.
     reg_submaps_insert_scan_dense_map is Submap::insertScanDenseMap (Submap.cpp:98-113) on submap idx, in this order:
       1. reg_dense_map_insert_scan with the stored scan parameters (the cropper's centre as given: zero is the reference);
       2. if perform_carving, the map is not empty and scans_inserted % carve_every_n_scans == 1: reg_dense_map_carve_scan of
          the scan -- raw (the reference's frame oddity), or transformed by T with carve_in_map_frame -- from the sensor at
          the translation of T;
       3. scans_inserted goes up by one.
     Oddities reproduced: carve_every_n_scans == 1 never carves (x % 1 is 0), and a submap's first insert never carves.
     Failure contract of the insert: argument errors and an unknown idx are detected before any device work; if step 1 fails
     nothing has changed; if step 2 fails after a committed step 1, the map keeps the inserted scan and scans_inserted is NOT
     advanced (repeating the call would insert the scan twice).
     reg_submaps_transform additionally applies reg_dense_map_transform -- the literal arithmetic of
     VoxelizedPointCloud::transform, wrong for t != 0 as that section says -- to every submap that receives an increment,
     right after that submap's map cloud and under the same per-submap commit rule.
   Out of scope: dumpToFile, the dense-map worker's thread and buffer, the feature thread, the mutexes.  Building the
     constraints is the section after this one. */
typedef struct reg_submaps reg_submaps;
typedef struct {
    int32_t struct_size;                  /* = sizeof(reg_submaps_params); checked */
    int32_t max_submaps;                  /* 1 .. 4096 (the reference reserves 500); default 64 */
    int32_t num_scans_overlap;            /* submaps_.numScansOverlap_ (3); >= 1 */
    int32_t min_num_range_data;           /* submaps_.minNumRangeData_ (5) */
    int32_t is_use_initial_map;           /* isUseInitialMap_ (0) */
    int32_t is_carving_enabled;           /* isCarvingEnabled_ (0, Parameters.hpp:181) */
    int32_t min_submaps_between_loop_closures;   /* placeRecognition_.minSubmapsBetweenLoopClosures_ (2) */
    int32_t reserved;
    int64_t max_num_points;               /* submaps_.maxNumPoints_ (400000); >= 0 */
    double  radius;                       /* submaps_.radius_ (20) */
    double  revisit_min_fitness;          /* submaps_.adjacencyBasedRevisitingMinFitness_ (0.4) */
    double  voxel_expansion_factor;       /* magic::voxelExpansionFactorAdjacencyBasedRevisiting (2.5); factor * voxel finite, > 0 */
    double  min_seconds_between_features; /* submaps_.minSecondsBetweenFeatureComputation_ (5) */
    double  loop_closure_search_radius;   /* placeRecognition_.loopClosureSearchRadius_ (20) */
    reg_map_cloud_params map;             /* of every submap's map cloud; map_voxel_size > 0 */
} reg_submaps_params;
typedef struct {
    int32_t struct_size;                  /* = sizeof(reg_submaps_info), set by the caller */
    int32_t n_submaps;
    int32_t active;                       /* activeSubmapIdx_ */
    int32_t force_new_submap;             /* isForceNewSubmapCreation_ */
    int32_t scans_in_active;              /* numScansMergedInActiveSubmap_ */
    int32_t ring_size;                    /* scans in the overlap buffer */
    int32_t n_finished;                   /* entries of the finished queue */
    int32_t n_loop_closure_candidates;
    int32_t last_finished;                /* lastFinishedSubmapIdx_ (0 at first) */
    int32_t reserved;
    int64_t total_points;                 /* getTotalNumPoints */
    int64_t stamp_ns;                     /* timestamp_ */
    double  T_map_to_sensor[16];          /* mapToRangeSensor_ */
} reg_submaps_info;
typedef struct {
    int32_t struct_size;                  /* = sizeof(reg_submap_info), set by the caller */
    int32_t id, parent;
    int32_t center_computed;              /* isCenterComputed_ */
    int32_t features_computed;            /* reg_submaps_compute_features has run on it */
    int32_t reserved;
    int64_t n_rows, scans_inserted;       /* of its map cloud */
    int64_t n_keys;                       /* occupied voxels of the occupancy set */
    double  origin[16];                   /* mapToSubmap_ */
    double  center[3];                    /* getMapToSubmapCenter(): the computed centre, else the origin's translation */
    double  crop_center[3];               /* the cropper centre of its map cloud */
    double  T_map_to_sensor[16];          /* the submap's own mapToRangeSensor_ */
    double  feature_clock;                /* now_seconds of the last feature computation */
} reg_submap_info;
typedef struct {
    int32_t struct_size;                  /* = sizeof(reg_submaps_insert_result), set by the caller */
    int32_t decision;                     /* the bits of reg_host_submaps_decide */
    int32_t previous_active, active;
    int32_t fitness_computed;             /* the revisiting check ran */
    int32_t ring_drained;                 /* scans moved from the ring into the now active submap */
    int64_t fitness_count;                /* its count */
    double  fitness;                      /* and its fitness (NaN for an empty scan) */
    reg_map_cloud_insert_result insert;   /* of the scan into the submap that received it with carving */
} reg_submaps_insert_result;
typedef struct {
    int32_t struct_size;                  /* = sizeof(reg_submap_feature_params); checked */
    int32_t normal_knn;                   /* placeRecognition_.normalKnn_ (10); 1 .. 32 */
    int32_t feature_knn;                  /* placeRecognition_.featureKnn_ (100); 2 .. 128 */
    int32_t reserved;
    double  feature_voxel_size;           /* placeRecognition_.featureVoxelSize_ (0.5); finite, > 0 */
    double  normal_radius;                /* placeRecognition_.normalEstimationRadius_ (1.0); > 0 */
    double  feature_radius;               /* placeRecognition_.featureRadius_ (2.5); finite, > 0 */
} reg_submap_feature_params;
REG_API void reg_default_submaps_params(reg_submaps_params* p);
REG_API void reg_default_submap_feature_params(reg_submap_feature_params* p);
/* The validation reg_submaps_create runs, without a device. */
REG_API reg_status reg_check_submaps_params(const reg_submaps_params* p);
/* sizeof of reg_submaps_params, reg_submaps_info, reg_submap_info, reg_submaps_insert_result, reg_submap_feature_params */
REG_API void reg_submaps_struct_sizes(int32_t sizes[5]);
REG_API reg_status reg_submaps_create(reg_handle* h, const reg_submaps_params* params, reg_submaps** out);
REG_API void reg_submaps_destroy(reg_submaps* s);   /* before reg_destroy of its handle */
REG_API reg_status reg_submaps_get_info(const reg_submaps* s, reg_submaps_info* info);
REG_API reg_status reg_submaps_get_submap_info(const reg_submaps* s, int32_t idx, reg_submap_info* info);
/* setMapToRangeSensor (SubmapCollection.cpp:34-36) */
REG_API reg_status reg_submaps_set_map_to_sensor(reg_submaps* s, const double T[16]);
/* raw_xyz: the raw scan in the sensor frame (the carve's rays; NULL with n_raw == 0); scan_*: the pre-processed scan in the
   sensor frame with exactly the fields of `map`; all host or all device pointers; result may be NULL and is written only
   by a call that returns REG_OK.  A host raw scan is uploaded only when the carve of the receiving map is due. */
REG_API reg_status reg_submaps_insert_scan(reg_submaps* s, const double* raw_xyz, int64_t n_raw, const double* scan_xyz,
                                           const double* scan_normals, const double* scan_covs, int64_t n_scan, int on_device,
                                           const double T_map_to_sensor[16], int64_t stamp_ns,
                                           reg_submaps_insert_result* result);
REG_API reg_status reg_submaps_force_new_submap(reg_submaps* s, reg_submaps_insert_result* result);
REG_API reg_status reg_submaps_compute_features(reg_submaps* s, int32_t idx, double now_seconds,
                                                const reg_submap_feature_params* params, int on_device, float* sparse_xyz,
                                                float* sparse_normals, double* fpfh, int64_t capacity_rows, int64_t* n_sparse,
                                                int32_t* computed);
/* The occupancy keys of a submap, ascending (a host array of capacity_rows uint64; may be NULL to learn *n_out). */
REG_API reg_status reg_submaps_get_keys(reg_submaps* s, int32_t idx, uint64_t* keys, int64_t capacity_rows, int64_t* n_out);
/* The factor-level hook of the revisiting check: count and fitness of a scan at pose T against the set of submap idx. */
REG_API reg_status reg_submaps_switch_fitness(reg_submaps* s, int32_t idx, const double* scan_xyz, int64_t n, int on_device,
                                              const double T[16], int64_t* count, double* fitness);
/* cropSubmap + initReference of the ACTIVE submap: reg_map_cloud_set_target of its map cloud. */
REG_API reg_status reg_submaps_set_target(reg_submaps* s, const reg_crop* crop, int64_t* n_kept);
/* One submap's map cloud as reg_map_cloud_export. */
REG_API reg_status reg_submaps_export_submap(reg_submaps* s, int32_t idx, int on_device, double* xyz, double* normals,
                                             double* covs, int64_t capacity_rows, int64_t* n_out);
/* Mapper::getAssembledMapPointCloud: every submap's rows in submap order, one copy per submap and column into the caller's
   arrays; capacity_rows < total_points returns REG_BAD_ARGUMENT, writing nothing. */
REG_API reg_status reg_submaps_export(reg_submaps* s, int on_device, double* xyz, double* normals, double* covs,
                                      int64_t capacity_rows, int64_t* n_out);
/* ids[n] with dT[16 n] (column-major), in the order of the reference's transformIncrements. */
REG_API reg_status reg_submaps_transform(reg_submaps* s, const int32_t* ids, const double* dT, int32_t n);
/* ---- the dense maps of the collection (the comment above) ---- */
typedef struct {
    int32_t struct_size;                  /* = sizeof(reg_submaps_dense_params); checked */
    int32_t carve_every_n_scans;          /* carving_.carveSpaceEveryNscans_ (10); >= 1 */
    int32_t carve_in_map_frame;           /* 0: the reference's frame oddity; 1: the scan is transformed before the carve */
    int32_t reserved;
    double  voxel_size;                   /* denseMapBuilder_.mapVoxelSize_ (0.03); finite, > 0 */
    reg_dense_scan_params  scan;          /* denseMapCropper_ (centre as given; zero is the reference) + colour range */
    reg_dense_carve_params carve;         /* checked against voxel_size as reg_dense_map_carve checks */
} reg_submaps_dense_params;
typedef struct {
    int32_t struct_size;                  /* = sizeof(reg_submaps_dense_insert_result), set by the caller */
    int32_t carved;                       /* the gate let the carve run */
    int64_t n_inserted;                   /* points that passed both croppers */
    int64_t n_voxels;                     /* of the submap's dense map after the call */
    int64_t n_removed;                    /* voxels the carve erased */
    int64_t scans_inserted;               /* nScansInsertedDenseMap_ after the call */
} reg_submaps_dense_insert_result;
/* shipped: every 10 scans, the reference's frame, voxel 0.03, no crop, colours within [0, 1], the shipped carve */
REG_API void reg_default_submaps_dense_params(reg_submaps_dense_params* p);
/* The validation reg_submaps_enable_dense_maps runs, without a device. */
REG_API reg_status reg_check_submaps_dense_params(const reg_submaps_dense_params* p);
/* sizeof of reg_submaps_dense_params, reg_submaps_dense_insert_result */
REG_API void reg_submaps_dense_struct_sizes(int32_t sizes[2]);
REG_API reg_status reg_submaps_enable_dense_maps(reg_submaps* s, const reg_submaps_dense_params* params);
/* xyz / normals / colors: the raw scan in the sensor frame, n x 3 doubles each (normals, colors may be NULL), all host or all
   device pointers; result may be NULL and is written only by a call that returns REG_OK. */
REG_API reg_status reg_submaps_insert_scan_dense_map(reg_submaps* s, int32_t idx, const double* xyz, const double* normals,
                                                     const double* colors, int64_t n, int on_device,
                                                     const double T_map_to_sensor[16], int32_t perform_carving,
                                                     reg_submaps_dense_insert_result* result);
/* reg_dense_map_get_info of submap idx and its nScansInsertedDenseMap_ (either output may be NULL). */
REG_API reg_status reg_submaps_get_dense_info(const reg_submaps* s, int32_t idx, reg_dense_map_info* info,
                                              int64_t* scans_inserted);
/* getDenseMapCopy().toPointCloud() of submap idx: reg_dense_map_export of its dense map, ascending key order. */
REG_API reg_status reg_submaps_export_dense_submap(reg_submaps* s, int32_t idx, int on_device, double* xyz, double* normals,
                                                   double* colors, int32_t* keys, int32_t* counts, int64_t capacity_rows,
                                                   int64_t* n_out);
/* updateAdjacencyMatrix (:75-81): per constraint addEdge(source, target), then both marked as loop-closure submaps. */
REG_API reg_status reg_submaps_add_loop_closure_edges(reg_submaps* s, const int32_t* source, const int32_t* target, int32_t n);
/* The adjacency matrix: adj (capacity x capacity bytes, row-major, 1 = an entry of adjacency_) and marks (capacity
   int32: -1 no entry in isLoopClosureSubmap_, 0 false, 1 true); capacity >= n_submaps, either output may be NULL. */
REG_API reg_status reg_submaps_get_adjacency(const reg_submaps* s, uint8_t* adj, int32_t* marks, int32_t capacity);
/* popFinishedSubmapIds / popLoopClosureCandidates: the queue in order, then emptied; capacity below the entries returns
   REG_BAD_ARGUMENT and pops nothing. */
REG_API reg_status reg_submaps_pop_finished(reg_submaps* s, int32_t* ids, int64_t* stamps_ns, int32_t capacity, int32_t* n_out);
REG_API reg_status reg_submaps_pop_loop_closure_candidates(reg_submaps* s, int32_t* ids, int64_t* stamps_ns, int32_t capacity,
                                                           int32_t* n_out);
REG_API reg_status reg_submaps_push_loop_closure_candidate(reg_submaps* s, int32_t id, int64_t stamp_ns);
/* getLoopClosureCandidatesIdxs for last_finished against the active submap, in ascending index order, with these tests in
   this order: i == active; isAdjacent(i, active); |i - last_finished| == 1 or isAdjacent(i, last_finished); centre distance
   > loop_closure_search_radius; |i - last_finished| <= ceil(search radius / radius); the BFS distance of last_finished
   to the nearest loop-closure submap < min_submaps_between_loop_closures. */
REG_API reg_status reg_submaps_loop_closure_candidates(const reg_submaps* s, int32_t last_finished, int32_t* out,
                                                       int32_t capacity, int32_t* n_out);
/* The pair selection of computeOdometryConstraints.  candidates != NULL (constraint_builders.cpp:92-106): per candidate id >=
   1 the pair (parent, id).  candidates == NULL (:108-118): every submap 1 .. n - 1 whose pair touches neither end the
   active submap.  A pair already in existing (n_existing x 2: source, target) or chosen earlier in this call is skipped
   (hasConstraint).  out: capacity x 2. */
REG_API reg_status reg_submaps_odometry_constraint_pairs(const reg_submaps* s, const int32_t* candidates, int32_t n_candidates,
                                                         const int32_t* existing, int32_t n_existing, int32_t* out,
                                                         int32_t capacity, int32_t* n_out);

/* Pure host functions (no device, no object). */
enum {
    REG_SUBMAPS_KEEP = 0, REG_SUBMAPS_SWITCH = 1, REG_SUBMAPS_CREATE = 2, REG_SUBMAPS_NEED_FITNESS = 3,   /* bits 0..1 */
    REG_SUBMAPS_ACTION_MASK = 3,
    REG_SUBMAPS_SET_FORCE_FLAG = 4,    /* the active map exceeds max_num_points: the flag is set for the NEXT call */
    REG_SUBMAPS_FORCED = 8             /* the force flag was consumed (and cleared) by this creation */
};
/* The branch table of updateActiveSubmap.  fitness_ok: 1 / 0 the verdict of the revisiting check, -1 not known yet: then
   REG_SUBMAPS_NEED_FITNESS is returned exactly where the reference would run the check (the caller computes it and asks
   again).  closest_is_active: findClosestSubmap returned the active index; adjacent: isAdjacent(closest, active). */
REG_API int32_t reg_host_submaps_decide(int32_t force_flag, int32_t scans_in_active, int32_t min_num_range_data,
                                        int32_t is_use_initial_map, int64_t active_points, int64_t max_num_points,
                                        int32_t closest_is_active, double distance_to_closest, double distance_to_active,
                                        double radius, int32_t adjacent, int32_t fitness_ok);
/* getDistanceToNearestLoopClosureSubmap on an n x n byte matrix and marks as reg_submaps_get_adjacency returns them:
   INT_MAX when no node has a mark entry; a BFS in ascending neighbour order from id to the first marked node popped;
   max(0, hops - 1); when no marked node is reachable the walk ends at the LAST node popped and its hops count (reproduced).
   -1: bad arguments, or the reference would throw (a popped node without a mark entry or without adjacency). */
REG_API int32_t reg_host_adjacency_distance(const uint8_t* adj, const int32_t* marks, int32_t n, int32_t id);
/* Which increment each submap receives in SubmapCollection::transform: plan[i] = the POSITION in ids of the increment
   applied to submap i (several listed entries for one id all apply, in list order: plan holds the last), or -1 for
   none.  Returns REG_BAD_TRANSFORM for "Stuck in a loop" and for a position beyond the list. */
REG_API reg_status reg_host_submaps_transform_plan(const int32_t* parents, int32_t n_submaps, const int32_t* ids, int32_t n,
                                                   int32_t* plan);
/* The Mapper's initial guess (Mapper.cpp:250-260) in fp64 with rigid inverses (as DESIGN 5z chose), column-major:
   Ci = calib^-1; A = odom_now Ci; B = odom_prev Ci; M = B^-1 A (odometryMotion); out = prev_map_to_sensor M.  Every product
   entry is ((a0 b0 + a1 b1) + a2 b2) + a3 b3; the rigid inverse is [R^T | -((R0i t0 + R1i t1) + R2i t2)]. */
REG_API reg_status reg_host_mapper_initial_guess(const double prev_map_to_sensor[16], const double odom_prev[16],
                                                 const double odom_now[16], const double calib[16], double out[16]);

/* ---- pose-graph constraints from the resident submap collection -----------------------------------------------
   buildConstraint (constraint_builders.cpp:43-90), the refinement half of buildLoopClosureConstraints
   (PlaceRecognition.cpp:97-149), computeOdometryConstraints (constraint_builders.cpp:92-118) with the list the reference's
   SubmapCollection owns (odometryConstraints_), and the per-submap store of Submap::sparseMapCloud_ / feature_ -- all on
   the map clouds where they live.  Everything here is an addition to the reg_submaps section above.

   reg_submaps_build_constraint runs, in this order and with both map clouds as device pointers:
     1. is_compute_overlap != 0: reg_set_pair_overlap_f64 with T_init as T_src_to_tgt (NULL stays NULL), overlap_voxel_size
        and min_points_per_voxel = 1; else reg_set_target_f64 of the target without a crop, then reg_set_source_f64 of the
        source.  The target's normals are passed only for REG_COST_O3D_P2PL, the covariances of both only for REG_COST_GICP,
        the source's normals never -- the fields the stateless builders pass;
     2. unless skip_refinement: reg_register from (float)T_init; T = the fp32 result widened.  Skipped: T = (float)T_init
        widened, fitness = inlier_rmse = 0, iterations = converged = 0;
     3. with estimate_information: reg_information_matrix at (float)T with information_max_distance; else the identity and
        n_info_pairs = 0.
   The steps run on a handle the collection owns, never on the collection's handle: one per cost in use, created by the
   first call that names the cost with reg_default_params + {cost, use_trimmed = 0, gicp_stop_rule = 1 for GICP}, on the
   collection's stream (re-read at every call, as the normals workspace does), max_dist = icp_max_correspondence_distance
   and max_iter = max_iteration set per call, destroyed with the collection.  The reference, the reading and the chain
   configuration of the collection's handle are not touched.  The arithmetic is that of the named operators: no kernel of
   its own.
   Statuses: REG_BAD_ARGUMENT for a NULL or wrongly sized params / result, a cost other than REG_COST_O3D_P2PL,
   REG_COST_O3D_P2P or REG_COST_GICP, max_iteration < 1, icp_max_correspondence_distance not finite or <= 0,
   information_max_distance not finite, <= 0 or > icp_max_correspondence_distance (the reach of the search structure both
   run on), an overlap voxel not finite or <= 0 with is_compute_overlap, an unknown index or source == target -- all
   before any device work; REG_EMPTY_TARGET for an empty submap of the pair or no shared voxel; REG_MISSING_FIELD for
   point-to-plane without target normals or GICP without covariances; otherwise what the named operator returns.  *out is
   written only on REG_OK; a failing call changes nothing in the collection (the text is in reg_last_error of its handle).
   Matrices: T double[16] column-major; information[36] as reg_information_matrix writes it. */
typedef struct {
    int32_t struct_size;                    /* = sizeof(reg_constraint_params); checked */
    int32_t cost;                           /* REG_COST_O3D_P2PL (buildConstraint), REG_COST_O3D_P2P or REG_COST_GICP */
    int32_t max_iteration;                  /* magic::icpRunUntilConvergenceNumberOfIterations (100) */
    int32_t is_compute_overlap;
    int32_t skip_refinement;
    int32_t estimate_information;
    double  overlap_voxel_size;
    double  icp_max_correspondence_distance;
    double  information_max_distance;
} reg_constraint_params;
typedef struct {
    int32_t struct_size;                    /* = sizeof(reg_constraint_result), set by the caller */
    int32_t source, target;
    int32_t iterations, converged;          /* of reg_result */
    int32_t refined;                        /* reg_register ran */
    int32_t information_estimated;          /* isInformationMatrixValid_ */
    int32_t reserved;
    int64_t n_source_selected, n_target_selected;   /* rows of the reading / the reference (all rows without the overlap) */
    int64_t n_info_pairs;
    double  fitness, inlier_rmse;           /* of reg_result */
    double  T[16];                          /* sourceToTarget_ */
    double  information[36];
} reg_constraint_result;
/* buildOdometryConstraint's arguments (constraint_builders.cpp:33-41): point-to-plane, 100 iterations, overlap at
   20 x the map voxel size, both distances 1.5 x it (0.04 m stands in for a map voxel size of zero, which getMapVoxelSize,
   helpers.cpp:356-358, takes to be |size| <= 1e-3), information estimated, skip_refinement = !refine. */
REG_API reg_status reg_default_odometry_constraint_params(const reg_submaps* s, int refine, reg_constraint_params* p);
/* The argument checks of reg_submaps_build_constraint on the params alone, without a device. */
REG_API reg_status reg_check_constraint_params(const reg_constraint_params* p);
/* sizeof of reg_constraint_params, reg_constraint_result */
REG_API void reg_constraints_struct_sizes(int32_t sizes[2]);
REG_API reg_status reg_submaps_build_constraint(reg_submaps* s, int32_t source, int32_t target,
                                                const reg_constraint_params* params,
                                                const double T_init[16] /* NULL: identity */, reg_constraint_result* out);
/* computeOdometryConstraints into the list the collection owns.  The pairs are those of
   reg_submaps_odometry_constraint_pairs against that list (candidates == NULL: the overload without candidates); each is
   built by reg_submaps_build_constraint from the identity and appended with isOdometryConstraint_ = 1.  params == NULL:
   reg_default_odometry_constraint_params without refinement.  All or nothing: when a pair fails, the status is that pair's
   and the list is as before.  n_added may be NULL. */
REG_API reg_status reg_submaps_compute_odometry_constraints(reg_submaps* s, const int32_t* candidates, int32_t n,
                                                            const reg_constraint_params* params, int32_t* n_added);
/* getOdometryConstraints: *n_out entries in list order; source / target (capacity int32 each), T (capacity x 16,
   column-major), information (capacity x 36), flags (bit 0: isInformationMatrixValid_, bit 1: isOdometryConstraint_); any
   array may be NULL (all NULL: the count).  capacity below the entries with an array given: REG_BAD_ARGUMENT. */
REG_API reg_status reg_submaps_get_odometry_constraints(const reg_submaps* s, int32_t capacity, int32_t* source, int32_t* target,
                                                        double* T, double* information, int32_t* flags, int32_t* n_out);
REG_API reg_status reg_submaps_clear_odometry_constraints(reg_submaps* s);
/* The feature store.  reg_submaps_compute_features with feature params, when it succeeds, also keeps the submap's sparse
   cloud (fp64 and fp32), its normals and its FPFH rows in buffers of that submap (device-to-device copies; 312 bytes per
   sparse row), so that the features of one submap outlive the computation of the next.  reg_submaps_get_features hands
   them out (host or device pointers by on_device; any may be NULL): xyz64 n x 3 doubles, xyz n x 3 floats, normals n x 3
   floats, fpfh n x 33 doubles.  A submap without stored features gives *n_out = 0; capacity_rows below the rows with an
   array given is REG_BAD_ARGUMENT.  reg_submaps_transform moves the stored sparse cloud of every submap it moves, as
   Submap::transform does (Submap.cpp:117): the fp64 point by the formula of reg_map_cloud_transform, the fp32 point is its
   cast, the normal (nx', ny', nz') = the rotation rows applied to the fp32 normal widened, each ((R0 nx + R1 ny) + R2 nz),
   cast back to fp32; the features stay. */
REG_API reg_status reg_submaps_get_features(reg_submaps* s, int32_t idx, int on_device, double* sparse_xyz64, float* sparse_xyz,
                                            float* sparse_normals, double* fpfh, int64_t capacity_rows, int64_t* n_out);
/* PlaceRecognition::isRegistrationConsistent (PlaceRecognition.cpp:182-229), host-only: T column-major; bounds = maxDrift
   roll, pitch, yaw [rad], x, y, z [m].  The rotation block becomes a quaternion as Eigen's Quaterniond(Matrix3d) forms it,
   is normalised, and toRPY (math.cpp:39-46) gives roll = atan2(2 (w x + y z), 1 - 2 (x x + y y)), pitch = asin(2 (w y - x z)),
   yaw = atan2(2 (w z + x y), 1 - 2 (y y + z z)).  *failed_mask gets bit k for every component k (roll, pitch, yaw, x, y, z) with
   fabs(value) > bounds[k] -- strictly greater, so a value on its bound passes and a NaN never fails (reproduced).
   Consistent == a mask of 0.  REG_BAD_ARGUMENT for a NULL argument. */
REG_API reg_status reg_host_registration_consistent(const double T[16], const double bounds[6], int32_t* failed_mask);
/* PlaceRecognition::buildLoopClosureConstraints (PlaceRecognition.cpp:50-176) for one finished submap, on the feature store:
   for every index of reg_submaps_loop_closure_candidates(last_finished), in order, with source = last_finished and
   target = the candidate:
     1. reg_match_features of the stored FPFH rows (33 columns) with the backward search and the mutual filter; the
        correspondences are the mutual pairs when there are at least ransac.ransac_n of them, else every (a, nn_ab[a]) -- as
        Open3D falls back; reg_ransac_correspondences on the stored fp64 sparse clouds with `ransac` as given (the seed
        included: the same for every candidate).  All arrays stay on the device.  n_correspondences = its n_inliers;
     2. n_correspondences < ransac_min_correspondence_set_size: REG_LC_RANSAC_SET_TOO_SMALL;
     3. reg_host_registration_consistent of the RANSAC transform with consistency_bounds fails: REG_LC_RANSAC_INCONSISTENT;
     4. reg_submaps_build_constraint(source, target, &refine, T_ransac): `constraint` is written, refined = 1;
     5. constraint.fitness < min_refinement_fitness: REG_LC_FITNESS_TOO_LOW;
     6. reg_host_registration_consistent of constraint.T fails: REG_LC_ICP_INCONSISTENT; else REG_LC_ACCEPTED.
   A source or a candidate without stored features takes step 2 with zero correspondences and the identity.  The feature
   steps run on the builders' point-to-point handle, not on the collection's.  Accepted constraints are NOT stored in the
   collection (the reference hands them to the optimisation problem; isOdometryConstraint_ = 0, timestamp_ = stamp_ns).
   verdicts: capacity records (may be NULL with capacity 0 when there is no candidate); the caller sets struct_size in the
   first, the call writes one whole record per candidate.  *n_candidates is set whenever the candidates could be listed.  capacity below the candidates, an unknown index, a wrong
   struct_size or refused `refine` parameters: REG_BAD_ARGUMENT before any device work.  A step that fails ends the call
   with its status; the verdicts are written only on REG_OK.  Nothing in the collection changes either way. */
enum {
    REG_LC_ACCEPTED = 0, REG_LC_RANSAC_SET_TOO_SMALL = 1, REG_LC_RANSAC_INCONSISTENT = 2, REG_LC_FITNESS_TOO_LOW = 3,
    REG_LC_ICP_INCONSISTENT = 4
};
typedef struct {
    int32_t struct_size;                    /* = sizeof(reg_loop_closure_params); checked */
    int32_t ransac_min_correspondence_set_size;   /* placeRecognition_.ransacMinCorrespondenceSetSize_ (25) */
    double  min_refinement_fitness;         /* placeRecognition_.minRefinementFitness_ */
    double  consistency_bounds[6];          /* consistencyCheck_: maxDrift roll, pitch, yaw [rad], x, y, z [m] */
    reg_ransac_params ransac;               /* struct_size checked by reg_ransac_correspondences */
    reg_constraint_params refine;
} reg_loop_closure_params;
typedef struct {
    int32_t struct_size;                    /* = sizeof(reg_loop_closure_verdict), set by the caller in the first record */
    int32_t source, candidate;
    int32_t verdict;                        /* REG_LC_* */
    int32_t ransac_failed_mask, icp_failed_mask;   /* of reg_host_registration_consistent, where it ran */
    int32_t refined;                        /* step 4 ran: `constraint` is valid */
    int32_t reserved;
    int64_t n_correspondences;              /* ransacResult.correspondence_set_.size() */
    int64_t ransac_iterations;              /* the stop index */
    int64_t stamp_ns;                       /* timestamp_ */
    double  ransac_fitness, ransac_inlier_rmse;
    double  T_ransac[16];                   /* column-major */
    reg_constraint_result constraint;
} reg_loop_closure_verdict;
/* sizeof of reg_loop_closure_params, reg_loop_closure_verdict */
REG_API void reg_loop_closure_struct_sizes(int32_t sizes[2]);
REG_API reg_status reg_submaps_build_loop_closure_constraints(reg_submaps* s, int32_t last_finished, int64_t stamp_ns,
                                                              const reg_loop_closure_params* params,
                                                              reg_loop_closure_verdict* verdicts, int32_t capacity,
                                                              int32_t* n_candidates);

#ifdef __cplusplus
}
#endif
#endif /* O3DSLAM_REG_H */
