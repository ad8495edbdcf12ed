/* =====================================================================================
 * clc.h — C-ABI of the MI355X-native point-to-plane extrinsic solver ("clc" = Cam-Laser
 * Calibration).  This is the drop-in boundary: host code (the C++ adapter in
 * include/LaseCamCalCeres.h, the Python mirror in camlasercalibratool_amd/) calls these
 * entry points; everything behind them is hand-written HIP for gfx950.
 *
 * Plain pointers and sizes only; no exceptions cross this boundary; every function returns
 * an int status (CLC_OK == 0, negative on error — the reference itself has no error
 * codes).  All arithmetic is IEEE FP64.  Host pointers unless a parameter
 * says "device".  Calls on one handle are blocking and must not overlap; different
 * handles are independent (one HIP stream per handle).
 *
 * Each entry point cites the reference interface it replaces (paths relative to the
 * reference root, MegviiRobot/CamLaserCalibraTool).
 * ===================================================================================== */
#ifndef CLC_H_
#define CLC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLC_VERSION 210

/* status codes */
#define CLC_OK 0
#define CLC_ERR_INVALID_ARG (-1)
#define CLC_ERR_HIP (-2)        /* HIP runtime / launch failure: see clc_last_error()        */
#define CLC_ERR_NONFINITE (-3)  /* non-finite input pose or evaluation                      */
#define CLC_ERR_EMPTY_SCAN (-4) /* boundary mode on an empty `points` (reference throws
                                   std::out_of_range at src/LaseCamCalCeres.cpp:278)         */
#define CLC_ERR_NO_DATA (-5)    /* solve/eval before upload                                 */
#define CLC_ERR_LINALG (-6)     /* (reserved; round 1 returned it for a rank-deficient 9x9 closed-form
                                   system — the pivoted LDLT back end now solves those like the reference) */
#define CLC_ERR_NO_DEVICE (-7)  /* no gfx950 device / HIP runtime unavailable                */
#define CLC_ERR_COMM (-8)       /* RCCL unavailable or a collective failed: see clc_last_error() */

/* termination codes of clc_summary.termination (ceres::TerminationType + which test) */
#define CLC_RUNNING 0
#define CLC_CONVERGENCE_GRADIENT 1
#define CLC_CONVERGENCE_PARAMETER 2
#define CLC_CONVERGENCE_FUNCTION 3
#define CLC_CONVERGENCE_RADIUS 4
#define CLC_NO_CONVERGENCE 5
#define CLC_FAILURE 6

typedef struct clc_handle clc_handle;

/* One residual block, exactly the state a PointInPlaneFactor + its CauchyLoss hold
 * (src/LaseCamCalCeres.cpp:19-21,249): 8 doubles = 64 bytes, the unit of algorithmic
 * traffic.  The observation array handed to clc_upload is an array of
 * these. */
typedef struct clc_observation {
  double n[3];  /* plane normal in the camera frame (planar_.head(3))                        */
  double d;     /* plane offset (planar_[3])                                                */
  double p[3];  /* laser point in the laser frame (point_)                                  */
  double scale; /* 1/sqrt(points in this scan) (scale_, :239-240); loss a = 0.05*scale       */
} clc_observation;

/* Solver options.  Defaults (clc_options_default) = what the reference runs:
 * src/LaseCamCalCeres.cpp:302-304 (DENSE_QR, 100 iterations) + Ceres defaults + the
 * hard-coded Cauchy loss of :212,:249. */
typedef struct clc_options {
  int32_t max_num_iterations;                /* 100                                          */
  int32_t max_num_consecutive_invalid_steps; /* 5                                            */
  int32_t jacobi_scaling;                    /* 1                                            */
  int32_t use_loss;                          /* 1  (#define LOSSFUNCTION)                    */
  double loss_scale_factor;                  /* 0.05  -> CauchyLoss(0.05*scale)              */
  double initial_trust_region_radius;        /* 1e4                                          */
  double max_trust_region_radius;            /* 1e16                                         */
  double min_trust_region_radius;            /* 1e-32                                        */
  double min_relative_decrease;              /* 1e-3                                         */
  double min_lm_diagonal;                    /* 1e-6                                         */
  double max_lm_diagonal;                    /* 1e32                                         */
  double function_tolerance;                 /* 1e-6                                         */
  double gradient_tolerance;                 /* 1e-10                                        */
  double parameter_tolerance;                /* 1e-8                                         */
  /* execution knobs (no effect on results beyond reduction order) */
  int32_t launch_ahead;  /* launch-ahead depth: LM iterations the host keeps queued beyond the
                             last one the device reported done (pinned mailbox, no blocking
                             sync); 0 = library default (2)                                  */
  int32_t profile_events; /* 1: bracket every evaluation-kernel launch with HIP events on the
                             handle's stream and report them in clc_summary (the solve then
                             uses the [evaluation, controller] launch pair, not the one-launch
                             step kernel); 2: when the solve is ONE launch (see clc_solve), an
                             event pair around it -> eval_kernel_ms, eval_kernel_launches = 1;
                             otherwise controller cycle stamps only (debug)                    */
} clc_options;

/* ceres::IterationSummary subset, one per recorded iteration (iteration 0 = initial
 * evaluation).  Replaces summary.FullReport() (src/LaseCamCalCeres.cpp:309). */
typedef struct clc_iteration {
  int32_t iteration;
  int32_t step_is_valid;
  int32_t step_is_successful;
  int32_t pad_;
  double cost;
  double cost_change;
  double gradient_max_norm;
  double step_norm;
  double relative_decrease;
  double trust_region_radius;
} clc_iteration;

typedef struct clc_summary {
  int32_t termination;            /* CLC_CONVERGENCE_* / CLC_NO_CONVERGENCE / CLC_FAILURE    */
  int32_t num_iterations;         /* recorded iterations - 1 (clc_solve: 0 when none was)    */
  int32_t num_successful_steps;
  int32_t num_unsuccessful_steps;
  int64_t num_evaluations;        /* fused residual+Jacobian passes over the observations    */
  double initial_cost;
  double final_cost;
  double solve_ms;                /* host wall time of the call                              */
  double eval_kernel_ms;          /* sum of evaluation-kernel durations (profile_events=1)   */
  int64_t eval_kernel_launches;   /* number of launches summed in eval_kernel_ms             */
} clc_summary;

/* ---- library ------------------------------------------------------------------------ */
int clc_version(void);
/* Last error text of the calling thread ("" if none). */
const char* clc_last_error(void);
void clc_options_default(clc_options* opt);

/* ---- handle ------------------------------------------------------------------------- */
/* Creates a solver context on HIP device `device` (one stream, scratch buffers).  It also loads the code objects of the single-problem
 * paths and pays what only the first launch / copy / allocation of a process pays (tens of ms next to the ~130-150 ms of HIP context
 * creation), so that the first call on the handle costs about what a warm one does — the reference's programs call the path once
 * per process (main/calibr_offline.cpp:166-170).  The batched kernels' code object is loaded by the first clc_upload_batched.
 * CLC_LAZY_MODULES=1 in the environment leaves all of it to the first launches.
 * CLC_ERR_NO_DEVICE without a GPU: there is no CPU fallback. */
int clc_create(clc_handle** out, int device);
void clc_destroy(clc_handle* h);
/* Run on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream);
 * NULL restores the handle's own stream.  The switch drains the previous stream first (a finished
 * solve may still have a few no-op launches queued on it), so work on the new stream never overlaps
 * work of this handle on the old one.  Device pointers handed to this library (clc_upload_device,
 * the *_device entry points) must be ready on the handle's CURRENT stream. */
int clc_set_stream(clc_handle* h, void* hip_stream);
/* Explicit choice of the streaming paths — what the A/B tests and the profiling scripts use; a caller keeps the default (-1).
 * grid_blocks = workgroups of the evaluation / step launches (0 = library default: one 512-thread workgroup per CU).
 * flags = -1: library default = 2|16|32|128|256|512 with the size-dependent choices made per launch (non-temporal loads and deeper
 *   pipelines beyond the 256 MiB Infinity Cache) AND the on-chip solve paths of clc_solve (clc_set_auto_paths).  Any explicit value
 *   selects the streaming paths only (clc_solve = step chain / launch pair), as a sum of:
 *      1  reference shuffle reduction instead of the butterfly          2  software prefetch of the next tile (64-byte tiles)
 *      4  non-temporal loads                                           16  compact 28-byte layout where available (lossless; arrays without
 *     32  512-thread workgroups (3:2 old/young wave shares)                dense scans, and the step chain below 2e5 observations)
 *     64  compact layout: two tiles in flight per wave                128  clc_solve = ONE step_kernel launch per LM iteration (needs 32 and 16 or 256)
 *    256  row layout (scans padded to rows of 64 points: 16 B/point + a 64-byte descriptor per row, per-scan moments; 24 B/point when p.z != 0)
 *    512  row layout: equal wave shares cut at scan starts           1024  batched row kernel in 256-thread workgroups (default: one wave each)
 *   2048  batched solver: lockstep [evaluation, controller] launches 4096  batched solver: not the on-chip resident kernel (at upload: its
 *   8192  resident layout over 512 lanes even where 256 hold it            layout is not built)
 * Results change only in summation order. */
int clc_set_launch(clc_handle* h, int grid_blocks, int flags);

/* Which of the size-chosen default paths of clc_solve (flags = -1 above) may run; disable_mask is a sum of
 * 1 = not the cooperative one-launch solve (11 264 < n <= 2.6e6 observations: 256 co-resident workgroups keep the problem on
 *     chip and exchange their rows through device memory — fast on an otherwise idle GPU; a launch whose workgroups are not all
 *     resident within 0.2 ms aborts, falls back to the step chain and rests the path on the handle for 16 solves, doubling):
 *     a process that shares the GPU with long-running kernels can switch it off here and keep every other default;
 * 2 = not the single-workgroup on-chip solve (n <= 11 264 observations);
 * 8 = (at upload) not the 32-workgroup one-hop form of the cooperative solve for problems of at most 106 496 observations
 *     (every workgroup reads all 32 rows itself: one store-to-load hop per pass instead of two) — the 256-workgroup form then.
 * 0 = library default: every bit of the mask DISABLES a path.  The environment variable CLC_AUTO_PATHS_DISABLE sets the initial mask
 * of every handle. */
int clc_set_auto_paths(clc_handle* h, int disable_mask);
/* Opt-in (at upload): a problem one workgroup holds (n <= 11 264) ALSO gets the cooperative layout and clc_solve runs it on 32 co-resident
 * workgroups first — 4.6 instead of 5.3-5.9 us per pass (C1 0.132 -> 0.116 ms per solve, 10 000 observations 0.135 -> 0.107) —, with the
 * single-workgroup kernel as the fall-back when that launch times out or rests.  Not the default: upload and first solve cost ~0.2 ms more
 * (a second layout, the exchange boards), which the reference's one calibration per process never earns back; worth it from about a
 * dozen solves per upload on an otherwise idle GPU.  CLC_SMALL_ON_COOP=1 in the environment sets it on every new handle. */
int clc_set_small_on_coop(clc_handle* h, int enable);

/* Which layouts the last clc_upload* / clc_select_observations / clc_upload_batched* built on this handle, and how the
 * cooperative path is doing: a caller that sizes its problems, or shares the GPU, can see whether clc_solve and
 * clc_solve_batched run from registers + LDS in one launch or on the streaming paths (operational query; no reference
 * counterpart). */
typedef struct clc_path_info {
  int32_t single_resident;         /* 1: clc_solve = ONE single-workgroup launch (<= 512 lanes x 22 points, a lane holds one scan's points) */
  int32_t single_lanes;
  int32_t single_points_per_lane;
  int32_t coop_resident;           /* 1: the lane layout of the cooperative kernel is built: clc_solve = ONE launch of 256 workgroups */
  int32_t coop_points_per_lane;    /* <= 40 (<= 26 when the points carry z) */
  int32_t coop_points_carry_z;     /* 1: some record has p.z != 0: 24-byte slots */
  int32_t coop_resting;            /* 1: after a launch that timed out the path rests (the step chain runs) until its back-off expires */
  int32_t coop_timeouts;           /* cooperative launches that timed out on this handle */
  int32_t batched_resident;        /* 1: clc_solve_batched = ONE launch of the resident kernel */
  int32_t batched_lanes;           /* 256 / 512 lanes per problem */
  int32_t batched_points_per_lane;
  int32_t rows_layout;             /* single problem's streaming row layout: 0 none, 1 (x, y) rows, 2 rows that carry z */
  int32_t batched_rows_layout;
  int32_t coop_workgroups;         /* 256, or 32: the one-hop form for problems of at most 32 x 256 x 13 points */
  int32_t batched_points_carry_z;  /* 1: the batch has p.z != 0 somewhere and is held on chip in 24-byte slots (512 lanes x <= 22 points per problem) */
  int32_t reserved_;
  int64_t coop_solves;             /* solves that ran on the cooperative kernel */
  int64_t batched_lane_rows;       /* point rows of the batched lane layout (x lanes x 16 bytes = its size) */
  int64_t n_rows;                  /* rows of 64 points of the streaming row layouts */
  int64_t batched_n_rows;
  int64_t coop_gate_waits_expired; /* cooperative solves that took the step chain because another handle of this process held the device's
                                    * one-cooperative-launch-at-a-time gate for more than 5 ms (clc_version() >= 210; fields are only appended) */
} clc_path_info;
int clc_get_path_info(const clc_handle* h, clc_path_info* out);

/* Name (NUL-terminated, truncated to name_cap) and compute-unit count of the handle's device; either out pointer may be NULL. */
int clc_device_info(clc_handle* h, char* name, int name_cap, int* num_cus);

/* ---- problem assembly (host) --------------------------------------------------------
 * Replaces the residual-block construction loop of CamLaserCalibration,
 * src/LaseCamCalCeres.cpp:222-295 (plane per pose :227-231, scale :239-240, board-edge
 * terms :258-294 with pi_from_ppp src/utilities.cpp:267-272).  Input is the flattened
 * std::vector<Oberserve> (include/LaseCamCalCeres.h:11-24): tag_q[n_poses*4] as (w,x,y,z),
 * tag_t[n_poses*3], CSR offsets/points for `points` and `points_on_line`.
 * records == NULL only counts.  *n_records receives N. */
int clc_flatten_observations(int n_poses, const double* tag_q_wxyz, const double* tag_t,
                             const int64_t* pts_off, const double* pts,
                             const int64_t* ptl_off, const double* ptl,
                             int use_linefitting_data, int use_boundary_constraint,
                             clc_observation* records, int64_t* n_records);

/* ---- resident scans + problem assembly on the device ------------------------------------
 * The same residual-block construction (src/LaseCamCalCeres.cpp:222-295), but the pose-major data of
 * std::vector<Oberserve> — tag poses and the scan points, 24 bytes per point — is what crosses PCIe, once, and
 * stays resident; the 64-byte records of any (use_linefitting_data, use_boundary_constraint) selection are then
 * built on the device, bitwise equal to clc_flatten_observations' (every operation individually rounded, same
 * order), and handed to the upload pipeline without touching the host.  This is how the drop-in header runs
 * closed form -> calibration -> analysis pass of main/calibr_offline.cpp:166-170 on ONE upload
 * (clc_adapter::Session).  Arguments as clc_flatten_observations.  clc_select_observations replaces the
 * observation array of the handle (as clc_upload would); CLC_ERR_EMPTY_SCAN as for the host path. */
/* Page-locked host memory for arrays handed to clc_store_observations / clc_upload*: from pageable memory the runtime
 * pins and unpins the caller's pages around every copy (tens of milliseconds for 50 MB when the buffer is a fresh
 * allocation each call); from these buffers the copy is a plain DMA.  NULL on failure. */
void* clc_pinned_alloc(size_t bytes);
void clc_pinned_free(void* p);
int clc_store_observations(clc_handle* h, int n_poses, const double* tag_q_wxyz, const double* tag_t,
                           const int64_t* pts_off, const double* pts, const int64_t* ptl_off, const double* ptl);
int clc_select_observations(clc_handle* h, int use_linefitting_data, int use_boundary_constraint,
                            int64_t* n_records);
/* Number of successful clc_store_observations calls on this handle so far (-1 for NULL).  The stored scans belong to the
 * handle, not to whoever stored them: a caller that keeps "its" scans across calls on a shared handle (the Session of
 * the drop-in header) remembers this stamp and re-stores, or refuses to go on, when it has moved. */
int64_t clc_store_generation(const clc_handle* h);

/* ---- observation array --------------------------------------------------------------
 * Copies N records to the device and re-tiles them for coalesced 16-byte loads.  Stays
 * resident until the next upload/destroy.  `clc_upload_device` takes a DEVICE pointer to
 * the same AoS layout (e.g. a torch tensor's data_ptr()). */
int clc_upload(clc_handle* h, const clc_observation* records, size_t n);
int clc_upload_device(clc_handle* h, const clc_observation* records_dev, size_t n);
size_t clc_num_observations(const clc_handle* h);

/* ---- plug-in level math (element-wise parity) ---------------------------------------
 * PointInPlaneFactor::Evaluate for every uploaded record at `pose` (src/LaseCamCalCeres.cpp
 * :43-66): residuals[N] (raw, before the loss) and, if non-NULL, jacobians[N*7] row-major
 * 1x7 rows exactly as the factor writes them (7th column zero, :60). */
int clc_factor_evaluate(clc_handle* h, const double pose[7], double* residuals,
                        double* jacobians);
/* PoseLocalParameterization::Plus, batched on the device
 * (src/pose_local_parameterization.cpp:15-31): x[n*7], delta[n*6] -> x_plus_delta[n*7]. */
int clc_pose_plus(clc_handle* h, const double* x, const double* delta, double* x_plus_delta,
                  size_t n);
/* PoseLocalParameterization::ComputeJacobian: 7x6 row-major [I6;0] (cpp:33-40). */
int clc_pose_plus_jacobian(const double x[7], double jacobian[42]);

/* ---- one evaluation pass --------------------------------------------------------------
 * What Ceres' evaluator + loss corrector produce per evaluation, reduced to the normal
 * equation: cost = 1/2 sum rho, g[6] = J~^T r~, H[21] = upper triangle of J~^T J~
 * (row-major: 00 01 .. 05 11 ..).  with_loss=0 drops the Cauchy loss (analysis pass,
 * src/LaseCamCalCeres.cpp:316-362).  g/H may be NULL (cost-only pass). */
int clc_eval(clc_handle* h, const double pose[7], int with_loss, double loss_scale_factor,
             double* cost, double g[6], double H[21]);

/* ---- the solve ------------------------------------------------------------------------
 * Replaces ceres::Solve on the problem built by CamLaserCalibration
 * (src/LaseCamCalCeres.cpp:299-307): Levenberg-Marquardt trust region with Jacobi scaling
 * on the uploaded observations, SE(3) local parameterisation, Cauchy loss; runs entirely
 * on the device.  pose is in/out = [tx,ty,tz,qx,qy,qz,qw] (:219, :311-314).
 * trace (nullable) receives up to trace_cap iteration records.
 * With the library's default launch flags the whole solve is ONE launch when the problem fits on chip:
 * up to 11 264 observations in one workgroup (all p.z == 0, every lane's points from one scan), up to ~2.6e6
 * across 256 co-resident workgroups (~1.7e6 when some p.z != 0: 24-byte slots) (csrc/clc_coop.hpp; needs a
 * 256-CU device, falls back by itself otherwise or when its exchange times out — see clc_set_auto_paths);
 * beyond that — or with explicit clc_set_launch flags — one launch per LM iteration.  Same LM
 * decisions on every path; sums are taken in different orders (results agree to rounding). */
int clc_solve(clc_handle* h, const clc_options* opt, double pose[7], clc_summary* summary,
              clc_iteration* trace, int trace_cap);

/* ---- post-solve analysis ---------------------------------------------------------------
 * src/LaseCamCalCeres.cpp:316-381: un-robustified H = sum J^T J (6x6 row-major),
 * b = -sum J^T r, chi2 = sum r^2, singular values of H (descending), V (columns), and the
 * count of singular values < 1e-8 (null-space dimension).  The caller uploads the point
 * residuals only (the reference skips the board-edge terms here). */
int clc_information(clc_handle* h, const double pose[7], double H[36], double b[6],
                    double* chi2, double sv[6], double V[36], int* n_null);

/* ---- closed-form initialiser ------------------------------------------------------------
 * CamLaserCalClosedSolution, src/LaseCamCalCeres.cpp:112-203, on the uploaded
 * points_on_line records (uses n, d, p.x, p.y only, :147): device reduction of the 9x9
 * normal equation (16 bytes per point on the row layout), host 9x9 pivoted LDL^T solve (Eigen's ldlt(),
 * :181, pseudo-inverse of D) + U V^T of the 3x3 SVD (:195-196).  Tlc[16] row-major 4x4;
 * *unobservable = 1 if any singular value of A^T A < 1e-10 (:164-171) — like the reference the
 * function then still returns the Tlc the factorisations give (CLC_ERR_NONFINITE only if that is not
 * finite; *unobservable is set either way); sv9 nullable. */
int clc_closed_form(clc_handle* h, double Tlc[16], int* unobservable, double sv9[9]);

/* ---- closed form and analysis pass of every problem of the uploaded batch --------------------
 * The first and the last of the reference's three steps (main/calibr_offline.cpp:166-170) for all P problems of
 * clc_upload_batched* at once, on the device: per problem a device reduction (split over several workgroups when the
 * batch is small), then one wave per problem runs the dense back end (same sweep order, stopping rule and pivot rule as
 * the single-problem calls).  Record-set rule, as for clc_closed_form / clc_information: the closed form takes the
 * points_on_line records, the analysis pass the point records without board-edge terms — a caller who solved with
 * board-edge terms uploads the point records again for these two calls.
 *
 * clc_closed_form_batched: CamLaserCalClosedSolution for every problem; each problem's records are taken as points_on_line
 * records (n, d, p.x, p.y; z ignored) exactly as clc_closed_form does.  status[P] (required): CLC_OK, CLC_ERR_NO_DATA
 * (empty problem), CLC_ERR_NONFINITE (non-finite solution).  One problem's failure does not fail the call.
 * poses[P*7] (nullable): the start pose Tcl = Tlc^-1 of every CLC_OK problem; other problems' poses are left as they were.
 * Passing the handle's own buffer (clc_batched_host_buffers) writes it in place, ready for clc_solve_batched in place.
 * Tlc[P*16], unobservable[P], sv9[P*9]: nullable (left as they were for an empty problem). */
int clc_closed_form_batched(clc_handle* h, double* poses, double* Tlc, int32_t* unobservable, double* sv9, int32_t* status);

/* clc_information_batched: the analysis pass of clc_information for every problem at poses[P*7] (may be the handle's own
 * buffer).  Poses are validated as in clc_solve_batched.  chi2[P], sv[P*6], n_null[P] required; H[P*36], b[P*6], V[P*36]
 * nullable.  An empty problem reports H = 0, chi2 = 0 and n_null = 6. */
int clc_information_batched(clc_handle* h, const double* poses, double* H, double* b, double* chi2, double* sv,
                            double* V, int32_t* n_null);

/* ---- batched independent problems ---------------------------------------------------------
 * P independent T_cl problems (own observations, own pose, own LM state), problem k owning
 * records [offsets[k], offsets[k+1]).  One workgroup per problem runs the whole LM loop on
 * the device.  poses[P*7] in/out, summaries[P]. */
int clc_upload_batched(clc_handle* h, const clc_observation* records, const int64_t* offsets,
                       size_t n_problems);
/* records_dev: DEVICE pointer to the same AoS records (ready on the handle's stream); offsets stay a host array. */
int clc_upload_batched_device(clc_handle* h, const clc_observation* records_dev, const int64_t* offsets,
                              size_t n_problems);
int clc_solve_batched(clc_handle* h, const clc_options* opt, double* poses,
                      clc_summary* summaries);
/* The handle's own page-locked, device-mapped arrays for the poses (in/out, [P*7]) and summaries ([P]) of the uploaded batch
 * (valid until the next clc_upload_batched* / clc_destroy).  Passing exactly these two pointers to clc_solve_batched solves
 * in place: the start poses are read and the results written over PCIe by the kernels themselves, and the two staging
 * copies per call (a megabyte at 8 192 problems, ~10 % of a C4-shard solve) are skipped. */
int clc_batched_host_buffers(clc_handle* h, double** poses, clc_summary** summaries);
size_t clc_num_problems(const clc_handle* h);

/* ---- scan line fitting (the step that produces points_on_line) -----------------------------
 * LineFittingCeres, src/LaseCamCalCeres.cpp:385-433, for n_scans scans at once.  Scan k owns
 * points [offsets[k], offsets[k+1]) of xy[2*M] (x, y of every scan point; z is not used, :412).
 * lines[2*n_scans] is in/out = (m0, m1) of the line m0 x + m1 y + 1 = 0: initial guess in (:403),
 * result out (:430-431).  Residual m0 x + m1 y + 1 (:391), CauchyLoss(opt->loss_scale_factor) per
 * point (:416), the same Ceres LM semantics as clc_solve.  clc_line_options_default() = Ceres
 * defaults with max_num_iterations = 10 and loss 0.05 (:416,:424-425).  summaries nullable.
 * A scan with a non-finite point has a non-finite cost at iteration 0: as in Ceres that scan ends
 * with termination = CLC_FAILURE and its line left as it was.  The call still returns CLC_OK, and
 * every other scan, the three that share its wavefront included, gets the bits it gets without
 * that scan.  Refused with CLC_ERR_INVALID_ARG: opt->use_loss with loss_scale_factor <= 0 or NaN,
 * max_num_iterations < 0, offsets that decrease.  Refused with CLC_ERR_NONFINITE: a non-finite
 * start line. */
void clc_line_options_default(clc_options* opt);
int clc_line_fit_batched(clc_handle* h, const clc_options* opt, const double* xy, const int64_t* offsets,
                         size_t n_scans, double* lines, clc_summary* summaries);
/* The same with every array in DEVICE memory (ready on the handle's stream; results are complete on that stream when
 * the call returns — it synchronises): xy_dev[2*M], offsets_dev[n_scans+1] (absolute, offsets_dev[0] may be > 0),
 * lines_dev[2*n_scans] in/out, summaries_dev nullable.  Offsets and start lines are not validated. */
int clc_line_fit_batched_device(clc_handle* h, const clc_options* opt, const double* xy_dev, const int64_t* offsets_dev,
                                size_t n_scans, double* lines_dev, clc_summary* summaries_dev);

/* TranScanToPoints, src/utilities.cpp:181-215, for n_scans (<= 65535) scans at once: scan k owns rays
 * [offsets[k], offsets[k+1]) of ranges[] (float32 as in sensor_msgs/LaserScan); ray i of scan k
 * sits at angle_min[k] + i * angle_increment[k] (:192-193) and becomes (r cos, r sin, 0), or
 * (1000, 1000, 0) when r is outside [range_min[k], 30) (:201-208).  points[3 * total rays]. */
int clc_scan_to_points(clc_handle* h, const float* ranges, const int64_t* offsets, size_t n_scans,
                       const float* angle_min, const float* angle_increment, const float* range_min,
                       double* points);
/* The same with every array in DEVICE memory (any number of scans; n_rays = offsets[n_scans] - offsets[0], which
 * the caller knows; offsets_dev[0] must be 0). */
int clc_scan_to_points_device(clc_handle* h, const float* ranges_dev, const int64_t* offsets_dev, size_t n_scans,
                              size_t n_rays, const float* angle_min_dev, const float* angle_increment_dev,
                              const float* range_min_dev, double* points_dev);

/* AutoGetLinePts, src/selectScanPoints.cpp:17-190 (the detection; the debug drawing is not reproduced), for n_scans scans at
 * once: the calibration board's segment in each scan.  Scan k owns points [offsets[k], offsets[k+1]) of points[3 * M]
 * ((x, y, z) doubles as clc_scan_to_points writes them).  The reference's quirks are kept: the search window is the middle
 * +-266 points (:36-45), every 3rd point is visited (:53-100), a segment still open when the loop ends is never pushed,
 * a current point at range == 100 or NaN never moves again (:96-99), each pushed segment is widened by up to 3 points at
 * either end, always against its original ends (:104-126), and the first of equally long segments wins (:139-148).
 * Ranges are |(x, y)| with each square and the sum rounded (no FMA), as Eigen's head(2).norm().
 * seg[2 * n_scans]: first and last index (inclusive, relative to the scan) of the chosen segment, or -1, -1.
 * status[n_scans] (nullable): CLC_SEG_FOUND, CLC_SEG_NONE, or CLC_SEG_REF_THROWS where the reference's points.at() raises
 * std::out_of_range — an empty scan (:46), or a pushed segment whose widening to the left would leave the scan (:121; possible
 * below 538 points, for any pushed segment, not only the chosen one; the widening to the right (:110) cannot leave it: the
 * point that closed the segment lies beyond it): seg is -1, -1 and the other scans are unaffected. */
#define CLC_SEG_FOUND 1
#define CLC_SEG_NONE 0
#define CLC_SEG_REF_THROWS (-1)
int clc_board_segments(clc_handle* h, const double* points, const int64_t* offsets, size_t n_scans, int64_t* seg, int32_t* status);
/* The same with every array in DEVICE memory (ready on the handle's stream; complete on return — it synchronises):
 * points_dev[3 * M], offsets_dev[n_scans + 1] (absolute, offsets_dev[0] may be > 0; not validated: monotone, and fewer than
 * 2^31 points per scan), seg_dev[2 * n_scans], status_dev nullable. */
int clc_board_segments_device(clc_handle* h, const double* points_dev, const int64_t* offsets_dev, size_t n_scans, int64_t* seg_dev,
                              int32_t* status_dev);

/* ---- the offline flow (K13): stamped tag poses + raw laser scans -> stored observations, main/calibr_offline.cpp:62-155 -----
 * Key frames (:62-78): pose 0 is kept; pose j is kept when dist > keyframe_dist_min || fabs(theta) > keyframe_theta_min against
 * the last kept pose, dist = |older.twc - newer.twc|, theta = 2 acos(w), w = (qo . qn) / |qo|^2 the scalar part of
 * older.qwc.inverse() * newer.qwc.  As in the reference: |w| > 1 gives NaN and the angle test is false, w < 0 gives theta > pi
 * (antipodal quaternions: kept), a NaN dist makes the distance test false.
 * Every scan goes through TranScanToPoints and AutoGetLinePts (clc_scan_to_points, clc_board_segments).  A scan with a segment
 * takes the key frame with the smallest fabs(pose_stamp - scan_stamp), the first of equal minima in key-frame order (:102-113: strict
 * <, from 10000; a NaN stamp is never chosen), accepted when that minimum < max_dt (:116).  The scans with a segment and a pose
 * become the observations, in scan order: points = the segment's points; tagPose_Qca = qwc.inverse(), tagPose_tca =
 * -Qca.toRotationMatrix() * twc (:145-146); a line is fitted to the points (clc_line_fit_batched under `line`, every fit started
 * at line0) and points_on_line = the two points of that line at the first and the LAST segment point's abscissa, or ordinate when
 * |dx| <= |dy| (:126-142; the reference reads points.end(), one past the end — the last point is used here), z = 0; a segment of
 * fewer than 2 points gets none.  A scan on which the reference's AutoGetLinePts throws (CLC_SEG_REF_THROWS: the reference's
 * program would terminate there) is dropped and counted.
 * The observations are left stored on the handle exactly as clc_store_observations leaves them (clc_store_generation is bumped):
 * clc_select_observations, clc_closed_form, clc_solve, clc_information follow as usual.  No observations at all: CLC_OK,
 * n_observations = 0, and the store is that of clc_store_observations with n_poses = 0.  The reference's gates "fewer than 10
 * poses" (:56) and "fewer than 5 observations" (:158) are the caller's. */
typedef struct clc_assemble_options {
  double keyframe_dist_min;  /* 0.20, :66 */
  double keyframe_theta_min; /* 3.1415926 * 10 / 180, :67 */
  double max_dt;             /* 0.02 s, :116 */
  double line0[2];           /* start of every line fit: (0, 0) */
  clc_options line;          /* clc_line_options_default */
} clc_assemble_options;
void clc_assemble_options_default(clc_assemble_options* opt);
typedef struct clc_assemble_info {
  int64_t n_keyframes;    /* poses the key-frame filter kept */
  int64_t n_segments;     /* scans with a board segment (CLC_SEG_FOUND) */
  int64_t n_ref_throws;   /* scans dropped with CLC_SEG_REF_THROWS */
  int64_t n_unmatched;    /* scans with a segment and no key frame within max_dt */
  int64_t n_observations; /* = n_segments - n_unmatched */
  int64_t n_points;       /* points of all observations */
  int64_t n_line_points;  /* points_on_line of all observations */
} clc_assemble_info;
#define CLC_SCAN_NO_SEGMENT (-1)
#define CLC_SCAN_REF_THROWS (-2)
#define CLC_SCAN_NO_POSE (-3)
/* The key-frame filter alone, on host arrays: q_wc_wxyz[4 * n_poses], t_wc[3 * n_poses] -> keep[n_poses] (1 / 0), *n_kept
 * (both nullable).  opt NULL: the defaults. */
int clc_keyframes(clc_handle* h, const clc_assemble_options* opt, size_t n_poses, const double* q_wc_wxyz, const double* t_wc,
                  uint8_t* keep, int64_t* n_kept);
/* pose_stamp[n_poses], q_wc_wxyz[4 * n_poses], t_wc[3 * n_poses]: every stamped tag pose (T_wc as in apriltag_pose.txt), in file
 * order.  Scan k owns rays [offsets[k], offsets[k+1]) of ranges[] (float32), with angle_min / angle_increment / range_min[k] and
 * the stamp scan_stamp[k]; any number of scans.  scan_pose[n_scans] (nullable): the ORIGINAL index of the pose a kept scan took,
 * or CLC_SCAN_NO_SEGMENT / CLC_SCAN_REF_THROWS / CLC_SCAN_NO_POSE.  info nullable.  Everything is uploaded once and computed on
 * the device; the counters, the offsets and (reference-size stores) the tag poses come back, point data does not.
 * CLC_ERR_INVALID_ARG: NULL arrays, offsets that decrease, a scan of 2^31 rays or more, 2^31 poses or more. */
int clc_assemble_observations(clc_handle* h, const clc_assemble_options* opt, size_t n_poses, const double* pose_stamp,
                              const double* q_wc_wxyz, const double* t_wc, const float* ranges, const int64_t* offsets, size_t n_scans,
                              const float* angle_min, const float* angle_increment, const float* range_min, const double* scan_stamp,
                              int32_t* scan_pose, clc_assemble_info* info);
/* The same with every array in DEVICE memory (ready on the handle's stream; complete on return — ONE synchronisation):
 * offsets_dev[n_scans + 1] with offsets_dev[0] == 0 and n_rays = offsets_dev[n_scans], which the caller knows (not validated:
 * monotone, fewer than 2^31 rays per scan); scan_pose_dev nullable (device memory); info on the host. */
int clc_assemble_observations_device(clc_handle* h, const clc_assemble_options* opt, size_t n_poses, const double* pose_stamp_dev,
                                     const double* q_wc_wxyz_dev, const double* t_wc_dev, const float* ranges_dev,
                                     const int64_t* offsets_dev, size_t n_scans, size_t n_rays, const float* angle_min_dev,
                                     const float* angle_increment_dev, const float* range_min_dev, const double* scan_stamp_dev,
                                     int32_t* scan_pose_dev, clc_assemble_info* info);
/* The scans stored on the handle (by clc_store_observations or clc_assemble_observations), copied back: *n_poses, tag_q_wxyz
 * [4 P], tag_t[3 P], pts_off[P + 1], pts[3 M], ptl_off[P + 1], ptl[3 ML]; every pointer nullable (a first call with the arrays
 * NULL gives n_poses, then the offsets give M and ML — or take them from clc_assemble_info).  CLC_ERR_NO_DATA: nothing stored. */
int clc_stored_observations(clc_handle* h, int* n_poses, double* tag_q_wxyz, double* tag_t, int64_t* pts_off, double* pts,
                            int64_t* ptl_off, double* ptl);

/* ---- static stations (K14): averaged tag poses and station-mode assembly, GetStaticPose, src/utilities.cpp:86-155 ----------
 * For recordings where the board is held still at stations.  The walk (:96-124): a run starts at pose a with xy_sum = t_a and
 * size = 1 (the pose is pushed); candidate j = a, a + 1, ... is a member iff |t_j - xy_sum / size| < center_dist_max (norm():
 * every square and sum rounded; the centre a per-component division) and then does xy_sum += t_j, ++size; the first candidate
 * that is no member closes the run [a, j - 1], is discarded, and the next run starts at j + 1.  As in the reference: the first
 * pose of a run is tested against itself and counted twice (in size, in the running centre and in the averages), so a run of k
 * distinct poses has k + 1 members; a run is a station iff members > min_members (30: k >= 30); a NaN translation is never a
 * member (at a run's start: a run of one member); the run still open at the end of the list is dropped, unless close_last_run.
 * The average (:129-152) of a station with members m0 (twice), m1, ...: t = sum t / n; q = the unit eigenvector of the largest
 * eigenvalue of A = sum q q^T / n, q as (w, x, y, z) (getAvergeQwc, :156-166; the reference takes Eigen::EigenSolver's vector,
 * whose sign is arbitrary — here cyclic Jacobi, and the sign is fixed: w > 0, or the first non-zero component positive when
 * w == 0); start_time / end_time = the stamps of the first and the last member (include/utilities.h:19-20).  A station whose
 * average is not finite gets status CLC_STATION_NONFINITE, q = (1, 0, 0, 0), t = 0, and takes no scan.
 * Station-mode assembly is clc_assemble_observations with a different tie between scans and poses: a scan with a board segment
 * takes the FIRST station, in station order, with start_time <= scan_stamp <= end_time (both ends inclusive; a NaN stamp never
 * matches) and becomes one observation with that station's averaged pose.  This interval matching is this library's design —
 * the reference has no node that consumes GetStaticPose.  Everything else (segments, line fits, points_on_line, the order of the
 * observations, how they are left stored on the handle) is as for clc_assemble_observations. */
typedef struct clc_station_options {
  double center_dist_max; /* 0.002 m, :108 */
  int64_t min_members;    /* 30, :119: a station has members > 30, the first pose counted twice */
  int32_t close_last_run; /* 0: the run open at the end of the list is dropped (the reference); 1: it is closed like any other */
  int32_t reserved;       /* 0 */
  double line0[2];        /* start of every line fit: (0, 0) */
  clc_options line;       /* clc_line_options_default */
} clc_station_options;
void clc_station_options_default(clc_station_options* opt);
typedef struct clc_station_info {
  int64_t n_runs;         /* runs the walk closed */
  int64_t n_stations;     /* those with members > min_members */
  int64_t n_nonfinite;    /* stations with status CLC_STATION_NONFINITE */
  int64_t n_segments;     /* scans with a board segment (CLC_SEG_FOUND) */
  int64_t n_ref_throws;   /* scans dropped with CLC_SEG_REF_THROWS */
  int64_t n_unmatched;    /* scans with a segment and no station that holds their stamp */
  int64_t n_observations; /* = n_segments - n_unmatched */
  int64_t n_points;       /* points of all observations */
  int64_t n_line_points;  /* points_on_line of all observations */
} clc_station_info;
#define CLC_STATION_OK 1
#define CLC_STATION_NONFINITE (-1)
/* The stations alone, on host arrays: pose_stamp[n_poses] (nullable: the stamps come back 0), q_wc_wxyz[4 * n_poses],
 * t_wc[3 * n_poses] -> *n_stations, the true count, and at most cap_stations rows of first / last (pose indices of the first and
 * the last member), start_time / end_time, q_avg_wxyz[4 *], t_avg[3 *], status (CLC_STATION_*).  Every output is nullable:
 * cap_stations = 0 is a count query.  n_poses = 0: 0 stations, CLC_OK (the reference asserts there).  opt NULL: the defaults.
 * CLC_ERR_INVALID_ARG: NULL inputs, 2^31 poses or more, center_dist_max not finite or < 0, min_members < 0. */
int clc_static_poses(clc_handle* h, const clc_station_options* opt, size_t n_poses, const double* pose_stamp, const double* q_wc_wxyz,
                     const double* t_wc, size_t cap_stations, int64_t* first, int64_t* last, double* start_time, double* end_time,
                     double* q_avg_wxyz, double* t_avg, int32_t* status, int64_t* n_stations);
/* clc_assemble_observations in station mode.  The arrays are those of clc_assemble_observations; scan_station[n_scans]
 * (nullable): the index of the station a kept scan took, or CLC_SCAN_NO_SEGMENT / CLC_SCAN_REF_THROWS / CLC_SCAN_NO_POSE (no
 * finite station holds the stamp).  No station or no observation at all: CLC_OK and an empty store.  The same
 * CLC_ERR_INVALID_ARG cases, and those of clc_static_poses' options. */
int clc_assemble_stations(clc_handle* h, const clc_station_options* opt, size_t n_poses, const double* pose_stamp,
                          const double* q_wc_wxyz, const double* t_wc, const float* ranges, const int64_t* offsets, size_t n_scans,
                          const float* angle_min, const float* angle_increment, const float* range_min, const double* scan_stamp,
                          int32_t* scan_station, clc_station_info* info);
/* The same with every array in DEVICE memory, as clc_assemble_observations_device (ONE synchronisation). */
int clc_assemble_stations_device(clc_handle* h, const clc_station_options* opt, size_t n_poses, const double* pose_stamp_dev,
                                 const double* q_wc_wxyz_dev, const double* t_wc_dev, const float* ranges_dev,
                                 const int64_t* offsets_dev, size_t n_scans, size_t n_rays, const float* angle_min_dev,
                                 const float* angle_increment_dev, const float* range_min_dev, const double* scan_stamp_dev,
                                 int32_t* scan_station_dev, clc_station_info* info);

/* ---- interpolated tag poses (K15): one observation per scan, the tag pose interpolated at the scan's stamp -------------------
 * For recordings where the board moves.  Key-frame mode takes the nearest key frame (a pose error of velocity x |dt|, and most
 * scans dropped), station mode needs the board held still; here every scan with a board segment takes the pose BETWEEN the two
 * stamped tag poses that bracket its stamp, and a constant offset between the camera's and the laser's clock is an option.
 * The rule below is this library's design — the reference interpolates nowhere (main/calibr_offline.cpp:102-116 takes the
 * nearest key frame):
 *   x = query_stamp + time_offset.  The bracket is the FIRST i in file order with both stamps finite,
 *   0 < stamp[i+1] - stamp[i] <= max_gap and stamp[i] <= x <= stamp[i+1] (both ends inclusive); a NaN x never matches.
 *   u = (x - stamp[i]) / (stamp[i+1] - stamp[i]);  t = t_i + u (t_{i+1} - t_i);  q on the stored (w, x, y, z) values, each
 *   normalised first, q_{i+1} negated when the dot product is < 0: slerp while dot <= 1 - 1e-10, normalised lerp above; the
 *   result normalised.  A result that is not finite (a NaN or zero quaternion in the bracket) counts as no bracket.
 * Stamps that never decrease are searched by bisection, any other list by the linear walk: the same answer either way. */
typedef struct clc_interp_options {
  double time_offset;     /* 0: added to every query stamp (the laser's clock -> the camera's) */
  double max_gap;         /* 0.1 s: the longest interval between two tag poses that is interpolated across */
  double line0[2];        /* start of every line fit: (0, 0) */
  clc_options line;       /* clc_line_options_default */
} clc_interp_options;
void clc_interp_options_default(clc_interp_options* opt);
/* The interpolation alone, on host arrays: pose_stamp[n_poses], q_wc_wxyz[4 * n_poses], t_wc[3 * n_poses] in file order,
 * query_stamp[n_queries] -> bracket[n_queries] (the index i of the bracket's first pose, or CLC_SCAN_NO_POSE), u[n_queries],
 * q_out_wxyz[4 * n_queries] (unit), t_out[3 * n_queries]; every output nullable.  A query without a pose gets u = 0,
 * q = (1, 0, 0, 0), t = 0.  opt NULL: the defaults (line0 / line are not looked at).  CLC_ERR_INVALID_ARG: NULL inputs, 2^31
 * poses or queries or more, max_gap not finite or <= 0, time_offset not finite. */
int clc_interpolate_poses(clc_handle* h, const clc_interp_options* opt, size_t n_poses, const double* pose_stamp,
                          const double* q_wc_wxyz, const double* t_wc, size_t n_queries, const double* query_stamp, int32_t* bracket,
                          double* u, double* q_out_wxyz, double* t_out);
/* clc_assemble_observations with the interpolated pose: every scan with a board segment and a bracket becomes one observation,
 * tagPose_Qca / tagPose_tca formed (:145-146) from the pose interpolated at scan_stamp + time_offset.  The arrays are those of
 * clc_assemble_observations; scan_bracket[n_scans] (nullable): the index of the bracket's first pose, or CLC_SCAN_NO_SEGMENT /
 * CLC_SCAN_REF_THROWS / CLC_SCAN_NO_POSE; scan_u[n_scans] (nullable): u of a kept scan, 0 elsewhere.  info: n_keyframes = the
 * pairs (i, i + 1) of the pose list that can bracket a stamp (finite stamps, 0 < gap <= max_gap), n_unmatched = scans with a
 * segment and no bracket; the rest as there.  Everything else (segments, line fits, points_on_line, the order of the observations,
 * how they are left stored on the handle) is as for clc_assemble_observations.  The same CLC_ERR_INVALID_ARG cases, and those of
 * clc_interpolate_poses' options. */
int clc_assemble_interpolated(clc_handle* h, const clc_interp_options* opt, size_t n_poses, const double* pose_stamp,
                              const double* q_wc_wxyz, const double* t_wc, const float* ranges, const int64_t* offsets, size_t n_scans,
                              const float* angle_min, const float* angle_increment, const float* range_min, const double* scan_stamp,
                              int32_t* scan_bracket, double* scan_u, clc_assemble_info* info);
/* The same with every array in DEVICE memory, as clc_assemble_observations_device (ONE synchronisation); scan_bracket_dev and
 * scan_u_dev nullable (device memory). */
int clc_assemble_interpolated_device(clc_handle* h, const clc_interp_options* opt, size_t n_poses, const double* pose_stamp_dev,
                                     const double* q_wc_wxyz_dev, const double* t_wc_dev, const float* ranges_dev,
                                     const int64_t* offsets_dev, size_t n_scans, size_t n_rays, const float* angle_min_dev,
                                     const float* angle_increment_dev, const float* range_min_dev, const double* scan_stamp_dev,
                                     int32_t* scan_bracket_dev, double* scan_u_dev, clc_assemble_info* info);

/* ---- the camera-laser clock sweep (K15) -------------------------------------------------------------------------------------
 * An estimate of the constant offset between the laser's and the camera's clock from the recording itself: n_offsets candidate
 * offsets D_j = offset_min + j (offset_max - offset_min) / (n_offsets - 1), one calibration problem each — the same scans, the same
 * points, the tag poses interpolated at scan_stamp + D_j — solved as ONE batch from the common start pose7 (T_cl as
 * [tx, ty, tz, qx, qy, qz, qw]); the final cost over the offsets is smallest where the clocks agree.
 *   Membership: a scan is used iff it has a board segment and a bracket (clc_interpolate_poses' rule, interp.max_gap;
 *   interp.time_offset is not looked at) at EVERY D_j, so all problems hold the same records and their costs are comparable.
 *   Decimation: from a segment of L points with L > m = points_per_scan > 0 the points at index floor((2 i + 1) L / (2 m)),
 *   i = 0 .. m - 1, are taken; otherwise all of them.
 *   Records: problem j's records are the reference's assembly loop (src/LaseCamCalCeres.cpp:222-254) on these scans with
 *   use_linefitting_data = false and no edge terms: plane n = R_ca e3, d = -n . t_ca of the pose interpolated at D_j,
 *   scale = 1 / sqrt(points taken).  They are built on the device and never cross PCIe.
 *   Solve: clc_upload_batched_device + clc_solve_batched under `solve`, unchanged.
 * Out (each array nullable): offsets[n_offsets], final_cost[n_offsets], poses[7 * n_offsets], summaries[n_offsets], and
 * *result: n_scans_used, records_per_problem, and clc_clock_offset_best's choice.  No scan used: CLC_OK, n_scans_used = 0,
 * best_index = -1, the arrays (offsets apart) untouched and nothing uploaded.
 * What the call leaves on the handle: the uploaded batch is the sweep's (as after clc_upload_batched: clc_solve_batched,
 * clc_information_batched ... follow on it); the observation store (clc_store_observations / clc_assemble_*) and the single
 * problem of clc_upload are not touched.
 * CLC_ERR_INVALID_ARG: as clc_assemble_interpolated, and n_offsets outside 3 .. 1024, offsets not finite or offset_max <=
 * offset_min, points_per_scan < 0, NULL pose7 or result; a non-finite pose7 is refused as clc_solve_batched refuses it. */
typedef struct clc_clock_offset_options {
  double offset_min;        /* -0.02 s */
  double offset_max;        /*  0.02 s */
  int32_t n_offsets;        /* 41: 3 .. 1024 */
  int32_t points_per_scan;  /* 16; 0 = all points of every segment */
  clc_interp_options interp; /* clc_interp_options_default (max_gap; the rest is not looked at) */
  clc_options solve;        /* clc_options_default */
} clc_clock_offset_options;
void clc_clock_offset_options_default(clc_clock_offset_options* opt);
typedef struct clc_clock_offset_result {
  int64_t n_scans_used;        /* scans every problem holds */
  int64_t records_per_problem;
  int32_t best_index;          /* clc_clock_offset_best */
  int32_t at_edge;
  double best_offset;
} clc_clock_offset_result;
/* The choice among the candidates, on host arrays (no device needed): *best_index = the argmin of final_cost over the problems
 * whose termination (nullable: none failed) is not CLC_FAILURE, the first of equal minima, a NaN cost never chosen; -1 when there
 * is none (*best_offset = NaN then).  *best_offset = the vertex of the parabola through best_index and its two neighbours; the
 * candidate's own offset with *at_edge = 1 when the minimum is the first or the last candidate, and with *at_edge = 0 when a
 * neighbour failed or the three points have no minimum of their own (not strictly convex). */
int clc_clock_offset_best(size_t n_offsets, const double* offsets, const double* final_cost, const int32_t* termination,
                         int32_t* best_index, double* best_offset, int32_t* at_edge);
int clc_clock_offset_sweep(clc_handle* h, const clc_clock_offset_options* opt, size_t n_poses, const double* pose_stamp,
                          const double* q_wc_wxyz, const double* t_wc, const float* ranges, const int64_t* offsets, size_t n_scans,
                          const float* angle_min, const float* angle_increment, const float* range_min, const double* scan_stamp,
                          const double pose7[7], double* offsets_out, double* final_cost, double* poses, clc_summary* summaries,
                          clc_clock_offset_result* result);
/* The same with the recording in DEVICE memory, as clc_assemble_observations_device; pose7 and every output on the host. */
int clc_clock_offset_sweep_device(clc_handle* h, const clc_clock_offset_options* opt, size_t n_poses, const double* pose_stamp_dev,
                                 const double* q_wc_wxyz_dev, const double* t_wc_dev, const float* ranges_dev,
                                 const int64_t* offsets_dev, size_t n_scans, size_t n_rays, const float* angle_min_dev,
                                 const float* angle_increment_dev, const float* range_min_dev, const double* scan_stamp_dev,
                                 const double pose7[7], double* offsets_out, double* final_cost, double* poses,
                                 clc_summary* summaries, clc_clock_offset_result* result);

/* ---- board poses from tag corners (the numeric half of CamPoseEst::calcCamPose, src/calcCamPose.cpp:270-303) -------------
 * The two camera models the reference's nodes select (main/kalibratag_detector_node.cpp:90-105), restated from camodocal:
 *   CLC_CAMERA_PINHOLE         PinholeCamera:     proj = fx fy cx cy, dist = k1 k2 p1 p2
 *   CLC_CAMERA_KANNALA_BRANDT  EquidistantCamera: proj = mu mv u0 v0, dist = k2 k3 k4 k5
 * Pinhole lift (liftProjective, camera_models/src/PinholeCamera.cc): mx_d = (1/fx) u + (-cx/fx) (inverse-K constants as at
 * :208-211), identity when k1 = k2 = p1 = p2 = 0 (:196-205), otherwise the recursive model, 8 evaluations of distortion()
 * (:401-415, :554-571).  Kannala-Brandt lift (EquidistantCamera.cc:342-356, backprojectSymmetric :632-733): theta = the
 * smallest real root >= -1e-10 (clamped to 0) of theta + k2 theta^3 + k3 theta^5 + k4 theta^7 + k5 theta^9 = |p_u|, the degree
 * dropping by 2 for every zero coefficient (:647-663); theta = |p_u| when no root qualifies; phi = 0 when |p_u| < 1e-10.  The
 * reference takes the eigenvalues of the companion matrix; here the first sign change on [0, inf) is bracketed and polished
 * (safeguarded Newton / bisection), the same root.  Project: spaceToPlane (PinholeCamera.cc:428-453, EquidistantCamera.cc:364-377). */
#define CLC_CAMERA_PINHOLE 1
#define CLC_CAMERA_KANNALA_BRANDT 2
typedef struct clc_camera {
  int32_t model;    /* CLC_CAMERA_* */
  int32_t reserved; /* 0 */
  double proj[4];   /* fx fy cx cy | mu mv u0 v0 */
  double dist[4];   /* k1 k2 p1 p2 | k2 k3 k4 k5 */
} clc_camera;       /* 72 bytes */

/* Pose status of clc_board_poses. */
#define CLC_POSE_OK 1
#define CLC_POSE_TOO_FEW 0        /* fewer than 4 corners (EstimatePose, src/calcCamPose.cpp:217) */
#define CLC_POSE_DEGENERATE (-1)  /* rank-deficient homography (e.g. collinear corners) */
#define CLC_POSE_NONFINITE (-2)   /* a non-finite corner, board point or result, or no start with every corner in front */

/* clc_options for clc_board_poses: Ceres defaults with no loss, function tolerance 1e-15, parameter tolerance 1e-14, gradient
 * tolerance 1e-16 and 50 iterations — the iterate reaches the least-squares minimiser of the float32-rounded lifted points. */
void clc_pose_options_default(clc_options* opt);
/* liftProjective of n pixels px[2n] (float32, as cornerSubPix writes them), on the device: xy_norm[2n] = x/z, y/z (unrounded). */
int clc_camera_lift(clc_handle* h, const clc_camera* cam, const float* px, size_t n, double* xy_norm);
/* spaceToPlane of n points pts[3n] after the transform pose7 = T_cl = [t, qx, qy, qz, qw] (p_c = R p + t, as the verification
 * overlay debug_code/showscan_node.cpp:96-130 maps laser points; NULL = identity), on the device: px[2n]. */
int clc_camera_project(clc_handle* h, const clc_camera* cam, const double pose7[7], const double* pts, size_t n, double* px);
/* One board pose per image (EstimatePose, src/calcCamPose.cpp:211-232, with calcCamPose's lift :277-287): image k owns corners
 * [offsets[k], offsets[k+1]) of corners_px[2M] (float32 pixels) and board_xy[2M] (float32 board-plane x, y; z = 0, the
 * cv::Point3f of every board type).  Per image: every corner lifted in fp64 and x/z, y/z rounded to float32 (:284-286);
 * a normalized-DLT homography, decomposed with the board in front; then Levenberg-Marquardt (no loss) on the K = I reprojection error
 * (R X + t)_xy / (R X + t)_z - x_lifted over the PoseLocalParameterization tangent — the least-squares minimiser that
 * cv::solvePnP (K = I, no distortion, :222-226) iterates towards.  Outputs: q_ca_wxyz[4n] (w >= 0) and t_ca[3n] of
 * T_ca = (R_cw, t_cw): p_c = R X + t, the tagPose_Qca / tagPose_tca of Oberserve (main/calibr_offline.cpp:145-146);
 * rms[n] (nullable): sqrt(sum |r|^2 / corners), normalized units; status[n] (required): CLC_POSE_*; summaries[n] (nullable).
 * An image that is not CLC_POSE_OK gets q = (1, 0, 0, 0), t = 0, rms = NaN; it never fails the call or affects other images.
 * opt NULL = clc_pose_options_default(). */
int clc_board_poses(clc_handle* h, const clc_camera* cam, const clc_options* opt, const float* corners_px, const float* board_xy,
                    const int64_t* offsets, size_t n_images, double* q_ca_wxyz, double* t_ca, double* rms, int32_t* status,
                    clc_summary* summaries);
/* The same with every array in DEVICE memory (ready on the handle's stream; complete on return — it synchronises):
 * offsets_dev[n_images + 1] absolute (offsets_dev[0] may be > 0; not validated: monotone). */
int clc_board_poses_device(clc_handle* h, const clc_camera* cam, const clc_options* opt, const float* corners_px_dev,
                           const float* board_xy_dev, const int64_t* offsets_dev, size_t n_images, double* q_ca_wxyz_dev,
                           double* t_ca_dev, double* rms_dev, int32_t* status_dev, clc_summary* summaries_dev);

/* Multi-hypothesis calibration on SHARED observations: n_starts independent LM solves (one ceres::Solve each, src/LaseCamCalCeres.cpp
 * :299-309) from n_starts start poses on the ONE problem the handle holds as a batch of one (clc_upload_batched* with n_problems = 1).
 * poses: n_starts x 7, in/out; summaries: n_starts.  Where the problem fits a workgroup (clc_path_info.batched_resident) ONE launch runs
 * every start — a workgroup per start, all of them loading the same on-chip layout: one copy of the observations in HBM instead of
 * n_starts uploaded copies — and the results are bit-identical to clc_solve_batched of n_starts copies; a larger problem runs its
 * starts one after the other on the batch's streaming path (a single problem beyond a workgroup is better served by clc_upload +
 * one clc_solve per start: the cooperative solve uses the whole GPU for each). */
int clc_solve_multistart(clc_handle* h, const clc_options* opt, size_t n_starts, double* poses_inout, clc_summary* summaries);

/* Resampled calibrations on SHARED observations (jackknife, bootstrap, random subsets of the poses): n_subsets independent LM solves on
 * the ONE problem the handle holds as a batch of one (clc_upload_batched* with n_problems = 1), each with some poses left out or
 * repeated.  The records are cut into n_blocks consecutive blocks — block_offsets[n_blocks + 1], block_offsets[0] = 0, last = the
 * record count, non-decreasing; one block per pose keeps a pose's point rows and edge rows together — and subset k is BY DEFINITION the
 * problem in which every record of block b appears weights[k * n_blocks + b] times (0: left out), each record with its own scale and
 * loss: exactly what clc_solve_batched computes for the sub-problem with those records repeated, to rounding (sums in another order).
 * poses: n_subsets x 7, in/out; summaries: n_subsets.  ONE launch, a workgroup per subset on the one on-chip layout; the layout is not
 * changed (clc_solve_multistart on the same upload is unaffected), the lane -> block map is kept on the handle until the offsets change
 * or the next upload.  A weight row of 1s returns the bits clc_solve_multistart returns.
 * CLC_ERR_NO_DATA unless a batch of one is uploaded.  CLC_ERR_INVALID_ARG: bad offsets; a block boundary inside a scan (the library
 * treats consecutive records with bitwise-equal planes as one scan; a block must hold whole scans — a boundary inside a scan is
 * accepted only where it happens to coincide with the library's own cut of that scan into lanes, which depends on all the scans of the
 * upload and may change between versions: do not rely on it); a problem that one workgroup does
 * not hold (clc_path_info.batched_resident == 0: materialise the subsets and use clc_solve_batched).
 * A subset with nothing in it (all weights 0) or with a non-finite end gets termination = CLC_FAILURE and keeps its pose; it does not
 * fail the call. */
int clc_solve_subsets(clc_handle* h, const clc_options* opt, size_t n_blocks, const int64_t* block_offsets, size_t n_subsets,
                      const uint8_t* weights, double* poses_inout, clc_summary* summaries);

/* Consensus scores on SHARED observations: n_poses candidate poses, each judged against EVERY block of the ONE problem the handle holds
 * as a batch of one (blocks as in clc_solve_subsets: one per recorded pose) — what a RANSAC / least-median step over recordings needs,
 * where clc_solve_subsets reports a subset's own total only.  Per pose k and block b, at index k * n_blocks + b (each table nullable):
 *   ssq      sum of r^2 over the block's records, r = scale * (n.(R p + t) + d) the factor's residual, no loss (one block per pose,
 *            point rows only: that pose's mean squared point-to-plane distance, scale^2 being 1 / count)
 *   cost     1/2 sum rho(r^2) under opt's loss (Cauchy, loss_scale_factor * scale per record, as the solves; use_loss = 0: ssq / 2)
 *   inliers  records with |n.(R p + t) + d| <= tau (the plane expression before the scale: metres for unit normals)
 * ONE launch, a workgroup per pose on the one on-chip layout, one evaluation pass; sums in a fixed order (two calls return the same
 * bits, and the sum over b agrees with clc_eval / clc_information to rounding).  The layout, the observations and what clc_solve_multistart /
 * clc_solve_subsets return afterwards are unchanged; the lane -> block map is the one clc_solve_subsets keeps (built once per offsets
 * and upload, by whichever call comes first).
 * Errors as clc_solve_subsets: CLC_ERR_NO_DATA unless a batch of one is uploaded; CLC_ERR_INVALID_ARG for bad offsets, a block boundary
 * inside a scan (as there: whole scans per block), tau = NaN, loss_scale_factor <= 0 with use_loss, or a problem that one workgroup does not hold
 * (clc_path_info.batched_resident == 0).  A pose with a non-finite entry does not fail the call: its row is NaN / NaN / 0.  A block
 * without records scores 0 / 0 / 0. */
int clc_score_blocks(clc_handle* h, const clc_options* opt, size_t n_blocks, const int64_t* block_offsets, size_t n_poses,
                     const double* poses /* n_poses x 7 */, double tau,
                     double* ssq, double* cost, int32_t* inliers /* each n_poses x n_blocks, each nullable */);

/* ---- multi-GPU: sharded batches + RCCL gather ------------------------------------------------
 * BASELINE.json configs[3]: independent T_cl problems shard across the GPUs of a node, one process
 * per GPU, no collective on the data path; the fixed-size result records of all ranks are gathered
 * once over xGMI.  The reference has no counterpart (single-threaded Ceres, src/LaseCamCalCeres.cpp
 * :302-304); the record is what its caller keeps of a solve: the pose written back at :311-314 and the
 * Solver::Summary fields printed at :309.
 *
 * RCCL is bound at run time (dlopen): the copy already loaded into the process (e.g. PyTorch's) is
 * reused, else librccl.so.1; CLC_RCCL_LIBRARY overrides.  Only these entry points need it. */
typedef struct clc_result_record {
  double pose[7];         /* [tx,ty,tz,qx,qy,qz,qw] */
  double final_cost;
  double initial_cost;
  double num_iterations;
  double termination;     /* CLC_CONVERGENCE_* ... as a double */
  double global_index;    /* global problem index; -1 marks a padding record */
} clc_result_record;      /* 12 doubles = 96 bytes */

#define CLC_COMM_ID_BYTES 128
typedef struct clc_comm clc_comm;
/* ncclGetUniqueId: called by ONE rank; the caller distributes the 128 bytes to the other ranks out of
 * band (torch.distributed store, MPI, a file). */
int clc_comm_unique_id(char id[CLC_COMM_ID_BYTES]);
/* ncclCommInitRank on the handle's device; collectives run on the handle's stream.  Collective call:
 * every rank of the job must enter it. */
int clc_comm_create(clc_comm** out, clc_handle* h, const char id[CLC_COMM_ID_BYTES], int rank, int world);
void clc_comm_destroy(clc_comm* c);
/* Rank and size of the communicator as RCCL itself reports them (ncclCommUserRank / ncclCommCount). */
int clc_comm_rank(const clc_comm* c);
int clc_comm_world(const clc_comm* c);
/* Path of the RCCL library the collectives are bound to at run time (the one already loaded in the process — torch's — or
 * librccl.so from the loader's path); "" before the first clc_comm_* call resolved it. */
const char* clc_comm_library(void);
/* WHERE the gathered records go (SURVEY.md §8e specifies a gather to rank 0).  root = -1 (default): every rank receives every
 * record — ncclAllGather, and every rank copies the other ranks' segments to its pinned host buffer.  root >= 0: only `root` does —
 * the collective is ncclGather to root (RCCL extension; ncclAllGather when the loaded librccl lacks it) and only root copies the other
 * segments down; every other rank returns from the gather calls below with ITS OWN segment valid (all_records / clc_comm_records())
 * and the other segments unspecified.  At N = 8 the all-ranks form costs every rank a 5.5 MB device-to-host copy per step; the rooted
 * form costs the root that copy (hidden behind the next step's kernel by the pipelined call below) and the other ranks nothing.
 * Every rank must set the same root before its next gather. */
int clc_comm_set_root(clc_comm* c, int root);
typedef struct clc_comm_info {
  int32_t struct_size;                 /* sizeof(clc_comm_info) of the library that filled it (fields are only ever appended) */
  int32_t rank, world, root;
  int32_t rooted_collective_available; /* the loaded RCCL exports ncclGather */
  int32_t copies_other_ranks_to_host;  /* this rank copies the other ranks' segments to its host (no root, or it is the root) */
  int32_t step_in_flight;              /* a pipelined step has been enqueued and not yet been returned */
  int32_t pad_;
  int64_t collectives;                 /* collectives enqueued on this communicator so far */
  int64_t rooted_collectives;          /* of them ncclGather */
  int64_t host_copies;                 /* device-to-host copy commands issued by the gather calls on this rank */
  int64_t host_copy_bytes;
  int64_t pipelined_steps;
} clc_comm_info;
int clc_comm_get_info(const clc_comm* c, clc_comm_info* out);

/* Gather (see clc_comm_set_root) of the result records the LAST clc_solve_batched on the comm's handle left in device
 * memory.  This rank owns global problem indices [first_global_index, first_global_index + P_local);
 * every rank contributes exactly cap_per_rank records (P_local <= cap_per_rank, the rest padded with
 * global_index = -1).  all_records (host, world * cap_per_rank records, rank-major; contiguous shards in
 * rank order make that the global problem order) is filled on every rank that passes one; NULL skips
 * the copy — the gathered records then stay readable in the communicator's pinned host buffer,
 * clc_comm_records(), until the next gather.  With a root set, ranks other than the root hold only their own segment.  Collective call. */
int clc_gather_results(clc_comm* c, int64_t first_global_index, size_t cap_per_rank,
                       clc_result_record* all_records);
const clc_result_record* clc_comm_records(const clc_comm* c);

/* clc_solve_batched + clc_gather_results as ONE enqueue — the step of a sharded batch (BASELINE.json configs[3]) when only the
 * gathered records are wanted.  The on-chip batched kernel writes every local problem's result record, global index
 * first_global_index + k, straight into this rank's segment of the communicator's gather buffer; the all-gather (in place) and ONE
 * copy of the gathered records to the host follow on the same stream, and the host synchronises once.  No per-problem poses or
 * summaries cross PCIe and nothing is packed or copied in between; what the two-call form returns per problem is in the records
 * (pose, costs, iterations, termination), and the local shard's totals come back in `stats` (nullable).
 * poses0: host, 7 doubles per LOCAL problem of the handle's uploaded batch (clc_upload_batched), or the handle's own pinned buffer
 * (clc_batched_host_buffers) already filled.  all_records / clc_comm_records() as in clc_gather_results.  A batch that does not run as
 * the one-launch on-chip solve falls back to the two calls (stats->fused = 0).  Collective call; same error convention as
 * clc_gather_results (a rank with a local error still takes part, with padding records, and reports afterwards). */
typedef struct clc_batch_stats {
  int64_t problems;        /* local problems solved by this call (-1 in all four counters: totals unknown for this call — the call
                            * after one that failed between its launch and its bookkeeping; the records are complete either way) */
  int64_t evaluations;     /* sum of their evaluation passes (clc_summary.num_evaluations) */
  int64_t iterations;      /* sum of their LM iterations */
  int64_t not_converged;   /* of them: terminated with CLC_NO_CONVERGENCE or CLC_FAILURE */
  int32_t fused;           /* 1: one launch + in-place all-gather + one copy; 0: the two-call fall-back ran */
  int32_t pad_;
  double kernel_ms;        /* profile_events = 1: HIP event pair around the solve launch (fused form) */
  double solve_ms;         /* host wall time of the call */
} clc_batch_stats;
int clc_solve_batched_gather(clc_comm* c, const clc_options* opt, const double* poses0, int64_t first_global_index,
                             size_t cap_per_rank, clc_result_record* all_records, clc_batch_stats* stats);

/* The same step for a STREAM of steps: the call enqueues step k (kernel + collective on the solver's stream) and returns the records
 * and totals of step k-1 (*prev_records = NULL on the first call).  The device-to-host copy of step k-1's other-rank segments runs on
 * the communicator's copy stream WHILE step k's kernel runs (step k's collective waits for it by event before it overwrites the
 * segments), and the host buffers alternate between two pinned twins: *prev_records stays valid and untouched while step k runs, until
 * the NEXT pipelined call or flush (whose step writes into that twin).  clc_gather_flush completes the last step (returns CLC_OK with *records = NULL when none is in flight).  Between a
 * pipelined call and its flush the other gather calls and clc_comm_set_root refuse.  The start poses of step k are read by its kernel:
 * `poses0` is copied into the handle's pinned buffer before the launch, the caller's array is free on return.  Requires the one-launch
 * on-chip batch (otherwise CLC_ERR_INVALID_ARG: use clc_solve_batched_gather).  Collective calls, same error convention: a LOCAL error
 * of step k-1 is returned by the call that hands back its records. */
int clc_solve_batched_gather_pipelined(clc_comm* c, const clc_options* opt, const double* poses0, int64_t first_global_index,
                                       size_t cap_per_rank, const clc_result_record** prev_records, clc_batch_stats* prev_stats);
int clc_gather_flush(clc_comm* c, const clc_result_record** records, clc_batch_stats* stats);

/* ---- robust board poses (K16): a consensus over the tags of an image ahead of clc_board_poses' planar PnP ------------------
 * clc_board_poses is a plain least-squares fit over every corner of an image: one AprilTag decoded with a wrong id (four corners
 * at the wrong place of the board) or one mis-refined corner bends the pose, and nothing downstream can tell.  The reference
 * left cv::solvePnPRansac commented out beside cv::solvePnP (src/calcCamPose.cpp:226-227).  A tag board needs no random
 * sampling: every tag is four corners of a planar square, and four planar correspondences fix a homography in closed form.
 * Per image, after clc_board_poses' own lift (fp64, x/z and y/z rounded to float32):
 *  1. Groups: group g = the image's corners 4g .. 4g+3 (the order FindTargetCorner emits tags).  A tail of 1-3 corners belongs
 *     to no group but is scored like every other corner.
 *  2. Hypothesis: H_g = S(lifted quad) adj(S(board quad)), S(p) the closed-form unit-square -> quad map: with
 *     sigma = p0 - p1 + p2 - p3, d1 = p1 - p2, d2 = p3 - p2, den = d1 x d2, g = (sigma x d2) / den, h = (d1 x sigma) / den its
 *     rows are (x1 - x0 + g x1, x3 - x0 + h x3, x0), (y1 - y0 + g y1, y3 - y0 + h y3, y0), (g, h, 1).  No pivoting, no
 *     iteration.  A group is invalid when either den is zero or not finite or an entry of H_g is not finite — so the groups
 *     of a chessboard, four consecutive collinear corners, are all invalid and a chessboard image ends CLC_POSE_NO_CONSENSUS:
 *     this call is for tag boards.
 *  3. Score: corner k under group g: (u, v, w) = H_g (X, Y, 1), e = (u/w - x)^2 + (v/w - y)^2; an inlier iff e is finite,
 *     e < hyp_threshold^2 and w w0 > 0, w0 the w of the group's first corner.  count_g = the inliers, cost_g = the sum of
 *     min(e, hyp_threshold^2) in corner order (a non-finite e adds the cap).  The winner: the largest count, then the smallest
 *     cost, then the smallest g.  Every product and sum is rounded on its own and the divisions are IEEE: counts, costs and
 *     the winner do not depend on the device.
 *  4. First set = the winner's inliers.  No valid group, or fewer than min_inliers of them: CLC_POSE_NO_CONSENSUS.
 *  5. Fit: clc_board_poses' per-image fit on the set's corners, compacted in corner order — the same code on the same input
 *     as clc_board_poses given those corners alone, hence the same bits.  A status other than CLC_POSE_OK ends the image
 *     with that status.
 *  6. Re-gate: with the fitted (R, t), P = R (X, Y, 0) + t, e = (P_x / P_z - x)^2 + (P_y / P_z - y)^2; an inlier iff P_z > 0, e
 *     finite and e < threshold^2.  Then, in this order: the set equals the one just fitted — done; fewer than min_inliers —
 *     CLC_POSE_NO_CONSENSUS; n_fits == max_fits — done with the last fit; otherwise a refit (5.) on the new set.
 * Outputs, per image: q / t / rms / summaries of the LAST fit (rms over the set it was fitted on); inlier[] = that set, indexed
 * like the corners (entries [offsets[0], offsets[n_images]) are written, 1 / 0); n_inliers = its size; best_group = the winner
 * (-1: none, or its set was too small); n_fits = the fits that ran.  An image that ends without a pose has q = (1, 0, 0, 0), t = 0,
 * rms = NaN, an all-zero mask and n_inliers = 0.  An image never fails the call and never affects another image.  A non-finite
 * corner is never an inlier; it does not condemn its image, as it does in clc_board_poses.
 * The default gates, 8 px and 2 px over the focal length, are DESIGN VALUES from a numpy experiment (6x6 board, tag 0.055 m, spacing
 * 0.3, f = 367 px, 0.3 px noise, 0.6-1.5 m): the best single-tag homography explains >= 126 of 144 clean corners within 8 px but only
 * about half within 3 px — a single tag extrapolates poorly, so the hypothesis gate is loose and the fitted pose re-gates tightly. */
#define CLC_POSE_NO_CONSENSUS (-3)   /* no valid hypothesis, or the best set has fewer than min_inliers corners */

typedef struct clc_robust_pose_options {
  double hyp_threshold;  /* gate of the per-tag hypotheses, normalized image plane units (pixels / focal) */
  double threshold;      /* gate of the re-scoring with the fitted pose, same units */
  int32_t min_inliers;   /* >= 4 */
  int32_t max_fits;      /* 1..8: fits per image at most */
} clc_robust_pose_options; /* 24 bytes */

/* hyp_threshold = 8 / sqrt(|proj[0] proj[1]|), threshold = 2 / sqrt(|proj[0] proj[1]|), min_inliers 4, max_fits 4 (cam NULL: both
 * gates 0, which the calls refuse — set them). */
void clc_robust_pose_options_default(clc_robust_pose_options* ropt, const clc_camera* cam);

/* Arrays as clc_board_poses; inlier[] required; rms, summaries, n_inliers, best_group, n_fits nullable; opt NULL =
 * clc_pose_options_default(), ropt NULL = clc_robust_pose_options_default().  CLC_ERR_INVALID_ARG: a gate that is not finite and
 * positive, hyp_threshold < threshold, min_inliers < 4, max_fits outside 1..8.  One enqueue — lift, consensus, (fit, re-gate) x
 * max_fits on the handle's stream, every launch sized by n_images — and one synchronisation at the end. */
int clc_board_poses_robust(clc_handle* h, const clc_camera* cam, const clc_options* opt, const clc_robust_pose_options* ropt,
                           const float* corners_px, const float* board_xy, const int64_t* offsets, size_t n_images,
                           double* q_ca_wxyz, double* t_ca, double* rms, int32_t* status, clc_summary* summaries,
                           uint8_t* inlier, int32_t* n_inliers, int32_t* best_group, int32_t* n_fits);
/* The same with every array in DEVICE memory (as clc_board_poses_device: offsets_dev[0] may be > 0; not validated: monotone). */
int clc_board_poses_robust_device(clc_handle* h, const clc_camera* cam, const clc_options* opt, const clc_robust_pose_options* ropt,
                                  const float* corners_px_dev, const float* board_xy_dev, const int64_t* offsets_dev, size_t n_images,
                                  double* q_ca_wxyz_dev, double* t_ca_dev, double* rms_dev, int32_t* status_dev,
                                  clc_summary* summaries_dev, uint8_t* inlier_dev, int32_t* n_inliers_dev, int32_t* best_group_dev,
                                  int32_t* n_fits_dev);

/* ---- the planar fit's second minimum (K17): the other pose of every image and how ambiguous the choice is -------------------
 * The reprojection cost of a planar target has two local minima: the true pose and its mirror about the line of sight
 * (Schweighofer-Pinz; IPPE; AprilTag's estimate_tag_pose returns both for this reason).  clc_board_poses returns the one its DLT
 * start leads to.  With the board far away or only a few tags decoded the two costs come close and noise decides which is lower:
 * the plane's normal is then wrong by twice the tilt while rms looks clean.  This call takes the poses of clc_board_poses or
 * clc_board_poses_robust and returns, per image k (corners [offsets[k], offsets[k+1]), status_in[k] the earlier call's status):
 *  1. Set: the corners with inlier[i] != 0, compacted in corner order (inlier NULL: all corners), after clc_board_poses' lift
 *     (fp64, x/z and y/z rounded to float32).  status_in[k] != CLC_POSE_OK, fewer than 4 corners in the set, or a non-finite
 *     lifted corner or board point in it: CLC_ALT_NONE.  A non-finite corner outside the set is ignored.
 *  2. Mirror start: Xbar = the set's mean board point, c = R Xbar + t, s = c / |c|, R' = (I - 2 s s^T) R diag(1, 1, -1),
 *     t' = c - R' Xbar.  R' is a rotation, the centroid stays where it is and every corner's offset from it is reflected through the
 *     plane perpendicular to the line of sight — the same image under weak perspective; the new normal is 2 (s.n) s - n.
 *     c zero or not finite, or a non-finite start: CLC_ALT_NONE.
 *  3. Fit: clc_board_poses' LM stage (K = I reprojection error, the same clc_options, opt NULL = clc_pose_options_default(), the
 *     same rule for a point behind the camera) from (R', t') on the set; no DLT.  A failed or non-finite fit: CLC_ALT_NONE.
 *  4. Costs: cost_in = 1/2 sum |r|^2 of the INPUT pose on the compacted set through the same evaluation — the per-corner
 *     arithmetic AND the summation order of the fit's own evaluations, so that `better` and a ratio near 1 compare like with
 *     like; cost_alt = the fit's final cost; ratio = cost_alt / cost_in (NaN when cost_in is zero or either cost is not finite).
 *  5. rot_angle = the angle of R^T R_alt, normal_angle = the angle between R e_z and R_alt e_z.  rot_angle < same_angle:
 *     CLC_ALT_SAME — the mirror start fell back into the input's minimum, the view is unambiguous; otherwise CLC_ALT_DISTINCT.
 *  6. ambiguous = 1 iff DISTINCT and ratio < ratio_gate; better = 1 iff DISTINCT and cost_alt < cost_in.
 * Outputs per image: q_alt_wxyz (w >= 0), t_alt, rms_alt (over the set), cost_in, cost_alt, ratio, rot_angle, normal_angle, kind,
 * ambiguous, better, summaries_alt.  A CLC_ALT_NONE image gets q = (1, 0, 0, 0), t = 0, NaN for every real output and 0 for both
 * flags.  An image never fails the call and never affects another image.  No existing call changes.
 * The defaults are DESIGN VALUES.  same_angle = 0.01 rad lies between the two clusters of a numpy / scipy experiment (DESIGN.md
 * K17): both starts in one minimum — rotations within 3.7e-4 rad (scipy's stopping); distinct minima — at least 0.18 rad apart;
 * with this library's LM the clusters are 3.4e-9 rad at most and 0.35 rad at least on the seeded test sets, 7.8e-3 and 1.8e-2 rad on
 * 4 x 10^4 random views whose tilt goes down to zero (profiles/board_poses_alternate.md).
 * A rot_angle near the gate is NOT a sharp classification: the two minima lie twice the tilt apart and merge as the board turns to
 * face the camera, the cost between them is flat, and the fit stops somewhere on the flat.  Below about half a degree of tilt SAME
 * and DISTINCT shade into each other (the normals then differ by a degree at most); move same_angle to class such views one way.
 * ratio_gate = 2: a pose whose mirror fits within a factor two is not a clean observation. */
#define CLC_ALT_NONE 0
#define CLC_ALT_SAME 1
#define CLC_ALT_DISTINCT 2

typedef struct clc_alt_pose_options {
  double same_angle; /* rad: below it the two fits are the same minimum; finite, > 0 */
  double ratio_gate; /* cost_alt / cost_in below it: ambiguous; finite, >= 1 */
} clc_alt_pose_options; /* 16 bytes */

/* same_angle 0.01, ratio_gate 2 (design values, see above). */
void clc_alt_pose_options_default(clc_alt_pose_options* aopt);

/* corners_px, board_xy, offsets as clc_board_poses; inlier (nullable) indexed like the corners; q_in_wxyz[4 n], t_in[3 n],
 * status_in[n]: the earlier call's results.  kind[n] required, every other output nullable (ambiguous, better: uint8).
 * CLC_ERR_INVALID_ARG: a same_angle that is not finite and positive, a ratio_gate that is not finite and >= 1 (checked before the
 * handle).  One enqueue — lift, start, fit on the handle's stream, every launch sized by n_images — and one synchronisation. */
int clc_board_poses_alternate(clc_handle* h, const clc_camera* cam, const clc_options* opt, const clc_alt_pose_options* aopt,
                              const float* corners_px, const float* board_xy, const int64_t* offsets, size_t n_images,
                              const uint8_t* inlier, const double* q_in_wxyz, const double* t_in, const int32_t* status_in,
                              double* q_alt_wxyz, double* t_alt, double* rms_alt, double* cost_in, double* cost_alt, double* ratio,
                              double* rot_angle, double* normal_angle, int32_t* kind, uint8_t* ambiguous, uint8_t* better,
                              clc_summary* summaries_alt);
/* The same with every array in DEVICE memory (as clc_board_poses_device: offsets_dev[0] may be > 0; not validated: monotone). */
int clc_board_poses_alternate_device(clc_handle* h, const clc_camera* cam, const clc_options* opt, const clc_alt_pose_options* aopt,
                                     const float* corners_px_dev, const float* board_xy_dev, const int64_t* offsets_dev,
                                     size_t n_images, const uint8_t* inlier_dev, const double* q_in_wxyz_dev, const double* t_in_dev,
                                     const int32_t* status_in_dev, double* q_alt_wxyz_dev, double* t_alt_dev, double* rms_alt_dev,
                                     double* cost_in_dev, double* cost_alt_dev, double* ratio_dev, double* rot_angle_dev,
                                     double* normal_angle_dev, int32_t* kind_dev, uint8_t* ambiguous_dev, uint8_t* better_dev,
                                     clc_summary* summaries_alt_dev);

/* ---- joint refinement of the board poses and the camera-laser extrinsic (K18) ------------------------------------------
 * One cost over T_cl and every board pose T_ca,i of a problem of P images:
 *   corner  ((R_i X + t_i)_xy / (R_i X + t_i)_z - x_lifted) / sigma_corner     x_lifted: the float32-rounded lift of clc_board_poses
 *   laser   e3^T R_i^T (R_cl p + t_cl - t_i) / sigma_laser                     the point-to-plane factor with n = R_i e3, d = -n.t_i
 * cost = 1/2 sum r^2, no loss; tangent [dt, dtheta] with t += dt, R <- R Exp(dtheta) for every pose.  The whole Levenberg-Marquardt
 * solve of a problem runs in one kernel launch (one workgroup per problem): per-image 6x6 blocks, a Schur complement onto the 6x6
 * system of T_cl, clc_options with the semantics of the other solves (opt NULL = clc_pose_options_default()).  Deterministic: the
 * same bits on every run, and a problem's result does not depend on the other problems of the call. */
typedef struct clc_joint_options {
  double sigma_corner;      /* normalized image units (pixels / focal), finite, > 0 */
  double sigma_laser;       /* metres, finite, > 0 */
  int32_t hold_board_poses; /* 1: only T_cl moves */
  int32_t hold_extrinsic;   /* 1: only the board poses move */
} clc_joint_options;        /* 24 bytes */

/* 0.3 px / sqrt(|proj0 proj1|) and 0.01 m, the noise levels of the project's simulations; cam NULL: sigma_corner 0 (refused). */
void clc_joint_options_default(clc_joint_options* jopt, const clc_camera* cam);

/* Image status of clc_joint_refine. */
#define CLC_JOINT_OK 1
#define CLC_JOINT_TOO_FEW 0      /* fewer than 4 corners */
#define CLC_JOINT_NOT_KEPT (-1)  /* keep[i] == 0, or the image belongs to no problem */
#define CLC_JOINT_NONFINITE (-2) /* a non-finite corner, board point, laser point or start pose */

/* Image i owns corners [corner_offsets[i], corner_offsets[i+1]) of corners_px / board_xy (as clc_board_poses) and laser points
 * [pts_offsets[i], pts_offsets[i+1]) of pts[3 N] (laser frame; none is allowed); problem k owns images [problem_offsets[k],
 * problem_offsets[k+1]) (NULL: one problem of all images).  keep[n_images] (nullable): 0 drops an image.  In / out: q_ca_wxyz[4 n]
 * (out: w >= 0), t_ca[3 n] — the start poses, e.g. clc_board_poses' — and poses_cl[7 n_problems] = [t, qx, qy, qz, qw] with
 * p_c = R_cl p + t_cl.  An image that takes no part (image_status != CLC_JOINT_OK) keeps its pose bit for bit.  A problem with no
 * participating image, a non-finite T_cl or a failed solve ends CLC_FAILURE with every pose untouched.  With no laser point in a
 * problem T_cl is returned bit for bit.  summaries[n_problems]: final_cost is the cost at the returned poses.  H_cl[36 n_problems]
 * (nullable): the information on T_cl with the board poses marginalised, C - sum B_i^T A_i^-1 B_i at the returned poses (undamped;
 * C itself with hold_board_poses; NaN where an A_i is not positive definite).  cost_parts[2 n_problems] (nullable): the corner and
 * the laser share of final_cost.  CLC_ERR_INVALID_ARG before any device work: NULL required pointers, a sigma that is not finite
 * and positive, both hold flags, offsets that decrease.  One enqueue (lift, then the solve) and one synchronisation. */
int clc_joint_refine(clc_handle* h, const clc_camera* cam, const clc_options* opt, const clc_joint_options* jopt,
                     const float* corners_px, const float* board_xy, const int64_t* corner_offsets, const double* pts,
                     const int64_t* pts_offsets, const uint8_t* keep, size_t n_images, const int64_t* problem_offsets, size_t n_problems,
                     double* q_ca_wxyz, double* t_ca, double* poses_cl, clc_summary* summaries, double* H_cl, double* cost_parts,
                     int32_t* image_status);
/* The same with every array in DEVICE memory.  The per-image arrays (offsets, keep, q, t, image_status) are indexed by the
 * absolute image index: the call covers the n_images images from problem_offsets_dev[0] on (from 0 when it is NULL); corner and
 * point offsets are absolute too.  The per-problem arrays start at problem 0.  Offsets are not validated beyond the ends of the
 * ranges, which are read back once to size the call's scratch ahead of its one enqueue. */
int clc_joint_refine_device(clc_handle* h, const clc_camera* cam, const clc_options* opt, const clc_joint_options* jopt,
                            const float* corners_px_dev, const float* board_xy_dev, const int64_t* corner_offsets_dev,
                            const double* pts_dev, const int64_t* pts_offsets_dev, const uint8_t* keep_dev, size_t n_images,
                            const int64_t* problem_offsets_dev, size_t n_problems, double* q_ca_wxyz_dev, double* t_ca_dev,
                            double* poses_cl_dev, clc_summary* summaries_dev, double* H_cl_dev, double* cost_parts_dev,
                            int32_t* image_status_dev);

/* ---- camera intrinsics from the board images (K19) ------------------------------------------------------------------------
 * One problem = one camera seen in P images of the board.  The cost 1/2 sum |(project(cam, R_i X + t_i) - u) / sigma_px|^2 (project:
 * spaceToPlane as clc_camera_project, pixels; no lift, no loss) is minimised over the 8 intrinsics in clc_camera order (proj[0..3],
 * dist[0..3], moved additively) and the tangent [dt, dtheta] of every board pose (t += dt, R <- R Exp(dtheta)).  The whole
 * Levenberg-Marquardt solve of a problem runs in one kernel launch (one workgroup per problem): per-image 6x6 blocks and a Schur
 * complement onto the system of the free intrinsics, clc_options with the semantics of the other solves (opt NULL =
 * clc_pose_options_default()), Jacobi scaling fixed at the first evaluation.  An evaluation with a corner at P_z <= 0 is invalid.
 * Deterministic: the same bits on every run, and a problem's result does not depend on the other problems of the call.
 * Kannala-Brandt's k4 and k5 are not observable in an ordinary field of view: they are held by default. */
typedef struct clc_camcal_options {
  double sigma_px;          /* pixels, finite, > 0 */
  uint32_t hold_mask;       /* bit j: intrinsic j (proj[0..3], dist[0..3]) is held */
  int32_t hold_board_poses; /* 1: only the free intrinsics move */
} clc_camcal_options;       /* 16 bytes */

/* 0.3 px; mask 0 for CLC_CAMERA_PINHOLE, bits 6 | 7 (k4, k5) for CLC_CAMERA_KANNALA_BRANDT. */
void clc_camcal_options_default(clc_camcal_options* copt, int32_t model);

/* Image status of clc_camera_calibrate. */
#define CLC_CAMCAL_OK 1
#define CLC_CAMCAL_TOO_FEW 0      /* fewer than 4 corners */
#define CLC_CAMCAL_NOT_KEPT (-1)  /* keep[i] == 0, or the image belongs to no problem */
#define CLC_CAMCAL_NONFINITE (-2) /* a non-finite corner, board point or start pose */

/* The closed-form start: per image (corners [offsets[k], offsets[k+1]) of corners_px / board_xy, as clc_board_poses) the homography
 * board -> pixel - (width / 2, height / 2) by clc_board_poses' normalized DLT (same degeneracy ratio), scaled to unit Frobenius
 * norm; then, over the usable images in image order, the one-unknown least squares for u = 1 / f^2 of h1^T w h2 = 0 and
 * h1^T w h1 = h2^T w h2, w = diag(u, u, 1), h1 and h2 the first two columns.  cam_out: model, fx = fy = 1 / sqrt(u), the principal
 * point at the image centre, zero distortion (for Kannala-Brandt a small-angle approximation: a start only).  *n_used (nullable):
 * the usable images.  CLC_ERR_LINALG when fewer than 2 images are usable or u is not positive and finite (cam_out untouched);
 * CLC_ERR_INVALID_ARG: a model that is neither of the two, width or height <= 0, NULL pointers, decreasing offsets. */
int clc_camera_guess(clc_handle* h, int32_t model, int32_t width, int32_t height, const float* corners_px, const float* board_xy,
                     const int64_t* offsets, size_t n_images, clc_camera* cam_out, int32_t* n_used);
/* The same with corners_px, board_xy and offsets in DEVICE memory (offsets_dev[0] may be > 0; not validated); cam_out and n_used on
 * the host.  The same bits as the host-array form. */
int clc_camera_guess_device(clc_handle* h, int32_t model, int32_t width, int32_t height, const float* corners_px_dev,
                            const float* board_xy_dev, const int64_t* offsets_dev, size_t n_images, clc_camera* cam_out,
                            int32_t* n_used);

/* Image i owns corners [corner_offsets[i], corner_offsets[i+1]) of corners_px / board_xy; problem k owns images
 * [problem_offsets[k], problem_offsets[k+1]) (NULL: one problem of all images) and the camera cams[k] (in: the start, e.g.
 * clc_camera_guess's; out: the minimiser; a held intrinsic keeps its bits).  keep[n_images] (nullable): 0 drops an image.  In / out:
 * q_ca_wxyz[4 n] (out: w >= 0), t_ca[3 n]: the start poses, e.g. clc_board_poses' under the start camera.  An image that takes no
 * part (image_status != CLC_CAMCAL_OK) keeps its pose bit for bit.  A problem with no participating image, a non-finite camera or a
 * failed solve ends CLC_FAILURE with its camera and every pose untouched.  summaries[n_problems]: final_cost is the cost at the
 * returned point.  H_cam[64 n_problems] (nullable): the information on the intrinsics with the board poses marginalised,
 * C - sum B_i^T A_i^-1 B_i at the returned point (undamped, unscaled; rows and columns of held intrinsics zero; C itself with
 * hold_board_poses; NaN where an A_i is not positive definite).  rms_px[n_problems] (nullable): sqrt(sum |project - u|^2 / corners)
 * over the participating images.  copt NULL: clc_camcal_options_default of cams[0].model.  CLC_ERR_INVALID_ARG before any device
 * work: NULL required pointers, a sigma_px that is not finite and positive, mask bits beyond the 8, all 8 bits together with
 * hold_board_poses, offsets that decrease, a camera whose model is neither of the two.  One enqueue, one synchronisation. */
int clc_camera_calibrate(clc_handle* h, const clc_options* opt, const clc_camcal_options* copt, const float* corners_px,
                         const float* board_xy, const int64_t* corner_offsets, const uint8_t* keep, size_t n_images,
                         const int64_t* problem_offsets, size_t n_problems, clc_camera* cams, double* q_ca_wxyz, double* t_ca,
                         clc_summary* summaries, double* H_cam, double* rms_px, int32_t* image_status);
/* The same with every array, cams included, in DEVICE memory; indexing as clc_joint_refine_device: the per-image arrays by the
 * absolute image index (the call covers the n_images images from problem_offsets_dev[0] on, from 0 when it is NULL), corner offsets
 * absolute, the per-problem arrays from problem 0.  Nothing is read back ahead of the enqueue: offsets are not validated, and a
 * camera with an unknown model ends its problem CLC_FAILURE.  copt NULL: sigma 0.3 px, nothing held (the models are not known to
 * the host). */
int clc_camera_calibrate_device(clc_handle* h, const clc_options* opt, const clc_camcal_options* copt, const float* corners_px_dev,
                                const float* board_xy_dev, const int64_t* corner_offsets_dev, const uint8_t* keep_dev, size_t n_images,
                                const int64_t* problem_offsets_dev, size_t n_problems, clc_camera* cams_dev, double* q_ca_wxyz_dev,
                                double* t_ca_dev, clc_summary* summaries_dev, double* H_cam_dev, double* rms_px_dev,
                                int32_t* image_status_dev);

/* ---- pose guidance: rank candidate board poses by predicted information (K20) ---------------------------------------------
 * clc_information's H = sum J^T J depends on the laser points and the poses, not on the residuals.  So for a candidate board pose
 * T_ca (board in the camera frame, the convention of clc_store_observations' tag_q_wxyz / tag_t) the H_add that H would gain at
 * the current T_cl = pose_cl ([t, qx qy qz qw]) if that pose were recorded is computed exactly, without a noise model:
 *   per candidate  n = R_ca e3, d = -n.t_ca, m = R_cl^T n, d_l = n.t_cl + d   (R_ca from q without normalisation, as Eigen)
 *   per ray i      dir_i = (cos th_i, sin th_i, 0), th_i = angle_min + i angle_increment in double;  rho_i = -d_l / (m.dir_i);
 *                  p_i = rho_i dir_i (laser frame);  X_i = R_ca^T (R_cl p_i + t_cl - t_ca) (board frame)
 *   hit            rho_i finite, range_min <= rho_i < range_max (TranScanToPoints), board_min <= (X_x, X_y) <= board_max (closed)
 *   c hits; seen when c >= min_points:  H_add = (1 / c) sum_hits u u^T, u = [n, p x m]  (the factor's Jacobian row with the
 *   reference's per-pose scale 1 / sqrt(c));  unseen: H_add = 0;  a candidate with a non-finite entry: unseen, n_hits = -1.
 * sv: the eigenvalues of M = H0 + H_add, descending, as clc_information reports them.  score: CLC_GUIDE_LOGDET
 * sum_k log max(sv_k, eig_floor), or CLC_GUIDE_MIN_EIG sv[5].  An unseen candidate scores as H0 itself.
 * H mixes metres and radians, as the reference's printed singular values do; the prediction is taken at pose_cl, which on a
 * degenerate recording is itself loose along the null directions. */
#define CLC_GUIDE_LOGDET 0
#define CLC_GUIDE_MIN_EIG 1
typedef struct clc_guidance_options {
  int32_t n_rays;         /* rays of a scan, 1 .. 2^24 */
  int32_t min_points;     /* fewest hits of a seen candidate, >= 1 */
  double angle_min;       /* rad */
  double angle_increment; /* rad */
  double range_min;       /* m; range_min < range_max */
  double range_max;
  double board_min[2];    /* the board rectangle in board coordinates, m; board_min <= board_max */
  double board_max[2];
  double eig_floor;       /* > 0 */
  int32_t criterion;      /* CLC_GUIDE_* */
  int32_t reserved;
} clc_guidance_options;   /* 88 bytes */

/* 1 081 rays over 270 degrees from -135 degrees, ranges [0.05, 30) (src/utilities.cpp:201), 50 points (the shortest segment
 * AutoGetLinePts accepts), the board [-0.043, 0.457]^2 (src/LaseCamCalCeres.cpp:262-268), floor 1e-8 (the reference's null-space
 * threshold, :371), CLC_GUIDE_LOGDET. */
void clc_guidance_options_default(clc_guidance_options* gopt);

/* n_cand candidates q_ca_wxyz[4 n], t_ca[3 n].  H0[36] (row-major, symmetric): the information already collected, clc_information's
 * H at pose_cl; NULL: zeros.  Outputs, every one nullable: n_hits[n], H_add[36 n] row-major, sv[6 n], score[n].  gopt NULL: the
 * defaults.  CLC_ERR_INVALID_ARG before any device work: NULL h, pose_cl or candidate arrays, n_rays <= 0 or > 2^24, min_points < 1,
 * range_min >= range_max or NaN, a non-finite angle, an empty board rectangle, eig_floor <= 0, an unknown criterion;
 * CLC_ERR_NONFINITE: a non-finite pose_cl or H0.  n_cand = 0: CLC_OK, nothing written.  One bad candidate never fails the call.
 * Deterministic: the same bits on every run, and for a candidate alone or in a batch.  One enqueue, one synchronisation. */
int clc_score_board_poses(clc_handle* h, const clc_guidance_options* gopt, const double pose_cl[7], const double* H0, size_t n_cand,
                          const double* q_ca_wxyz, const double* t_ca, int32_t* n_hits, double* H_add, double* sv, double* score);
/* The same with the candidate arrays and the per-candidate outputs in DEVICE memory (ready on the handle's stream); gopt, pose_cl
 * and H0 on the host.  The same bits as the host-array form. */
int clc_score_board_poses_device(clc_handle* h, const clc_guidance_options* gopt, const double pose_cl[7], const double* H0,
                                 size_t n_cand, const double* q_ca_wxyz_dev, const double* t_ca_dev, int32_t* n_hits_dev,
                                 double* H_add_dev, double* sv_dev, double* score_dev);

/* A greedy choice of k candidates without replacement: M_0 = H0; round r picks the seen candidate not yet chosen with the largest
 * score of M_r + H_add (ties: the lowest index; a score that is NaN is never picked), then M_{r+1} = M_r + H_add[chosen], a plain
 * add in chosen order.  It stops when no such candidate remains.  chosen[k]: the indices in order, padded with -1;
 * sv_after[6 k], score_after[k] (nullable): the eigenvalues and the score of M_{r+1} (NaN in the padding); H_after[36] (nullable):
 * the last M; *n_chosen (nullable).  The rays are cast once; the k rounds are enqueued back to back and the call synchronises once.
 * Errors as clc_score_board_poses, and k < 1 or chosen NULL: CLC_ERR_INVALID_ARG.  n_cand = 0: CLC_OK, nothing written. */
int clc_select_board_poses(clc_handle* h, const clc_guidance_options* gopt, const double pose_cl[7], const double* H0, size_t n_cand,
                           const double* q_ca_wxyz, const double* t_ca, size_t k, int64_t* chosen, double* sv_after,
                           double* score_after, double* H_after, int32_t* n_chosen);
/* The same with the candidate arrays in DEVICE memory; the k-sized results and H_after on the host. */
int clc_select_board_poses_device(clc_handle* h, const clc_guidance_options* gopt, const double pose_cl[7], const double* H0,
                                  size_t n_cand, const double* q_ca_wxyz_dev, const double* t_ca_dev, size_t k, int64_t* chosen,
                                  double* sv_after, double* score_after, double* H_after, int32_t* n_chosen);

/* ---- laser range offset and scale in the joint refinement (K21) ----------------------------------------------------------
 * clc_joint_refine's cost with the scanner's own two parameters: the measured point p (laser frame) is corrected along its ray,
 *   p' = (1 + kappa + b / |p|) p        true range = (1 + kappa) measured + b;  b: range offset (metres), kappa: range scale
 * and takes p's place in the laser term.  The shared block of the solve has 8 parameters [dt_cl, dtheta_cl, b, kappa]; b and kappa
 * move additively.  One kernel launch per call (one workgroup per problem), clc_options as in clc_joint_refine, deterministic.
 * b and kappa separate only through a spread of ranges, and b separates from t_cl only through a spread of plane normals and ray
 * directions: a recording at a single range cannot have both free (the damping keeps the solve finite; H_cr shows it) — hold one
 * of them there. */
typedef struct clc_range_options {
  double sigma_corner;      /* as clc_joint_options; not looked at with hold_board_poses */
  double sigma_laser;       /* metres, finite, > 0 */
  int32_t hold_board_poses; /* 1: the board poses stay; the corner terms are constant and left out, no corner is read */
  int32_t hold_extrinsic;   /* 1: T_cl stays */
  int32_t hold_range_mask;  /* bit 0: the offset is held, bit 1: the scale is held; a held parameter is still applied */
  int32_t reserved;         /* 0 */
} clc_range_options;        /* 32 bytes */

/* clc_joint_options_default's sigmas, nothing held; cam NULL: sigma_corner 0 (refused unless hold_board_poses is set). */
void clc_range_options_default(clc_range_options* ropt, const clc_camera* cam);

/* The arguments of clc_joint_refine, and range[2 n_problems] in / out: b, kappa of every problem (the start, e.g. zeros; a held
 * one keeps its bits).  image_status: the CLC_JOINT_* values; a laser point that is non-finite or has |p| = 0 (the scanner's "no
 * return") makes its image CLC_JOINT_NONFINITE.  With hold_board_poses an image needs no corners: it takes part if it is kept and
 * its points and start pose are finite; corners_px, board_xy and corner_offsets may then be NULL (they are not read), cam may be
 * NULL, and the corner share of the cost is 0.  Without it fewer than 4 corners give CLC_JOINT_TOO_FEW.  With no laser point in a
 * problem T_cl and range come back bit for bit; hold_extrinsic leaves T_cl bit for bit while the free range parameters move.  A
 * problem with no participating image, a non-finite T_cl or range, or a failed solve ends CLC_FAILURE with everything untouched.
 * H_cr[64 n_problems] (nullable): the information on [T_cl tangent, b, kappa] with the board poses marginalised, at the returned
 * point, undamped (C itself with hold_board_poses; NaN where an A_i is not positive definite; rows and columns of held parameters,
 * T_cl's with hold_extrinsic, zero).  summaries, cost_parts: as clc_joint_refine.  ropt NULL: the defaults.
 * CLC_ERR_INVALID_ARG before any device work: NULL required pointers, a sigma that is not finite and positive (sigma_corner only
 * without hold_board_poses), both hold flags, a mask outside 0..3, reserved != 0, offsets that decrease, corner arrays NULL without
 * hold_board_poses.  One enqueue (lift, then the solve) and one synchronisation. */
int clc_joint_refine_range(clc_handle* h, const clc_camera* cam, const clc_options* opt, const clc_range_options* ropt,
                           const float* corners_px, const float* board_xy, const int64_t* corner_offsets, const double* pts,
                           const int64_t* pts_offsets, const uint8_t* keep, size_t n_images, const int64_t* problem_offsets,
                           size_t n_problems, double* q_ca_wxyz, double* t_ca, double* poses_cl, double* range, clc_summary* summaries,
                           double* H_cr, double* cost_parts, int32_t* image_status);
/* The same with every array in DEVICE memory; the conventions of clc_joint_refine_device. */
int clc_joint_refine_range_device(clc_handle* h, const clc_camera* cam, const clc_options* opt, const clc_range_options* ropt,
                                  const float* corners_px_dev, const float* board_xy_dev, const int64_t* corner_offsets_dev,
                                  const double* pts_dev, const int64_t* pts_offsets_dev, const uint8_t* keep_dev, size_t n_images,
                                  const int64_t* problem_offsets_dev, size_t n_problems, double* q_ca_wxyz_dev, double* t_ca_dev,
                                  double* poses_cl_dev, double* range_dev, clc_summary* summaries_dev, double* H_cr_dev,
                                  double* cost_parts_dev, int32_t* image_status_dev);

/* out[3 n] = p' of pts[3 n] for range = {b, kappa}; a point that is non-finite or has |p| = 0 becomes NaN.  out may be pts.
 * CLC_ERR_INVALID_ARG: NULL h, range, or (n > 0) pts / out; CLC_ERR_NONFINITE: a non-finite b or kappa.  n = 0: CLC_OK. */
int clc_range_correct(clc_handle* h, const double range[2], const double* pts, size_t n, double* out);
/* The same with pts and out in DEVICE memory (ready on the handle's stream); range on the host.  The same bits. */
int clc_range_correct_device(clc_handle* h, const double range[2], const double* pts_dev, size_t n, double* out_dev);

/* ---- robust joint refinement: a Cauchy loss per corner and per laser point (K22) -------------------------------------------
 * clc_joint_refine's model, tangent, sigmas, hold flags, image status, keep, offsets and clc_options, under the cost
 *   1/2 sum rho_ac(|e_j|^2) + 1/2 sum rho_al(r_k^2),   rho_a(z) = a^2 log1p(z / a^2),  rho_a'(z) = 1 / (1 + z / a^2)
 * with e_j the corner's residual 2-vector over sigma_corner (one loss on its squared norm, a 2-D residual block under a Ceres
 * LossFunction) and r_k the laser residual over sigma_laser.  The scales a are in units of sigma; a = 0: no loss on that term.
 * The Gauss-Newton blocks follow Ceres' corrector for rho'' <= 0: the rows and the residual of an observation are scaled by
 * sqrt(rho'), so the blocks take w J^T J and the gradients w J^T r, w = rho'(z).  keep drops whole images, K16 whole tags and K12
 * whole poses; this cost is the way out for a single bad laser point inside a board segment or a single bad corner.
 * One workgroup per problem and the whole solve in one launch, as clc_joint_refine; deterministic. */
typedef struct clc_joint_loss_options {
  double loss_corner;  /* Cauchy scale of a corner's residual vector in units of sigma_corner; 0: no loss */
  double loss_laser;   /* Cauchy scale of a laser residual in units of sigma_laser; 0: no loss */
} clc_joint_loss_options;   /* 16 bytes */

/* loss_laser = 0.05 / jopt->sigma_laser: the reference's CauchyLoss(0.05) in metres (5 at the default 0.01 m; 5 with jopt NULL).
 * loss_corner = 3: a design value of this library (0.9 px at the default 0.3 px); the reference puts no loss on corners. */
void clc_joint_loss_options_default(clc_joint_loss_options* lopt, const clc_joint_options* jopt);

/* The arguments of clc_joint_refine in its order, lopt after jopt (NULL: the defaults for the call's jopt), and two outputs:
 * w_corner (nullable; indexed as corners_px: one value per corner) and w_laser (nullable; indexed as pts: one per point) =
 * rho'(z) of every observation at the returned poses — 1 where that term has no loss, NaN for an image that takes no part (any
 * status but CLC_JOINT_OK, or outside every problem) and for a problem that ended CLC_FAILURE.  w >= 0.5 is the same statement
 * as |residual| <= a sigma.  summaries[k].final_cost is the robust cost at the returned point, cost_parts its corner and laser
 * shares, H_cl the Schur complement of the weighted blocks there.  An evaluation with a corner at depth <= 0 is invalid, as in
 * clc_joint_refine.  With both scales 0 the call returns clc_joint_refine's bits (and weights 1).
 * CLC_ERR_INVALID_ARG before any device work: everything clc_joint_refine refuses, with its messages behind this function's
 * name, and a loss scale that is negative or not finite ("loss_corner must be finite and >= 0", "loss_laser ...").
 * One enqueue (lift, solve, weights) and one synchronisation. */
int clc_joint_refine_robust(clc_handle* h, const clc_camera* cam, const clc_options* opt, const clc_joint_options* jopt,
                            const clc_joint_loss_options* lopt, const float* corners_px, const float* board_xy,
                            const int64_t* corner_offsets, const double* pts, const int64_t* pts_offsets, const uint8_t* keep,
                            size_t n_images, const int64_t* problem_offsets, size_t n_problems, double* q_ca_wxyz, double* t_ca,
                            double* poses_cl, clc_summary* summaries, double* H_cl, double* cost_parts, int32_t* image_status,
                            double* w_corner, double* w_laser);
/* The same with every array in DEVICE memory; the conventions of clc_joint_refine_device.  w_corner_dev and w_laser_dev are
 * indexed by the absolute corner / point offsets; the entries of images outside every problem are left as they are. */
int clc_joint_refine_robust_device(clc_handle* h, const clc_camera* cam, const clc_options* opt, const clc_joint_options* jopt,
                                   const clc_joint_loss_options* lopt, const float* corners_px_dev, const float* board_xy_dev,
                                   const int64_t* corner_offsets_dev, const double* pts_dev, const int64_t* pts_offsets_dev,
                                   const uint8_t* keep_dev, size_t n_images, const int64_t* problem_offsets_dev, size_t n_problems,
                                   double* q_ca_wxyz_dev, double* t_ca_dev, double* poses_cl_dev, clc_summary* summaries_dev,
                                   double* H_cl_dev, double* cost_parts_dev, int32_t* image_status_dev, double* w_corner_dev,
                                   double* w_laser_dev);

/* ---- one robust cost over intrinsics, board poses, T_cl and range (K23) ------------------------------------------------------
 * The call at the end of the flow: one problem is one camera, one scanner and P images, and everything is refined under one cost,
 *   corner j of image i   e_j = (project(cam, R_i X_j + t_i) - u_j) / sigma_px                  clc_camera_calibrate's residual, pixels
 *   laser point k         r_k = e3^T R_i^T (R_cl p'_k + t_cl - t_i) / sigma_laser,  p' = (1 + kappa + b / |p|) p   clc_joint_refine_range's
 *   cost = 1/2 sum rho_ac(|e_j|^2) + 1/2 sum rho_al(r_k^2)                                      clc_joint_refine_robust's loss and corrector
 * over the tangent [dt, dtheta] of every board pose and a shared block of 16 in this order:
 *   [dt_cl(3), dtheta_cl(3), b, kappa, proj[0..3], dist[0..3]]
 * (the leading 8 laid out as H_cr, the trailing 8 in clc_camera order; b, kappa and the intrinsics move additively).  The laser rows
 * do not depend on the intrinsics and the corner rows not on T_cl, b, kappa: the two groups couple only through the board poses.
 * One workgroup per problem and the whole Levenberg-Marquardt solve in one launch, clc_options as in the other solves (opt NULL =
 * clc_pose_options_default()); deterministic: the same bits on every run, for a problem alone or in a batch, and through both forms. */
typedef struct clc_full_options {
  double sigma_px;               /* pixels, finite, > 0 (only looked at while the corners take part) */
  double sigma_laser;            /* metres, finite, > 0 */
  double loss_corner;            /* Cauchy scale of a corner's residual vector in units of sigma_px; 0: no loss; finite, >= 0 */
  double loss_laser;             /* Cauchy scale of a laser residual in units of sigma_laser; 0: no loss; finite, >= 0 */
  uint32_t hold_intrinsics_mask; /* bit j: intrinsic j (proj[0..3], dist[0..3]) is held */
  int32_t hold_range_mask;       /* bit 0: b is held, bit 1: kappa is held; a held one is still applied */
  int32_t hold_board_poses;      /* 1: the board poses stay */
  int32_t hold_extrinsic;        /* 1: T_cl stays */
} clc_full_options;              /* 48 bytes */

/* 0.3 px, 0.01 m, loss scales 3 and 5 (clc_joint_loss_options_default's at those sigmas); for CLC_CAMERA_KANNALA_BRANDT k4 and k5
 * are held (clc_camcal_options_default); nothing else is held. */
void clc_full_options_default(clc_full_options* fopt, int32_t model);

/* The arguments of clc_joint_refine_range in its order, with cams[n_problems] in / out (one start camera per problem, as
 * clc_camera_calibrate; a held intrinsic keeps its bits) in place of cam, and the outputs summaries, H_full[256 n_problems],
 * cost_parts[2 n_problems], rms_px[n_problems], image_status, w_corner (one per corner, indexed as corners_px) and w_laser (one per
 * point, indexed as pts); all of them nullable except summaries and image_status.  image_status: the CLC_JOINT_* values, a corner at
 * a non-finite pixel or a point that is non-finite or has |p| = 0 makes its image CLC_JOINT_NONFINITE; an evaluation with a corner
 * at P_z <= 0 is invalid.  H_full: the information on the 16 shared parameters with the board poses marginalised,
 * C - sum B_i^T A_i^-1 B_i of the weighted blocks at the returned point, undamped and unscaled; rows and columns of held parameters
 * zero; C itself with hold_board_poses; NaN where an A_i is not positive definite.  rms_px: sigma_px sqrt(2 cost_corner / corners)
 * over the participating images — clc_camera_calibrate's RMS where loss_corner is 0.  w_corner, w_laser: rho' of every observation
 * at the returned point, clc_joint_refine_robust's conventions (1 without a loss, NaN for an image that takes no part or a failed
 * problem).  A held parameter keeps its bits: the intrinsics and b, kappa bit by bit, T_cl with hold_extrinsic, the board poses
 * with hold_board_poses; a problem without a laser point holds T_cl, b and kappa by itself.  With hold_board_poses and all 8
 * intrinsics held the corner terms are constant: they are left out, no corner is read (the corner arrays may be NULL), an image
 * needs no corners, the corner share of the cost is 0 and no w_corner is written.  Both hold flags together are allowed as long as
 * something else moves.  A problem with no participating image, a non-finite start or a failed solve ends CLC_FAILURE with
 * everything of the problem untouched.  fopt NULL: clc_full_options_default of cams[0].model.
 * CLC_ERR_INVALID_ARG before any device work: NULL required pointers, a sigma that is not finite and positive, a loss scale that is
 * negative or not finite, mask bits out of range, all 16 shared parameters held together with hold_board_poses, offsets that
 * decrease, a camera whose model is neither of the two.  One enqueue (solve, weights) and one synchronisation. */
int clc_calibrate_full(clc_handle* h, clc_camera* cams, const clc_options* opt, const clc_full_options* fopt, const float* corners_px,
                       const float* board_xy, const int64_t* corner_offsets, const double* pts, const int64_t* pts_offsets,
                       const uint8_t* keep, size_t n_images, const int64_t* problem_offsets, size_t n_problems, double* q_ca_wxyz,
                       double* t_ca, double* poses_cl, double* range, clc_summary* summaries, double* H_full, double* cost_parts,
                       double* rms_px, int32_t* image_status, double* w_corner, double* w_laser);
/* The same with every array, cams included, in DEVICE memory; the indexing conventions of clc_joint_refine_device.  Nothing is
 * read back ahead of the enqueue (the workspace is sized from n_images alone, as clc_camera_calibrate_device): offsets are not
 * validated, and a camera with an unknown model ends its problem CLC_FAILURE.  fopt NULL: the defaults of CLC_CAMERA_PINHOLE (the
 * models are not known to the host).  The entries of w_corner_dev / w_laser_dev of images outside every problem are left as they
 * are. */
int clc_calibrate_full_device(clc_handle* h, clc_camera* cams_dev, const clc_options* opt, const clc_full_options* fopt,
                              const float* corners_px_dev, const float* board_xy_dev, const int64_t* corner_offsets_dev,
                              const double* pts_dev, const int64_t* pts_offsets_dev, const uint8_t* keep_dev, size_t n_images,
                              const int64_t* problem_offsets_dev, size_t n_problems, double* q_ca_wxyz_dev, double* t_ca_dev,
                              double* poses_cl_dev, double* range_dev, clc_summary* summaries_dev, double* H_full_dev,
                              double* cost_parts_dev, double* rms_px_dev, int32_t* image_status_dev, double* w_corner_dev,
                              double* w_laser_dev);

/* ---- sub-pixel corner refinement: batched cornerSubPix (K24) -----------------------------------------------------------------
 * What the reference runs on every detection ahead of its pose estimate (cv::cornerSubPix, src/calcCamPose.cpp:20-22 with
 * half-window 11 on the chessboard, :86-89 with half-window 3 on the Kalibr tag grid; 30 iterations, eps 0.1), restated from
 * the published algorithm (DESIGN.md K24 holds every rounding step; the gap to OpenCV's own bits is NOT measured: OpenCV does not
 * exist where this library is built).  Per corner, from cI = the start, in float32:
 *   the (2 win_x + 3) x (2 win_y + 3) patch about cI, bilinear with ONE fractional pair for the whole patch and the border
 *   replicated (getRectSubPix);  central differences tgx, tgy on the (2 win_x + 1) x (2 win_y + 1) window;  with the mask
 *   m = exp(-(i / win_y)^2) exp(-(j / win_x)^2), 0 inside the zero zone:  a = sum m tgx^2, b = sum m tgx tgy, c = sum m tgy^2,
 *   bb1 = sum m (tgx^2 px + tgx tgy py), bb2 = sum m (tgx tgy px + tgy^2 py) in double;  cI += [[a, b], [b, c]]^-1 [bb1, bb2];
 *   until the squared shift is <= eps^2, max_iter iterations are done, the matrix is singular (|det| <= DBL_EPSILON^2) or cI has
 *   left the image;  a result farther than the half-window from the start in x or y is given up: the start comes back.
 * Two additions over OpenCV, both per corner and never an error of the call: a non-finite start comes back unchanged
 * (CLC_SUBPIX_NONFINITE), and so does a start outside [0, width) x [0, height) (CLC_SUBPIX_LEFT_IMAGE, 0 iterations). */
#define CLC_SUBPIX_MAX_WIN 15
#define CLC_SUBPIX_CONVERGED 1   /* the last shift was <= eps */
#define CLC_SUBPIX_MAX_ITER 0    /* max_iter iterations, the result kept */
#define CLC_SUBPIX_SINGULAR -1   /* a flat or edge-only window: the iterate before it is returned */
#define CLC_SUBPIX_LEFT_IMAGE -2 /* the iterate (or the start) is outside the image; the iterate is returned as it is */
#define CLC_SUBPIX_REVERTED -3   /* farther than the half-window from the start: the start is returned; over every other status */
#define CLC_SUBPIX_NONFINITE -4  /* a non-finite start, returned unchanged */
typedef struct clc_subpix_options {
  int32_t win_x, win_y;   /* half sizes of the window, 1 .. CLC_SUBPIX_MAX_WIN */
  int32_t zero_x, zero_y; /* half sizes of the zero zone; off when either is negative or it is not smaller than the window */
  int32_t max_iter;       /* 1 .. 100 */
  int32_t reserved;       /* 0 */
  double eps;             /* pixels, finite, >= 0 */
} clc_subpix_options;     /* 32 bytes */

/* win_x = win_y = win (win <= 0: 3, the reference's Kalibr call), no zero zone, 30 iterations, eps 0.1. */
void clc_subpix_options_default(clc_subpix_options* sopt, int32_t win);

/* images[n_images][height][pitch] uint8 grey (pitch >= width bytes per row), corners_in[2 M] float32 (x, y) pixels grouped per
 * image by offsets[n_images + 1] (absolute indices into the corner arrays; offsets[0] may be > 0).  corners_out[2 M] (required;
 * may be corners_in), and, every one nullable, status[M] (CLC_SUBPIX_*), iterations[M], strength[M]: the smaller eigenvalue of
 * [[a, b], [b, c]] / sum m at the last evaluated iterate (NaN where none was evaluated) — a measure to drop weak corners by.
 * All of them indexed as corners_in.  sopt NULL: the defaults of win 3.  CLC_ERR_INVALID_ARG before any device work: NULL h,
 * images, corners_in, offsets or corners_out, width or height < 1, pitch < width, a half-window outside 1 .. 15, max_iter outside
 * 1 .. 100, eps negative or not finite, reserved != 0, offsets that decrease.  n_images = 0 or no corner: CLC_OK, nothing
 * written.  One wave per corner; deterministic: the same bits on every run, for a corner alone or in a batch, and through both
 * forms.  One enqueue, one synchronisation. */
int clc_corner_subpix(clc_handle* h, const clc_subpix_options* sopt, const uint8_t* images, int32_t width, int32_t height,
                      int64_t pitch, size_t n_images, const float* corners_in, const int64_t* offsets, float* corners_out,
                      int32_t* status, int32_t* iterations, double* strength);
/* The same with every array in DEVICE memory (ready on the handle's stream); complete on return.  The two ends of offsets_dev
 * are read ahead of the enqueue; the offsets in between are not validated. */
int clc_corner_subpix_device(clc_handle* h, const clc_subpix_options* sopt, const uint8_t* images_dev, int32_t width, int32_t height,
                             int64_t pitch, size_t n_images, const float* corners_in_dev, const int64_t* offsets_dev,
                             float* corners_out_dev, int32_t* status_dev, int32_t* iterations_dev, double* strength_dev);

/* ---- chessboard corners from images: detect, order, refine (K25) ----------------------------------------------------------------
 * The step the reference takes from OpenCV ahead of cornerSubPix on its chessboard (cv::findChessboardCorners,
 * src/calcCamPose.cpp:10-47), by an algorithm of this library's own (nothing of OpenCV's implementation is used or
 * matched).  Detection on the device: the ChESS response (Bennett & Lasenby) scaled by 5, exact int32 arithmetic on the uint8 image.
 * Integer pixel coordinates are pixel centres.  With I the image, the ring (dx, dy), n = 0 .. 15:
 *   (0,-5) (2,-5) (3,-3) (5,-2) (5,0) (5,2) (3,3) (2,5) (0,5) (-2,5) (-3,3) (-5,2) (-5,0) (-5,-2) (-3,-3) (-2,-5)
 * and the cross (0,0) (1,0) (-1,0) (0,1) (0,-1):  SR = sum_{n<4} |(s_n + s_{n+8}) - (s_{n+4} + s_{n+12})|,
 * DR = sum_{n<8} |s_n - s_{n+8}|, ring = sum s_n, loc = sum cross, R5 = 5 SR - 5 DR - |5 ring - 16 loc| on the domain
 * 5 <= x < width - 5, 5 <= y < height - 5 (empty where width < 11 or height < 11: CLC_OK, no candidate).
 * A domain pixel p is a raw candidate iff R5(p) >= threshold and every other domain pixel q within nms_radius in x and in y has
 * R5(q) < R5(p), or R5(q) == R5(p) and comes after p in raster order (y, then x).  Of the raw candidates those with
 * 1000 R5 >= rel_permille x the image's largest R5 are kept, ordered by (-R5, y, x), and the first max_per_image are returned.
 * An image with more than CLC_CHESS_RAW_CAP raw candidates has status CLC_CHESS_OVERFLOW and no candidate. */
#define CLC_CHESS_MAX_CANDIDATES 1024
#define CLC_CHESS_RAW_CAP 4096
#define CLC_CHESS_OK 1        /* detection: the image's candidates are complete */
#define CLC_CHESS_FOUND 1     /* ordering: index holds the board's grid */
#define CLC_CHESS_TOO_FEW 0   /* ordering: fewer than cols x rows candidates */
#define CLC_CHESS_NO_GRID -1  /* ordering: no valid labeling */
#define CLC_CHESS_OVERFLOW -2 /* detection: more than CLC_CHESS_RAW_CAP raw candidates; passed through by the ordering */
typedef struct clc_chess_options {
  int32_t threshold;     /* on R5, >= 1 */
  int32_t nms_radius;    /* 1 .. 7 */
  int32_t rel_permille;  /* 0 .. 1000 */
  int32_t max_per_image; /* 1 .. CLC_CHESS_MAX_CANDIDATES: the stride of the candidate arrays */
  int32_t reserved;      /* 0 */
} clc_chess_options;     /* 20 bytes */
typedef struct clc_chessorder_options {
  double tol;            /* the largest match distance over the smallest predicted spacing, in (0, 0.5] */
  int32_t reserved, reserved2; /* 0 */
} clc_chessorder_options; /* 16 bytes */

/* threshold 500, nms_radius 3, rel_permille 250, max_per_image 256. */
void clc_chess_options_default(clc_chess_options* copt);
/* tol 0.3. */
void clc_chessorder_options_default(clc_chessorder_options* oopt);

/* images[n_images][height][pitch] uint8 grey, as clc_corner_subpix takes them.  With stride = max_per_image:
 * cand_xy[n_images stride 2] float32 the integer pixels (x, y) in the order above, NaN in the unused slots (the whole array can go
 * to clc_corner_subpix_device with offsets k stride: a non-finite start comes back unchanged); cand_r5[n_images stride] (nullable;
 * 0 in the unused slots); count[n_images]; count_raw[n_images] (nullable; the raw candidates, also beyond the cap);
 * status[n_images] (CLC_CHESS_OK / CLC_CHESS_OVERFLOW).  copt NULL: the defaults.  CLC_ERR_INVALID_ARG before any device work: an
 * option outside its range, width or height < 1, pitch < width, more than 2^31 - 1 images or tiles of 64 x 16 pixels, NULL images,
 * cand_xy, count or status, NULL h.  n_images = 0: CLC_OK, nothing written.  Deterministic: the same bits on every run, for an image
 * alone or in a batch, and through both forms.  One enqueue (in chunks of 170 images on the handle's stream), one synchronisation. */
int clc_chess_corners(clc_handle* h, const clc_chess_options* copt, const uint8_t* images, int32_t width, int32_t height, int64_t pitch,
                      size_t n_images, float* cand_xy, int32_t* cand_r5, int32_t* count, int32_t* count_raw, int32_t* status);
/* The same with every array in DEVICE memory (ready on the handle's stream); complete on return. */
int clc_chess_corners_device(clc_handle* h, const clc_chess_options* copt, const uint8_t* images_dev, int32_t width, int32_t height,
                             int64_t pitch, size_t n_images, float* cand_xy_dev, int32_t* cand_r5_dev, int32_t* count_dev,
                             int32_t* count_raw_dev, int32_t* status_dev);

/* Host code, no handle and no device: the first cols x rows candidates of every image (cand_xy[n_images stride 2], count[n_images]
 * as clc_chess_corners wrote them) ordered into the board's grid of cols x rows inner corners.  Per image: the convex hull of the
 * integer pixels; the 4 hull vertices of the largest quadrilateral; for each of its 4 rotations as the images of the grid nodes
 * (0, 0), (cols - 1, 0), (cols - 1, rows - 1), (0, rows - 1) the 4-point homography, every node's nearest candidate, valid iff a
 * bijection with every distance <= tol x the smallest predicted spacing, then the least-squares homography of all matches and the
 * matching once more.  The board is taken to be seen from its front, so 2 labelings are valid on a rectangular grid and up to 4 on a
 * square one: the one whose node (0, 0) comes first in raster order (y, then x) is returned; the colour of the squares is not
 * consulted (cv::findChessboardCorners leaves the same half turn open).  index[n_images cols rows]: index[i cols + j] = the candidate
 * slot of node (j, i), -1 where status != CLC_CHESS_FOUND, the order of the reference's board points (j square, i square, 0),
 * src/calcCamPose.cpp:26-36.  status[n_images] is read and written: CLC_CHESS_OVERFLOW on entry stays; otherwise CLC_CHESS_FOUND,
 * CLC_CHESS_TOO_FEW (count < cols rows) or CLC_CHESS_NO_GRID.  n_labelings[n_images], worst[n_images] (the largest distance /
 * spacing ratio of the last pass; NaN where no grid was found): nullable.  oopt NULL: tol 0.3.  CLC_ERR_INVALID_ARG: tol outside
 * (0, 0.5], reserved != 0, cols or rows < 2, cols rows > CLC_CHESS_MAX_CANDIDATES, stride < cols rows, a NULL required array.
 * A board under strong fisheye distortion is beyond one homography: CLC_CHESS_NO_GRID. */
int clc_chessboard_order(const float* cand_xy, const int32_t* count, int64_t stride, size_t n_images, int32_t cols, int32_t rows,
                         const clc_chessorder_options* oopt, int32_t* index, int32_t* status, int32_t* n_labelings, double* worst);

/* Images in, ordered corners out (host arrays): the detection on the device, the ordering on the host, and with sopt != NULL the
 * refinement of the ordered pixels by clc_corner_subpix_device on the images already uploaded (the reference's chessboard call:
 * clc_subpix_options_default(&s, 11)); sopt NULL: the integer pixels.  corners[n_images cols rows 2], found[n_images] (1 / 0),
 * strength[n_images cols rows] (nullable; clc_corner_subpix's).  An image without a board has NaN corners and found = 0 and never
 * fails the call.  copt->max_per_image must be >= cols rows.  Every CLC_ERR_INVALID_ARG of the three calls, before any device work. */
int clc_find_chessboard(clc_handle* h, const clc_chess_options* copt, const clc_chessorder_options* oopt, const clc_subpix_options* sopt,
                        const uint8_t* images, int32_t width, int32_t height, int64_t pitch, size_t n_images, int32_t cols, int32_t rows,
                        float* corners, int32_t* found, double* strength);

/* ---- the ordering on the device (K26) ------------------------------------------------------------------------------------------
 * clc_chessboard_order on device arrays, one wave per image, rule for rule the host code: index, status and n_labelings are the
 * host call's values; worst agrees with it to a few units in the last place (the predicted spacing is sqrt(dx dx + dy dy) where the
 * host calls hypot) and is the same bits from call to call.  One enqueue on the handle's stream and one synchronisation; the arrays
 * must be ready on that stream.  n_labelings_dev and worst_dev are nullable.  It refuses what clc_chessboard_order refuses, in the
 * same order, then a NULL handle; all before any device work. */
int clc_chessboard_order_device(clc_handle* h, const float* cand_xy_dev, const int32_t* count_dev, int64_t stride, size_t n_images,
                                int32_t cols, int32_t rows, const clc_chessorder_options* oopt, int32_t* index_dev, int32_t* status_dev,
                                int32_t* n_labelings_dev, double* worst_dev);

/* clc_find_chessboard on device arrays: detection, ordering, the gather of the ordered pixels and with sopt != NULL the refinement,
 * all on the device with nothing read back in between.  corners_dev[n_images cols rows 2], found_dev[n_images], strength_dev
 * [n_images cols rows] (nullable; NaN with sopt NULL).  The results are clc_find_chessboard's.  It refuses what clc_find_chessboard
 * refuses, in the same order. */
int clc_find_chessboard_device(clc_handle* h, const clc_chess_options* copt, const clc_chessorder_options* oopt,
                               const clc_subpix_options* sopt, const uint8_t* images_dev, int32_t width, int32_t height, int64_t pitch,
                               size_t n_images, int32_t cols, int32_t rows, float* corners_dev, int32_t* found_dev, double* strength_dev);

/* clc_find_chessboard with the ordering on the device (host arrays): the images go up once, clc_find_chessboard_device's stages run,
 * corners, found and strength come back. */
int clc_find_chessboard_gpu(clc_handle* h, const clc_chess_options* copt, const clc_chessorder_options* oopt, const clc_subpix_options* sopt,
                            const uint8_t* images, int32_t width, int32_t height, int64_t pitch, size_t n_images, int32_t cols, int32_t rows,
                            float* corners, int32_t* found, double* strength);

/* ---- tag-grid corners from images: quads, decode, refine (K27) -------------------------------------------------------------------
 * The reference's default board (KALIBR_TAG_PATTERN, src/calcCamPose.cpp:48-139): a grid of cols x rows square tags, tag id =
 * row cols + col, with a black spacer square at every grid intersection, so that every tag corner is an X-junction and K25's response
 * finds it.  Per image: K25's candidates; the directed edges between candidates that have the tag's black border on their right-hand
 * side (image coordinates, y down) and white on the other; the directed 4-cycles of such edges (the quads, in lexicographic order of
 * their slots); per quad one homography from the unit square (K26's 4-point solve), the dd x dd cells sampled at their centres against
 * the mean of the 48 edge samples, the border ring checked, the payload word compared with every code of the family under its four
 * rotations, the best under (Hamming, id, rotation) accepted at a distance <= max_hamming.  DESIGN.md K27 holds every rule.  The code
 * table is the caller's: this library ships none.  A tag cut by the image border is not seen; the others are. */
#define CLC_TAG_MAX_QUADS 1024
#define CLC_TAG_MAX_OUT 4     /* kept directed edges per candidate */
#define CLC_TAG_MAX_TAGS 1024 /* cols x rows */
#define CLC_TAG_MAX_CODES 4096
#define CLC_TAG_OK 1
#define CLC_TAG_OVERFLOW -2   /* the image's detection ended CLC_CHESS_OVERFLOW: no tag */
typedef struct clc_tag_family {
  int32_t side;          /* payload cells per side d, 3 .. 7 */
  int32_t border;        /* black border in cells b, 1 .. 2; dd = d + 2 b */
  int32_t n_codes;       /* 1 .. CLC_TAG_MAX_CODES */
  int32_t max_hamming;   /* a decode is accepted at a distance <= this, 0 .. d d / 2 */
  const uint64_t* codes; /* [n_codes], host memory; bit d d - 1 = payload cell (row 0, col 0) of the upright tag, row-major, top row first */
} clc_tag_family;
typedef struct clc_tag_options {
  int32_t min_side_px;       /* >= 8: shorter candidate pairs are not tested */
  int32_t max_side_px;       /* 0: min(width, height); otherwise >= min_side_px */
  int32_t contrast;          /* 1 .. 255: min(outside) - max(inside) of an edge's samples */
  int32_t max_border_errors; /* 0 .. 8 white cells in the border ring */
  int32_t max_quads;         /* 1 .. CLC_TAG_MAX_QUADS quads decoded per image */
  int32_t reserved;          /* 0 */
} clc_tag_options;           /* 24 bytes */

/* min_side_px 16, max_side_px 0, contrast 40, max_border_errors 0, max_quads 256. */
void clc_tag_options_default(clc_tag_options* topt);

/* images[n_images][height][pitch] uint8 grey, as clc_chess_corners takes them; T = cols rows tags.  corners[n_images T 4 2]: the
 * tag's corners 0 .. 3 in the order of the reference's TagDetection::p (counter-clockwise on the upright printed tag from its
 * bottom-left corner: board points (X0, Y0), (X0 + a, Y0), (X0 + a, Y0 + a), (X0, Y0 + a) with (X0, Y0) = (col, row) a (1 + spacing),
 * src/calcCamPose.cpp:104-137), integer pixels, or with sopt != NULL refined by clc_corner_subpix_device on the resident images
 * (the reference's call: clc_subpix_options_default(&s, 3)); NaN for a tag not seen.  hamming[n_images T]: the decode's distance,
 * -1 for a tag not seen.  count[n_images]: tags seen.  status[n_images]: CLC_TAG_OK / CLC_TAG_OVERFLOW.  Nullable: n_quads[n_images]
 * (every quad, also those past max_quads), n_foreign[n_images] (decodes of an id >= T), n_edges_dropped[n_images] (passing edges past
 * CLC_TAG_MAX_OUT of their candidate), strength[n_images T 4] (clc_corner_subpix's; NaN with sopt NULL).  topt NULL: the defaults;
 * copt NULL: K25's defaults with max_per_image 1024.  CLC_ERR_INVALID_ARG before any device work: an option or a family field out
 * of range, a code with bits above d d, reserved != 0, cols rows < 1 or > CLC_TAG_MAX_TAGS, what clc_chess_corners refuses, a NULL
 * required array.  An image without a tag never fails the call; the bits are the same on every run, alone or in a batch. */
int clc_tag_grid(clc_handle* h, const clc_tag_family* family, const clc_tag_options* topt, const clc_chess_options* copt,
                 const clc_subpix_options* sopt, const uint8_t* images, int32_t width, int32_t height, int64_t pitch, size_t n_images,
                 int32_t cols, int32_t rows, float* corners, int32_t* hamming, int32_t* count, int32_t* status, int32_t* n_quads,
                 int32_t* n_foreign, int32_t* n_edges_dropped, double* strength);

/* clc_tag_grid on device arrays (the family stays a host struct: the call stages its codes): every stage is enqueued on the handle's
 * stream with nothing read back in between, and the call returns after one wait at its end (with sopt: clc_corner_subpix_device's). */
int clc_tag_grid_device(clc_handle* h, const clc_tag_family* family, const clc_tag_options* topt, const clc_chess_options* copt,
                        const clc_subpix_options* sopt, const uint8_t* images_dev, int32_t width, int32_t height, int64_t pitch,
                        size_t n_images, int32_t cols, int32_t rows, float* corners_dev, int32_t* hamming_dev, int32_t* count_dev,
                        int32_t* status_dev, int32_t* n_quads_dev, int32_t* n_foreign_dev, int32_t* n_edges_dropped_dev,
                        double* strength_dev);

/* The compaction of clc_tag_grid_device's result for clc_board_poses_device: the corners of the tags seen (hamming >= 0), image by
 * image in id order, corners_px_dev[2 M] float32 and their board points board_xy_dev[2 M] float32 (tag_size a and tag_spacing as in
 * the reference's board file), offsets_dev[n_images + 1] int64 (rows; offsets[0] = 0, M = offsets[n_images] <= the capacity
 * n_images 4 cols rows the caller allocates).  CLC_ERR_INVALID_ARG: cols rows out of range, tag_size not finite or <= 0,
 * tag_spacing not finite or < 0, a NULL array. */
int clc_tag_grid_points_device(clc_handle* h, const float* corners_dev, const int32_t* hamming_dev, size_t n_images, int32_t cols,
                               int32_t rows, double tag_size, double tag_spacing, float* corners_px_dev, float* board_xy_dev,
                               int64_t* offsets_dev);

#ifdef __cplusplus
}
#endif
#endif /* CLC_H_ */
