/*
 * rsba.h — C ABI of the MI355X-native bundle-adjustment path (librsba.so).
 *
 * Drop-in boundary for the hot path of ajingu/RealSenseCalibration: everything that
 * Main_Calibration/bundle_adjustment.h + bundle_adjustment_manager.h hand to Ceres
 * (problem container, reprojection-error cost, Levenberg-Marquardt + DENSE_SCHUR solve, result
 * export).  Plain pointers and sizes only; no C++/torch types.  Each entry point names the
 * reference interface it replaces (paths relative to the reference repository root).
 *
 * Parameter layouts are the reference's own:
 *   point model        [C cameras x (rvec3, tvec3) | P points x xyz]
 *                      Test1_BundleAdjustment/bundle_adjustmenter.cpp:35-53
 *   marker-chain model [C cameras | T times | M markers] x (rvec3, tvec3)
 *                      Main_Calibration/bundle_adjustment.cpp:64-87
 * Solutions are written in place into the problem's parameter array, exactly as Ceres writes
 * through the raw pointers BALProblem hands out; blocks that no residual references are untouched.
 *
 * All compute runs on the GPU (gfx950).  There is no CPU fallback: every solve entry point returns
 * RSBA_ERR_NO_DEVICE when no HIP device is present.
 */
#ifndef RSBA_H_
#define RSBA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSBA_VERSION 100

/* ---- return codes (the reference exits the process instead: bundle_adjustment_manager.cpp:8-13) */
enum {
  RSBA_OK = 0,
  RSBA_ERR_IO = 1,        /* file could not be opened (BALProblem::loadFile returns false)   */
  RSBA_ERR_FORMAT = 2,    /* short or malformed file (reference: fscanfOrDie / unchecked)    */
  RSBA_ERR_ARG = 3,       /* NULL / out-of-range argument                                    */
  RSBA_ERR_HIP = 4,       /* a HIP runtime call failed                                       */
  RSBA_ERR_NO_DEVICE = 5, /* no gfx950 device visible: the product has no CPU path           */
  RSBA_ERR_COMM = 6,      /* RCCL failure                                                    */
  RSBA_ERR_UNSUPPORTED = 7,
  RSBA_ERR_RANK_DEFICIENT = 8 /* rsba_solver_covariance_compute: J'J is singular (Covariance::Compute returns false) */
};

/* ---- models */
enum {
  RSBA_MODEL_POINTS = 0,             /* ReprojectionError<2,6,3>, Test1_BundleAdjustment/bundle_adjustmenter.cpp:106-148 */
  RSBA_MODEL_MARKER_CHAIN = 1,       /* four functors + wiring of Main_Calibration/bundle_adjustment_manager.cpp:21-88  */
  RSBA_MODEL_MARKER_CHAIN_TEST2 = 2  /* two functors + wiring of Test2_BundleAdjustment/main.cpp:64-96                  */
};

/* ---- ceres::TerminationType as Summary reports it (bundle_adjustment_manager.cpp:95 FullReport) */
enum { RSBA_CONVERGENCE = 0, RSBA_NO_CONVERGENCE = 1, RSBA_FAILURE = 2 };
enum {
  RSBA_STOP_NONE = 0, RSBA_STOP_GRADIENT = 1, RSBA_STOP_PARAMETER = 2, RSBA_STOP_FUNCTION = 3,
  RSBA_STOP_MAX_ITERATIONS = 4, RSBA_STOP_MIN_RADIUS = 5, RSBA_STOP_INVALID_STEPS = 6,
  RSBA_STOP_INITIAL_FAILURE = 7, RSBA_STOP_MAX_TIME = 8
};

enum rsba_loss { RSBA_LOSS_HUBER = 0, RSBA_LOSS_CAUCHY = 1 };

typedef struct rsba_problem rsba_problem; /* BALProblem (bundle_adjustment.h:18-54) */
typedef struct rsba_solver rsba_solver;   /* device-resident state of one ceres::Solve call */

/* ceres::Solver::Options as bundle_adjustment_manager.cpp:90-92 leaves it (linear_solver_type =
 * DENSE_SCHUR, everything else Ceres 1.14 defaults), plus the knobs this implementation adds. */
typedef struct rsba_options {
  int32_t max_num_iterations;                /* 50 */
  int32_t max_num_consecutive_invalid_steps; /* 5 */
  int32_t jacobi_scaling;                    /* 1 */
  int32_t minimizer_progress_to_stdout;      /* 0 (the reference sets true, :92) */
  double initial_trust_region_radius;        /* 1e4 */
  double max_trust_region_radius;            /* 1e16 */
  double min_trust_region_radius;            /* 1e-32 */
  double min_relative_decrease;              /* 1e-3 */
  double min_lm_diagonal;                    /* 1e-6 */
  double max_lm_diagonal;                    /* 1e32 */
  double function_tolerance;                 /* 1e-6 */
  double gradient_tolerance;                 /* 1e-10 */
  double parameter_tolerance;                /* 1e-8 */
  double huber_delta;                        /* the loss function's parameter a; 0 = no loss (the reference passes NULL, :38) */
  /* --- implementation knobs --- */
  int32_t device;          /* HIP device ordinal, -1 = current                                  */
  int32_t schur_impl;      /* point model: 0 = reference kernel (global atomics), 1 = tiled (default).          */
                           /* marker-chain: 0 = dense normal equations in one workgroup, 1 = eliminate the time */
                           /* blocks when the dense system has more than 384 unknowns, 2 = always eliminate,    */
                           /* 3 = as 2, and a solver with free intrinsics (rsba_problem_set_intrinsics_free)    */
                           /* eliminates the time blocks too: its intrinsics blocks join the reduced system.    */
                           /* Without free intrinsics 3 is 2 bit for bit; on the point model 3 means "not 0"    */
  int32_t profile_kernels; /* HIP events on the solver stream (rsba_solver_kernel_stats): 1 = around every kernel,
                              2 = only around the Schur pair kernel and the reduced-system solve */
  int32_t rank;            /* multi-GPU: this process' rank, 0..world_size-1                     */
  int32_t world_size;      /* 1 = single GPU.  >1: the problem handed in is this rank's point   */
                           /* shard (all cameras, its own points); the reduced camera system is */
                           /* all-reduced over RCCL each iteration                               */
  int32_t loss_type;       /* with huber_delta = a > 0: RSBA_LOSS_HUBER (0) = ceres::HuberLoss(a),       */
                           /* RSBA_LOSS_CAUCHY (1) = ceres::CauchyLoss(a); both have rho'' <= 0, so the  */
                           /* corrector scales residual and Jacobians by sqrt(rho') (corrector.cc)      */
                           /* per residual block: a point's 2 residuals, a marker-chain observation's 8   */
                           /* (both marker-chain paths: dense and time-eliminating)                     */
  const void* comm_unique_id; /* world_size > 1: the 128-byte id from rsba_comm_unique_id (rank 0's) */
  void* stream;               /* hipStream_t to run on, NULL = a private stream                    */
  double max_solver_time_in_seconds; /* 1e9 (Ceres' default; Solver::Options, left alone by bundle_adjustment_manager.cpp:90-92): checked
                                        once per iteration IN FRONT OF the iteration limit and for the first time right behind
                                        iteration 0, against minimiser + set-up (preprocessor) time, as TrustRegionMinimizer's
                                        FinalizeIterationAndCheckIfMinimizerCanContinue does -> NO_CONVERGENCE, RSBA_STOP_MAX_TIME;
                                        a budget of 0 returns the start with no step taken.  Several ranks (round 6): RANK 0's clock decides for all of them —
                                        what it says when a step is launched is all-reduced with that step's candidate scalars, so every rank
                                        stops on the same iteration, one step behind the clock.
                                        Solver::Options::use_nonmonotonic_steps has no field: the reference leaves it false, and the
                                        device-side step decision (DecideStep) implements the monotonic rule only. */
} rsba_options;

typedef struct rsba_summary {
  int32_t termination_type; /* RSBA_CONVERGENCE / NO_CONVERGENCE / FAILURE */
  int32_t stop_reason;      /* RSBA_STOP_* */
  int32_t num_successful_steps;
  int32_t num_unsuccessful_steps;
  int32_t num_iterations; /* successful + unsuccessful, iteration 0 excluded */
  int32_t reserved;
  double initial_cost;
  double final_cost;
  double minimizer_seconds; /* wall time of the LM loop only (inputs already on the device) */
  double setup_seconds;     /* ordering + upload */
} rsba_summary;

/* one row per iteration (0 = initial evaluation), Ceres' progress table columns */
typedef struct rsba_iteration {
  int32_t iteration;
  int32_t step_is_valid;
  int32_t step_is_successful;
  int32_t linear_solver_iterations; /* ls_iter: 1 for the direct DENSE_SCHUR solve, 0 for row 0 */
  double cost, cost_change, gradient_max_norm, step_norm, relative_decrease, trust_region_radius;
  double iteration_time_in_seconds;  /* iter_time */
  double cumulative_time_in_seconds; /* total_time, since the start of the minimiser loop */
} rsba_iteration;

/* Which schedule a solver runs and what has gone wrong so far (bench.py prints it; a first run on new hardware reads it) */
typedef struct rsba_schedule_info {
  int32_t schedule;        /* 0 sequential, 1 pipelined (factorisation gated on the Schur kernel's stages), 2 pipelined multi-GPU */
  int32_t stalls;          /* steps whose in-kernel wait ran out of its budget and were repeated sequentially */
  int32_t fallbacks;       /* permanent fallbacks taken (third pipeline stall; one-workgroup / multi-launch factorisation) */
  int32_t comm_nranks;     /* ranks of the communicator (1: none) */
  int32_t chol_workgroups; /* workgroups of the reduced system's factorisation (resident tiles above 64 cameras; 33 .. 64 cameras on one rank: six + the border's) */
  int32_t schur_impl;      /* as run: 0 when a shard with duplicate observations fell back to the atomic kernel */
  char comm_kind[16];      /* "none" | "rccl" | "loopback" | "shm" */
} rsba_schedule_info;

typedef struct rsba_kernel_stat {
  char name[48];
  int64_t launches;
  double total_ms; /* HIP-event time on the solver stream, profile_kernels = 1 only */
} rsba_kernel_stat;

int rsba_version(void);
int rsba_device_count(void);
const char* rsba_error_string(int code);

/* ------------------------------------------------------------------ problem container */
/* Point model from arrays (what Test1's BALProblem::LoadFile builds, bundle_adjustmenter.cpp:55-85).
 * intrinsics: 4 doubles per camera (fx, fy, ppx, ppy) = K(0,0), K(1,1), K(0,2), K(1,2)
 * (ReprojectionError ctor, :113-120).  Arrays are copied. */
int rsba_problem_create_points(int32_t num_cameras, int32_t num_points, int64_t num_observations,
                               const int32_t* camera_index, const int32_t* point_index,
                               const double* observations /* 2 per observation */,
                               const double* parameters /* 6C + 3P */,
                               const double* intrinsics /* 4C */, rsba_problem** out);

/* Marker-chain problem from arrays (what BALProblem::loadFile, bundle_adjustment.cpp:132-187, leaves in memory): one row
 * per detected marker = residual block; observations 8 per row (4 corners x (u, v)); parameters [C | T | M] x 6
 * (rvec, tvec), camera 0 / marker 0 being the fixed base blocks of RSBA_MODEL_MARKER_CHAIN. */
int rsba_problem_create_marker_chain(int32_t model, int32_t num_cameras, int32_t num_times, int32_t num_markers,
                                     int64_t num_observations, const int32_t* time_index, const int32_t* camera_index,
                                     const int32_t* marker_index, const double* observations, const double* parameters,
                                     const double* intrinsics, double marker_side, rsba_problem** out);

/* ceres::Problem::SetParameterBlockConstant on a camera block of the point model (not used by the reference; SURVEY
 * §8f rank 4): the camera keeps its value, has no columns in the linear system and does not count in the norms of the
 * convergence tests.  Fixing one camera removes the gauge freedom of a free network. */
int rsba_problem_set_camera_constant(rsba_problem* p, int32_t camera_idx, int32_t constant);
/* ... on a POINT block (round 6): the point keeps its value, is not eliminated (no block in the Schur complement, no step), its
 * observations still count in the cost and in their cameras' blocks, and it is left out of the norms of the convergence tests —
 * Ceres removes a constant block from the program.  The tiled Schur kernel only (schur_impl != 0; rsba_solver_create returns
 * RSBA_ERR_UNSUPPORTED with the atomic kernel, also when duplicate observations select it). */
int rsba_problem_set_point_constant(rsba_problem* p, int32_t point_idx, int32_t constant);
/* ceres::Problem::SetParameterBlockConstant(values) as the reference would call it — with the block's place in the parameter array
 * (`parameter_offset` = values - parameters_: a multiple of 6 for a pose block, 6 C + 3 j for point j of the point model).  Point model: the
 * two calls above.  Marker-chain models: any camera / time / marker block of [C | T | M] (bundle_adjustment.cpp:64-87) — the
 * block keeps its transform in every residual that names it and leaves the program (no columns, no step, out of the norms and the
 * Jacobi scaling; residuals with no free block count in the cost only).  Both paths take constant blocks: the time-eliminating one
 * gives constant cameras and markers no reduced column and eliminates a constant time with E = 0; with every camera and marker
 * constant only the time blocks are solved, each on its own (rsba_solver_time_elimination tells which path a solver runs). */
int rsba_problem_set_parameter_block_constant(rsba_problem* p, int64_t parameter_offset, int32_t constant);

/* ceres::SubsetParameterization(6, constant_parameters) on a pose block of the marker-chain models: single components of a block
 * held constant.  `parameter_offset` names the block as above (a multiple of 6 inside [C | T | M]); bit q of `constant_mask` set
 * means component q of (rvec[0..2], tvec[0..2]) is constant.  Ceres 1.14's semantics:
 *   - a constant component never moves: it keeps its bits through every step, accepted or rejected, in the download and in
 *     rsba_problem_parameters; cost and residuals use its value;
 *   - it has no column in the linear system: the free components' step, their Jacobi scales, the damping, the model cost change,
 *     the gradient and gradient_max_norm are those of the program without it, for any option values (min_lm_diagonal = 0 included);
 *   - the norms of the convergence tests are ambient, as TrustRegionMinimizer's x_.norm() is: |x| counts the constant components
 *     of a partly constant block, the step norm gets 0 from them; a wholly constant block stays out as before;
 *   - a block that is also constant as a whole (rsba_problem_set_parameter_block_constant), a fixed base block (camera 0 / marker 0
 *     of the wiring) or a block no residual names: the mask is ignored.
 * A mask of 0 removes the subset.  A mask of all six bits (63; Ceres CHECK-fails: use the block call), bits above 5, a negative
 * mask, an offset that is no multiple of 6 or outside [C | T | M]: RSBA_ERR_ARG, nothing changes.  The point model:
 * RSBA_ERR_UNSUPPORTED (its camera rows sit in the headline kernels).  Host only.
 * rsba_solve and rsba_solver_create honour the masks; they are fixed at create, like constant blocks.  No mask, or only zero masks:
 * the kernels and the bits of a problem without them.  Any non-zero mask: both paths take it, together with a robust loss, weights,
 * distortion and constant blocks; the path rule (rsba_solver_time_elimination) does not read the masks.  On the time-eliminating
 * path a masked solver always runs the split elimination and the split back-substitution (the masks are applied to their small
 * products), whatever RSBA_MT_SPLIT, RSBA_MT_SPLIT_BACKSUB and RSBA_MT_BACKSUB_WG say (MarkerSwitches, csrc/ba_marker_plan.hpp).
 * Queries on such a solver: rsba_solver_evaluate writes 0.0 in the masked slots of the gradient.  rsba_solver_jacobian_structure
 * is unchanged — the block keeps its six columns — and rsba_solver_evaluate_jacobian writes exact 0.0 in the masked columns, so
 * J'r equals the gradient slot for slot.  THIS DEPARTS FROM CERES, whose CRS matrix has the block's local size (6 - k) columns.
 * rsba_solver_set_parameters takes new values for masked components too; they are held at the new values.
 * rsba_solver_covariance_compute inverts the system of the free components only (a constant component is decoupled, with a unit
 * diagonal, where the system is formed) and reports no rank deficiency because of a constant component; rsba_solver_covariance_block,
 * rsba_solver_covariance_blocks and rsba_solver_time_covariances return exact zeros in the rows and columns of constant components —
 * Ceres' lift of the local covariance through the parameterisation's Jacobian. */
int rsba_problem_set_parameter_subset_constant(rsba_problem* p, int64_t parameter_offset, int32_t constant_mask);
/* the block's mask; 0 when it has none (or the arguments name no block) */
int32_t rsba_problem_parameter_subset_constant(const rsba_problem* p, int64_t parameter_offset);

/* A Gaussian prior on a camera or marker block of the marker-chain models: what `problem.AddResidualBlock(new ceres::NormalPrior(A, b),
 * NULL, block)` does (Ceres 1.14 normal_prior.h).  `parameter_offset` names the block as above; A is 6 x 6 row-major, b is 6, in the
 * block's own coordinates (rvec, tvec).  The residual is A (x - b) with the plain difference of the six parameters (no difference on
 * SO(3)), its Jacobian is A.  Fewer than six rows are written as zero rows; A may be dense and rank deficient.
 *   - cost: the block adds 1/2 |A (x - b)|^2.  No loss applies to it, whatever huber_delta / loss_type are, and observation weights
 *     do not touch it;
 *   - linear system: J'J gets A'A on the block's diagonal 6 x 6, the gradient A'A (x - b).  The Jacobi scale of the block's columns
 *     and the clamp of the LM damping are taken from the diagonal including diag(A'A); the model cost change and the candidate's cost
 *     include the prior's six rows; gradient_max_norm, the iteration log's cost and cost_change, initial_cost and final_cost too;
 *   - the raw reprojection metric never sees a prior: rsba_reprojection_error, the second output of rsba_solver_final_costs, RMS;
 *   - a block that is constant as a whole: the prior counts in the cost only.  A partly constant block: its constant components
 *     have no column in the prior's rows either; its residual uses the held values.
 * NULL A removes the prior.  A non-finite entry, NULL b, an offset that starts no block, a fixed base block (camera 0 / marker 0 of
 * RSBA_MODEL_MARKER_CHAIN, camera 0 of _TEST2: no parameter blocks): RSBA_ERR_ARG.  A time block (the eliminated blocks) and the
 * point model: RSBA_ERR_UNSUPPORTED.  Either way nothing changes.  Host only.
 * rsba_solve and rsba_solver_create honour the priors on both paths; which blocks carry one is fixed at create.  A prior on a block no
 * observation names: RSBA_ERR_UNSUPPORTED from both (THIS DEPARTS FROM CERES, where the prior alone puts the block into the program;
 * here the column maps come from the observations).  A problem without priors runs the kernels and returns the bits it always did;
 * the path rule (rsba_solver_time_elimination) does not read priors.  A solver with priors runs the loss instances of the marker-chain
 * kernels, as one with observation weights does (rho(s) = s without a loss): they carry the cost apart from the raw sum of squares,
 * which is how a prior stays out of the reprojection metric.  The consequences:
 *   - on the time-eliminating path such a solver runs the split elimination whatever RSBA_MT_SPLIT says (k_time_eliminate takes no
 *     priors), as a solver with a robust loss does;
 *   - an iteration costs what a weights-only solver's costs, plus the prior kernels: at 8 x 5000 x 16 about 0.035 ms of loss
 *     instances and 0.01 ms of prior kernels on a 0.32 ms iteration — most of the price of a prior is the former;
 *   - rsba_solver_set_observation_weights is accepted on it (it starts from all ones), although its problem carried no weights.
 * Queries on a solver created with K priors:
 *   - rsba_solver_num_residuals is 8 N + 6 K: the prior of the k-th block in ascending parameter offset owns the residuals
 *     8 N + 6 k .. + 5 = A (x - b); the observations' keep their places.  rsba_solver_full_report counts N + K residual blocks;
 *   - rsba_solver_evaluate: cost and gradient include the priors for either value of apply_loss_function;
 *   - rsba_solver_jacobian_structure / rsba_solver_evaluate_jacobian: six more rows per prior, each holding the block's six columns
 *     with the values A[i][q]; zero entries are stored (zero rows of A, exact 0.0 in the columns of constant components); the rows
 *     of a prior on a constant block are empty.  J'r stays the gradient slot for slot;
 *   - rsba_solver_covariance_compute inverts J'J + sum A'A, so a prior can cure a rank deficiency, and every block query is answered
 *     from that inverse. */
int rsba_problem_set_block_prior(rsba_problem* p, int64_t parameter_offset, const double* A /* 36 */, const double* b /* 6 */);
/* 1 and the copies when the block has a prior, 0 otherwise; A / b may be NULL */
int rsba_problem_block_prior(const rsba_problem* p, int64_t parameter_offset, double* A, double* b);
int32_t rsba_problem_num_block_priors(const rsba_problem* p);

/* Per-observation weights on the marker-chain models: what `new ceres::ScaledLoss(loss_or_NULL, a_i, TAKE_OWNERSHIP)` around each
 * residual block's loss does (Ceres 1.14 loss_function.h, corrector.cc).  One weight a_i >= 0 per residual block (one detected
 * marker, 8 residuals), in the problem's observation order.  With s_i = |r_i|^2 over the block's 8 residuals and rho the
 * configured loss (Huber or Cauchy; rho(s) = s when huber_delta == 0):
 *   - block i contributes 1/2 a_i rho(s_i) to the cost;
 *   - rho'' <= 0 still holds, so the corrector scales the block's residuals and Jacobian rows by sqrt(a_i rho'(s_i)); gradient, Jacobi
 *     scales, J'J, model cost change and candidate cost all come from the corrected rows, as with a loss alone;
 *   - the raw sum of squares is never weighted: the RMS metric, rsba_solver_final_costs' second output, rsba_reprojection_error;
 *   - apply_loss_function = 0 (evaluate, Jacobian, covariance) ignores the weights together with the loss, as Ceres ignores the
 *     whole LossFunction.
 * A weight of 0 is legal and leaves the block's rows zero (dropping a detection without a new problem).  A free pose block all of
 * whose observations have weight 0 stays in the program — zero diagonal, damping from min_lm_diagonal, a zero step, its bits
 * unchanged, as in Ceres — and rsba_solver_covariance_compute then returns RSBA_ERR_RANK_DEFICIENT.
 * Host only; the array is copied; NULL removes the weights.  A negative or non-finite value: RSBA_ERR_ARG, nothing changes.  The point
 * model: RSBA_ERR_UNSUPPORTED.  rsba_solve and rsba_solver_create honour the problem's weights; a problem that carries weights (all
 * ones included) also makes its solvers accept rsba_solver_set_observation_weights. */
int rsba_problem_set_observation_weights(rsba_problem* p, const double* weights /* num_observations, or NULL */);
/* the problem's copy of the weights; NULL when it has none */
const double* rsba_problem_observation_weights(const rsba_problem* p);

/* Lens distortion on the marker-chain models: OpenCV's five coefficients k1 k2 p1 p2 k3, as cv::projectPoints applies a 5 x 1 distCoeffs,
 * on the corner (X, Y, Z) in the detecting camera's frame:
 *   x = X / Z, y = Y / Z, r2 = x^2 + y^2,  rad = 1 + k1 r2 + k2 r2^2 + k3 r2^3
 *   xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2),  yd = y rad + p1 (r2 + 2 y^2) + 2 p2 x y,  u = fx xd + ppx, v = fy yd + ppy
 * dist: 5 doubles per camera index in that order, indexed as the intrinsics are (the detecting camera, whether or not its pose is
 * a parameter).  Like the intrinsics they are constants of the problem (the reference hands dist_coeffs to every functor and then
 * projects without them, bundle_adjustment.h:117-118); refining them is not offered.
 * Host only; the array is copied; NULL removes the coefficients.  A non-finite value: RSBA_ERR_ARG, nothing changes.  The point model:
 * RSBA_ERR_UNSUPPORTED (its projection sits in the headline kernels).  rsba_solve, rsba_solver_create and rsba_reprojection_error honour
 * the problem's coefficients, and so does every call on a solver created from it (run, evaluate, evaluate_jacobian,
 * covariance_compute and the block queries, set_parameters); there is no solver-level setter: fixed at create, like the intrinsics.
 * Which kernels run is decided at create: no coefficients, or all exactly zero — the instances and the bits of a problem without
 * them; any non-zero coefficient — the distortion instances for the whole solver (a camera whose five are zero then agrees with
 * the pinhole form to rounding, not bit for bit).  The path (rsba_solver_time_elimination) does not depend on the coefficients.
 * OpenCV's 8 / 12 / 14-coefficient models, the fisheye model and RealSense's inverse Brown-Conrady are not offered. */
int rsba_problem_set_distortion(rsba_problem* p, const double* dist /* 5 per camera, or NULL */);
/* the problem's copy of the coefficients; NULL when it has none */
const double* rsba_problem_distortion(const rsba_problem* p);

/* Free intrinsics on the marker-chain models: the solve refines a camera's fx fy cx cy k1 k2 (in Ceres: one more parameter block of six
 * per camera handed to the functor, a SubsetParameterization holding the components that stay fixed).
 * camera_idx: the detecting camera, indexed as the intrinsics and the coefficients are, the base camera included.  free_mask: bit q set =
 * component q of (fx, fy, cx, cy, k1, k2) is refined; 0 (the default): the camera has no block, its values are constants of the
 * problem.  p1 p2 k3 always are.  The projection is the five-coefficient model of rsba_problem_set_distortion; nothing about it changes.
 * Host only.  camera_idx out of range, or bits above 5: RSBA_ERR_ARG.  The point model: RSBA_ERR_UNSUPPORTED.
 * The masks are read at rsba_solver_create / rsba_solve and fixed for that solver.  With any mask non-zero:
 *   - under schur_impl 0, 1 and 2 the solver takes the dense path (rsba_solver_time_elimination reports 0); the columns of its linear
 *     system are the pose columns in their order, then the intrinsics blocks in ascending camera index, six columns each.  Under
 *     schur_impl = 3 the time blocks are eliminated (rsba_solver_time_elimination reports 1) and the intrinsics blocks are the last
 *     blocks of the reduced system, in the same order; the limit of 8192 columns below, which guards the dense matrix, does not
 *     apply.  Where the planner refuses the problem (duplicate detections, a time too wide for the split accumulation — the
 *     intrinsics blocks of the cameras that detect in a time count in its width) the solver falls back to the dense path silently,
 *     with that path's rules.  Everything below holds on both paths.  A held
 *     component of a block is treated as a constant component of a pose block is (rsba_problem_set_parameter_subset_constant): zero
 *     rows, a zero step, its bits kept, and it counts in |x| — the parameter-tolerance test sees all six values of every block;
 *   - a non-zero mask on a camera no observation names, or (dense path) a dense system of more than 8192 columns: RSBA_ERR_UNSUPPORTED from
 *     rsba_solver_create / rsba_solve, before anything is allocated;
 *   - rsba_solve and rsba_solver_download write the refined values into the problem's intrinsics and distortion arrays (the problem
 *     gets a distortion array, zeros elsewhere, when k1 or k2 is free and it had none): rsba_reprojection_error, rsba_write_outputs
 *     and a later solver see them.  The parameter array, rsba_problem_num_parameters and every offset stay as they are;
 *   - rsba_solver_run restarts from the uploaded state, intrinsics included; the summary, the iteration log, the progress table and
 *     the full report (whose parameter counts include the blocks) work as before; so do rsba_solver_set_observation_weights and
 *     rsba_solver_set_block_prior, a robust loss, constant blocks, constant components and priors on pose blocks;
 *   - rsba_solver_evaluate, rsba_solver_evaluate_jacobian, rsba_solver_jacobian_structure, rsba_solver_covariance_compute and
 *     rsba_solver_set_parameters return RSBA_ERR_UNSUPPORTED: their outputs are indexed by parameter offset and have no place for the
 *     intrinsics blocks.  rsba_solver_set_extended_layout (below) gives them one: evaluate, set_parameters and the covariance then
 *     work; the two Jacobian calls stay refused.
 * All masks zero: the kernels and the bits of a problem on which this was never called. */
int rsba_problem_set_intrinsics_free(rsba_problem* p, int32_t camera_idx, int32_t free_mask);
/* the camera's mask; 0 when none was set */
int32_t rsba_problem_intrinsics_free(const rsba_problem* p, int32_t camera_idx);
/* the problem's intrinsics, 4 per camera (fx fy ppx ppy): the values it was created with, or a solve's refined ones */
const double* rsba_problem_intrinsics(const rsba_problem* p);

/* Test1 file "two_cam_data.txt": `C P`, P rows `cam pt u v` (one observation per point,
 * bundle_adjustmenter.cpp:62-64), C x (rvec row, tvec row), P rows xyz.  Also accepts the extended
 * first line `C P N` with N observation rows.  One intrinsics 4-vector is used for every
 * observation, as Test1_BundleAdjustment/main.cpp:73-74 does. */
int rsba_problem_load_points_file(const char* path, const double* intrinsics4, rsba_problem** out);

/* BALProblem::loadFile for correspondence.txt (bundle_adjustment.cpp:132-187).
 * model: RSBA_MODEL_MARKER_CHAIN or RSBA_MODEL_MARKER_CHAIN_TEST2; marker_side: my_const.h:9;
 * intrinsics: 4 per camera index, in SERIAL_NUMBERS order (my_const.h:15). */
int rsba_problem_load_correspondence(const char* path, int32_t model, double marker_side,
                                     const double* intrinsics /* 4C */, rsba_problem** out);

/* ------------------------------------------------------------------ initial guesses (the reference's front end)
 * What Correspondencer computes between the ArUco detections and correspondence.txt, without OpenCV.  Poses are
 * 6 doubles (rvec, tvec), p_out = R(rvec) p_in + tvec.  Host code.  The routines see pinhole pixels: detections of a lens with
 * distortion coefficients go through rsba_undistort_points first (include/rsba/correspondencer.h does); the marker-pose entries at the
 * end of this section take the coefficients themselves. */
/* correspondencer.cpp:119-127: the base marker's pose in the main camera from the detection of another marker and
 * that marker's pose in the base marker's frame (my_io GetMarkerGeometry). */
int rsba_base_pose_from_marker_detection(const double* marker_from_camera, const double* marker_from_base,
                                         double* base_from_camera);
/* correspondencer.cpp:137-147: marker i in the main camera = base pose o (marker i in the base marker's frame). */
int rsba_marker_pose_in_camera(const double* base_from_camera, const double* marker_from_base, double* marker_from_camera);
/* Correspondencer::GetCornersInCameraWorld (correspondencer.cpp:5-39): top-left, top-right, bottom-right, bottom-left. */
int rsba_marker_corners_in_camera(const double* pose, double marker_side, double* out12);
/* cv::undistortPoints(src, dst, K, dist, noArray(), K) for the five-coefficient model (k1 k2 p1 p2 k3): pixel coordinates of distorted
 * detections -> pixel coordinates of the ideal pinhole camera with the same intrinsics.  Fixed-point iteration on the normalised
 * point until the update is below 1e-14, 50 iterations at most; a point that does not converge (coefficients too strong at its
 * radius): RSBA_ERR_UNSUPPORTED.  out may be image_points.  All-zero coefficients return the input's bits.  No digit-for-digit claim
 * against OpenCV. */
int rsba_undistort_points(int32_t n, const double* image_points /* 2n */, const double* intrinsics4, const double* dist5,
                          double* out /* 2n */);
/* cv::solvePnP(object, image, K, dist = 0, rvec, tvec, false, SOLVEPNP_EPNP) as correspondencer.cpp:192-195 calls it.
 * n >= 4 points (the reference exits below 4, :185-190); RSBA_ERR_UNSUPPORTED for a coplanar point set. */
int rsba_solve_pnp_epnp(int32_t n, const double* object_points /* 3n */, const double* image_points /* 2n */,
                        const double* intrinsics4, double* pose);
/* Correspondencer::CalculateTransforms (correspondencer.cpp:178-205) on a marker-chain problem whose time and marker
 * blocks are filled: camera 0 := identity, every other camera := EPnP over the corners of all markers it detected (undistorted
 * first when the problem carries distortion coefficients). */
int rsba_problem_initial_camera_poses(rsba_problem* p);
/* aruco::estimatePoseSingleMarkers for ONE detection (correspondencer.cpp:80): the pose of a square marker of side marker_side from
 * its four image corners (u, v) in the order top-left, top-right, bottom-right, bottom-left; object points (-s/2, s/2, 0), (s/2, s/2, 0),
 * (s/2, -s/2, 0), (-s/2, -s/2, 0).  pose6 = (rvec, tvec), p_cam = R(rvec) p_marker + tvec: the local minimiser of the four corners'
 * reprojection error under the project's camera model (pinhole, or with dist5 = k1 k2 p1 p2 k3), reached by Levenberg-Marquardt from
 * the homography of the square — what SOLVEPNP_ITERATIVE does for a planar target; no digit-for-digit claim against OpenCV.  *rms: the
 * RMS of the eight residuals in pixels.  *status: 0 converged; 1 the iteration cap was reached (pose and RMS of the last iterate);
 * 2 degenerate (singular homography, non-positive depth, a non-finite intermediate, an undistortion that did not converge): pose zeros,
 * RMS -1, and the call returns RSBA_ERR_UNSUPPORTED as coplanar EPnP does.  RSBA_ERR_ARG: a null pointer, a non-finite value,
 * marker_side <= 0.  A planar target has TWO such minimisers, the pose and its mirror image about the line of sight; this entry returns
 * the one in whose basin the homography start falls — for a small or nearly frontal marker the wrong one in a quarter to a third of the
 * cases, at an RMS that does not give it away.  rsba_marker_pose_from_corners_both returns both.  Host code. */
int rsba_marker_pose_from_corners(const double* corners8, const double* intrinsics4, const double* dist5_or_null, double marker_side,
                                  double* pose6, double* rms_or_null, int32_t* status_or_null);
/* Both poses of the planar marker.  poses12 = solution 0, then solution 1; rms2 and status2 likewise.  The order is fixed, not sorted.
 *   solution 0   rsba_marker_pose_from_corners, bit for bit
 *   solution 1   exists when solution 0 has status 0 or 1: the same Levenberg-Marquardt loop started from the mirror image of solution 0,
 *                R' = (I - 2 v v') R diag(1, 1, -1), t' = t with v = t / |t| — the marker's in-plane axes reflected in the plane
 *                perpendicular to the line of sight.  (Not IPPE's closed form: a minimiser of the same reprojection error.)
 *                status 0, 1 as above; 2: no solution 0, or the mirrored start is unusable (not finite, a corner behind the camera);
 *                3 (RSBA_MARKER_POSE_SAME): the fit ended at solution 0 — no entry of the two rotation matrices or translations differs
 *                by 1e-5 — as for a close-up, where perspective leaves one minimum.  Statuses 2 and 3: pose zeros, RMS -1.
 * What is and is not resolved: both candidates are returned; WHICH is the marker's pose four corners cannot say (the two RMS values differ
 * by less than the noise for a small marker; compare them only for a large or strongly tilted one).  A block's cost over several detections
 * does say: rsba_problem_start_rig2 / _scene2 with RSBA_START_BOTH_SOLUTIONS.
 * Return codes as rsba_marker_pose_from_corners: RSBA_ERR_UNSUPPORTED only when solution 0 is degenerate.  Host code. */
#define RSBA_MARKER_POSE_SAME 3
int rsba_marker_pose_from_corners_both(const double* corners8, const double* intrinsics4, const double* dist5_or_null, double marker_side,
                                       double* poses12, double* rms2_or_null, int32_t* status2_or_null);
/* The same fit for n detections in ONE kernel launch on the GPU, one detection per thread.  camera_index selects each detection's
 * row of intrinsics (4 per camera) and of dist (5 per camera, or NULL: no distortion); device: a HIP device, -1 = the current one.
 * RSBA_ERR_NO_DEVICE without a device; n == 0 is RSBA_OK and launches nothing; n < 0, a null required pointer, a camera index outside
 * [0, num_cameras), a non-finite input or marker_side <= 0: RSBA_ERR_ARG before any device work, nothing written.  A degenerate detection
 * does not fail the call: it gets status 2 (pose zeros, RMS -1) and its neighbours are unaffected — a detection's result does not depend
 * on its place in the batch. */
int rsba_marker_poses_from_corners(int64_t n, const double* corners /* 8n */, const int32_t* camera_index /* n, or NULL = all camera 0 */,
                                   int32_t num_cameras, const double* intrinsics /* 4 per camera */, const double* dist /* 5 per camera, or NULL */,
                                   double marker_side, int32_t device /* -1 = current */, double* poses /* 6n */, double* rms /* n, or NULL */,
                                   int32_t* status /* n, or NULL */);
/* rsba_marker_pose_from_corners_both for n detections on the GPU, in TWO launches: k_marker_pose (solution 0: the bits of
 * rsba_marker_poses_from_corners), then k_marker_pose_mirror (solution 1 from solution 0), one detection per thread each.  Arguments,
 * checks in the same order and error codes as rsba_marker_poses_from_corners; detection i's results are poses[12 i .. 12 i + 11],
 * rms[2 i], rms[2 i + 1], status[2 i], status[2 i + 1].  A degenerate detection gets statuses (2, 2).  RSBA_RUNPROF=1: each launch's
 * HIP-event time on stderr. */
int rsba_marker_poses_from_corners_both(int64_t n, const double* corners /* 8n */, const int32_t* camera_index /* n, or NULL = all camera 0 */,
                                        int32_t num_cameras, const double* intrinsics /* 4 per camera */, const double* dist /* 5 per camera, or NULL */,
                                        double marker_side, int32_t device /* -1 = current */, double* poses /* 12n */, double* rms /* 2n, or NULL */,
                                        int32_t* status /* 2n, or NULL */);
/* correspondencer.cpp:100-127 on a marker-chain problem whose marker blocks are filled, the twin of rsba_problem_initial_camera_poses:
 * at every time, camera 0's detection with the lowest marker index is fitted with the problem's intrinsics (and distortion coefficients,
 * if it carries any); marker 0's pose is the base pose, another marker's goes through rsba_base_pose_from_marker_detection with the
 * problem's block of that marker; the result is written into the time block.  A time at which camera 0 detected nothing (the reference
 * leaves it uninitialised) or only degenerately keeps its bits and is counted in *num_missing_or_null.  The point model:
 * RSBA_ERR_UNSUPPORTED.  Host code. */
int rsba_problem_initial_time_poses(rsba_problem* p, int32_t* num_missing_or_null);
/* The start of a WHOLE rig from its detections, on the GPU: replaces rsba_problem_initial_time_poses + rsba_problem_initial_camera_poses
 * where camera 0 does not see every shot.  Marker blocks are inputs (the board geometry), as for those two; rsba_problem_start_scene
 * below fits them too.
 *   block resection   one pose block (a time or a camera) is fitted to ALL the detections that name it, the other two blocks of each
 *                     detection held: the minimiser of their marker-chain reprojection cost (8 residuals each, through the model's functors,
 *                     base blocks the identity, the problem's distortion coefficients applied) — ceres::Solve with every other block
 *                     constant.  Levenberg-Marquardt with the rules of rsba_marker_pose_from_corners and one more — a step must realise a
 *                     quarter of the decrease its damped model predicts, or the damping is raised — from the best of up to four candidate
 *                     poses: the own fits (that entry's) of the block's detections with the lowest RMS, composed with their known blocks, the
 *                     block cost evaluated at each.  A second detection so resolves the planar ambiguity of the first — when its own fit
 *                     fell into the right basin.  A block whose detections all fell into the wrong one, or that has a single detection,
 *                     starts mirrored: rsba_problem_start_rig2 with RSBA_START_BOTH_SOLUTIONS puts both poses of each candidate detection
 *                     on the list.
 *   propagation       from the known blocks — those flagged in known_blocks (C cameras, then T times), the base camera always — round 0 fits
 *                     every unknown time some known camera detected, the next round every unknown camera that detected a known time, and so on
 *                     in turns until nothing is added.  A detection counts for a block only when its other block (the camera of a time's
 *                     detection, the time of a camera's) is known.  Then refine_sweeps passes: all fitted times, then all fitted cameras, each
 *                     from its value with every usable detection.  1 is recommended: a block fitted in an early round saw only the
 *                     neighbours known then; further sweeps are block coordinate descent, which rsba_solve does better.  0 = the rounds alone.
 * Blocks flagged in known_blocks keep their bits (new shots on a calibrated rig: flag the cameras; new cameras on solved shots: the times).
 * block_status (C + T): 0 converged; 1 the iteration cap was reached (the last iterate); 2 degenerate — usable detections but no start with
 * a finite cost and every corner in front — the block keeps its bits; 3 unreached — no usable detection — the block keeps its bits; 4 given,
 * or the base camera.  block_rms: the RMS of the block's usable residuals in pixels at its last fit, -1 for statuses 2 to 4.  The counters
 * count the blocks with status 2 or 3.  A block's result does not depend on its place in a launch and is bit-identical between calls.
 * Observation weights, constant blocks, subset masks and priors of the problem play no part.
 * RSBA_ERR_ARG (before any device work, nothing written): a null problem, refine_sweeps < 0, device < -1 or >= the device count;
 * RSBA_ERR_UNSUPPORTED: the point model; RSBA_ERR_NO_DEVICE without a device.  RSBA_RUNPROF=1: each launch's HIP-event time on stderr. */
int rsba_problem_start_rig(rsba_problem* p, const uint8_t* known_blocks /* C + T, or NULL: only the base camera */,
                           int32_t refine_sweeps, int32_t device /* -1 = current */,
                           int32_t* num_missing_times, int32_t* num_missing_cameras,
                           int32_t* block_status /* C + T, or NULL */,
                           double* block_rms /* C + T, or NULL */);
/* rsba_problem_start_rig with flags.  flags = 0 IS rsba_problem_start_rig (that entry calls this one: the same host path, the same kernel
 * instances, the same bits).  RSBA_START_BOTH_SOLUTIONS: k_marker_pose_mirror runs once after the own fits, and a block that is not yet
 * known takes its start from up to EIGHT candidates — the same up-to-four detections in the same (solution-0 RMS, observation index) order,
 * each contributing its solution 0 and then, where it has status 0 or 1, its solution 1 (rsba_marker_pose_from_corners_both), the lowest
 * block cost taken, the earlier candidate on a tie.  The unflagged list is contained in the flagged one in the same order, so the chosen
 * start's block cost is never higher with the flag.  What that resolves: a time, camera or marker block whose own fits are all mirrored,
 * provided the block's cost tells the two apart (two detections, or one beside known neighbours).  What it does not: a WHOLE board that
 * is mirrored consistently, which is a true local minimum of the scene; a block with one detection of one marker, where
 * both candidates cost almost the same and the lower one wins by noise.  Refits, sweeps, statuses and RMS are unchanged.  The flagged
 * launches are kernel instances of their own.  Any other bit of flags: RSBA_ERR_ARG before any device work. */
#define RSBA_START_BOTH_SOLUTIONS 1u
int rsba_problem_start_rig2(rsba_problem* p, const uint8_t* known_blocks /* C + T, or NULL: only the base camera */,
                            int32_t refine_sweeps, int32_t device /* -1 = current */, uint32_t flags,
                            int32_t* num_missing_times, int32_t* num_missing_cameras,
                            int32_t* block_status /* C + T, or NULL */,
                            double* block_rms /* C + T, or NULL */);
/* rsba_problem_start_rig for a scene whose board geometry nobody measured (markers on a wall, a floor, a folded board): the marker blocks
 * are a third kind of block to be fitted, by the same block resection.
 *   a marker's fit    the points entering the fitted transform are the raw corners (+-half, +-half, 0), the known transform behind it is
 *                     camera o time (the time alone for the base camera); a candidate is the detection's own fit D = camera o time o marker
 *                     solved for the marker.  A marker is a block per 256-lane workgroup, as a camera.
 *   propagation       known_blocks flags C cameras, T times, then M markers; the base camera is always known, and so is marker 0 of
 *                     RSBA_MODEL_MARKER_CHAIN (the base marker, the identity; it gets status 4).  In RSBA_MODEL_MARKER_CHAIN_TEST2 marker 0
 *                     is an ordinary block, known only if flagged — with nothing flagged that model has no gauge and nothing is reached.
 *                     A detection counts for a block only when BOTH its other blocks are known.  Rounds go time, marker, camera in turn; a
 *                     round that would fit nothing is not launched, three empty rounds in a row end the propagation.  Then refine_sweeps
 *                     passes: all fitted times, then markers, then cameras.  With every marker flagged the call launches and computes
 *                     what rsba_problem_start_rig does, bit for bit.
 * The gauge is the base camera's frame and, at every time, the base marker's: a scene in which the base camera never sees the base marker
 * (or a flagged one) has no first round, and every block comes back unreached.  A planar board seen by few cameras has a mirrored pose
 * that is a true local minimum of the whole problem; the candidates' block cost resolves it where a block has enough detections, not
 * always; rsba_problem_start_scene2's RSBA_START_BOTH_SOLUTIONS widens the candidates, and does not promise it either.  Statuses, RMS, errors and RSBA_RUNPROF as for rsba_problem_start_rig, over C + T + M blocks. */
int rsba_problem_start_scene(rsba_problem* p, const uint8_t* known_blocks /* C + T + M, or NULL */,
                             int32_t refine_sweeps, int32_t device /* -1 = current */,
                             int32_t* num_missing_times, int32_t* num_missing_cameras, int32_t* num_missing_markers,
                             int32_t* block_status /* C + T + M, or NULL */,
                             double* block_rms /* C + T + M, or NULL */);
/* rsba_problem_start_scene with flags, as rsba_problem_start_rig2 is to rsba_problem_start_rig: 0 is that entry bit for bit,
 * RSBA_START_BOTH_SOLUTIONS widens the candidates of time, marker and camera blocks alike, any other bit is RSBA_ERR_ARG. */
int rsba_problem_start_scene2(rsba_problem* p, const uint8_t* known_blocks /* C + T + M, or NULL */,
                              int32_t refine_sweeps, int32_t device /* -1 = current */, uint32_t flags,
                              int32_t* num_missing_times, int32_t* num_missing_cameras, int32_t* num_missing_markers,
                              int32_t* block_status /* C + T + M, or NULL */,
                              double* block_rms /* C + T + M, or NULL */);

void rsba_problem_free(rsba_problem* p);

/* BALProblem accessors (bundle_adjustment.h:36-53) */
int32_t rsba_problem_model(const rsba_problem* p);
int32_t rsba_problem_num_cameras(const rsba_problem* p);
int32_t rsba_problem_num_points(const rsba_problem* p);  /* point model; 0 otherwise */
int32_t rsba_problem_num_times(const rsba_problem* p);   /* marker-chain; 0 otherwise */
int32_t rsba_problem_num_markers(const rsba_problem* p); /* marker-chain; 0 otherwise */
int64_t rsba_problem_num_observations(const rsba_problem* p);
int64_t rsba_problem_num_parameters(const rsba_problem* p);
/* count x 4 corners, as BALProblem::num_observations_per_time_camera returns (bundle_adjustment.cpp:29-32) */
int32_t rsba_problem_num_observations_per_time_camera(const rsba_problem* p, int32_t time_idx, int32_t camera_idx);
const double* rsba_problem_observations(const rsba_problem* p);
double* rsba_problem_parameters(rsba_problem* p); /* mutable: results land here */
int32_t rsba_problem_camera_idx(const rsba_problem* p, int64_t observation);
int32_t rsba_problem_point_idx(const rsba_problem* p, int64_t observation);  /* point model */
int32_t rsba_problem_time_idx(const rsba_problem* p, int64_t observation);   /* marker-chain */
int32_t rsba_problem_marker_idx(const rsba_problem* p, int64_t observation); /* marker-chain */
double* rsba_problem_camera_parameters(rsba_problem* p, int32_t camera_idx);
double* rsba_problem_marker_transform(rsba_problem* p, int32_t marker_idx);
/* BALProblem::getPoint3dCoordinates (bundle_adjustment.cpp:89-130): 4 corners x xyz per observation */
int rsba_problem_point3d_coordinates(const rsba_problem* p, double* out /* 12 per observation */);

/* ------------------------------------------------------------------ solve */
void rsba_options_default(rsba_options* o);

/* BAManager::StartBA / ceres::Solve (bundle_adjustment_manager.cpp:16-96; Test1 main.cpp:63-87):
 * upload, minimise on the GPU, write the solution back into the problem's parameter array. */
int rsba_solve(rsba_problem* p, const rsba_options* o, rsba_summary* summary);

/* The same in three steps, so a caller (bench.py) can time the minimiser with inputs resident in HBM. */
int rsba_solver_create(rsba_problem* p, const rsba_options* o, rsba_solver** out);
int rsba_solver_run(rsba_solver* s, rsba_summary* summary); /* LM loop; restarts from the uploaded state */
int rsba_solver_download(rsba_solver* s);                    /* device state -> problem parameters */
/* ceres::Solve takes its Solver::Options per call (bundle_adjustment_manager.cpp:90-94): the next rsba_solver_run of this
 * solver stops after max_num_iterations and records kernel times as profile_kernels says (rsba_options); the kernel
 * statistics collected so far are dropped.  bench.py warms a solver up with W iterations, then times K on the same one. */
int rsba_solver_configure_run(rsba_solver* s, int32_t max_num_iterations, int32_t profile_kernels);
int rsba_solver_iterations(const rsba_solver* s, rsba_iteration* out, int32_t capacity); /* rows written */
int rsba_solver_kernel_stats(const rsba_solver* s, rsba_kernel_stat* out, int32_t capacity);
/* final 1/2 sum rho and sum of squared raw residuals of the last run (all ranks' total) */
/* Summary::FullReport() of the latest run (the reference prints it, bundle_adjustment_manager.cpp:95): problem sizes,
 * costs, iteration counts, times and the termination message.  snprintf semantics: returns the length needed. */
int rsba_solver_full_report(const rsba_solver* s, char* buf, int32_t capacity);
int rsba_solver_final_costs(const rsba_solver* s, double* cost, double* sum_sq_residuals);
void rsba_solver_destroy(rsba_solver* s);

/* ------------------------------------------------------------------ covariance of the solution (ceres::Covariance)
 * Not used by the reference; how well the solve determined each block.  The result is (J'J)^-1 of the unscaled parameters,
 * J evaluated at the solver's current device parameters (after rsba_solver_run: the solution; before it: the uploaded start),
 * with no sigma^2 factor and no LM damping, as Covariance::Compute gives it.  Blocks are named by their parameter offsets
 * (the convention of rsba_problem_set_parameter_block_constant).  A constant block has a zero covariance; a block no residual
 * references is RSBA_ERR_ARG.  The solver's trust radius, scales, iteration log, parameters and schedule are left untouched.
 *
 * Two queries.  rsba_solver_covariance_blocks is the GENERAL one, Covariance::GetCovarianceBlock for any pair: on the point model
 * any two of the camera and point blocks (camera x point is 6 x 3, point x point' 3 x 3), on the marker-chain models any two of the
 * camera, time and marker blocks, on the dense and the time-eliminating path alike (the eliminated time blocks and the points are
 * back-substituted into S^-1 on the GPU); rsba_solver_time_covariances is the bulk form of the time marginals, the twin of
 * rsba_solver_point_covariances.  rsba_solver_covariance_block is the older single-pair call and keeps its narrower contract: on
 * the point model every camera x camera block (6 x 6) and the 3 x 3 marginal of every point, camera x point and cross-point blocks
 * are RSBA_ERR_UNSUPPORTED; on the marker-chain models every camera / marker x camera / marker block (6 x 6), time blocks are
 * RSBA_ERR_UNSUPPORTED.  apply_loss_function applies the solve's corrector in both models (the marker chain: sqrt(rho') of each
 * observation's 8 residuals).
 *
 * The state a result belongs to: the parameters at rsba_solver_covariance_compute.  A result survives rsba_solver_run, and every
 * query after compute -> run still describes the state at compute — the general queries re-linearise from a snapshot that the
 * compute keeps on the device (the marker chain's pose constants, rows, observations and weights; the point model's camera
 * constants and a copy of its points), never from the live parameters.  rsba_solver_set_parameters and
 * rsba_solver_set_observation_weights drop the result.
 *
 * A solver with a communicator (point model; world_size > 1, or the one-rank communicator of RSBA_FORCE_COMM):
 * rsba_solver_covariance_compute is COLLECTIVE (the collective contract below).  Every rank linearises its shard into its part of
 * U - sum W V^-1 W' over one column map — the free cameras SOME rank references, from all-reduced flags, so the layout is the
 * same everywhere —, the upper triangles are summed over the ranks in one all-reduce (with them the shards' rank-deficient point
 * flags: a positive total is RSBA_ERR_RANK_DEFICIENT on every rank), every rank inverts the identical sum (so the pivot test fires
 * identically everywhere) and forms the marginals of its own points against it.  The block queries are local: camera x camera
 * blocks on every rank (a camera another shard alone observes included), bit-identical across the ranks of a loopback or
 * shared-memory group; point blocks on the owning rank, by that rank's offsets.  The constant flags of the cameras must be the
 * same on every rank, as for the solve. */
typedef struct rsba_covariance_options { /* ceres::Covariance::Options, Ceres 1.14 defaults */
  double min_reciprocal_condition_number; /* 1e-14: a Cholesky pivot of the Jacobi-scaled reduced system (or of a point block)
                                             at or below this -> RSBA_ERR_RANK_DEFICIENT */
  int32_t apply_loss_function;            /* 1: J through the solve's loss corrector (sqrt(rho') scaling) */
  int32_t reserved;
} rsba_covariance_options;

void rsba_covariance_options_default(rsba_covariance_options* o);
/* Linearise at the current parameters, invert the reduced camera system and form the point marginals on the GPU (o: NULL =
 * defaults).  RSBA_ERR_RANK_DEFICIENT leaves no result: the block queries then return RSBA_ERR_ARG. */
int rsba_solver_covariance_compute(rsba_solver* s, const rsba_covariance_options* o);
/* Covariance block of the blocks at parameter offsets a and b: na x nb, row-major.  block(b, a) is block(a, b)' exactly.  Time
 * blocks, camera x point and cross-point pairs are RSBA_ERR_UNSUPPORTED here: rsba_solver_covariance_blocks is the general call. */
int rsba_solver_covariance_block(const rsba_solver* s, int64_t offset_a, int64_t offset_b, double* out);
/* Point model: P x 3 x 3 marginals in the problem's point order (zeros for constant and unreferenced points); RSBA_ERR_UNSUPPORTED otherwise. */
int rsba_solver_point_covariances(const rsba_solver* s, double* out);
/* Covariance::GetCovarianceBlock for ANY pairs, in one call.  Pair i = blocks at parameter offsets a[i], b[i] (the convention of
 * rsba_solver_covariance_block); its na x nb block, row-major, in out[36 i .. 36 i + na nb), the rest of the 36 set to 0.0.
 * Marker-chain models: any two of camera, time and marker blocks; point model: any two of camera and point blocks.  A pair that
 * names a constant block gives zeros.  An offset that starts no block or names a block no residual references (the fixed base
 * blocks included) is RSBA_ERR_ARG for the whole call, and nothing is written; so are NULL arguments, num_pairs < 0 and a solver
 * without a valid result (no compute yet, a failed one, or a result dropped by set_parameters / set_observation_weights).
 * num_pairs == 0 is RSBA_OK and launches nothing.  A pair that rsba_solver_covariance_block answers gives the same bits here;
 * blocks(b, a) is blocks(a, b)' exactly for every kind of pair (one orientation is computed, the other transposed on output), and
 * two calls after one compute return identical bits.  Nothing the solve, evaluate or the Jacobian reads is written.  RSBA_ERR_UNSUPPORTED:
 * a time of a marker-chain problem touches more than 170 camera / marker blocks.  On a sharded solver the call is LOCAL (no
 * collective): camera offsets are valid on every rank, point offsets are this rank's own. */
int rsba_solver_covariance_blocks(rsba_solver* s, int64_t num_pairs, const int64_t* offsets_a, const int64_t* offsets_b, double* out);
/* Marker-chain models: T x 6 x 6 marginals of the time blocks in the problem's time order (zeros for constant and unreferenced
 * times); RSBA_ERR_UNSUPPORTED on the point model — the twin of rsba_solver_point_covariances.  Formed by the first call after a
 * compute and kept until the result is dropped; the (t, t) blocks of rsba_solver_covariance_blocks bit for bit.  RSBA_ERR_ARG
 * without a valid result. */
int rsba_solver_time_covariances(rsba_solver* s, double* out);

/* ------------------------------------------------------------------ evaluate and re-solve (ceres::Problem::Evaluate; values changed in place)
 * Not used by the reference, which looks at its residuals by eye (ReprojectionCheck::Reproject draws every reprojected corner beside its
 * detection, reprojection_check.cpp:68-88).  rsba_solver_evaluate is Problem::Evaluate's cost, residuals and gradient, at the solver's current
 * device parameters — after rsba_solver_run: the solution; before it: the uploaded start, or what rsba_solver_set_parameters set.
 * Any output may be NULL (all three: RSBA_OK, nothing is launched).
 *   residuals  rsba_solver_num_residuals doubles in the PROBLEM's observation order (the arrays given to rsba_problem_create_*, the rows
 *              of the loaded file): observation i owns [2i, 2i+1] = (u, v) on the point model, [8i .. 8i+7] = 4 corners x (u, v), top-left,
 *              top-right, bottom-right, bottom-left, on the marker-chain models; projected minus detected.  With apply_loss_function and a
 *              loss configured (rsba_options.huber_delta > 0) every residual block is multiplied by sqrt(rho'(s)), s its squared norm — the
 *              corrector the solve applies; raw otherwise.
 *   cost       1/2 sum rho(s_i) with the loss applied, 1/2 sum s_i without, over EVERY residual block (those all of whose parameter
 *              blocks are constant included).
 *   gradient   rsba_problem_num_parameters doubles in the problem's parameter layout: J'r of the (corrected) residuals, unscaled (no
 *              Jacobi scale, no damping).  Exactly 0.0 in the slots of constant blocks, of blocks no residual references and of the fixed
 *              base blocks of the marker-chain models (camera 0 and marker 0 of RSBA_MODEL_MARKER_CHAIN, camera 0 of _TEST2): Ceres'
 *              ProgramEvaluator leaves such blocks out in the same way.
 * The solver's parameters, scales, kept linearisation, iteration log, schedule and covariance result are left untouched: run ->
 * evaluate -> run gives the bits of run -> run, and two consecutive calls return the same bits in every output (every sum is taken in a
 * fixed order).  Scratch is kept by the solver and only grows.  The Jacobian, Problem::Evaluate's fourth output, has entry points of its
 * own below (rsba_solver_jacobian_structure, rsba_solver_evaluate_jacobian): the solve never forms it in memory.
 *
 * A solver with a communicator (point model): a call with cost or gradient non-NULL is COLLECTIVE (the contract below); one that
 * asks for residuals alone is local and issues no collective.
 *   residuals  this rank's shard, in this rank's problem's observation order.
 *   cost       the all-ranks total: each rank's cost as above, then one sum over the ranks.
 *   gradient   rsba_problem_num_parameters doubles of THIS rank's problem.  The point slots are this rank's own.  The 6C camera
 *              slots are the all-ranks sum of the shards' sums; cost, camera slots and the cameras' "referenced" flags travel in one
 *              group of all-reduces (6C + 1 + C doubles).  A camera slot is exactly 0.0 when the camera is constant or NO rank
 *              references it — the mask comes from the summed flags: a camera this shard never observes but another does carries
 *              the other ranks' sum.
 * On loopback and shared-memory groups the partials are added in rank order: two consecutive calls return identical bits on every
 * rank, and cost and camera slots are bit-identical across the ranks.  Over RCCL cost and camera slots are identical across the ranks
 * as well (one all-reduce result) and repeatable as far as RCCL's choice of algorithm is.
 *
 * THE COLLECTIVE CONTRACT of rsba_solver_evaluate (cost or gradient asked for), rsba_solver_set_parameters and
 * rsba_solver_covariance_compute on a solver with a communicator.  Every rank of the group calls the entry point, in the same order
 * relative to its other collective calls (rsba_solver_run included); the call takes the device as rsba_solver_run does (a loopback
 * rank launches on its turn only).  rsba_solver_covariance_block and rsba_solver_point_covariances are local.  Each collective call
 * opens with one small all-reduce, the request word: which entry point, which of cost / gradient are wanted, apply_loss_function,
 * min_reciprocal_condition_number, and a "bad" flag for an argument error only one rank can see (a NULL pointer or a non-finite
 * value in rsba_solver_set_parameters, a negative min_reciprocal_condition_number).  Every value travels beside its negation under
 * one max, so disagreement is detected on EVERY rank: all ranks then return RSBA_ERR_ARG, nothing has changed on any of them and no
 * further collective is issued (the next matching call succeeds).  A HIP error or a failed collective aborts the communicator
 * before it returns, as rsba_solver_create does: the other ranks leave their waits with RSBA_ERR_COMM.  No path returns early on
 * one rank while the others enter a collective.  A solver WITHOUT a communicator runs none of this. */
typedef struct rsba_evaluate_options { /* ceres::Problem::EvaluateOptions */
  int32_t apply_loss_function;         /* 1 */
  int32_t reserved;
} rsba_evaluate_options;

void rsba_evaluate_options_default(rsba_evaluate_options* o);
/* 2 N (point model), 8 N (marker-chain models); for a NULL solver the negative code -RSBA_ERR_ARG, which is no count. */
int64_t rsba_solver_num_residuals(const rsba_solver* s);
int rsba_solver_evaluate(rsba_solver* s, const rsba_evaluate_options* o /* NULL = defaults */, double* cost, double* residuals, double* gradient);
/* The Jacobian of the residual vector rsba_solver_evaluate returns, at the same parameters, in compressed-row form (ceres::CRSMatrix):
 * row r's entries are cols[row_ptr[r] .. row_ptr[r + 1]) and the values at the same positions.
 *   rows     rsba_solver_num_residuals, in the problem's observation order: observation i owns rows 2i, 2i+1 (point model) or
 *            8i .. 8i+7 (marker-chain models; the corner order of the residuals).
 *   columns  rsba_problem_num_parameters, in the problem's parameter layout: column index = parameter offset, the convention of the
 *            gradient and of rsba_problem_set_parameter_block_constant.  THIS DEPARTS FROM CERES, which renumbers the columns after
 *            dropping the constant blocks; it is chosen so that J'r is the gradient rsba_solver_evaluate returns, slot for slot.
 *   nonzeros a row holds all 6 (or 3) columns of every parameter block its observation names as a parameter and that is free, by
 *            the constant flags the solver took at create: camera then point; camera, time, marker — ascending columns.  Constant
 *            blocks and the fixed base blocks of the marker-chain models (no parameters of any functor) are left out, not stored as
 *            zeros: a row whose blocks are all constant is empty.  An entry that happens to be 0.0 is still stored; duplicate
 *            observations give duplicate rows; the columns of unreferenced blocks have no entries.
 *   values   with apply_loss_function and a loss configured the rows of a residual block are multiplied by sqrt(rho'(s)) of that
 *            block, the corrector the solve and the residual output apply; raw otherwise.  No Jacobi scale, no damping.
 * rsba_solver_jacobian_structure: any output may be NULL (ask for the three counts, then for the arrays: row_ptr num_rows + 1,
 * cols num_nonzeros).  The structure depends on the index arrays and the constant flags at create alone — the same before and after
 * a run — and nothing is launched on the device.  rsba_solver_evaluate_jacobian writes num_nonzeros values in the structure's order.
 * Nothing of the solver's state is written (run -> jacobian -> run gives the bits of run -> run), and no sum is taken anywhere: two
 * calls return identical bits, and a dense-path and a time-eliminating marker-chain solver agree bit for bit at the same parameters.
 * Errors, before any device work: NULL solver or NULL values RSBA_ERR_ARG; more than INT32_MAX parameters or observations
 * RSBA_ERR_UNSUPPORTED.
 * A solver with a communicator (point model): both calls are LOCAL and issue no collective, like a residuals-only evaluate.  The
 * matrix is that of this rank's problem: its shard's observations, the shared cameras, then its own points. */
int rsba_solver_jacobian_structure(rsba_solver* s, int64_t* num_rows, int64_t* num_cols, int64_t* num_nonzeros,
                                   int64_t* row_ptr /* num_rows + 1, or NULL */, int32_t* cols /* num_nonzeros, or NULL */);
int rsba_solver_evaluate_jacobian(rsba_solver* s, const rsba_evaluate_options* o /* NULL = defaults */, double* values /* num_nonzeros */);
/* Ceres keeps the values in the caller's arrays: change them and Solve again, the Problem is not rebuilt.  Here: rsba_problem_num_parameters
 * new values into the solver's start state (what rsba_solver_run restarts from), which also become the current state that
 * rsba_solver_evaluate, rsba_solver_covariance_compute and rsba_solver_download read.  Nothing is planned or allocated again — the
 * plan depends on the index arrays alone.  Constant and unreferenced blocks take the new values too (constant during a solve, not
 * immutable).  The problem's own parameter array is not touched until rsba_solver_download; a covariance result is dropped (block
 * queries: RSBA_ERR_ARG until the next compute); the iteration log and last summary stay until the next run.  A non-finite value:
 * RSBA_ERR_ARG, nothing changes.
 *
 * A solver with a communicator (point model): COLLECTIVE (the contract above).  Each rank passes its own problem's layout — the
 * shared cameras, then its own points.  Behind the request word the ranks verify that all of them passed the same camera blocks
 * (one max over [cameras, -cameras], 12C doubles, compared as values); a mismatch is RSBA_ERR_ARG on every rank with nothing
 * changed.  A sharded group set to x1 then runs the bits of a group created at x1. */
int rsba_solver_set_parameters(rsba_solver* s, const double* parameters);

/* The extended layout of a marker-chain solver with free intrinsics (rsba_problem_set_intrinsics_free), on either of its paths: the
 * solver's own state layout — the problem's num_parameters pose values, then six values fx fy cx cy k1 k2 per camera index, camera k
 * at offset num_parameters + 6 k.  EVERY camera index has a slot, with a mask or without.  rsba_solver_num_extended_parameters is
 * its length, num_parameters + 6 num_cameras (num_parameters on the point model, which has no such slots); NULL: -RSBA_ERR_ARG.
 * on = 0 (the default): every query behaves as described at rsba_problem_set_intrinsics_free, refusals included.  The point model,
 * and a marker-chain solver without free intrinsics (its intrinsics are constants of the problem with no state slot):
 * RSBA_ERR_UNSUPPORTED.  Switching it, in either direction, drops a covariance result as rsba_solver_set_parameters does and
 * changes nothing else: a run's bits are the same.  With on != 0:
 *   - rsba_solver_evaluate: residuals and cost by the rules above (the problem's observation order, loss and weights under
 *     apply_loss_function, prior residuals behind the observations'), evaluated with the STATE's fx fy cx cy k1 k2; p1 p2 k3 stay the
 *     problem's.  The gradient has rsba_solver_num_extended_parameters entries: the pose slots as on any solver, an intrinsics slot
 *     J'r of that component's column, and 0.0 for a held component (mask bit clear), a camera with mask 0 and a camera no observation
 *     names.  The dense and the time-eliminating path return identical bits at identical values; two calls return identical bits.
 *   - rsba_solver_set_parameters takes rsba_solver_num_extended_parameters values.  All 6 num_cameras trailing values go into the
 *     start state and the current state: a held component or a camera with mask 0 is a constant whose value the caller may change.
 *     A solver created at x0 and set to x1 then runs the bits of a solver created from a problem whose parameters, intrinsics and
 *     k1 k2 are x1.  rsba_solver_download writes the state's six values of EVERY camera into the problem's intrinsics and distortion
 *     arrays — the refined ones and the held or mask-0 ones this call changed — so that the problem is consistent with the poses
 *     it gets (without this call those keep their bits: the state started from them; a problem without a distortion array gets one
 *     when k1 or k2 is free or was set to a non-zero value).
 *   - rsba_solver_covariance_compute works on both paths: an intrinsics block with a mask is one more block with six columns in the
 *     system, behind the pose blocks' (time-eliminating path: the time blocks are eliminated over camera, marker and intrinsics
 *     blocks).  rsba_solver_covariance_block and rsba_solver_covariance_blocks take num_parameters + 6 k as the offset of camera k's
 *     block: any pair among camera, marker and intrinsics blocks is a 6 x 6 block of the inverse; a camera with mask 0 gives zeros, a
 *     held component zero rows and columns (a constant component, as of a pose block); a camera no observation names: RSBA_ERR_ARG.
 *     Pairs with time blocks and rsba_solver_time_covariances work on the dense path; on the time-eliminating path of such a solver
 *     they return RSBA_ERR_UNSUPPORTED (the cross-block kernel does not know the intrinsics blocks yet).  An unobservable intrinsic
 *     is RSBA_ERR_RANK_DEFICIENT, as any singular system.
 *   - rsba_solver_jacobian_structure and rsba_solver_evaluate_jacobian: RSBA_ERR_UNSUPPORTED, as with the layout off. */
int rsba_solver_set_extended_layout(rsba_solver* s, int32_t on);
int64_t rsba_solver_num_extended_parameters(const rsba_solver* s);
/* New observation weights (rsba_problem_set_observation_weights: semantics and validation) on a resident marker-chain solver, the way
 * rsba_solver_set_parameters changes values: they take effect with the next run, evaluate, Jacobian or covariance call.  Nothing is
 * planned or allocated again; parameters, iteration log and last summary stay; a covariance result is dropped.  The problem's own copy
 * is not touched.  The intended loop: solve with Huber, evaluate raw residuals (apply_loss_function = 0), set the offenders' weights
 * to 0, run again on the same solver.
 * Which solvers take weights is decided once, at create, with the kernels the solver runs: those created with a robust loss
 * (huber_delta > 0; they start from all ones) and those whose problem carried weights at create (all ones counts: that is how a
 * caller asks for the capability without a loss).  Such a solver runs the loss instances of the marker-chain kernels, with every
 * consequence the robust loss has for the path (rsba_solver_time_elimination keeps reporting it).  Any other marker-chain solver, and
 * every point-model solver: RSBA_ERR_UNSUPPORTED, nothing changes.  NULL weights, a negative or non-finite value: RSBA_ERR_ARG, nothing
 * changes. */
int rsba_solver_set_observation_weights(rsba_solver* s, const double* weights /* num_observations */);

/* New (A, b) for a block that had a prior when the solver was created: takes effect with the next run, nothing is planned or allocated
 * again, parameters and iteration log stay, a covariance result is dropped.  The problem's own copy is not touched.  A block without a
 * prior at create, a solver without priors, the point model: RSBA_ERR_UNSUPPORTED.  NULL or a non-finite value: RSBA_ERR_ARG.  Either
 * way nothing changes. */
int rsba_solver_set_block_prior(rsba_solver* s, int64_t parameter_offset, const double* A /* 36 */, const double* b /* 6 */);

/* Stage-level entry (tests): one linearisation of the point model at the current parameters with a
 * given trust-region radius.  Any output may be NULL.
 *   S       (6C)^2 reduced camera matrix, Jacobi-scaled, LM-damped, full symmetric, row-major
 *   rhs     6C
 *   delta   6C + 3P: the LM step in parameter space (x_candidate - x)
 *   scalars [0] cost at x, [1] model cost change, [2] max|gradient|, [3] 1 if the Cholesky succeeded,
 *           [4] cost at x + delta, [5] |delta|, [6] |x| */
int rsba_points_linearize_and_step(rsba_problem* p, const rsba_options* o, double radius, double* S,
                                   double* rhs, double* delta, double* scalars /* 8 */);

/* Stage-level entry (tests): the first step rsba_solver_run would take on this problem, with these options and the RSBA_*
 * environment — its schedule, factorisation and back-substitution — at the given radius.  Any output may be NULL.
 *   S, rhs    as in rsba_points_linearize_and_step, formed again after the step from the reduced system the factorisation read
 *   dcam      6C: the camera step as the kernels wrote it (= -scale_c * y, y the solution of S y = rhs)
 *   scale_c   6C: the Jacobi scale of the step
 *   delta     6C + 3P: x_candidate - x
 *   scalars   [0..7] as in rsba_points_linearize_and_step, [7] the candidate's sum of squares;
 *             [8] 1 pipelined schedule, 0 sequential; [9] factorisation: 0 one workgroup, 1 diagonal chain, 2 diagonal chain +
 *             border, 3 persistent tiles at 64 cameras or fewer (RSBA_TILES_SMALL), 4 persistent tiles, 5 one launch per panel;
 *             [10] its workgroups (5: of the first panel's launch); [11] the border's first column (2 only); [12] resident tiles; [13] back-substitution:
 *             0 inside the factorisation, 1 one workgroup, 2 block owners, 3 chain with helpers; [14] 1: the tiles built the
 *             system themselves; [15] stalls during the step; [16] fallbacks taken */
#define RSBA_SOLVE_STAGE_SCALARS 17
int rsba_points_solve_stage(rsba_problem* p, const rsba_options* o, double radius, double* S, double* rhs, double* dcam,
                            double* scale_c, double* delta, double* scalars /* RSBA_SOLVE_STAGE_SCALARS */);

/* Stage-level entry (tests): the payload the multi-GPU path all-reduces after one linearisation of this problem
 * (a rank's point shard, or the whole problem): S (6C)^2 unscaled / undamped, full symmetric | g_c (6C) | rhs
 * correction (6C) | diag U (6C) | 8 scalars (cost sum, |points|^2, failed point blocks, ...), followed by the one value
 * that is max-reduced (max |g_p|).  Additive over disjoint point shards: the sum of the shards' payloads is the
 * payload of the union.  payload == NULL: only *count (doubles needed) is returned. */
int rsba_points_linearize_payload(rsba_problem* p, const rsba_options* o, double radius, double* payload, int64_t capacity,
                                  int64_t* count);

/* ------------------------------------------------------------------ multi-GPU bootstrap */
/* ncclGetUniqueId: rank 0 calls this and ships the 128 bytes to the other ranks (bench.py does it
 * through torch.distributed); every rank then passes it in rsba_options.comm_unique_id. */
int rsba_comm_unique_id(void* out128);
/* The same 128 bytes for a LOOPBACK group: world_size solver objects of ONE process on ONE GPU, each created and run by its own
 * host thread with this id in rsba_options.comm_unique_id (and its rank).  The collectives of the multi-GPU schedule are then
 * sums over the group's solvers on that GPU instead of ncclAllReduce over xGMI (csrc/ba_comm.hpp): the whole N > 1 schedule
 * — sharded upload, three collectives per LM step, the summed stall flag — on a one-GPU box.  The ranks take turns on the
 * device, so it measures nothing; it is how the multi-rank code path is tested where only one GPU is visible.  The reference
 * has no counterpart (single-threaded: Main_Calibration/bundle_adjustment_manager.cpp:90-92). */
int rsba_comm_loopback_id(void* out128);
/* The same 128 bytes for a SHARED-MEMORY group (round 5): world_size PROCESSES of one host — on one GPU or several — whose
 * collectives are staged through a POSIX shared-memory segment named after `name` ([A-Za-z0-9_.-], at most 80 characters, the
 * same string on every rank, unique per group and run) and added on the host in rank order.  It is how one process per rank,
 * bench.py's own launcher and the id bootstrap run end to end where RCCL cannot (two ranks on one device); sequential multi-GPU
 * schedule only.  No counterpart in the reference (single process, single thread). */
int rsba_comm_shm_id(const char* name, void* out128);
/* Destroys every RCCL communicator this process still holds (ncclCommDestroy); call once, after the last solver is destroyed and
 * before the process tears the HIP runtime down.  Optional: communicators otherwise live until exit. */
void rsba_comm_finalize(void);
/* ncclCommCount of the solver's communicator: the number of ranks its all-reduces really span (1 without a
 * communicator).  bench.py prints it as `rccl_nranks` and refuses to report a line when it differs from --gpus. */
int rsba_solver_comm_nranks(const rsba_solver* s);
/* A rank that gives up OUTSIDE the library (its host code failed between two collective calls) says so here, so that the ranks
 * already waiting for it in a collective leave with RSBA_ERR_COMM instead of waiting out the time limit.  The communicator is
 * unusable afterwards, as after any failed collective.  No-op without a communicator; may be called from any thread. */
int rsba_solver_comm_abort(rsba_solver* s);
/* The schedule in effect and the stalls / fallbacks so far (rsba_schedule_info).  The reference has no counterpart: Ceres runs
 * one thread (bundle_adjustment_manager.cpp:90-92). */
int rsba_solver_schedule_info(const rsba_solver* s, rsba_schedule_info* out);
/* Marker-chain models: which path the solver runs.  *eliminates_times = 1 when the time blocks are eliminated (rsba_options.schur_impl 2
 * or 3, or 1 above RSBA_CHOL_MAXN unknowns; with free intrinsics, rsba_problem_set_intrinsics_free: schur_impl 3 only), 0 on the dense
 * one-workgroup path — the choice falls back to it silently for duplicate
 * detections, a time that touches more than 170 camera / marker blocks, or a solver that needs the split elimination (a robust
 * loss, observation weights, priors or subset masks) with times too wide for the split accumulation (about 120 camera / marker
 * blocks).  The rules, and the RSBA_MT_* environment switches of the time-eliminating path (RSBA_MT_SPLIT, RSBA_MT_ACC_MFMA,
 * RSBA_MT_CHUNKS, RSBA_MT_BACKSUB_WG, RSBA_MT_SPLIT_BACKSUB, RSBA_MT_FORK, RSBA_MT_SOLVE_LDS), are in one place:
 * PlanMarkerChain and MarkerSwitches::FromEnv, the switches' single reader, in csrc/ba_marker_plan.hpp; they are read at every
 * rsba_solver_create.  RSBA_ERR_UNSUPPORTED for the point model, RSBA_ERR_ARG for NULL. */
int rsba_solver_time_elimination(const rsba_solver* s, int32_t* eliminates_times);

/* ------------------------------------------------------------------ files either side of the path */
/* IO::GetIntrinsics (my_io.cpp:5-31) without OpenCV: reads <intrinsics> 3x3 from an OpenCV
 * FileStorage XML and returns fx, fy, ppx, ppy. */
int rsba_read_intrinsics_xml(const char* path, double* out4);
/* The same, and <distCoeffs> (my_io.cpp reads it beside <intrinsics>): out5 = k1 k2 p1 p2 k3.  A 4 x 1 or 1 x 4 vector sets k3 = 0, a
 * 5 x 1 or 1 x 5 one is read as it is, a missing node gives zeros.  8, 12 or 14 entries (OpenCV's rational, thin-prism and tilted
 * models): RSBA_ERR_UNSUPPORTED; any other shape: RSBA_ERR_FORMAT. */
int rsba_read_intrinsics_xml_dist(const char* path, double* out4, double* out5);

/* BAManager::Write (bundle_adjustment_manager.cpp:98-175).  Any path may be NULL to skip that file.
 *   camera_transform_xml : R{i} 3x3 (Main) or rvec 3x1 (Test2 variant, main.cpp:128) + t{i}
 *   extrinsics_dir       : mat{i}.txt = [R^T | -R^T t] one value per line (:135-149)
 *   point3d_txt          : `4N T C`, count rows, 4N xyz rows (:154-174) */
int rsba_write_outputs(rsba_problem* p, const char* camera_transform_xml, const char* extrinsics_dir,
                       const char* point3d_txt);

/* ReprojectionCheck::Reproject's metric (reprojection_check.cpp:76-101) from the current
 * parameters, evaluated on the GPU: error = sum((du^2+dv^2)/2), rms = sqrt(2 error / (2 n_points)). */
int rsba_reprojection_error(rsba_problem* p, const rsba_options* o, double* error, double* rms);

/* ReprojectionCheck::Reproject end to end from the files it reads (reprojection_check.cpp:5-101): the 6-digit 3D
 * corners of point3d.txt, R{i} (3x3, or the 3x1 rvec of the Test2 variant) and t{i} of Camera_Transform.xml, and the
 * detected corners — taken from correspondence.txt and rounded to float32 as the reference holds them (Point2f,
 * :78) — projected on the GPU with zero distortion (:69): this call stays pinhole, its signature has no place for coefficients
 * (rsba_reprojection_error on a problem with rsba_problem_set_distortion is the one that honours them).  intrinsics: fx, fy, ppx,
 * ppy per camera.  On the
 * committed hongo files this prints the reference's 143.64 / 0.726696 (vs 0.726670 from the unrounded parameters). */
int rsba_reprojection_check_files(const char* correspondence_txt, const char* point3d_txt, const char* camera_transform_xml,
                                  const double* intrinsics, double* error, double* rms);

#ifdef __cplusplus
}
#endif
#endif /* RSBA_H_ */
