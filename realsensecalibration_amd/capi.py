"""ctypes binding of librsba.so (include/rsba.h).  Plumbing for tests and bench.py; the product is the
shared library.  Loading fails loudly when the library has not been built: there is no fallback."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# RSBA_LIB: another build of the library (tools/ build diagnostic variants to a scratch path and point this at them — the packaged
# library is never overwritten)
LIB_PATH = os.environ.get("RSBA_LIB") or os.path.join(HERE, "librsba.so")

OK, ERR_IO, ERR_FORMAT, ERR_ARG, ERR_HIP, ERR_NO_DEVICE, ERR_COMM, ERR_UNSUPPORTED, ERR_RANK_DEFICIENT = range(9)
MODEL_POINTS, MODEL_MARKER_CHAIN, MODEL_MARKER_CHAIN_TEST2 = 0, 1, 2
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2

EXPORTS = [
    "rsba_version", "rsba_device_count", "rsba_error_string", "rsba_problem_create_points", "rsba_problem_create_marker_chain",
    "rsba_problem_load_points_file",
    "rsba_problem_load_correspondence", "rsba_problem_free", "rsba_problem_model", "rsba_problem_num_cameras",
    "rsba_problem_num_points", "rsba_problem_num_times", "rsba_problem_num_markers", "rsba_problem_num_observations",
    "rsba_problem_num_parameters", "rsba_problem_num_observations_per_time_camera", "rsba_problem_observations",
    "rsba_problem_parameters", "rsba_problem_camera_idx", "rsba_problem_point_idx", "rsba_problem_time_idx",
    "rsba_problem_marker_idx", "rsba_problem_camera_parameters", "rsba_problem_marker_transform",
    "rsba_problem_point3d_coordinates", "rsba_options_default", "rsba_solve", "rsba_solver_create", "rsba_solver_run",
    "rsba_solver_download", "rsba_solver_iterations", "rsba_solver_kernel_stats", "rsba_solver_final_costs",
    "rsba_solver_destroy", "rsba_points_linearize_and_step", "rsba_points_solve_stage", "rsba_points_linearize_payload", "rsba_comm_unique_id", "rsba_comm_loopback_id", "rsba_read_intrinsics_xml",
    "rsba_write_outputs", "rsba_reprojection_error", "rsba_reprojection_check_files",
    "rsba_base_pose_from_marker_detection", "rsba_marker_pose_in_camera", "rsba_marker_corners_in_camera", "rsba_solve_pnp_epnp",
    "rsba_problem_initial_camera_poses", "rsba_problem_set_camera_constant", "rsba_problem_set_point_constant", "rsba_problem_set_parameter_block_constant", "rsba_solver_full_report", "rsba_solver_configure_run",
    "rsba_solver_comm_nranks", "rsba_solver_schedule_info", "rsba_comm_shm_id", "rsba_comm_finalize",
    "rsba_covariance_options_default", "rsba_solver_covariance_compute", "rsba_solver_covariance_block", "rsba_solver_point_covariances",
    "rsba_solver_time_elimination", "rsba_solver_covariance_blocks", "rsba_solver_time_covariances",
    "rsba_evaluate_options_default", "rsba_solver_num_residuals", "rsba_solver_evaluate", "rsba_solver_set_parameters",
    "rsba_solver_jacobian_structure", "rsba_solver_evaluate_jacobian",
    "rsba_solver_comm_abort",
    "rsba_problem_set_observation_weights", "rsba_problem_observation_weights", "rsba_solver_set_observation_weights",
    "rsba_problem_set_parameter_subset_constant", "rsba_problem_parameter_subset_constant", "rsba_problem_set_distortion", "rsba_problem_distortion", "rsba_read_intrinsics_xml_dist", "rsba_undistort_points",
    "rsba_problem_set_block_prior", "rsba_problem_block_prior", "rsba_problem_num_block_priors", "rsba_solver_set_block_prior",
    "rsba_marker_pose_from_corners", "rsba_marker_poses_from_corners", "rsba_problem_initial_time_poses", "rsba_problem_start_rig", "rsba_problem_start_scene",
    "rsba_marker_pose_from_corners_both", "rsba_marker_poses_from_corners_both", "rsba_problem_start_rig2", "rsba_problem_start_scene2",
    "rsba_problem_set_intrinsics_free", "rsba_problem_intrinsics_free", "rsba_problem_intrinsics",
    "rsba_solver_set_extended_layout", "rsba_solver_num_extended_parameters",
]
INTRINSICS_COMPONENTS = ("fx", "fy", "cx", "cy", "k1", "k2")   # bit q of rsba_problem_set_intrinsics_free's mask
START_BOTH_SOLUTIONS = 1   # RSBA_START_BOTH_SOLUTIONS
MARKER_POSE_SAME = 3       # RSBA_MARKER_POSE_SAME
_SYMBOLS = EXPORTS   # (every symbol of include/rsba.h that load() checks)


class Options(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int32), ("max_num_consecutive_invalid_steps", C.c_int32),
                ("jacobi_scaling", C.c_int32), ("minimizer_progress_to_stdout", C.c_int32),
                ("initial_trust_region_radius", C.c_double), ("max_trust_region_radius", C.c_double),
                ("min_trust_region_radius", C.c_double), ("min_relative_decrease", C.c_double),
                ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double), ("function_tolerance", C.c_double),
                ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double), ("huber_delta", C.c_double),
                ("device", C.c_int32), ("schur_impl", C.c_int32), ("profile_kernels", C.c_int32), ("rank", C.c_int32),
                ("world_size", C.c_int32), ("loss_type", C.c_int32), ("comm_unique_id", C.c_void_p), ("stream", C.c_void_p),
                ("max_solver_time_in_seconds", C.c_double)]


class Summary(C.Structure):
    _fields_ = [("termination_type", C.c_int32), ("stop_reason", C.c_int32), ("num_successful_steps", C.c_int32),
                ("num_unsuccessful_steps", C.c_int32), ("num_iterations", C.c_int32), ("reserved", C.c_int32),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("minimizer_seconds", C.c_double),
                ("setup_seconds", C.c_double)]


class Iteration(C.Structure):
    _fields_ = [("iteration", C.c_int32), ("step_is_valid", C.c_int32), ("step_is_successful", C.c_int32),
                ("linear_solver_iterations", C.c_int32), ("cost", C.c_double), ("cost_change", C.c_double),
                ("gradient_max_norm", C.c_double), ("step_norm", C.c_double), ("relative_decrease", C.c_double),
                ("trust_region_radius", C.c_double), ("iteration_time_in_seconds", C.c_double),
                ("cumulative_time_in_seconds", C.c_double)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("total_ms", C.c_double)]


class ScheduleInfo(C.Structure):
    _fields_ = [("schedule", C.c_int32), ("stalls", C.c_int32), ("fallbacks", C.c_int32), ("comm_nranks", C.c_int32),
                ("chol_workgroups", C.c_int32), ("schur_impl", C.c_int32), ("comm_kind", C.c_char * 16)]


class CovarianceOptions(C.Structure):
    _fields_ = [("min_reciprocal_condition_number", C.c_double), ("apply_loss_function", C.c_int32), ("reserved", C.c_int32)]


class EvaluateOptions(C.Structure):
    _fields_ = [("apply_loss_function", C.c_int32), ("reserved", C.c_int32)]


class RsbaError(RuntimeError):
    def __init__(self, code, what):
        self.code = code
        super().__init__("%s: %s (code %d)" % (what, error_string(code), code))


_LIB = None


def load():
    """dlopen librsba.so and check that every symbol of include/rsba.h is exported."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError("librsba.so is not built: run `python __graft_entry__.py` (hipcc --offload-arch=gfx950). "
                          "There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    missing = [s for s in EXPORTS if not hasattr(lib, s)]
    if missing:
        raise ImportError("librsba.so lacks symbols declared in include/rsba.h: %s" % missing)
    lib.rsba_error_string.restype = C.c_char_p
    lib.rsba_problem_parameters.restype = C.POINTER(C.c_double)
    lib.rsba_problem_observations.restype = C.POINTER(C.c_double)
    lib.rsba_problem_camera_parameters.restype = C.POINTER(C.c_double)
    lib.rsba_problem_marker_transform.restype = C.POINTER(C.c_double)
    lib.rsba_problem_num_observations.restype = C.c_int64
    lib.rsba_problem_num_parameters.restype = C.c_int64
    lib.rsba_problem_create_points.argtypes = [C.c_int32, C.c_int32, C.c_int64] + [C.c_void_p] * 6
    lib.rsba_problem_create_marker_chain.argtypes = [C.c_int32] * 4 + [C.c_int64] + [C.c_void_p] * 6 + [C.c_double, C.c_void_p]
    lib.rsba_problem_load_points_file.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p]
    lib.rsba_problem_load_correspondence.argtypes = [C.c_char_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]
    lib.rsba_problem_free.argtypes = [C.c_void_p]
    for f in ("rsba_problem_model", "rsba_problem_num_cameras", "rsba_problem_num_points", "rsba_problem_num_times",
              "rsba_problem_num_markers", "rsba_problem_num_observations", "rsba_problem_num_parameters",
              "rsba_problem_parameters", "rsba_problem_observations"):
        getattr(lib, f).argtypes = [C.c_void_p]
    lib.rsba_problem_num_observations_per_time_camera.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    for f in ("rsba_problem_camera_idx", "rsba_problem_point_idx", "rsba_problem_time_idx", "rsba_problem_marker_idx"):
        getattr(lib, f).argtypes = [C.c_void_p, C.c_int64]
    lib.rsba_problem_camera_parameters.argtypes = [C.c_void_p, C.c_int32]
    lib.rsba_problem_marker_transform.argtypes = [C.c_void_p, C.c_int32]
    lib.rsba_problem_point3d_coordinates.argtypes = [C.c_void_p, C.c_void_p]
    lib.rsba_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rsba_solver_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rsba_solver_run.argtypes = [C.c_void_p, C.c_void_p]
    lib.rsba_solver_download.argtypes = [C.c_void_p]
    lib.rsba_solver_iterations.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.rsba_solver_kernel_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.rsba_solver_full_report.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    lib.rsba_solver_configure_run.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.rsba_solver_final_costs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rsba_solver_destroy.argtypes = [C.c_void_p]
    lib.rsba_solver_comm_nranks.argtypes = [C.c_void_p]
    lib.rsba_solver_schedule_info.argtypes = [C.c_void_p, C.c_void_p]
    lib.rsba_solver_time_elimination.argtypes = [C.c_void_p, C.c_void_p]
    lib.rsba_comm_shm_id.argtypes = [C.c_char_p, C.c_void_p]
    lib.rsba_points_linearize_and_step.argtypes = [C.c_void_p, C.c_void_p, C.c_double] + [C.c_void_p] * 4
    lib.rsba_points_solve_stage.argtypes = [C.c_void_p, C.c_void_p, C.c_double] + [C.c_void_p] * 6
    lib.rsba_points_linearize_payload.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int64, C.c_void_p]
    lib.rsba_comm_unique_id.argtypes = [C.c_void_p]
    lib.rsba_comm_loopback_id.argtypes = [C.c_void_p]
    lib.rsba_read_intrinsics_xml.argtypes = [C.c_char_p, C.c_void_p]
    lib.rsba_write_outputs.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p]
    lib.rsba_reprojection_error.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rsba_reprojection_check_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rsba_base_pose_from_marker_detection.argtypes = [C.c_void_p] * 3
    lib.rsba_marker_pose_in_camera.argtypes = [C.c_void_p] * 3
    lib.rsba_marker_corners_in_camera.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
    lib.rsba_solve_pnp_epnp.argtypes = [C.c_int32] + [C.c_void_p] * 4
    lib.rsba_problem_initial_camera_poses.argtypes = [C.c_void_p]
    lib.rsba_problem_set_camera_constant.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.rsba_problem_set_point_constant.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.rsba_problem_set_parameter_block_constant.argtypes = [C.c_void_p, C.c_int64, C.c_int32]
    lib.rsba_covariance_options_default.argtypes = [C.c_void_p]
    lib.rsba_solver_covariance_compute.argtypes = [C.c_void_p, C.c_void_p]
    lib.rsba_solver_covariance_block.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.rsba_solver_point_covariances.argtypes = [C.c_void_p, C.c_void_p]
    lib.rsba_solver_covariance_blocks.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rsba_solver_time_covariances.argtypes = [C.c_void_p, C.c_void_p]
    lib.rsba_evaluate_options_default.argtypes = [C.c_void_p]
    lib.rsba_solver_num_residuals.argtypes = [C.c_void_p]
    lib.rsba_solver_num_residuals.restype = C.c_int64
    lib.rsba_solver_evaluate.argtypes = [C.c_void_p] * 5
    lib.rsba_solver_jacobian_structure.argtypes = [C.c_void_p] * 6
    lib.rsba_solver_evaluate_jacobian.argtypes = [C.c_void_p] * 3
    lib.rsba_solver_set_parameters.argtypes = [C.c_void_p, C.c_void_p]
    lib.rsba_solver_set_extended_layout.argtypes = [C.c_void_p, C.c_int32]
    lib.rsba_solver_num_extended_parameters.argtypes = [C.c_void_p]
    lib.rsba_solver_num_extended_parameters.restype = C.c_int64
    lib.rsba_solver_comm_abort.argtypes = [C.c_void_p]
    lib.rsba_problem_set_observation_weights.argtypes = [C.c_void_p, C.c_void_p]
    lib.rsba_problem_observation_weights.argtypes = [C.c_void_p]
    lib.rsba_problem_observation_weights.restype = C.POINTER(C.c_double)
    lib.rsba_solver_set_observation_weights.argtypes = [C.c_void_p, C.c_void_p]
    lib.rsba_problem_set_parameter_subset_constant.argtypes = [C.c_void_p, C.c_int64, C.c_int32]
    lib.rsba_problem_parameter_subset_constant.argtypes = [C.c_void_p, C.c_int64]
    lib.rsba_problem_parameter_subset_constant.restype = C.c_int32
    lib.rsba_problem_set_distortion.argtypes = [C.c_void_p, C.c_void_p]
    lib.rsba_problem_distortion.argtypes = [C.c_void_p]
    lib.rsba_problem_distortion.restype = C.POINTER(C.c_double)
    lib.rsba_problem_set_intrinsics_free.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.rsba_problem_intrinsics_free.argtypes = [C.c_void_p, C.c_int32]
    lib.rsba_problem_intrinsics_free.restype = C.c_int32
    lib.rsba_problem_intrinsics.argtypes = [C.c_void_p]
    lib.rsba_problem_intrinsics.restype = C.POINTER(C.c_double)
    lib.rsba_read_intrinsics_xml_dist.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p]
    lib.rsba_undistort_points.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rsba_problem_set_block_prior.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.rsba_problem_block_prior.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.rsba_problem_num_block_priors.argtypes = [C.c_void_p]
    lib.rsba_problem_num_block_priors.restype = C.c_int32
    lib.rsba_solver_set_block_prior.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.rsba_marker_pose_from_corners.argtypes = [C.c_void_p] * 3 + [C.c_double] + [C.c_void_p] * 3
    lib.rsba_marker_poses_from_corners.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_int32] + [C.c_void_p] * 3
    lib.rsba_problem_initial_time_poses.argtypes = [C.c_void_p, C.c_void_p]
    lib.rsba_problem_start_rig.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 4
    lib.rsba_problem_start_scene.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 5
    lib.rsba_marker_pose_from_corners_both.argtypes = lib.rsba_marker_pose_from_corners.argtypes
    lib.rsba_marker_poses_from_corners_both.argtypes = lib.rsba_marker_poses_from_corners.argtypes
    lib.rsba_problem_start_rig2.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32] + [C.c_void_p] * 4
    lib.rsba_problem_start_scene2.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32] + [C.c_void_p] * 5
    _LIB = lib
    return lib


def error_string(code):
    return load().rsba_error_string(code).decode()


def _chk(code, what):
    if code != OK:
        raise RsbaError(code, what)


def default_options(**kw):
    o = Options()
    load().rsba_options_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _prior_arrays(A, b):
    A = np.ascontiguousarray(A, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    if A.ndim != 2 or A.shape[1] != 6 or not 1 <= A.shape[0] <= 6 or b.shape != (6,):
        raise ValueError("a block prior takes A of up to 6 x 6 and b of 6 values")
    full = np.zeros((6, 6))
    full[:A.shape[0]] = A
    return full, b


class Problem:
    """Owns an rsba_problem*.  `params` is a numpy view of the problem's own parameter array."""

    def __init__(self, handle):
        self.h = handle
        self._fit_constants = None   # (intrinsics C x 4, marker side) of a marker-chain problem: the C ABI has no reader for them
        lib = load()
        n = lib.rsba_problem_num_parameters(self.h)
        self.params = np.ctypeslib.as_array(lib.rsba_problem_parameters(self.h), shape=(n,))

    @classmethod
    def points(cls, prob):
        h = C.c_void_p()
        cam = np.ascontiguousarray(prob["cam_idx"], np.int32)
        pt = np.ascontiguousarray(prob["pt_idx"], np.int32)
        obs = np.ascontiguousarray(prob["obs"], np.float64)
        par = np.ascontiguousarray(prob["params"], np.float64)
        intr = np.ascontiguousarray(prob["intr"], np.float64)
        _chk(load().rsba_problem_create_points(prob["C"], prob["P"], prob["N"], _vp(cam), _vp(pt), _vp(obs), _vp(par), _vp(intr),
                                               C.byref(h)), "rsba_problem_create_points")
        return cls(h)

    @classmethod
    def marker_chain(cls, prob, model=MODEL_MARKER_CHAIN):
        """prob: dict with T, C, M, N, t, c, m (int32 per row), obs (N x 8), params (6 (C + T + M)), intr (C x 4), marker_side, and
        optionally dist (C x 5: k1 k2 p1 p2 k3 per camera, set_distortion)."""
        h = C.c_void_p()
        t, c, m = (np.ascontiguousarray(prob[k], np.int32) for k in ("t", "c", "m"))
        obs = np.ascontiguousarray(prob["obs"], np.float64)
        par = np.ascontiguousarray(prob["params"], np.float64)
        intr = np.ascontiguousarray(prob["intr"], np.float64)
        _chk(load().rsba_problem_create_marker_chain(model, prob["C"], prob["T"], prob["M"], prob["N"], _vp(t), _vp(c), _vp(m), _vp(obs),
                                                     _vp(par), _vp(intr), C.c_double(prob["marker_side"]), C.byref(h)),
             "rsba_problem_create_marker_chain")
        p = cls(h)
        p._fit_constants = (intr.reshape(-1, 4).copy(), float(prob["marker_side"]))
        if prob.get("dist") is not None:
            try:
                p.set_distortion(prob["dist"])
            except Exception:
                p.close()
                raise
        return p

    @classmethod
    def points_file(cls, path, intrinsics4):
        h = C.c_void_p()
        k = np.ascontiguousarray(intrinsics4, np.float64)
        _chk(load().rsba_problem_load_points_file(path.encode(), _vp(k), C.byref(h)), "rsba_problem_load_points_file")
        return cls(h)

    @classmethod
    def correspondence(cls, path, model, marker_side, intrinsics):
        h = C.c_void_p()
        k = np.ascontiguousarray(intrinsics, np.float64)
        _chk(load().rsba_problem_load_correspondence(path.encode(), model, marker_side, _vp(k), C.byref(h)),
             "rsba_problem_load_correspondence")
        p = cls(h)
        p._fit_constants = (k.reshape(-1, 4).copy(), float(marker_side))
        return p

    def __getattr__(self, name):
        f = {"model": "rsba_problem_model", "num_cameras": "rsba_problem_num_cameras", "num_points": "rsba_problem_num_points",
             "num_times": "rsba_problem_num_times", "num_markers": "rsba_problem_num_markers",
             "num_observations": "rsba_problem_num_observations", "num_parameters": "rsba_problem_num_parameters"}.get(name)
        if f is None:
            raise AttributeError(name)
        return getattr(load(), f)(self.h)

    def num_observations_per_time_camera(self, t, c):
        return load().rsba_problem_num_observations_per_time_camera(self.h, t, c)

    def point3d(self):
        out = np.zeros((4 * self.num_observations, 3))
        _chk(load().rsba_problem_point3d_coordinates(self.h, _vp(out)), "rsba_problem_point3d_coordinates")
        return out

    def write_outputs(self, xml=None, extrinsics_dir=None, point3d=None):
        e = lambda s: s.encode() if s else None  # noqa: E731
        _chk(load().rsba_write_outputs(self.h, e(xml), e(extrinsics_dir), e(point3d)), "rsba_write_outputs")

    def reprojection_error(self, opts=None):
        err, rms = C.c_double(), C.c_double()
        o = opts or default_options()
        _chk(load().rsba_reprojection_error(self.h, C.byref(o), C.byref(err), C.byref(rms)), "rsba_reprojection_error")
        return err.value, rms.value

    def set_camera_constant(self, camera_idx, constant=True):
        _chk(load().rsba_problem_set_camera_constant(self.h, camera_idx, 1 if constant else 0), "rsba_problem_set_camera_constant")

    def set_point_constant(self, point_idx, constant=True):
        _chk(load().rsba_problem_set_point_constant(self.h, point_idx, 1 if constant else 0), "rsba_problem_set_point_constant")

    def set_parameter_block_constant(self, parameter_offset, constant=True):
        _chk(load().rsba_problem_set_parameter_block_constant(self.h, parameter_offset, 1 if constant else 0), "rsba_problem_set_parameter_block_constant")

    def set_parameter_subset_constant(self, parameter_offset, components):
        """Marker-chain models: hold single components of the pose block at parameter_offset (ceres::SubsetParameterization).
        components: a 6-bit mask (bit q = component q of rvec, tvec) or an iterable of component indices; 0 / empty removes it."""
        if isinstance(components, (int, np.integer)):
            mask = int(components)
        else:
            mask = 0
            for q in components:
                q = int(q)
                if q < 0 or q > 5:
                    raise ValueError("set_parameter_subset_constant: component %d is not in 0..5" % q)
                mask |= 1 << q
        _chk(load().rsba_problem_set_parameter_subset_constant(self.h, parameter_offset, mask), "rsba_problem_set_parameter_subset_constant")

    def parameter_subset_constant(self, parameter_offset):
        """The block's mask of constant components; 0 when it has none."""
        return int(load().rsba_problem_parameter_subset_constant(self.h, parameter_offset))

    def set_observation_weights(self, w):
        """Marker-chain models: one weight a_i >= 0 per residual block (ceres::ScaledLoss), the problem's observation order; None
        removes them.  A solver created from a problem that carries weights takes new ones later (Solver.set_observation_weights)."""
        if w is None:
            _chk(load().rsba_problem_set_observation_weights(self.h, None), "rsba_problem_set_observation_weights")
            return
        w = np.ascontiguousarray(w, np.float64)
        if w.shape != (self.num_observations,):
            raise ValueError("set_observation_weights: %d values expected" % self.num_observations)
        _chk(load().rsba_problem_set_observation_weights(self.h, _vp(w)), "rsba_problem_set_observation_weights")

    @property
    def observation_weights(self):
        """A copy of the problem's weights, or None when it has none."""
        q = load().rsba_problem_observation_weights(self.h)
        return np.ctypeslib.as_array(q, shape=(self.num_observations,)).copy() if q else None

    def set_distortion(self, dist):
        """Marker-chain models: OpenCV's k1 k2 p1 p2 k3 per camera index (C x 5), constants of the problem like the intrinsics; None
        removes them.  Solvers created afterwards honour them (all zeros: the kernels and bits of a problem without)."""
        if dist is None:
            _chk(load().rsba_problem_set_distortion(self.h, None), "rsba_problem_set_distortion")
            return
        d = np.ascontiguousarray(dist, np.float64)
        if d.size != 5 * self.num_cameras:
            raise ValueError("set_distortion: %d x 5 values expected" % self.num_cameras)
        _chk(load().rsba_problem_set_distortion(self.h, _vp(d)), "rsba_problem_set_distortion")

    @property
    def distortion(self):
        """A copy of the problem's distortion coefficients (C x 5), or None when it has none."""
        q = load().rsba_problem_distortion(self.h)
        return np.ctypeslib.as_array(q, shape=(self.num_cameras, 5)).copy() if q else None

    def set_intrinsics_free(self, camera, components):
        """Marker-chain models: let the solve refine components of camera index `camera`'s intrinsics block fx fy cx cy k1 k2
        (rsba_problem_set_intrinsics_free).  components: a 6-bit mask (bit q = component q is refined) or an iterable of names among
        "fx", "fy", "cx", "cy", "k1", "k2"; 0 / empty: the camera's values are constants again.  Solvers created afterwards take the
        dense path and write the refined values back into the problem (intrinsics, distortion) on download."""
        if isinstance(components, (int, np.integer)):
            mask = int(components)
        else:
            mask = 0
            for name in ([components] if isinstance(components, str) else components):
                if name not in INTRINSICS_COMPONENTS:
                    raise ValueError("set_intrinsics_free: %r is not one of %s" % (name, ", ".join(INTRINSICS_COMPONENTS)))
                mask |= 1 << INTRINSICS_COMPONENTS.index(name)
        _chk(load().rsba_problem_set_intrinsics_free(self.h, int(camera), mask), "rsba_problem_set_intrinsics_free")

    def intrinsics_free(self, camera):
        """The camera's mask of refined intrinsics components; 0 when it has none."""
        return int(load().rsba_problem_intrinsics_free(self.h, int(camera)))

    @property
    def intrinsics(self):
        """A copy of the problem's intrinsics (C x 4: fx fy ppx ppy): the values it was created with, or a solve's refined ones."""
        q = load().rsba_problem_intrinsics(self.h)
        return np.ctypeslib.as_array(q, shape=(self.num_cameras, 4)).copy()

    def set_block_prior(self, parameter_offset, A, b=None):
        """Marker-chain models: a Gaussian prior (ceres::NormalPrior) on the camera or marker block at `parameter_offset`: the
        residual A (x - b), A 6 x 6 (fewer rows: zero rows), b 6, no loss.  A = None removes it."""
        if A is None:
            _chk(load().rsba_problem_set_block_prior(self.h, parameter_offset, None, None), "rsba_problem_set_block_prior")
            return
        A, b = _prior_arrays(A, b)
        _chk(load().rsba_problem_set_block_prior(self.h, parameter_offset, _vp(A), _vp(b)), "rsba_problem_set_block_prior")

    def block_prior(self, parameter_offset):
        """(A 6 x 6, b 6) of the block's prior, or None when it has none."""
        A, b = np.zeros((6, 6)), np.zeros(6)
        return (A, b) if load().rsba_problem_block_prior(self.h, parameter_offset, _vp(A), _vp(b)) else None

    @property
    def num_block_priors(self):
        return int(load().rsba_problem_num_block_priors(self.h))

    def initial_camera_poses(self):
        _chk(load().rsba_problem_initial_camera_poses(self.h), "rsba_problem_initial_camera_poses")

    def initial_time_poses(self):
        """Marker-chain models: every time block from camera 0's detection with the lowest marker index at that time
        (correspondencer.cpp:100-127).  Returns how many times kept their values because camera 0 detected nothing usable there."""
        missing = C.c_int32(0)
        _chk(load().rsba_problem_initial_time_poses(self.h, C.byref(missing)), "rsba_problem_initial_time_poses")
        return int(missing.value)

    def start_rig(self, known=None, refine_sweeps=1, device=-1, both_solutions=False):
        """Marker-chain models: the camera and time blocks of the whole rig from its detections, on the GPU (rsba_problem_start_rig):
        block resection — one block fitted to all its detections, the others held — propagated over the co-visibility graph from the
        known blocks.  known: C + T flags (cameras, then times) of blocks that keep their values, or None (only the base camera).
        refine_sweeps: passes over all fitted times, then all fitted cameras, after the rounds (1 is recommended).  Returns
        (missing_times, missing_cameras, status C + T, rms C + T): status 0 converged, 1 iteration cap, 2 degenerate, 3 unreached, 4 given
        or the base camera; blocks with status 2 to 4 keep their bits and have rms -1.
        both_solutions (rsba_problem_start_rig2, RSBA_START_BOTH_SOLUTIONS): a block's start is taken from both poses of each candidate
        detection (marker_pose_from_corners_both), so a block whose own fits are all the mirror image can still start right."""
        nb = self.num_cameras + (self.num_times if self.model != MODEL_POINTS else 0)
        k = None
        if known is not None:
            k = np.ascontiguousarray(known, np.uint8).reshape(-1)
            if k.size != nb:
                raise ValueError("start_rig: one flag per camera and time block expected")
        mt, mc = C.c_int32(0), C.c_int32(0)
        status, rms = np.zeros(nb, np.int32), np.zeros(nb)
        if both_solutions:
            _chk(load().rsba_problem_start_rig2(self.h, None if k is None else _vp(k), int(refine_sweeps), int(device), START_BOTH_SOLUTIONS,
                                                C.byref(mt), C.byref(mc), _vp(status), _vp(rms)), "rsba_problem_start_rig2")
            return int(mt.value), int(mc.value), status, rms
        _chk(load().rsba_problem_start_rig(self.h, None if k is None else _vp(k), int(refine_sweeps), int(device), C.byref(mt), C.byref(mc),
                                           _vp(status), _vp(rms)), "rsba_problem_start_rig")
        return int(mt.value), int(mc.value), status, rms

    def start_scene(self, known=None, refine_sweeps=1, device=-1, both_solutions=False):
        """Marker-chain models: start_rig for a scene whose board geometry is not known (rsba_problem_start_scene): the marker blocks are
        fitted by block resection too, in rounds of times, markers, cameras from the known blocks.  known: C + T + M flags (cameras, times,
        markers) of blocks that keep their values, or None (the base camera, and the base marker of MODEL_MARKER_CHAIN).  A detection
        counts for a block only when both its other blocks are known.  Returns (missing_times, missing_cameras, missing_markers,
        status C + T + M, rms C + T + M) with start_rig's statuses; 4 also for the base marker.  both_solutions: as for start_rig
        (rsba_problem_start_scene2)."""
        nb = self.num_cameras + (self.num_times + self.num_markers if self.model != MODEL_POINTS else 0)
        k = None
        if known is not None:
            k = np.ascontiguousarray(known, np.uint8).reshape(-1)
            if k.size != nb:
                raise ValueError("start_scene: one flag per camera, time and marker block expected")
        mt, mc, mm = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        status, rms = np.zeros(nb, np.int32), np.zeros(nb)
        if both_solutions:
            _chk(load().rsba_problem_start_scene2(self.h, None if k is None else _vp(k), int(refine_sweeps), int(device), START_BOTH_SOLUTIONS,
                                                  C.byref(mt), C.byref(mc), C.byref(mm), _vp(status), _vp(rms)), "rsba_problem_start_scene2")
            return int(mt.value), int(mc.value), int(mm.value), status, rms
        _chk(load().rsba_problem_start_scene(self.h, None if k is None else _vp(k), int(refine_sweeps), int(device), C.byref(mt), C.byref(mc),
                                             C.byref(mm), _vp(status), _vp(rms)), "rsba_problem_start_scene")
        return int(mt.value), int(mc.value), int(mm.value), status, rms

    def detection_poses(self, device=-1):
        """Marker-chain models: (poses N x 6, rms N, status N) of every observation's own single-marker fit, one batch on the GPU over
        the problem's observations, camera indices, intrinsics and distortion coefficients (marker_poses_from_corners)."""
        lib = load()
        if self.model == MODEL_POINTS:
            raise RsbaError(ERR_UNSUPPORTED, "detection_poses")
        n, nc = self.num_observations, self.num_cameras
        obs = np.ctypeslib.as_array(lib.rsba_problem_observations(self.h), shape=(n, 8)).copy()
        cam = np.array([lib.rsba_problem_camera_idx(self.h, i) for i in range(n)], np.int32)
        intr, side = self._intrinsics_and_side()
        return marker_poses_from_corners(obs, cam, intr, self.distortion, side, device=device, num_cameras=nc)

    def _intrinsics_and_side(self):
        if getattr(self, "_fit_constants", None) is None:
            raise ValueError("detection_poses: the problem's intrinsics and marker side are known for problems made by "
                             "Problem.marker_chain and Problem.correspondence")
        return self._fit_constants

    def solve(self, opts=None):
        s = Summary()
        o = opts or default_options()
        _chk(load().rsba_solve(self.h, C.byref(o), C.byref(s)), "rsba_solve")
        return s

    def close(self):
        if self.h:
            self.params = None
            load().rsba_problem_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Solver:
    def __init__(self, problem, opts=None):
        self.problem = problem
        self.opts = opts or default_options()
        self.h = C.c_void_p()
        self._extended = False   # what set_extended_layout() last told the library: the length of evaluate()'s gradient and set_parameters()'s vector
        _chk(load().rsba_solver_create(problem.h, C.byref(self.opts), C.byref(self.h)), "rsba_solver_create")

    def run(self):
        s = Summary()
        _chk(load().rsba_solver_run(self.h, C.byref(s)), "rsba_solver_run")
        return s

    def configure_run(self, max_num_iterations, profile_kernels=0):
        """Options of the next run() of this solver (ceres::Solve takes them per call); drops the kernel statistics."""
        _chk(load().rsba_solver_configure_run(self.h, int(max_num_iterations), int(profile_kernels)), "rsba_solver_configure_run")

    def download(self):
        _chk(load().rsba_solver_download(self.h), "rsba_solver_download")

    def iterations(self, cap=256):
        arr = (Iteration * cap)()
        n = load().rsba_solver_iterations(self.h, arr, cap)
        return np.array([[a.iteration, a.cost, a.cost_change, a.gradient_max_norm, a.step_norm, a.relative_decrease,
                          a.trust_region_radius, a.step_is_valid + 2 * a.step_is_successful] for a in arr[:n]])

    def iteration_times(self, cap=256):
        """iteration_time_in_seconds of the latest run's rows (row 0: the evaluation at the start), as the host observed them."""
        arr = (Iteration * cap)()
        n = load().rsba_solver_iterations(self.h, arr, cap)
        return np.array([a.iteration_time_in_seconds for a in arr[:n]])

    def kernel_stats(self, cap=32):
        arr = (KernelStat * cap)()
        n = load().rsba_solver_kernel_stats(self.h, arr, cap)
        return {a.name.decode(): (a.launches, a.total_ms) for a in arr[:n]}

    def comm_nranks(self):
        """ncclCommCount of the solver's communicator (1 without one)."""
        return int(load().rsba_solver_comm_nranks(self.h))

    def schedule_info(self):
        """Which schedule this solver runs and what stalled so far (rsba_schedule_info) as a dict."""
        i = ScheduleInfo()
        _chk(load().rsba_solver_schedule_info(self.h, C.byref(i)), "rsba_solver_schedule_info")
        return {"schedule": ("sequential", "pipelined", "pipelined_mg")[i.schedule], "stalls": int(i.stalls), "fallbacks": int(i.fallbacks),
                "comm_nranks": int(i.comm_nranks), "chol_workgroups": int(i.chol_workgroups), "schur_impl": int(i.schur_impl),
                "comm_kind": i.comm_kind.decode()}

    def eliminates_times(self):
        """Marker-chain models: 1 when this solver eliminates the time blocks, 0 on the dense path (rsba_solver_time_elimination)."""
        v = C.c_int32()
        _chk(load().rsba_solver_time_elimination(self.h, C.byref(v)), "rsba_solver_time_elimination")
        return int(v.value)

    def full_report(self):
        n = load().rsba_solver_full_report(self.h, None, 0)
        if n < 0:
            raise RsbaError(3, "rsba_solver_full_report")
        buf = C.create_string_buffer(n + 1)
        load().rsba_solver_full_report(self.h, buf, n + 1)
        return buf.value.decode()

    # ---- covariance of the solution (ceres::Covariance)
    def covariance_compute(self, **opts):
        """(J'J)^-1 at the solver's current parameters.  opts: min_reciprocal_condition_number, apply_loss_function.
        Raises RsbaError with code ERR_RANK_DEFICIENT when J'J is singular."""
        o = CovarianceOptions()
        load().rsba_covariance_options_default(C.byref(o))
        for k, v in opts.items():
            setattr(o, k, v)
        _chk(load().rsba_solver_covariance_compute(self.h, C.byref(o)), "rsba_solver_covariance_compute")

    def covariance_block(self, offset_a, offset_b):
        """Covariance block of the parameter blocks at offsets a and b (camera_offset / point_offset)."""
        na, nb = self._block_size(offset_a), self._block_size(offset_b)
        out = np.zeros((na, nb))
        _chk(load().rsba_solver_covariance_block(self.h, int(offset_a), int(offset_b), _vp(out)), "rsba_solver_covariance_block")
        return out

    def point_covariances(self):
        """P x 3 x 3 marginals of the points, in the problem's point order."""
        out = np.zeros((self.problem.num_points, 3, 3))
        _chk(load().rsba_solver_point_covariances(self.h, _vp(out)), "rsba_solver_point_covariances")
        return out

    def covariance_blocks(self, pairs):
        """Covariance blocks of ANY pairs of parameter blocks, in one call: pairs = [(offset_a, offset_b), ...] (camera_offset,
        point_offset, time_offset, marker_offset) -> a list of (na, nb) arrays.  The general query: time blocks, camera x point
        and point x point' pairs included; a constant block gives zeros."""
        pairs = [(int(a), int(b)) for a, b in pairs]
        n = len(pairs)
        oa = np.array([a for a, _ in pairs], np.int64).reshape(n)
        ob = np.array([b for _, b in pairs], np.int64).reshape(n)
        out = np.zeros((max(n, 1), 36))
        _chk(load().rsba_solver_covariance_blocks(self.h, n, _vp(oa) if n else _vp(np.zeros(1, np.int64)), _vp(ob) if n else _vp(np.zeros(1, np.int64)),
                                                  _vp(out)), "rsba_solver_covariance_blocks")
        res = []
        for i, (a, b) in enumerate(pairs):
            na, nb = self._block_size(a), self._block_size(b)
            res.append(out[i, :na * nb].reshape(na, nb).copy())
        return res

    def time_covariances(self):
        """Marker-chain models: T x 6 x 6 marginals of the time blocks, in the problem's time order (zeros for constant and
        unreferenced times)."""
        out = np.zeros((self.problem.num_times, 6, 6))
        _chk(load().rsba_solver_time_covariances(self.h, _vp(out)), "rsba_solver_time_covariances")
        return out

    def camera_offset(self, camera_idx):
        return 6 * int(camera_idx)

    def point_offset(self, point_idx):
        return 6 * self.problem.num_cameras + 3 * int(point_idx)

    def time_offset(self, time_idx):
        return 6 * (self.problem.num_cameras + int(time_idx))

    def marker_offset(self, marker_idx):
        return 6 * (self.problem.num_cameras + self.problem.num_times + int(marker_idx))

    # ---- free intrinsics: the extended layout (rsba_solver_set_extended_layout)
    def set_extended_layout(self, on=True):
        """A marker-chain solver with free intrinsics: evaluate(), set_parameters() and the covariance calls index the solver's
        state layout — the problem's parameters, then fx fy cx cy k1 k2 of every camera index (intrinsics_offset).  Off (the
        default): those calls are refused on such a solver.  Drops a covariance result; the run's bits do not change."""
        _chk(load().rsba_solver_set_extended_layout(self.h, 1 if on else 0), "rsba_solver_set_extended_layout")
        self._extended = bool(on)

    def num_extended_parameters(self):
        n = int(load().rsba_solver_num_extended_parameters(self.h))
        if n < 0:
            raise RsbaError(-n, "rsba_solver_num_extended_parameters")
        return n

    def intrinsics_offset(self, camera_idx):
        """The offset of camera camera_idx's intrinsics block under the extended layout."""
        return self.problem.num_parameters + 6 * int(camera_idx)

    def _num_values(self):
        return self.num_extended_parameters() if self._extended else self.problem.num_parameters

    def _block_size(self, offset):
        if self.problem.model == MODEL_POINTS and offset >= 6 * self.problem.num_cameras:
            return 3
        return 6

    # ---- ceres::Problem::Evaluate (the Jacobian: jacobian_structure / evaluate_jacobian) and values changed in place
    @property
    def num_residuals(self):
        return int(load().rsba_solver_num_residuals(self.h))

    def evaluate(self, residuals=True, gradient=True, apply_loss_function=True):
        """(cost, residuals, gradient) at the solver's current parameters; None for an output not asked for.  Residuals in the
        problem's observation order, the gradient in its parameter layout (0.0 for constant, unreferenced and base blocks)."""
        o = EvaluateOptions()
        load().rsba_evaluate_options_default(C.byref(o))
        o.apply_loss_function = 1 if apply_loss_function else 0
        cost = C.c_double()
        r = np.zeros(self.num_residuals) if residuals else None
        g = np.zeros(self._num_values()) if gradient else None
        _chk(load().rsba_solver_evaluate(self.h, C.byref(o), C.byref(cost), _vp(r) if residuals else None, _vp(g) if gradient else None),
             "rsba_solver_evaluate")
        return cost.value, r, g

    def jacobian_structure(self):
        """((rows, cols), indptr int64, indices int32) of the Jacobian of evaluate()'s residuals: compressed rows in the problem's
        observation order, column index = parameter offset; constant and base blocks are structurally absent.  The triple
        (values, indices, indptr) is what a CSR constructor takes."""
        nr, nc, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(load().rsba_solver_jacobian_structure(self.h, C.byref(nr), C.byref(nc), C.byref(nnz), None, None), "rsba_solver_jacobian_structure")
        indptr, indices = np.zeros(nr.value + 1, np.int64), np.zeros(nnz.value, np.int32)
        _chk(load().rsba_solver_jacobian_structure(self.h, None, None, None, _vp(indptr), _vp(indices)), "rsba_solver_jacobian_structure")
        return (int(nr.value), int(nc.value)), indptr, indices

    def evaluate_jacobian(self, apply_loss_function=True):
        """The values of that matrix at the solver's current parameters, in the structure's order."""
        o = EvaluateOptions()
        load().rsba_evaluate_options_default(C.byref(o))
        o.apply_loss_function = 1 if apply_loss_function else 0
        nnz = C.c_int64()
        _chk(load().rsba_solver_jacobian_structure(self.h, None, None, C.byref(nnz), None, None), "rsba_solver_jacobian_structure")
        values = np.zeros(max(nnz.value, 1))   # (never a NULL pointer: an empty matrix is no argument error)
        _chk(load().rsba_solver_evaluate_jacobian(self.h, C.byref(o), _vp(values)), "rsba_solver_evaluate_jacobian")
        return values[:nnz.value]

    def set_parameters(self, x):
        """New values for every parameter (the problem's layout; under the extended layout the cameras' six values behind it): the
        start of the next run() and the current state that evaluate(), covariance_compute() and download() read.  Nothing is
        planned again."""
        x = np.ascontiguousarray(x, np.float64)
        if x.shape != (self._num_values(),):
            raise ValueError("set_parameters: %d values expected" % self._num_values())
        _chk(load().rsba_solver_set_parameters(self.h, _vp(x)), "rsba_solver_set_parameters")

    def set_observation_weights(self, w):
        """New weights (one per residual block, >= 0) for the next run(), evaluate() or covariance_compute() of a marker-chain
        solver that was created with a robust loss or from a problem that carried weights; parameters, log and summary stay."""
        w = np.ascontiguousarray(w, np.float64)
        if w.shape != (self.problem.num_observations,):
            raise ValueError("set_observation_weights: %d values expected" % self.problem.num_observations)
        _chk(load().rsba_solver_set_observation_weights(self.h, _vp(w)), "rsba_solver_set_observation_weights")

    def set_block_prior(self, parameter_offset, A, b):
        """New (A, b) for a block that had a prior when the solver was created, for the next run(), evaluate(), Jacobian or
        covariance_compute(); parameters, log and summary stay."""
        A, b = _prior_arrays(A, b)
        _chk(load().rsba_solver_set_block_prior(self.h, parameter_offset, _vp(A), _vp(b)), "rsba_solver_set_block_prior")

    def final_costs(self):
        c, ss = C.c_double(), C.c_double()
        _chk(load().rsba_solver_final_costs(self.h, C.byref(c), C.byref(ss)), "rsba_solver_final_costs")
        return c.value, ss.value

    def close(self):
        if self.h:
            load().rsba_solver_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def solve_points(prob, opts=None):
    """dict from synthetic.make_problem -> (parameters, Summary, iteration log)."""
    p = Problem.points(prob)
    o = opts or default_options(huber_delta=prob.get("huber_delta", 0.0))
    sv = Solver(p, o)
    try:
        s = sv.run()
        sv.download()
        log = sv.iterations()
        return p.params.copy(), s, log
    finally:
        sv.close()
        p.close()


def points_linearize_and_step(prob, radius, opts=None):
    p = Problem.points(prob)
    nc, n = 6 * prob["C"], 6 * prob["C"] + 3 * prob["P"]
    S, rhs, delta, scal = np.zeros((nc, nc)), np.zeros(nc), np.zeros(n), np.zeros(8)
    o = opts or default_options()
    try:
        _chk(load().rsba_points_linearize_and_step(p.h, C.byref(o), radius, _vp(S), _vp(rhs), _vp(delta), _vp(scal)),
             "rsba_points_linearize_and_step")
    finally:
        p.close()
    return dict(S=S, rhs=rhs, delta=delta, cost=scal[0], model_cost_change=scal[1], gradient_max_norm=scal[2],
                solve_ok=bool(scal[3]), cost_candidate=scal[4], step_norm=scal[5], x_norm=scal[6])


# rsba_points_solve_stage's path scalars (include/rsba.h)
STAGE_FACTORISATIONS = ("one_wg", "diag", "diag_border", "tiles_small", "tiled", "multi_launch")
STAGE_BACKSUBS = ("in_kernel", "one_wg", "multi", "chain")


def points_solve_stage(prob, radius, opts=None):
    """The first step rsba_solver_run takes on this problem (its own schedule and factorisation): S, rhs, dcam, scale_c, delta,
    the step's scalars and the path that ran."""
    p = Problem.points(prob)
    nc, n = 6 * prob["C"], 6 * prob["C"] + 3 * prob["P"]
    S, rhs, dcam, scale_c, delta, scal = np.zeros((nc, nc)), np.zeros(nc), np.zeros(nc), np.zeros(nc), np.zeros(n), np.zeros(17)
    o = opts or default_options()
    try:
        _chk(load().rsba_points_solve_stage(p.h, C.byref(o), radius, _vp(S), _vp(rhs), _vp(dcam), _vp(scale_c), _vp(delta), _vp(scal)),
             "rsba_points_solve_stage")
    finally:
        p.close()
    path = dict(schedule="pipelined" if scal[8] else "sequential", factorisation=STAGE_FACTORISATIONS[int(scal[9])],
                workgroups=int(scal[10]), border_cols=int(scal[11]), tiles=int(scal[12]), backsub=STAGE_BACKSUBS[int(scal[13])],
                sys_fused=bool(scal[14]), stalls=int(scal[15]), fallbacks=int(scal[16]))
    return dict(S=S, rhs=rhs, dcam=dcam, scale_c=scale_c, delta=delta, cost=scal[0], model_cost_change=scal[1],
                gradient_max_norm=scal[2], solve_ok=bool(scal[3]), cost_candidate=scal[4], step_norm=scal[5], x_norm=scal[6],
                path=path)


def points_linearize_payload(prob, radius, opts=None):
    """The all-reduce payload of one linearisation (see rsba.h); returns (payload without the last value, max |g_p|)."""
    problem = Problem.points(prob)
    o = opts or default_options()
    n = C.c_int64()
    _chk(load().rsba_points_linearize_payload(problem.h, C.byref(o), C.c_double(radius), None, 0, C.byref(n)), "rsba_points_linearize_payload")
    buf = np.zeros(n.value)
    _chk(load().rsba_points_linearize_payload(problem.h, C.byref(o), C.c_double(radius), _vp(buf), n.value, C.byref(n)), "rsba_points_linearize_payload")
    problem.close()
    return buf[:-1], buf[-1]


def comm_unique_id():
    buf = (C.c_char * 128)()
    _chk(load().rsba_comm_unique_id(buf), "rsba_comm_unique_id")
    return bytes(buf)


def comm_loopback_id():
    """Id of a loopback group: the ranks are solvers of this process on one GPU (rsba.h)."""
    buf = (C.c_char * 128)()
    _chk(load().rsba_comm_loopback_id(buf), "rsba_comm_loopback_id")
    return bytes(buf)


def comm_shm_id(name):
    """128-byte id of a SHARED-MEMORY group: the ranks are processes on one host (one GPU or several); `name` must be the same
    string on every rank and unique per group (rsba_comm_shm_id)."""
    buf = (C.c_char * 128)()
    _chk(load().rsba_comm_shm_id(name.encode(), buf), "rsba_comm_shm_id")
    return bytes(buf)


def solve_points_sharded_loopback(shards, opts_kw=None, max_iterations=None):
    """The multi-rank schedule on ONE GPU: shard r of `shards` (dicts from synthetic.make_problem(..., point_range=...), all
    with the same cameras) is rank r of a loopback group, created and run by its own host thread, as one process per GPU
    would.  Returns a list of (parameters, Summary, iteration log, comm_nranks) per rank; raises if a rank failed."""
    import threading
    world = len(shards)
    uid = C.create_string_buffer(comm_loopback_id(), 128)
    out, err = [None] * world, [None] * world

    def rank_main(r):
        p = sv = None
        try:
            o = default_options(rank=r, world_size=world, **(opts_kw or {}))
            o.comm_unique_id = C.cast(uid, C.c_void_p)
            p = Problem.points(shards[r])
            sv = Solver(p, o)
            if max_iterations is not None:
                sv.configure_run(max_iterations)
            nr = sv.comm_nranks()
            s = sv.run()
            sv.download()
            out[r] = (p.params.copy(), s, sv.iterations(), nr)
        except Exception as e:  # noqa: BLE001 (reported by the caller's thread)
            err[r] = e
        finally:
            if sv is not None:
                sv.close()
            if p is not None:
                p.close()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for r, e in enumerate(err):
        if e is not None:
            raise RuntimeError("loopback rank %d failed: %s" % (r, e))
    return out


class ShardedLoopbackGroup:
    """A loopback group that stays alive between calls: shard r of `shards` is rank r, its problem and solver created, used and
    closed by ONE host thread of its own, as one process per GPU would.  `prepare(r, problem)` runs before rank r's solver is
    created (constant blocks).  `run(fn)` calls fn(r, solver, problem) on every rank's thread against the live solver and returns
    the per-rank results in rank order — what the collective entry points (run, evaluate, set_parameters, covariance_compute)
    need: every rank calling, in the same order.  If fn raises on a rank, that rank aborts the group's communicator
    (rsba_solver_comm_abort), so no other rank is left waiting in a collective, and run() re-raises in the caller; the group is
    then good for close() only.  An error code that the ranks share (RSBA_ERR_ARG after a refused request) is no reason to raise:
    let fn catch it and return the code.  Use as a context manager, or call close()."""

    def __init__(self, shards, opts_kw=None, prepare=None):
        import queue
        import threading
        self.world = len(shards)
        self.solvers, self.problems = [None] * self.world, [None] * self.world
        self._uid = C.create_string_buffer(comm_loopback_id(), 128)
        self._jobs = [queue.Queue() for _ in range(self.world)]
        self._done = queue.Queue()
        self._failed = False
        self._threads = [threading.Thread(target=self._rank_main, args=(r, shards[r], dict(opts_kw or {}), prepare)) for r in range(self.world)]
        for t in self._threads:
            t.start()
        try:
            self._collect()
        except Exception:
            self.close()
            raise

    def _create(self, r, shard, opts_kw, prepare):
        o = default_options(rank=r, world_size=self.world, **opts_kw)
        o.comm_unique_id = C.cast(self._uid, C.c_void_p)
        self.problems[r] = Problem.points(shard)
        if prepare is not None:
            prepare(r, self.problems[r])
        self.solvers[r] = Solver(self.problems[r], o)

    def _rank_main(self, r, shard, opts_kw, prepare):
        fn = lambda *_: self._create(r, shard, opts_kw, prepare)  # noqa: E731
        while fn is not None:
            try:
                self._done.put((r, fn(r, self.solvers[r], self.problems[r]), None))
            except Exception as e:  # noqa: BLE001 (re-raised by the caller's thread)
                if self.solvers[r] is not None:
                    load().rsba_solver_comm_abort(self.solvers[r].h)
                self._done.put((r, None, e))
            fn = self._jobs[r].get()
        for h in (self.solvers[r], self.problems[r]):
            if h is not None:
                h.close()

    def _collect(self):
        out, err = [None] * self.world, [None] * self.world
        for _ in range(self.world):
            r, res, e = self._done.get()
            out[r], err[r] = res, e
        bad = [(r, e) for r, e in enumerate(err) if e is not None]
        if bad:
            self._failed = True
            # the rank that gave up first, not the ones its abort released (RSBA_ERR_COMM)
            bad.sort(key=lambda re: isinstance(re[1], RsbaError) and re[1].code == ERR_COMM)
            raise RuntimeError("loopback rank %d failed: %s" % bad[0]) from bad[0][1]
        return out

    def run(self, fn):
        if self._failed or self._threads is None:
            raise RuntimeError("the loopback group has failed or is closed")
        for q in self._jobs:
            q.put(fn)
        return self._collect()

    def close(self):
        if self._threads is not None:
            for q in self._jobs:
                q.put(None)
            for t in self._threads:
                t.join()
            self._threads = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_intrinsics_xml(path):
    out = np.zeros(4)
    _chk(load().rsba_read_intrinsics_xml(path.encode(), _vp(out)), "rsba_read_intrinsics_xml")
    return out


def read_intrinsics_xml_dist(path):
    """(fx, fy, ppx, ppy), (k1, k2, p1, p2, k3) of an OpenCV FileStorage XML with <intrinsics> and, optionally, <distCoeffs>."""
    k, d = np.zeros(4), np.zeros(5)
    _chk(load().rsba_read_intrinsics_xml_dist(str(path).encode(), _vp(k), _vp(d)), "rsba_read_intrinsics_xml_dist")
    return k, d


def undistort_points(image_points, intrinsics4, dist5):
    """Pixel coordinates of distorted detections (n x 2) -> pixel coordinates of the ideal pinhole camera with the same intrinsics."""
    img = np.ascontiguousarray(image_points, np.float64).reshape(-1, 2)
    k, d = np.ascontiguousarray(intrinsics4, np.float64), np.ascontiguousarray(dist5, np.float64)
    if k.size != 4 or d.size != 5:
        raise ValueError("undistort_points: 4 intrinsics and 5 coefficients expected")
    out = np.zeros_like(img)
    _chk(load().rsba_undistort_points(len(img), _vp(img), _vp(k), _vp(d), _vp(out)), "rsba_undistort_points")
    return out


def reprojection_check_files(correspondence_txt, point3d_txt, camera_transform_xml, intrinsics):
    """ReprojectionCheck::Reproject from its files (reprojection_check.cpp:5-101); returns (error, rms)."""
    intr = np.ascontiguousarray(intrinsics, dtype=np.float64)
    err, rms = C.c_double(), C.c_double()
    _chk(load().rsba_reprojection_check_files(str(correspondence_txt).encode(), str(point3d_txt).encode(),
                                               str(camera_transform_xml).encode(), _vp(intr), C.byref(err), C.byref(rms)),
         "rsba_reprojection_check_files")
    return err.value, rms.value


def _pose_op(fn, a, b):
    a, b, out = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64), np.zeros(6)
    _chk(fn(_vp(a), _vp(b), _vp(out)), "pose composition")
    return out


def base_pose_from_marker_detection(marker_from_camera, marker_from_base):
    return _pose_op(load().rsba_base_pose_from_marker_detection, marker_from_camera, marker_from_base)


def marker_pose_in_camera(base_from_camera, marker_from_base):
    return _pose_op(load().rsba_marker_pose_in_camera, base_from_camera, marker_from_base)


def marker_corners_in_camera(pose, marker_side):
    pose, out = np.ascontiguousarray(pose, np.float64), np.zeros((4, 3))
    _chk(load().rsba_marker_corners_in_camera(_vp(pose), C.c_double(marker_side), _vp(out)), "rsba_marker_corners_in_camera")
    return out


def marker_pose_from_corners(corners8, intrinsics4, dist5, marker_side):
    """One detection's pose on the host (aruco::estimatePoseSingleMarkers): corners 4 x (u, v), top-left first, clockwise; dist5 may be
    None.  Returns (pose6, rms, status); a degenerate detection raises RsbaError with code ERR_UNSUPPORTED."""
    c = np.ascontiguousarray(corners8, np.float64).reshape(-1)
    k = np.ascontiguousarray(intrinsics4, np.float64).reshape(-1)
    d = None if dist5 is None else np.ascontiguousarray(dist5, np.float64).reshape(-1)
    if c.size != 8 or k.size != 4 or (d is not None and d.size != 5):
        raise ValueError("marker_pose_from_corners: 8 corner values, 4 intrinsics and 5 coefficients (or None) expected")
    pose, rms, status = np.zeros(6), C.c_double(), C.c_int32()
    _chk(load().rsba_marker_pose_from_corners(_vp(c), _vp(k), None if d is None else _vp(d), C.c_double(marker_side), _vp(pose), C.byref(rms),
                                              C.byref(status)), "rsba_marker_pose_from_corners")
    return pose, rms.value, int(status.value)


def marker_pose_from_corners_both(corners8, intrinsics4, dist5, marker_side):
    """Both poses of one planar marker on the host (rsba_marker_pose_from_corners_both): solution 0 is marker_pose_from_corners', solution
    1 the minimiser reached from its mirror image.  Returns (poses 2 x 6, rms 2, status 2), in that fixed order; solution 1 has status 2
    (unusable start) or 3 (MARKER_POSE_SAME: it ended at solution 0) with pose zeros and rms -1 where there is no second solution.  A
    degenerate solution 0 raises RsbaError with code ERR_UNSUPPORTED."""
    c = np.ascontiguousarray(corners8, np.float64).reshape(-1)
    k = np.ascontiguousarray(intrinsics4, np.float64).reshape(-1)
    d = None if dist5 is None else np.ascontiguousarray(dist5, np.float64).reshape(-1)
    if c.size != 8 or k.size != 4 or (d is not None and d.size != 5):
        raise ValueError("marker_pose_from_corners_both: 8 corner values, 4 intrinsics and 5 coefficients (or None) expected")
    poses, rms, status = np.zeros((2, 6)), np.zeros(2), np.zeros(2, np.int32)
    _chk(load().rsba_marker_pose_from_corners_both(_vp(c), _vp(k), None if d is None else _vp(d), C.c_double(marker_side), _vp(poses), _vp(rms),
                                                   _vp(status)), "rsba_marker_pose_from_corners_both")
    return poses, rms, status


def marker_poses_from_corners_both(corners, camera_index, intrinsics, dist, marker_side, device=-1, num_cameras=None):
    """marker_pose_from_corners_both for a batch on the GPU, two kernel launches.  Arguments as marker_poses_from_corners.  Returns
    (poses n x 2 x 6, rms n x 2, status n x 2); a degenerate detection has statuses (2, 2)."""
    c = np.ascontiguousarray(corners, np.float64).reshape(-1, 8)
    k = np.ascontiguousarray(intrinsics, np.float64).reshape(-1, 4)
    nc = len(k) if num_cameras is None else int(num_cameras)
    d = None if dist is None else np.ascontiguousarray(dist, np.float64).reshape(-1, 5)
    ci = None if camera_index is None else np.ascontiguousarray(camera_index, np.int32).reshape(-1)
    if len(k) != nc or (d is not None and len(d) != nc) or (ci is not None and len(ci) != len(c)):
        raise ValueError("marker_poses_from_corners_both: one camera index per detection, 4 intrinsics and 5 coefficients per camera expected")
    n = len(c)
    poses, rms, status = np.zeros((n, 2, 6)), np.zeros((n, 2)), np.zeros((n, 2), np.int32)
    _chk(load().rsba_marker_poses_from_corners_both(n, _vp(c), None if ci is None else _vp(ci), nc, _vp(k), None if d is None else _vp(d),
                                                    C.c_double(marker_side), int(device), _vp(poses), _vp(rms), _vp(status)),
         "rsba_marker_poses_from_corners_both")
    return poses, rms, status


def marker_poses_from_corners(corners, camera_index, intrinsics, dist, marker_side, device=-1, num_cameras=None):
    """A batch of detections on the GPU, one kernel launch: corners n x 8, camera_index n (None: all camera 0), intrinsics C x 4, dist
    C x 5 or None.  Returns (poses n x 6, rms n, status n); a degenerate detection has status 2, pose zeros and rms -1."""
    c = np.ascontiguousarray(corners, np.float64).reshape(-1, 8)
    k = np.ascontiguousarray(intrinsics, np.float64).reshape(-1, 4)
    nc = len(k) if num_cameras is None else int(num_cameras)
    d = None if dist is None else np.ascontiguousarray(dist, np.float64).reshape(-1, 5)
    ci = None if camera_index is None else np.ascontiguousarray(camera_index, np.int32).reshape(-1)
    if len(k) != nc or (d is not None and len(d) != nc) or (ci is not None and len(ci) != len(c)):
        raise ValueError("marker_poses_from_corners: one camera index per detection, 4 intrinsics and 5 coefficients per camera expected")
    n = len(c)
    poses, rms, status = np.zeros((n, 6)), np.zeros(n), np.zeros(n, np.int32)
    _chk(load().rsba_marker_poses_from_corners(n, _vp(c), None if ci is None else _vp(ci), nc, _vp(k), None if d is None else _vp(d),
                                               C.c_double(marker_side), int(device), _vp(poses), _vp(rms), _vp(status)),
         "rsba_marker_poses_from_corners")
    return poses, rms, status


def solve_pnp_epnp(object_points, image_points, intrinsics4):
    obj = np.ascontiguousarray(object_points, np.float64).reshape(-1, 3)
    img = np.ascontiguousarray(image_points, np.float64).reshape(-1, 2)
    k, out = np.ascontiguousarray(intrinsics4, np.float64), np.zeros(6)
    _chk(load().rsba_solve_pnp_epnp(len(obj), _vp(obj), _vp(img), _vp(k), _vp(out)), "rsba_solve_pnp_epnp")
    return out
