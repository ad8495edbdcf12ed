"""ctypes binding of the C-ABI (include/clc.h) exported by csrc/libclc_hip.so.

There is no CPU fallback: if the HIP extension is missing this module raises on first use,
and every entry point that needs the device raises when no gfx950 GPU is present."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _build

CLC_OK = 0
ERRORS = {
    -1: "CLC_ERR_INVALID_ARG", -2: "CLC_ERR_HIP", -3: "CLC_ERR_NONFINITE", -4: "CLC_ERR_EMPTY_SCAN",
    -5: "CLC_ERR_NO_DATA", -6: "CLC_ERR_LINALG", -7: "CLC_ERR_NO_DEVICE", -8: "CLC_ERR_COMM",
}
TERMINATION = {
    0: "RUNNING", 1: "CONVERGENCE(gradient)", 2: "CONVERGENCE(parameter)", 3: "CONVERGENCE(function)",
    4: "CONVERGENCE(radius)", 5: "NO_CONVERGENCE", 6: "FAILURE",
}

# every symbol include/clc.h declares (checked by tests/test_abi_symbols.py)
EXPORTED = [
    "clc_version", "clc_last_error", "clc_options_default", "clc_create", "clc_destroy", "clc_set_stream",
    "clc_set_launch", "clc_set_auto_paths", "clc_set_small_on_coop", "clc_flatten_observations", "clc_upload", "clc_upload_device", "clc_num_observations",
    "clc_factor_evaluate", "clc_pose_plus", "clc_pose_plus_jacobian", "clc_eval", "clc_solve",
    "clc_information", "clc_closed_form", "clc_upload_batched", "clc_solve_batched", "clc_solve_multistart", "clc_num_problems",
    "clc_line_options_default", "clc_line_fit_batched", "clc_scan_to_points",
    "clc_comm_unique_id", "clc_comm_create", "clc_comm_destroy", "clc_comm_rank", "clc_comm_world",
    "clc_gather_results", "clc_comm_records", "clc_solve_batched_gather", "clc_comm_set_root", "clc_comm_get_info",
    "clc_solve_batched_gather_pipelined", "clc_gather_flush",
    "clc_store_observations", "clc_select_observations", "clc_upload_batched_device", "clc_line_fit_batched_device",
    "clc_scan_to_points_device", "clc_pinned_alloc", "clc_pinned_free", "clc_store_generation", "clc_batched_host_buffers",
    "clc_get_path_info", "clc_device_info", "clc_comm_library", "clc_board_segments", "clc_board_segments_device",
    "clc_closed_form_batched", "clc_information_batched",
    "clc_pose_options_default", "clc_camera_lift", "clc_camera_project", "clc_board_poses", "clc_board_poses_device",
    "clc_robust_pose_options_default", "clc_board_poses_robust", "clc_board_poses_robust_device",
    "clc_alt_pose_options_default", "clc_board_poses_alternate", "clc_board_poses_alternate_device",
    "clc_joint_options_default", "clc_joint_refine", "clc_joint_refine_device",
    "clc_camcal_options_default", "clc_camera_guess", "clc_camera_guess_device", "clc_camera_calibrate", "clc_camera_calibrate_device",
    "clc_guidance_options_default", "clc_score_board_poses", "clc_score_board_poses_device", "clc_select_board_poses",
    "clc_select_board_poses_device",
    "clc_range_options_default", "clc_joint_refine_range", "clc_joint_refine_range_device", "clc_range_correct", "clc_range_correct_device",
    "clc_joint_loss_options_default", "clc_joint_refine_robust", "clc_joint_refine_robust_device",
    "clc_full_options_default", "clc_calibrate_full", "clc_calibrate_full_device",
    "clc_solve_subsets", "clc_score_blocks",
    "clc_assemble_options_default", "clc_keyframes", "clc_assemble_observations", "clc_assemble_observations_device",
    "clc_stored_observations",
    "clc_station_options_default", "clc_static_poses", "clc_assemble_stations", "clc_assemble_stations_device",
    "clc_subpix_options_default", "clc_corner_subpix", "clc_corner_subpix_device",
    "clc_chess_options_default", "clc_chessorder_options_default", "clc_chess_corners", "clc_chess_corners_device",
    "clc_chessboard_order", "clc_find_chessboard",
    "clc_chessboard_order_device", "clc_find_chessboard_device", "clc_find_chessboard_gpu",
    "clc_tag_options_default", "clc_tag_grid", "clc_tag_grid_device", "clc_tag_grid_points_device",
    "clc_interp_options_default", "clc_interpolate_poses", "clc_assemble_interpolated", "clc_assemble_interpolated_device",
    "clc_clock_offset_options_default", "clc_clock_offset_best", "clc_clock_offset_sweep", "clc_clock_offset_sweep_device",
]
# test / profiling hooks: NOT in include/clc.h and not in the product library; exported by the -DCLC_TEST_HOOKS builds
# (csrc/libclc_hip_hooks.so) only (tests/test_abi_symbols.py checks both directions)
HOOKS = [
    "clc_debug_flatten_device", "clc_debug_math", "clc_debug_wave_reduce", "clc_debug_build_features", "clc_debug_rows",
    "clc_debug_wave_split", "clc_debug_resident", "clc_debug_resident_single", "clc_debug_coop", "clc_debug_coop_control",
    "clc_debug_coop_set_tag", "clc_debug_layout", "clc_debug_lm_profile", "clc_time_steps", "clc_time_batched_eval", "clc_time_eval",
    "clc_debug_comm_create_layout", "clc_debug_single_controller", "clc_debug_fast_small",
    "clc_debug_lane_map_builds", "clc_debug_assemble_lines", "clc_debug_station_walk", "clc_debug_sweep_records",
    "clc_debug_guidance_dirs", "clc_debug_guidance_score_rows",
]


class Options(C.Structure):
    _fields_ = [
        ("max_num_iterations", C.c_int32),
        ("max_num_consecutive_invalid_steps", C.c_int32),
        ("jacobi_scaling", C.c_int32),
        ("use_loss", C.c_int32),
        ("loss_scale_factor", C.c_double),
        ("initial_trust_region_radius", C.c_double),
        ("max_trust_region_radius", C.c_double),
        ("min_trust_region_radius", C.c_double),
        ("min_relative_decrease", C.c_double),
        ("min_lm_diagonal", C.c_double),
        ("max_lm_diagonal", C.c_double),
        ("function_tolerance", C.c_double),
        ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double),
        ("launch_ahead", C.c_int32),
        ("profile_events", C.c_int32),
    ]


class Iteration(C.Structure):
    _fields_ = [
        ("iteration", C.c_int32),
        ("step_is_valid", C.c_int32),
        ("step_is_successful", C.c_int32),
        ("pad_", C.c_int32),
        ("cost", C.c_double),
        ("cost_change", C.c_double),
        ("gradient_max_norm", C.c_double),
        ("step_norm", C.c_double),
        ("relative_decrease", C.c_double),
        ("trust_region_radius", C.c_double),
    ]


class Summary(C.Structure):
    _fields_ = [
        ("termination", C.c_int32),
        ("num_iterations", C.c_int32),
        ("num_successful_steps", C.c_int32),
        ("num_unsuccessful_steps", C.c_int32),
        ("num_evaluations", C.c_int64),
        ("initial_cost", C.c_double),
        ("final_cost", C.c_double),
        ("solve_ms", C.c_double),
        ("eval_kernel_ms", C.c_double),
        ("eval_kernel_launches", C.c_int64),
    ]


class BatchStats(C.Structure):
    """clc_batch_stats (include/clc.h): the local shard's totals of one clc_solve_batched_gather."""
    _fields_ = [("problems", C.c_int64), ("evaluations", C.c_int64), ("iterations", C.c_int64), ("not_converged", C.c_int64),
                ("fused", C.c_int32), ("pad_", C.c_int32), ("kernel_ms", C.c_double), ("solve_ms", C.c_double)]


class CommInfo(C.Structure):
    """clc_comm_info (include/clc.h)."""
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "rank", "world", "root", "rooted_collective_available", "copies_other_ranks_to_host",
                                         "step_in_flight", "pad_")] + \
               [(n, C.c_int64) for n in ("collectives", "rooted_collectives", "host_copies", "host_copy_bytes", "pipelined_steps")]


class PathInfo(C.Structure):
    """clc_path_info (include/clc.h)."""
    _fields_ = [(n, C.c_int32) for n in ("single_resident", "single_lanes", "single_points_per_lane", "coop_resident", "coop_points_per_lane",
                                         "coop_points_carry_z", "coop_resting", "coop_timeouts", "batched_resident", "batched_lanes", "batched_points_per_lane",
                                         "rows_layout", "batched_rows_layout", "coop_workgroups", "batched_points_carry_z", "reserved_")] + \
               [(n, C.c_int64) for n in ("coop_solves", "batched_lane_rows", "n_rows", "batched_n_rows", "coop_gate_waits_expired")]


class AssembleOptions(C.Structure):
    """clc_assemble_options (include/clc.h)."""
    _fields_ = [("keyframe_dist_min", C.c_double), ("keyframe_theta_min", C.c_double), ("max_dt", C.c_double), ("line0", C.c_double * 2),
                ("line", Options)]


class AssembleInfo(C.Structure):
    """clc_assemble_info (include/clc.h)."""
    _fields_ = [(n, C.c_int64) for n in ("n_keyframes", "n_segments", "n_ref_throws", "n_unmatched", "n_observations", "n_points",
                                         "n_line_points")]


SCAN_NO_SEGMENT, SCAN_REF_THROWS, SCAN_NO_POSE = -1, -2, -3  # CLC_SCAN_*


class StationOptions(C.Structure):
    """clc_station_options (include/clc.h)."""
    _fields_ = [("center_dist_max", C.c_double), ("min_members", C.c_int64), ("close_last_run", C.c_int32), ("reserved", C.c_int32),
                ("line0", C.c_double * 2), ("line", Options)]


class StationInfo(C.Structure):
    """clc_station_info (include/clc.h)."""
    _fields_ = [(n, C.c_int64) for n in ("n_runs", "n_stations", "n_nonfinite", "n_segments", "n_ref_throws", "n_unmatched", "n_observations",
                                         "n_points", "n_line_points")]


STATION_OK, STATION_NONFINITE = 1, -1  # CLC_STATION_*


class InterpOptions(C.Structure):
    """clc_interp_options (include/clc.h)."""
    _fields_ = [("time_offset", C.c_double), ("max_gap", C.c_double), ("line0", C.c_double * 2), ("line", Options)]


class RobustPoseOptions(C.Structure):
    """clc_robust_pose_options (include/clc.h): the gates in normalized image plane units (pixels / focal)."""
    _fields_ = [("hyp_threshold", C.c_double), ("threshold", C.c_double), ("min_inliers", C.c_int32), ("max_fits", C.c_int32)]


class AltPoseOptions(C.Structure):
    """clc_alt_pose_options (include/clc.h): same_angle in rad, ratio_gate a cost ratio."""
    _fields_ = [("same_angle", C.c_double), ("ratio_gate", C.c_double)]


class JointOptions(C.Structure):
    """clc_joint_options (include/clc.h): sigma_corner in normalized image units (pixels / focal), sigma_laser in metres."""
    _fields_ = [("sigma_corner", C.c_double), ("sigma_laser", C.c_double), ("hold_board_poses", C.c_int32), ("hold_extrinsic", C.c_int32)]


class RangeOptions(C.Structure):
    """clc_range_options (include/clc.h): clc_joint_options and hold_range_mask (bit 0: the range offset is held, bit 1: the scale)."""
    _fields_ = [("sigma_corner", C.c_double), ("sigma_laser", C.c_double), ("hold_board_poses", C.c_int32), ("hold_extrinsic", C.c_int32),
                ("hold_range_mask", C.c_int32), ("reserved", C.c_int32)]


class JointLossOptions(C.Structure):
    """clc_joint_loss_options (include/clc.h): the Cauchy scales of K22 in units of sigma_corner / sigma_laser; 0: no loss."""
    _fields_ = [("loss_corner", C.c_double), ("loss_laser", C.c_double)]


class FullOptions(C.Structure):
    """clc_full_options (include/clc.h): the options of K23.  sigma_px in pixels, sigma_laser in metres; the Cauchy scales in units of
    sigma (0: no loss); bit j of hold_intrinsics_mask holds intrinsic j (proj[0..3], dist[0..3]); hold_range_mask bit 0: b, bit 1:
    kappa."""
    _fields_ = [("sigma_px", C.c_double), ("sigma_laser", C.c_double), ("loss_corner", C.c_double), ("loss_laser", C.c_double),
                ("hold_intrinsics_mask", C.c_uint32), ("hold_range_mask", C.c_int32), ("hold_board_poses", C.c_int32),
                ("hold_extrinsic", C.c_int32)]


class CamcalOptions(C.Structure):
    """clc_camcal_options (include/clc.h): sigma_px in pixels; bit j of hold_mask holds intrinsic j (proj[0..3], dist[0..3])."""
    _fields_ = [("sigma_px", C.c_double), ("hold_mask", C.c_uint32), ("hold_board_poses", C.c_int32)]


class GuidanceOptions(C.Structure):
    """clc_guidance_options (include/clc.h): the scan model, the board rectangle in board coordinates and the criterion of K20."""
    _fields_ = [("n_rays", C.c_int32), ("min_points", C.c_int32), ("angle_min", C.c_double), ("angle_increment", C.c_double),
                ("range_min", C.c_double), ("range_max", C.c_double), ("board_min", C.c_double * 2), ("board_max", C.c_double * 2),
                ("eig_floor", C.c_double), ("criterion", C.c_int32), ("reserved", C.c_int32)]


class SubpixOptions(C.Structure):
    """clc_subpix_options (include/clc.h): the half-window, the zero zone (-1: none) and the stopping rule of K24."""
    _fields_ = [("win_x", C.c_int32), ("win_y", C.c_int32), ("zero_x", C.c_int32), ("zero_y", C.c_int32), ("max_iter", C.c_int32),
                ("reserved", C.c_int32), ("eps", C.c_double)]


class ChessOptions(C.Structure):
    """clc_chess_options (include/clc.h): the threshold on R5, the suppression radius, the relative gate and the stride of K25."""
    _fields_ = [("threshold", C.c_int32), ("nms_radius", C.c_int32), ("rel_permille", C.c_int32), ("max_per_image", C.c_int32),
                ("reserved", C.c_int32)]


class ChessOrderOptions(C.Structure):
    """clc_chessorder_options (include/clc.h): the match gate of the grid ordering of K25."""
    _fields_ = [("tol", C.c_double), ("reserved", C.c_int32), ("reserved2", C.c_int32)]


class TagFamilyC(C.Structure):
    """clc_tag_family (include/clc.h): the payload side d, the border b, the code table (host memory) and the accepted distance of K27."""
    _fields_ = [("side", C.c_int32), ("border", C.c_int32), ("n_codes", C.c_int32), ("max_hamming", C.c_int32), ("codes", C.c_void_p)]


class TagOptions(C.Structure):
    """clc_tag_options (include/clc.h): the side range of a tag in pixels, the edge contrast, the border errors and the quads decoded (K27)."""
    _fields_ = [("min_side_px", C.c_int32), ("max_side_px", C.c_int32), ("contrast", C.c_int32), ("max_border_errors", C.c_int32),
                ("max_quads", C.c_int32), ("reserved", C.c_int32)]


TAG_MAX_QUADS, TAG_MAX_OUT, TAG_MAX_TAGS, TAG_MAX_CODES, TAG_OK, TAG_OVERFLOW = 1024, 4, 1024, 4096, 1, -2  # CLC_TAG_*
SUBPIX_MAX_WIN = 15  # CLC_SUBPIX_MAX_WIN
CHESS_MAX_CANDIDATES, CHESS_RAW_CAP = 1024, 4096  # CLC_CHESS_*
CHESS_OK, CHESS_FOUND, CHESS_TOO_FEW, CHESS_NO_GRID, CHESS_OVERFLOW = 1, 1, 0, -1, -2
SUBPIX_CONVERGED, SUBPIX_MAX_ITER, SUBPIX_SINGULAR, SUBPIX_LEFT_IMAGE, SUBPIX_REVERTED, SUBPIX_NONFINITE = 1, 0, -1, -2, -3, -4  # CLC_SUBPIX_*
GUIDE_LOGDET, GUIDE_MIN_EIG = 0, 1  # CLC_GUIDE_*
JOINT_OK, JOINT_TOO_FEW, JOINT_NOT_KEPT, JOINT_NONFINITE = 1, 0, -1, -2  # CLC_JOINT_*
CAMCAL_OK, CAMCAL_TOO_FEW, CAMCAL_NOT_KEPT, CAMCAL_NONFINITE = 1, 0, -1, -2  # CLC_CAMCAL_*
POSE_OK, POSE_TOO_FEW, POSE_DEGENERATE, POSE_NONFINITE, POSE_NO_CONSENSUS = 1, 0, -1, -2, -3  # CLC_POSE_*
ALT_NONE, ALT_SAME, ALT_DISTINCT = 0, 1, 2  # CLC_ALT_*


class ClcError(RuntimeError):
    def __init__(self, code: int, where: str, detail: str):
        super().__init__(f"{where}: {ERRORS.get(code, code)} — {detail}")
        self.code = code


_lib = None


def lib_path() -> str:
    return _build.LIB_PATH


def _preload_process_hip_runtime() -> None:
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so (same
    SONAME as /opt/rocm's).  If this extension pulled in the system copy first, a later
    `import torch` would find no GPUs; so when torch is installed (it is the plumbing for
    device memory / streams / torch.distributed), its runtime is loaded first and the extension
    binds to it.  CLC_HIP_RUNTIME=system skips this."""
    if os.environ.get("CLC_HIP_RUNTIME", "").lower() == "system":
        return
    import sys
    if "torch" in sys.modules:
        return  # torch already brought its runtime in
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass  # fall back to whatever the dynamic loader resolves


_libs = {}


def load(path: str):
    """Load one build of the library (cached per path) and declare the non-int signatures."""
    path = os.path.abspath(path)
    L = _libs.get(path)
    if L is None:
        if not os.path.exists(path):
            raise RuntimeError(
                f"HIP extension {path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(needs hipcc).  camlasercalibratool_amd has no CPU fallback.")
        _preload_process_hip_runtime()
        L = C.CDLL(path)
        L.clc_last_error.restype = C.c_char_p
        L.clc_num_observations.restype = C.c_size_t
        L.clc_num_problems.restype = C.c_size_t
        L.clc_num_observations.argtypes = [C.c_void_p]
        L.clc_num_problems.argtypes = [C.c_void_p]
        L.clc_destroy.argtypes = [C.c_void_p]
        L.clc_store_generation.argtypes = [C.c_void_p]
        L.clc_store_generation.restype = C.c_int64
        L.clc_destroy.restype = None
        L.clc_comm_destroy.argtypes = [C.c_void_p]
        L.clc_comm_destroy.restype = None
        L.clc_comm_rank.argtypes = [C.c_void_p]
        L.clc_comm_world.argtypes = [C.c_void_p]
        L.clc_comm_library.restype = C.c_char_p
        L.clc_solve_batched_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_size_t, C.c_void_p, C.c_void_p]
        L.clc_solve_batched_gather.restype = C.c_int
        L.clc_solve_batched_gather_pipelined.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_size_t, C.c_void_p, C.c_void_p]
        L.clc_solve_batched_gather_pipelined.restype = C.c_int
        L.clc_gather_flush.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.clc_gather_flush.restype = C.c_int
        L.clc_solve_subsets.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.c_size_t, C.POINTER(C.c_uint8),
                                        C.POINTER(C.c_double), C.c_void_p]
        L.clc_solve_subsets.restype = C.c_int
        L.clc_score_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.c_size_t, C.POINTER(C.c_double), C.c_double,
                                       C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
        L.clc_score_blocks.restype = C.c_int
        L.clc_comm_set_root.argtypes = [C.c_void_p, C.c_int]
        L.clc_comm_get_info.argtypes = [C.c_void_p, C.c_void_p]
        L.clc_comm_records.argtypes = [C.c_void_p]
        L.clc_comm_records.restype = C.POINTER(C.c_double)
        L.clc_get_path_info.argtypes = [C.c_void_p, C.c_void_p]
        P = C.POINTER
        L.clc_closed_form_batched.argtypes = [C.c_void_p, P(C.c_double), P(C.c_double), P(C.c_int32), P(C.c_double), P(C.c_int32)]
        L.clc_closed_form_batched.restype = C.c_int
        L.clc_information_batched.argtypes = [C.c_void_p, P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_double), P(C.c_double),
                                              P(C.c_double), P(C.c_int32)]
        L.clc_information_batched.restype = C.c_int
        V = C.c_void_p
        L.clc_assemble_options_default.argtypes = [V]
        L.clc_assemble_options_default.restype = None
        L.clc_keyframes.argtypes = [V, V, C.c_size_t, V, V, V, V]
        L.clc_assemble_observations.argtypes = [V, V, C.c_size_t, V, V, V, V, V, C.c_size_t, V, V, V, V, V, V]
        L.clc_assemble_observations_device.argtypes = [V, V, C.c_size_t, V, V, V, V, V, C.c_size_t, C.c_size_t, V, V, V, V, V, V]
        L.clc_stored_observations.argtypes = [V, V, V, V, V, V, V, V]
        if hasattr(L, "clc_static_poses"):  # (a build of an older tree loaded through CLC_LIBRARY has none of these)
            L.clc_station_options_default.argtypes = [V]
            L.clc_station_options_default.restype = None
            L.clc_static_poses.argtypes = [V, V, C.c_size_t, V, V, V, C.c_size_t, V, V, V, V, V, V, V, V]
            L.clc_assemble_stations.argtypes = [V, V, C.c_size_t, V, V, V, V, V, C.c_size_t, V, V, V, V, V, V]
            L.clc_assemble_stations_device.argtypes = [V, V, C.c_size_t, V, V, V, V, V, C.c_size_t, C.c_size_t, V, V, V, V, V, V]
        if hasattr(L, "clc_interpolate_poses"):
            L.clc_interp_options_default.argtypes = [V]
            L.clc_interp_options_default.restype = None
            L.clc_interpolate_poses.argtypes = [V, V, C.c_size_t, V, V, V, C.c_size_t, V, V, V, V, V]
            L.clc_assemble_interpolated.argtypes = [V, V, C.c_size_t, V, V, V, V, V, C.c_size_t, V, V, V, V, V, V, V]
            L.clc_assemble_interpolated_device.argtypes = [V, V, C.c_size_t, V, V, V, V, V, C.c_size_t, C.c_size_t, V, V, V, V, V, V, V]
            L.clc_clock_offset_options_default.argtypes = [V]
            L.clc_clock_offset_options_default.restype = None
            L.clc_clock_offset_best.argtypes = [C.c_size_t, V, V, V, V, V, V]
            L.clc_clock_offset_sweep.argtypes = [V, V, C.c_size_t, V, V, V, V, V, C.c_size_t, V, V, V, V, V, V, V, V, V, V]
            L.clc_clock_offset_sweep_device.argtypes = [V, V, C.c_size_t, V, V, V, V, V, C.c_size_t, C.c_size_t, V, V, V, V, V, V, V, V, V, V]
        if hasattr(L, "clc_board_poses_robust"):
            L.clc_robust_pose_options_default.argtypes = [V, V]
            L.clc_robust_pose_options_default.restype = None
            L.clc_board_poses_robust.argtypes = [V, V, V, V, V, V, V, C.c_size_t] + [V] * 9
            L.clc_board_poses_robust_device.argtypes = [V, V, V, V, V, V, V, C.c_size_t] + [V] * 9
        if hasattr(L, "clc_board_poses_alternate"):
            L.clc_alt_pose_options_default.argtypes = [V]
            L.clc_alt_pose_options_default.restype = None
            L.clc_board_poses_alternate.argtypes = [V, V, V, V, V, V, V, C.c_size_t] + [V] * 16
            L.clc_board_poses_alternate_device.argtypes = [V, V, V, V, V, V, V, C.c_size_t] + [V] * 16
        if hasattr(L, "clc_joint_refine"):
            L.clc_joint_options_default.argtypes = [V, V]
            L.clc_joint_options_default.restype = None
            L.clc_joint_refine.argtypes = [V] * 10 + [C.c_size_t, V, C.c_size_t] + [V] * 7
            L.clc_joint_refine_device.argtypes = [V] * 10 + [C.c_size_t, V, C.c_size_t] + [V] * 7
        if hasattr(L, "clc_joint_refine_range"):
            L.clc_range_options_default.argtypes = [V, V]
            L.clc_range_options_default.restype = None
            L.clc_joint_refine_range.argtypes = [V] * 10 + [C.c_size_t, V, C.c_size_t] + [V] * 8
            L.clc_joint_refine_range_device.argtypes = [V] * 10 + [C.c_size_t, V, C.c_size_t] + [V] * 8
            L.clc_range_correct.argtypes = [V, V, V, C.c_size_t, V]
            L.clc_range_correct_device.argtypes = [V, V, V, C.c_size_t, V]
        if hasattr(L, "clc_joint_refine_robust"):
            L.clc_joint_loss_options_default.argtypes = [V, V]
            L.clc_joint_loss_options_default.restype = None
            L.clc_joint_refine_robust.argtypes = [V] * 11 + [C.c_size_t, V, C.c_size_t] + [V] * 9
            L.clc_joint_refine_robust_device.argtypes = [V] * 11 + [C.c_size_t, V, C.c_size_t] + [V] * 9
        if hasattr(L, "clc_calibrate_full"):
            L.clc_full_options_default.argtypes = [V, C.c_int32]
            L.clc_full_options_default.restype = None
            L.clc_calibrate_full.argtypes = [V] * 10 + [C.c_size_t, V, C.c_size_t] + [V] * 11
            L.clc_calibrate_full_device.argtypes = [V] * 10 + [C.c_size_t, V, C.c_size_t] + [V] * 11
        if hasattr(L, "clc_camera_calibrate"):
            L.clc_camcal_options_default.argtypes = [V, C.c_int32]
            L.clc_camcal_options_default.restype = None
            L.clc_camera_guess.argtypes = [V, C.c_int32, C.c_int32, C.c_int32, V, V, V, C.c_size_t, V, V]
            L.clc_camera_guess_device.argtypes = [V, C.c_int32, C.c_int32, C.c_int32, V, V, V, C.c_size_t, V, V]
            L.clc_camera_calibrate.argtypes = [V] * 7 + [C.c_size_t, V, C.c_size_t] + [V] * 7
            L.clc_camera_calibrate_device.argtypes = [V] * 7 + [C.c_size_t, V, C.c_size_t] + [V] * 7
        if hasattr(L, "clc_score_board_poses"):
            L.clc_guidance_options_default.argtypes = [V]
            L.clc_guidance_options_default.restype = None
            L.clc_score_board_poses.argtypes = [V, V, V, V, C.c_size_t] + [V] * 6
            L.clc_score_board_poses_device.argtypes = [V, V, V, V, C.c_size_t] + [V] * 6
            L.clc_select_board_poses.argtypes = [V, V, V, V, C.c_size_t, V, V, C.c_size_t] + [V] * 5
            L.clc_select_board_poses_device.argtypes = [V, V, V, V, C.c_size_t, V, V, C.c_size_t] + [V] * 5
        if hasattr(L, "clc_corner_subpix"):
            L.clc_subpix_options_default.argtypes = [V, C.c_int32]
            L.clc_subpix_options_default.restype = None
            L.clc_corner_subpix.argtypes = [V, V, V, C.c_int32, C.c_int32, C.c_int64, C.c_size_t] + [V] * 6
            L.clc_corner_subpix_device.argtypes = [V, V, V, C.c_int32, C.c_int32, C.c_int64, C.c_size_t] + [V] * 6
        if hasattr(L, "clc_chess_corners"):
            L.clc_chess_options_default.argtypes = [V]
            L.clc_chess_options_default.restype = None
            L.clc_chessorder_options_default.argtypes = [V]
            L.clc_chessorder_options_default.restype = None
            L.clc_chess_corners.argtypes = [V, V, V, C.c_int32, C.c_int32, C.c_int64, C.c_size_t] + [V] * 5
            L.clc_chess_corners_device.argtypes = [V, V, V, C.c_int32, C.c_int32, C.c_int64, C.c_size_t] + [V] * 5
            L.clc_chessboard_order.argtypes = [V, V, C.c_int64, C.c_size_t, C.c_int32, C.c_int32] + [V] * 5
            L.clc_find_chessboard.argtypes = [V, V, V, V, V, C.c_int32, C.c_int32, C.c_int64, C.c_size_t, C.c_int32, C.c_int32] + [V] * 3
        if hasattr(L, "clc_tag_grid"):
            L.clc_tag_options_default.argtypes = [V]
            L.clc_tag_options_default.restype = None
            L.clc_tag_grid.argtypes = [V] * 6 + [C.c_int32, C.c_int32, C.c_int64, C.c_size_t, C.c_int32, C.c_int32] + [V] * 8
            L.clc_tag_grid_device.argtypes = [V] * 6 + [C.c_int32, C.c_int32, C.c_int64, C.c_size_t, C.c_int32, C.c_int32] + [V] * 8
            L.clc_tag_grid_points_device.argtypes = [V, V, V, C.c_size_t, C.c_int32, C.c_int32, C.c_double, C.c_double, V, V, V]
        if hasattr(L, "clc_chessboard_order_device"):
            L.clc_chessboard_order_device.argtypes = [V, V, V, C.c_int64, C.c_size_t, C.c_int32, C.c_int32] + [V] * 5
            L.clc_find_chessboard_device.argtypes = [V, V, V, V, V, C.c_int32, C.c_int32, C.c_int64, C.c_size_t, C.c_int32, C.c_int32] + [V] * 3
            L.clc_find_chessboard_gpu.argtypes = [V, V, V, V, V, C.c_int32, C.c_int32, C.c_int64, C.c_size_t, C.c_int32, C.c_int32] + [V] * 3
        L.has_hooks = hasattr(L, "clc_debug_build_features")
        _libs[path] = L
    return L


def lib():
    """The library the package runs on: csrc/libclc_hip.so (the product build) unless CLC_LIBRARY names another build."""
    global _lib
    if _lib is None:
        _lib = load(_build.LIB_PATH)
    return _lib


def hooks_lib():
    """The -DCLC_TEST_HOOKS build (product + clc_debug_* / clc_time_*): the default library itself when it has the hooks."""
    L = lib()
    return L if L.has_hooks else load(_build.HOOKS_LIB_PATH)


def check(rc: int, where: str) -> None:
    if rc != CLC_OK:
        # clc_last_error is per library (and thread): with more than one build loaded, take the message of the call that failed
        msgs = [L.clc_last_error().decode("utf-8", "replace") for L in _libs.values()]
        detail = next((m for m in msgs if m.startswith(where)), next((m for m in msgs if m), ""))
        raise ClcError(rc, where, detail)


def dptr(a):
    if a is None:
        return None
    assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags["C_CONTIGUOUS"], "need C-contiguous float64"
    return a.ctypes.data_as(C.POINTER(C.c_double))


def iptr(a):
    if a is None:
        return None
    assert isinstance(a, np.ndarray) and a.dtype == np.int64 and a.flags["C_CONTIGUOUS"], "need C-contiguous int64"
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def default_options() -> Options:
    o = Options()
    lib().clc_options_default(C.byref(o))
    return o


def default_pose_options() -> Options:
    """clc_pose_options_default: no loss, tolerances tight enough for the float32-rounding floor of the lifted corners."""
    o = Options()
    lib().clc_pose_options_default(C.byref(o))
    return o


def default_robust_pose_options(camera) -> RobustPoseOptions:
    """clc_robust_pose_options_default: gates of 8 px (per-tag hypotheses) and 2 px (re-gate with the fitted pose) over the camera's
    focal length — design values from the numpy experiment of DESIGN.md K16 —, at least 4 inliers, at most 4 fits."""
    o = RobustPoseOptions()
    c = camera.to_c()
    lib().clc_robust_pose_options_default(C.byref(o), C.byref(c))
    return o


def default_alt_pose_options() -> AltPoseOptions:
    """clc_alt_pose_options_default: same_angle 0.01 rad, ratio_gate 2 — design values."""
    o = AltPoseOptions()
    lib().clc_alt_pose_options_default(C.byref(o))
    return o


def default_joint_options(camera) -> JointOptions:
    """clc_joint_options_default: 0.3 px over the camera's focal length and 0.01 m, nothing held."""
    o = JointOptions()
    c = camera.to_c()
    lib().clc_joint_options_default(C.byref(o), C.byref(c))
    return o


def default_range_options(camera=None) -> RangeOptions:
    """clc_range_options_default: clc_joint_options_default's sigmas, nothing held; camera None: sigma_corner 0 (for hold_board_poses)."""
    o = RangeOptions()
    c = camera.to_c() if camera is not None else None
    lib().clc_range_options_default(C.byref(o), C.byref(c) if c is not None else None)
    return o


def default_joint_loss_options(joint=None) -> JointLossOptions:
    """clc_joint_loss_options_default: loss_laser = 0.05 m over the sigma_laser of `joint` (5 without it), loss_corner = 3 (a design
    value: 0.9 px at 0.3 px)."""
    o = JointLossOptions()
    lib().clc_joint_loss_options_default(C.byref(o), C.byref(joint) if joint is not None else None)
    return o


def default_full_options(model: int) -> FullOptions:
    """clc_full_options_default: 0.3 px, 0.01 m, loss scales 3 and 5; k4 and k5 (bits 6, 7) held for KANNALA_BRANDT, nothing else."""
    o = FullOptions()
    lib().clc_full_options_default(C.byref(o), C.c_int32(model))
    return o


def default_guidance_options() -> GuidanceOptions:
    """clc_guidance_options_default: 1 081 rays over 270 degrees, ranges [0.05, 30), 50 points, the board [-0.043, 0.457]^2, floor 1e-8,
    the floored log-determinant."""
    o = GuidanceOptions()
    lib().clc_guidance_options_default(C.byref(o))
    return o


def default_chess_options() -> ChessOptions:
    """clc_chess_options_default: threshold 500 on R5, suppression radius 3, relative gate 250 permille, 256 candidates per image."""
    o = ChessOptions()
    lib().clc_chess_options_default(C.byref(o))
    return o


def default_tag_options() -> TagOptions:
    """clc_tag_options_default: sides from 16 px, contrast 40, no white border cell, 256 quads per image."""
    o = TagOptions()
    lib().clc_tag_options_default(C.byref(o))
    return o


def default_chessorder_options() -> ChessOrderOptions:
    """clc_chessorder_options_default: tol 0.3."""
    o = ChessOrderOptions()
    lib().clc_chessorder_options_default(C.byref(o))
    return o


def default_subpix_options(win: int = 3) -> SubpixOptions:
    """clc_subpix_options_default: the half-window `win` on both axes (<= 0: 3, the reference's Kalibr call; its chessboard call uses
    11), no zero zone, 30 iterations, eps 0.1."""
    o = SubpixOptions()
    lib().clc_subpix_options_default(C.byref(o), C.c_int32(win))
    return o


def default_camcal_options(model: int) -> CamcalOptions:
    """clc_camcal_options_default: 0.3 px; nothing held for PINHOLE, k4 and k5 (bits 6, 7) held for KANNALA_BRANDT."""
    o = CamcalOptions()
    lib().clc_camcal_options_default(C.byref(o), C.c_int32(model))
    return o


def default_assemble_options() -> AssembleOptions:
    """The reference's settings, main/calibr_offline.cpp:66-67,:116: 0.20 m, 10 degrees (with pi = 3.1415926), 20 ms; line fits from (0, 0)."""
    o = AssembleOptions()
    lib().clc_assemble_options_default(C.byref(o))
    return o


def default_station_options() -> StationOptions:
    """The reference's settings, src/utilities.cpp:108,:119: 2 mm, more than 30 members; the open last run dropped; line fits from (0, 0)."""
    o = StationOptions()
    lib().clc_station_options_default(C.byref(o))
    return o


class TimeOffsetOptions(C.Structure):
    """clc_clock_offset_options (include/clc.h)."""
    _fields_ = [("offset_min", C.c_double), ("offset_max", C.c_double), ("n_offsets", C.c_int32), ("points_per_scan", C.c_int32),
                ("interp", InterpOptions), ("solve", Options)]


class TimeOffsetResult(C.Structure):
    """clc_clock_offset_result (include/clc.h)."""
    _fields_ = [("n_scans_used", C.c_int64), ("records_per_problem", C.c_int64), ("best_index", C.c_int32), ("at_edge", C.c_int32),
                ("best_offset", C.c_double)]


def default_time_offset_options() -> TimeOffsetOptions:
    """41 candidates over -20 .. +20 ms, 16 points per scan; the interpolation's and the solve's defaults."""
    o = TimeOffsetOptions()
    lib().clc_clock_offset_options_default(C.byref(o))
    return o


def time_offset_best(offsets, final_cost, termination=None):
    """clc_clock_offset_best (host code, no device): -> (best_index, best_offset, at_edge)."""
    x = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1)
    c = np.ascontiguousarray(final_cost, dtype=np.float64).reshape(-1)
    assert x.shape == c.shape
    tm = None if termination is None else np.ascontiguousarray(termination, dtype=np.int32).reshape(-1)
    assert tm is None or tm.shape == x.shape
    bi, ae, bo = C.c_int32(), C.c_int32(), C.c_double()
    check(lib().clc_clock_offset_best(x.shape[0], x.ctypes.data if x.size else None, c.ctypes.data if x.size else None,
                                     None if tm is None else tm.ctypes.data, C.byref(bi), C.byref(bo), C.byref(ae)), "clc_clock_offset_best")
    return bi.value, bo.value, ae.value


def default_interp_options() -> InterpOptions:
    """No clock offset, tag poses at most 0.1 s apart are interpolated across; line fits from (0, 0)."""
    o = InterpOptions()
    lib().clc_interp_options_default(C.byref(o))
    return o


def default_line_options() -> Options:
    """Ceres defaults + LineFittingCeres' settings (10 iterations, CauchyLoss(0.05))."""
    o = Options()
    lib().clc_line_options_default(C.byref(o))
    return o
