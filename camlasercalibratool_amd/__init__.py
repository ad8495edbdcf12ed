"""camlasercalibratool_amd — MI355X-native (gfx950) solver for CamLaserCalibraTool's
point-to-plane camera/2-D-lidar extrinsic least-squares path.

The package is a thin host layer over a C-ABI shared library of hand-written HIP kernels
(csrc/, include/clc.h).  It mirrors the reference's call surface
(CamLaserCalibration / CamLaserCalClosedSolution / Oberserve) and has no CPU fallback."""
from .simdata import GenerateSimData, Oberserve, ObservationSet  # noqa: F401
from ._capi import AssembleInfo, AssembleOptions, default_assemble_options, StationInfo, StationOptions, default_station_options, InterpOptions, default_interp_options, TimeOffsetOptions, default_time_offset_options, ClcError, GuidanceOptions, default_guidance_options, Options, Summary, Iteration, TERMINATION, default_line_options, default_options  # noqa: F401
from .solver import Solver, SolveResult, flatten_observations, chessboard_order, TagFamily  # noqa: F401
from .calib import (CamLaserCalibration, CamLaserCalClosedSolution, CamLaserCalibrationFromStarts, CamLaserCalibrationResample, CamLaserCalibrationConsensus, CamLaserCalibrationBatch, CalibrationReport,  # noqa: F401
                    AutoGetLinePts, LineFittingCeres, CalcCamPoses, CornerSubPix, FindChessboardCorners, FindTagGridCorners, CalcCamPosesRobust, BoardPosesChecked, CamLaserCalibrationJoint, CamLaserCalibrationJointBatch, CalibrateCamera, SuggestBoardPoses, GuidanceReport, Session, points_on_fitted_lines, CalibrateOffline, CalibrateOfflineStations, CalibrateOfflineInterpolated, GetStaticPose,
                    CamLaserCalibrationRange, CamLaserCalibrationRangeBatch, ApplyRangeCorrection,
                    CamLaserCalibrationJointRobust, CamLaserCalibrationJointRobustBatch, CalibrateFull, CalibrateFullBatch)
from ._capi import RangeOptions, default_range_options  # noqa: F401
from ._capi import JointLossOptions, default_joint_loss_options  # noqa: F401
from ._capi import FullOptions, default_full_options  # noqa: F401
from ._capi import SubpixOptions, default_subpix_options  # noqa: F401
from ._capi import ChessOptions, ChessOrderOptions, default_chess_options, default_chessorder_options  # noqa: F401
from ._capi import TagOptions, default_tag_options  # noqa: F401
from .camera import Camera  # noqa: F401
from . import resample  # noqa: F401

__all__ = [
    "CamLaserCalibration", "CamLaserCalClosedSolution", "CamLaserCalibrationFromStarts", "CamLaserCalibrationResample", "CamLaserCalibrationConsensus", "CamLaserCalibrationBatch", "CamLaserCalibrationJoint", "CamLaserCalibrationJointBatch", "CamLaserCalibrationRange", "CamLaserCalibrationRangeBatch", "ApplyRangeCorrection", "RangeOptions", "default_range_options", "CamLaserCalibrationJointRobust", "CamLaserCalibrationJointRobustBatch", "JointLossOptions", "default_joint_loss_options", "CalibrateFull", "CalibrateFullBatch", "FullOptions", "default_full_options", "CalibrateCamera", "SuggestBoardPoses", "GuidanceReport", "GuidanceOptions", "default_guidance_options", "CalcCamPoses", "CornerSubPix", "FindChessboardCorners", "FindTagGridCorners", "TagFamily", "TagOptions", "default_tag_options", "chessboard_order", "ChessOptions", "ChessOrderOptions", "default_chess_options", "default_chessorder_options", "SubpixOptions", "default_subpix_options", "CalcCamPosesRobust", "BoardPosesChecked", "Camera", "AutoGetLinePts", "LineFittingCeres", "Oberserve", "ObservationSet", "GenerateSimData",
    "Session", "CalibrateOffline", "CalibrateOfflineStations", "CalibrateOfflineInterpolated", "GetStaticPose", "InterpOptions", "default_interp_options", "TimeOffsetOptions", "default_time_offset_options", "StationOptions", "StationInfo", "default_station_options", "AssembleOptions", "AssembleInfo", "default_assemble_options", "Solver", "SolveResult", "Options", "default_options", "flatten_observations", "ClcError",
]
