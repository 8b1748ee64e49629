"""lili_om_amd — MI355X (gfx950) native hot path of LiLi-OM: feature extraction + scan-to-map matcher.

The product is liblili_hip.so (hand-written HIP kernels behind the C ABI of include/lili_hip.h);
this package is the thin host-side binding used by tests and bench.py.  No CPU fallback exists.
"""
from . import api  # noqa: F401
from .loop import LoopClosure  # noqa: F401
from .archive import KeyframeArchive, GlobalMap, ARCHIVE_EDGE, ARCHIVE_SURF, ARCHIVE_FULL  # noqa: F401
from .place import PlaceRecognition, place_frame, place_guess, place_layout, place_relative  # noqa: F401
from .localize import MapLocalizer  # noqa: F401
from .local_graph import LocalGraph, FrameTrajectory  # noqa: F401
from .pose_graph import PoseGraph, correct_poses, loop_measurement, relative_covariance  # noqa: F401
from .api import (Context, ScanToMapMatcher, RotExtractor, LivoxExtractor, LocalMap, FrontendOdometry, RotFrontendOdometry, BackendKeyframes, WindowSolver, WindowCycleOptions, WindowCycleResult, ImuPreintegrator, LiliError, make_params,  # noqa: F401
                  KeyframeRule, pose_relative, keyframe_undistort,
                  load_library, KIND_SURF, KIND_EDGE, MASK_SURF, MASK_EDGE)

__all__ = ["api", "Context", "ScanToMapMatcher", "RotExtractor", "LivoxExtractor", "LocalMap", "FrontendOdometry", "RotFrontendOdometry", "BackendKeyframes", "WindowSolver", "WindowCycleOptions", "WindowCycleResult", "ImuPreintegrator", "LiliError", "make_params", "load_library",
           "KIND_SURF", "KIND_EDGE", "MASK_SURF", "MASK_EDGE", "LoopClosure", "KeyframeArchive", "GlobalMap", "LocalGraph", "FrameTrajectory", "PoseGraph", "correct_poses", "loop_measurement", "relative_covariance",
           "ARCHIVE_EDGE", "ARCHIVE_SURF", "ARCHIVE_FULL", "KeyframeRule", "pose_relative", "keyframe_undistort", "PlaceRecognition", "place_guess", "place_layout", "place_frame", "place_relative", "MapLocalizer"]
