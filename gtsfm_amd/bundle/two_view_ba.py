"""``TwoViewBundleAdjustment`` with the constructor of ``gtsfm/bundle/two_view_ba.py`` (``BundleAdjustmentOptimizer.__init__``,
``bundle_adjustment.py:64-87``), for the graph ``TwoViewEstimator.__init__`` configures (``two_view_estimator.py:86-99``): it turns the
reference's arguments into the options of the device call ``gtsfm_two_view_ba_f64`` and runs a verifier launch through it.

PARITY UNPINNED towards gtsam (tests/two_view_ba_reference.py is the specification): its Levenberg-Marquardt path and retraction, the
cheirality convention, the pivot thresholds, calibrations HELD FIXED (the reference's calibration priors have sigma 1e-5, which fixes
them for every practical purpose) and no pose priors. What the restatement does not cover raises ``NotImplementedError`` naming itself:
a relative pose prior, ``robust_ba_mode`` other than HUBER / NONE, GNC, a Karcher mean factor, shared calibration, more than one entry
in ``reproj_error_thresholds``. The object holds plain Python state until its first run, so it pickles."""

from __future__ import annotations

import dataclasses
import math
from enum import Enum
from typing import Dict, Optional, Sequence

POINT_PRIOR_SIGMA = 0.1  # bundle_adjustment.py: PriorFactorPoint3 on the first point, Isotropic.Sigma(3, 0.1)


class RobustBAMode(Enum):
    """``bundle_adjustment.py:45-51``."""

    NONE = "NONE"
    HUBER = "HUBER"
    GMC = "GMC"
    TLS = "TLS"


@dataclasses.dataclass(frozen=True)
class TwoViewOptions:
    """What ``TwoViewEstimator`` and its ``InlierSupportProcessor`` are configured with in ``unified.yaml``, for ``VerifiedScene.two_view``."""

    bundle_adjust_2view: bool = True
    bundle_adjust_2view_maxiters: int = 100
    ba_reproj_error_thresholds: Sequence[Optional[float]] = (0.5,)
    allow_indeterminate_linear_system: bool = False
    min_num_inliers_est_model: int = 15
    min_inlier_ratio_est_model: float = 0.1
    triangulation_reproj_error_threshold: float = math.inf  # TriangulationOptions(mode=NO_RANSAC) of the estimator
    triangulation_min_angle_deg: float = 0.0

    def optimizer(self) -> "TwoViewBundleAdjustment":
        """The optimiser ``TwoViewEstimator.__init__`` builds (``two_view_estimator.py:86-99``)."""
        return TwoViewBundleAdjustment(reproj_error_thresholds=self.ba_reproj_error_thresholds, robust_ba_mode=RobustBAMode.HUBER,
                                       max_iterations=self.bundle_adjust_2view_maxiters, allow_indeterminate_linear_system=self.allow_indeterminate_linear_system,
                                       use_first_point_prior=True, use_calibration_prior=True, robust_noise_basin=1.345, use_karcher_mean_factor=False,
                                       calibration_prior_focal_sigma=1e-5, calibration_prior_dist_sigma=1e-5, cam_pose3_prior_noise_sigma=0.1,
                                       measurement_noise_sigma=1.0)


class TwoViewBundleAdjustment:
    def __init__(self, reproj_error_thresholds: Sequence[Optional[float]] = (None,), robust_ba_mode: RobustBAMode = RobustBAMode.NONE, shared_calib: bool = False,
                 max_iterations: Optional[int] = None, cam_pose3_prior_noise_sigma: float = 0.1, calibration_prior_focal_sigma: float = 20.0,
                 calibration_prior_dist_sigma: float = 0.1, measurement_noise_sigma: float = 2.0, allow_indeterminate_linear_system: bool = True,
                 print_summary: bool = False, ordering_type: str = "METIS", save_iteration_visualization: bool = False, robust_noise_basin: float = 1.345,
                 use_karcher_mean_factor: bool = True, use_pose_prior: bool = False, use_calibration_prior: bool = True, use_first_point_prior: bool = False,
                 use_gnc: bool = False, gnc_loss="GMC", factor_weight_outlier_threshold: float = 0.0, min_track_length: int = 2) -> None:
        mode = RobustBAMode(getattr(robust_ba_mode, "value", robust_ba_mode))
        if mode not in (RobustBAMode.HUBER, RobustBAMode.NONE):
            raise NotImplementedError(f"robust_ba_mode {mode.name}: the device two-view bundle adjustment has HUBER and NONE only")
        if use_gnc:
            raise NotImplementedError("use_gnc: graduated non-convexity is not implemented in the device two-view bundle adjustment")
        if use_karcher_mean_factor:
            raise NotImplementedError("use_karcher_mean_factor: a Karcher mean factor is not implemented in the device two-view bundle adjustment")
        if shared_calib:
            raise NotImplementedError("shared_calib: calibrations are held fixed per camera in the device two-view bundle adjustment")
        if len(list(reproj_error_thresholds)) != 1:
            raise NotImplementedError("reproj_error_thresholds: the device two-view bundle adjustment runs one round with one threshold")
        if use_pose_prior:
            raise NotImplementedError("use_pose_prior: absolute pose priors beyond the first camera's are not implemented")
        if not use_first_point_prior or not use_calibration_prior:
            raise NotImplementedError("use_first_point_prior / use_calibration_prior = False: the device graph is the one TwoViewEstimator configures")
        if min_track_length != 2:
            raise NotImplementedError("min_track_length: two-view tracks have two measurements")
        threshold = list(reproj_error_thresholds)[0]
        self._reproj_error_threshold = math.inf if threshold is None else float(threshold)
        self._huber_k = float(robust_noise_basin) if mode is RobustBAMode.HUBER else math.inf
        self._max_iterations = 100 if max_iterations is None else int(max_iterations)  # gtsam's LevenbergMarquardtParams default
        self._pose_prior_sigma = float(cam_pose3_prior_noise_sigma)
        self._measurement_sigma = float(measurement_noise_sigma)
        self._allow_indeterminate = bool(allow_indeterminate_linear_system)
        self._engine = None

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_engine"] = None
        return state

    def options(self, min_verified: int = 15, triangulation_threshold: float = math.inf, triangulation_min_angle_deg: float = 0.0):
        from gtsfm_amd.runtime.two_view_ba_engine import TwoViewBAOptions

        return TwoViewBAOptions(max_iterations=self._max_iterations, reproj_error_threshold=self._reproj_error_threshold, huber_k=self._huber_k,
                                measurement_sigma=self._measurement_sigma, pose_prior_sigma=self._pose_prior_sigma, point_prior_sigma=POINT_PRIOR_SIGMA,
                                min_verified=int(min_verified), allow_indeterminate=self._allow_indeterminate,
                                triangulation_threshold=float(triangulation_threshold), triangulation_min_angle_deg=float(triangulation_min_angle_deg))

    @staticmethod
    def pair_intrinsics(camera_intrinsics_i1, camera_intrinsics_i2):
        """One row of the device call's ``intrinsics`` [P, 8]; a calibration that is not a pure pinhole raises ``NotImplementedError`` naming it
        (its distortion must not be dropped silently), as ``Point3dInitializer`` does."""
        from gtsfm_amd.common.calibration import pinhole_parameters

        row = []
        for which, cal in (("i1", camera_intrinsics_i1), ("i2", camera_intrinsics_i2)):
            fx, fy, cx, cy, pure = pinhole_parameters(cal)
            if not pure:
                raise NotImplementedError(f"camera {which}: calibration {type(cal).__name__} is not a pure pinhole; the device two-view bundle adjustment holds "
                                          "fx, fy, cx, cy fixed and has no distortion model")
            row += [fx, fy, cx, cy]
        return row

    def run_launch(self, launch: Dict[str, object], relative_pose_priors=None, device=None, **option_overrides) -> Dict[str, object]:
        """One verifier launch (``TwoViewBAEngine.run``'s arrays) through the device call; only the per-pair stats come back to the host."""
        if relative_pose_priors:
            raise NotImplementedError("relative pose priors (BetweenFactorPose3) are not implemented in the device two-view bundle adjustment")
        if self._engine is None:
            from gtsfm_amd.runtime.two_view_ba_engine import TwoViewBAEngine

            self._engine = TwoViewBAEngine(device)
        return self._engine.run(launch, self.options(**option_overrides))
