"""Drop-in for ``gtsfm/two_view_estimator.py``'s ``TwoViewEstimator``: ``run_2view`` = verify -> two-view bundle adjustment -> inlier
support (``:350-481``), with the bundle adjustment on the device (``gtsfm_two_view_ba_f64``; one pair per call here, a whole scene per
launch in ``VerifiedScene.two_view``). Rotations and directions are the objects the ``Ransac`` plugin returns.

Kept from the reference: the early returns of ``bundle_adjust`` (``:244-245, 262-263, 274-276``), the hack
``post_ba_inlier_ratio = pre_ba_inlier_ratio`` (``:423-426``), the report's fields. With ground-truth cameras only ``R_error_deg`` /
``U_error_deg`` are filled; ``gt_scene_mesh`` and a relative pose prior raise ``NotImplementedError``; the Postgres code is not ported.
PARITY UNPINNED towards gtsam: see ``tests/two_view_ba_reference.py``. The object holds plain Python state until first use, so it pickles."""

from __future__ import annotations

import dataclasses
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from gtsfm_amd.bundle.two_view_ba import RobustBAMode, TwoViewBundleAdjustment
from gtsfm_amd.common.two_view_estimation_report import TwoViewEstimationReport
from gtsfm_amd.frontend.inlier_support_processor import InlierSupportProcessor

NONE_TRIANGULATED, INDETERMINATE = 3, 4


@dataclasses.dataclass
class TwoViewResult:
    i2Ri1: Optional[Any]
    i2Ui1: Optional[Any]
    v_corr_idxs: np.ndarray
    pre_ba_report: Optional[TwoViewEstimationReport]
    post_ba_report: Optional[TwoViewEstimationReport]
    post_isp_report: Optional[TwoViewEstimationReport]
    putative_corr_idxs: Optional[np.ndarray] = None
    relative_pose_prior: Optional[Any] = None


def _matrix(rotation) -> np.ndarray:
    return np.asarray(rotation.matrix() if hasattr(rotation, "matrix") else rotation, dtype=np.float64).reshape(3, 3)


def _vector(direction) -> np.ndarray:
    if hasattr(direction, "point3"):
        direction = direction.point3()
    return np.asarray(direction, dtype=np.float64).reshape(3)


def _angle_deg(cosine: float) -> float:
    return float(np.degrees(np.arccos(np.clip(cosine, -1.0, 1.0))))


def compute_relative_pose_metrics(i2Ri1_computed, i2Ui1_computed, wTi1_expected, wTi2_expected) -> Tuple[Optional[float], Optional[float]]:
    """Rotation and unit-translation error in degrees against the expected poses (``two_view_estimator.py:705-731``); ``None`` for a missing
    expected pose, and per entry for a missing estimate."""
    if wTi1_expected is None or wTi2_expected is None:
        return None, None
    r1, r2 = _matrix(wTi1_expected.rotation()), _matrix(wTi2_expected.rotation())
    t1, t2 = _vector(wTi1_expected.translation()), _vector(wTi2_expected.translation())
    rot, trans = r2.T @ r1, r2.T @ (t1 - t2)  # wTi2.between(wTi1)
    r_err = None if i2Ri1_computed is None else _angle_deg((np.trace(rot.T @ _matrix(i2Ri1_computed)) - 1.0) / 2.0)
    u_err = None
    if i2Ui1_computed is not None:
        u = _vector(i2Ui1_computed)
        u_err = _angle_deg(float(u @ trans) / (np.linalg.norm(u) * np.linalg.norm(trans)))
    return r_err, u_err


def generate_two_view_report(inlier_ratio_est_model: float, v_corr_idxs: np.ndarray, R_error_deg: Optional[float] = None, U_error_deg: Optional[float] = None,
                             v_corr_idxs_inlier_mask_gt: Optional[np.ndarray] = None, reproj_error_gt_model: Optional[np.ndarray] = None) -> TwoViewEstimationReport:
    """``two_view_estimator.py:663-702``."""
    nan = float("nan")
    gt = dict(num_inliers_gt_model=0, inlier_ratio_gt_model=nan, inlier_avg_reproj_error_gt_model=nan, outlier_avg_reproj_error_gt_model=nan)
    if v_corr_idxs_inlier_mask_gt is not None and reproj_error_gt_model is not None:
        mask, err = np.asarray(v_corr_idxs_inlier_mask_gt, dtype=bool), np.asarray(reproj_error_gt_model, dtype=np.float64)
        hits = int(np.count_nonzero(mask))

        def mean_of(sel):
            vals = err[sel]
            vals = vals[~np.isnan(vals)]
            return float(vals.mean()) if vals.size else nan

        gt = dict(num_inliers_gt_model=hits, inlier_ratio_gt_model=hits / v_corr_idxs.shape[0] if len(v_corr_idxs) > 0 else 0.0,
                  inlier_avg_reproj_error_gt_model=mean_of(mask), outlier_avg_reproj_error_gt_model=mean_of(~mask))
    return TwoViewEstimationReport(v_corr_idxs=v_corr_idxs, num_inliers_est_model=v_corr_idxs.shape[0], inlier_ratio_est_model=inlier_ratio_est_model,
                                   v_corr_idxs_inlier_mask_gt=v_corr_idxs_inlier_mask_gt, R_error_deg=R_error_deg, U_error_deg=U_error_deg,
                                   reproj_error_gt_model=reproj_error_gt_model, **gt)


class TwoViewEstimator:
    def __init__(self, verifier, inlier_support_processor: InlierSupportProcessor, bundle_adjust_2view: bool, eval_threshold_px: float, triangulation_options,
                 bundle_adjust_2view_maxiters: int = 100, ba_reproj_error_thresholds: Sequence[Optional[float]] = (0.5,),
                 allow_indeterminate_linear_system: bool = False) -> None:
        self._verifier = verifier
        self.processor = inlier_support_processor
        self._bundle_adjust_2view = bundle_adjust_2view
        self._corr_metric_dist_threshold = eval_threshold_px
        self._triangulation_options = triangulation_options
        self._ba_optimizer = TwoViewBundleAdjustment(
            reproj_error_thresholds=list(ba_reproj_error_thresholds), robust_ba_mode=RobustBAMode.HUBER, max_iterations=bundle_adjust_2view_maxiters,
            allow_indeterminate_linear_system=allow_indeterminate_linear_system, use_first_point_prior=True, use_calibration_prior=True, robust_noise_basin=1.345,
            use_karcher_mean_factor=False, calibration_prior_focal_sigma=1e-5, calibration_prior_dist_sigma=1e-5, cam_pose3_prior_noise_sigma=0.1,
            measurement_noise_sigma=1.0)

    def get_corr_metric_dist_threshold(self) -> float:
        return self._corr_metric_dist_threshold

    def _triangulation_settings(self) -> Tuple[float, float]:
        opt = self._triangulation_options
        mode = getattr(getattr(opt, "mode", "NO_RANSAC"), "name", getattr(opt, "mode", "NO_RANSAC"))
        if opt is not None and str(mode) != "NO_RANSAC":
            raise NotImplementedError(f"triangulation mode {mode}: the device two-view triangulation is NO_RANSAC, as the reference's configs set it")
        return float(getattr(opt, "reproj_error_threshold", np.inf)), float(getattr(opt, "min_triangulation_angle", 0.0))

    def triangulate_two_view_correspondences(self, cameras: Dict[int, Any], keypoints_i1, keypoints_i2, corr_ind: np.ndarray) -> Tuple[List[int], List[Any]]:
        """``:165-210``: the correspondences as two-measurement tracks through ``Point3dInitializer`` in one launch; the indices and tracks that succeed."""
        from gtsfm_amd.common.sfm_track import SfmMeasurement, SfmTrack2d
        from gtsfm_amd.data_association.point3d_initializer import Point3dInitializer

        tracks = [SfmTrack2d([SfmMeasurement(0, keypoints_i1.coordinates[a]), SfmMeasurement(1, keypoints_i2.coordinates[b])]) for a, b in np.asarray(corr_ind).reshape(-1, 2)]
        results = Point3dInitializer(cameras, self._triangulation_options).triangulate_batch(tracks) if tracks else []
        indices = [j for j, res in enumerate(results) if res[0] is not None]
        return indices, [results[j][0] for j in indices]

    def bundle_adjust(self, keypoints_i1, keypoints_i2, verified_corr_idxs: np.ndarray, camera_intrinsics_i1, camera_intrinsics_i2, i2Ri1_initial, i2Ui1_initial,
                      i2Ti1_prior=None) -> Tuple[Optional[Any], Optional[Any], np.ndarray]:
        """``:212-288`` for one pair, on the device. Returns the reference's triples, early returns included."""
        return self.bundle_adjust_with_stats(keypoints_i1, keypoints_i2, verified_corr_idxs, camera_intrinsics_i1, camera_intrinsics_i2, i2Ri1_initial,
                                             i2Ui1_initial, i2Ti1_prior)[:3]

    def bundle_adjust_with_stats(self, keypoints_i1, keypoints_i2, verified_corr_idxs: np.ndarray, camera_intrinsics_i1, camera_intrinsics_i2, i2Ri1_initial,
                                 i2Ui1_initial, i2Ti1_prior=None) -> Tuple[Optional[Any], Optional[Any], np.ndarray, Optional[np.ndarray]]:
        """``bundle_adjust`` and the device call's stats row [8] (``None`` without an initial pose: nothing ran)."""
        from gtsfm_amd.frontend.verifier.ransac import _to_pose_types

        if i2Ti1_prior is not None:
            raise NotImplementedError("a relative pose prior (BetweenFactorPose3) is not implemented in the device two-view bundle adjustment")
        if i2Ri1_initial is None or i2Ui1_initial is None:
            return None, None, verified_corr_idxs, None
        corr = np.asarray(verified_corr_idxs).reshape(-1, 2)
        xy1, xy2 = np.asarray(keypoints_i1.coordinates, np.float32).reshape(-1, 2), np.asarray(keypoints_i2.coordinates, np.float32).reshape(-1, 2)
        threshold, angle = self._triangulation_settings()
        launch = {"kp_xy": np.concatenate([xy1, xy2]), "kp_off1": [0], "kp_off2": [len(xy1)], "match_idx": corr.astype(np.int32), "match_off": [0, len(corr)],
                  "match_count": None, "inlier_mask": np.ones(len(corr), np.uint8),
                  "intrinsics": [TwoViewBundleAdjustment.pair_intrinsics(camera_intrinsics_i1, camera_intrinsics_i2)], "rotation": _matrix(i2Ri1_initial)[None],
                  "translation": _vector(i2Ui1_initial)[None]}
        out = self._ba_optimizer.run_launch(launch, min_verified=0, triangulation_threshold=threshold, triangulation_min_angle_deg=angle)
        row = out["stats"][0]
        empty = np.zeros(shape=(0, 2), dtype=np.int32)
        if int(row[0]) == NONE_TRIANGULATED:
            return i2Ri1_initial, i2Ui1_initial, empty, row
        rot, trans = out["rotation"].cpu().numpy()[0], out["translation"].cpu().numpy()[0]
        if not (np.isfinite(rot).all() and np.isfinite(trans).all()):  # an indeterminate linear system that is not allowed
            return None, None, empty, row
        valid = out["valid_mask"].cpu().numpy().astype(bool)
        return (*_to_pose_types(rot, trans), np.asarray(verified_corr_idxs)[valid], row)

    def _report(self, i2Ri1, i2Ui1, v_corr_idxs, ratio, gt_camera_i1, gt_camera_i2, gt_scene_mesh) -> TwoViewEstimationReport:
        if gt_scene_mesh is not None:
            raise NotImplementedError("gt_scene_mesh: correspondence metrics against a scene mesh are not implemented")
        r_err = u_err = None
        if gt_camera_i1 and gt_camera_i2:
            r_err, u_err = compute_relative_pose_metrics(i2Ri1, i2Ui1, gt_camera_i1.pose(), gt_camera_i2.pose())
        return generate_two_view_report(ratio, v_corr_idxs, R_error_deg=r_err, U_error_deg=u_err)

    def run_2view(self, keypoints_i1, keypoints_i2, putative_corr_idxs: np.ndarray, camera_intrinsics_i1, camera_intrinsics_i2, i2Ti1_prior=None,
                  gt_camera_i1=None, gt_camera_i2=None, gt_scene_mesh=None, i1: Optional[int] = None, i2: Optional[int] = None) -> TwoViewResult:
        pre_r, pre_u, pre_corr, pre_ratio = self._verifier.verify(keypoints_i1, keypoints_i2, putative_corr_idxs, camera_intrinsics_i1, camera_intrinsics_i2)
        pre_report = self._report(pre_r, pre_u, pre_corr, pre_ratio, gt_camera_i1, gt_camera_i2, gt_scene_mesh)
        if self._bundle_adjust_2view and len(pre_corr) >= self.processor._min_num_inliers_est_model:
            post_r, post_u, post_corr = self.bundle_adjust(keypoints_i1, keypoints_i2, pre_corr, camera_intrinsics_i1, camera_intrinsics_i2, pre_r, pre_u, i2Ti1_prior)
            # the reference overwrites len(post) / len(putative) with the verifier's ratio until its consumers can take the lower one
            post_report = self._report(post_r, post_u, post_corr, pre_ratio, gt_camera_i1, gt_camera_i2, gt_scene_mesh)
        else:
            post_r, post_u, post_corr, post_report = pre_r, pre_u, pre_corr, dataclasses.replace(pre_report)
        isp_r, isp_u, isp_corr, isp_report = self.processor.run_inlier_support(post_r, post_u, post_corr, post_report)
        return TwoViewResult(i2Ri1=isp_r, i2Ui1=isp_u, v_corr_idxs=isp_corr, pre_ba_report=pre_report, post_ba_report=post_report, post_isp_report=isp_report,
                             putative_corr_idxs=putative_corr_idxs, relative_pose_prior=i2Ti1_prior)
