"""``BundleAdjustmentOptimizer`` with the constructor of ``gtsfm/bundle/bundle_adjustment.py:64-87``, for the graph ``unified.yaml`` /
``deep_front_end.yaml`` configure as ``bundle_adjustment_module`` (HUBER, ``measurement_noise_sigma: 1.0``, ``reproj_error_thresholds:
[10, 5, 3]``): it turns the reference's arguments into the options of the device call ``gtsfm_global_ba_f64`` and runs the adjustment on
the triangulation's arrays.

THE THRESHOLD LIST. The reference restarts every entry of ``reproj_error_thresholds`` from the same ``initial_data``
(``bundle_adjustment.py:617-625``): the stages are identical optimisations and only the last threshold shapes the result. This drop-in
therefore runs the optimisation once and filters at the last threshold (None: no filter).

PARITY UNPINNED towards gtsam (tests/global_ba_reference.py is the specification): gtsam's Levenberg-Marquardt path, elimination ordering
and retraction; the Karcher-mean factor and the soft prior (sigma 0.1) in place of ONE HARD ANCHOR; calibration variables, their priors
and ``shared_calib`` (calibrations are HELD FIXED); GNC / GMC / TLS; relative and absolute pose priors; the marginals check;
``select_largest_connected_component`` (here: the anchor's component); the metrics group.

What the restatement does not cover raises ``NotImplementedError`` naming the argument: ``robust_ba_mode`` GMC / TLS, ``use_gnc``,
``shared_calib``, ``use_pose_prior``, ``use_first_point_prior``, a calibration that is not a pure pinhole, non-empty relative or absolute
pose priors. ACCEPTED AND IGNORED, because the hard anchor and the fixed calibrations stand in their place or they do not touch the
result: ``use_karcher_mean_factor``, ``use_calibration_prior``, ``ordering_type``, ``cam_pose3_prior_noise_sigma``,
``calibration_prior_focal_sigma``, ``calibration_prior_dist_sigma``, ``print_summary``, ``save_iteration_visualization``,
``allow_indeterminate_linear_system`` (there is no marginals check), ``gnc_loss`` and ``factor_weight_outlier_threshold`` (GNC only).
The object holds plain Python state until its first run, so it pickles."""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from gtsfm_amd.bundle.two_view_ba import RobustBAMode  # noqa: F401 - re-exported

__all__ = ["BundleAdjustmentOptimizer", "RobustBAMode"]


class BundleAdjustmentOptimizer:
    def __init__(self, reproj_error_thresholds: Sequence[Optional[float]] = (None,), robust_ba_mode: RobustBAMode = RobustBAMode.NONE, shared_calib: bool = False,
                 max_iterations: Optional[int] = None, cam_pose3_prior_noise_sigma: float = 0.1, calibration_prior_focal_sigma: float = 20.0,
                 calibration_prior_dist_sigma: float = 0.1, measurement_noise_sigma: float = 2.0, allow_indeterminate_linear_system: bool = True,
                 print_summary: bool = False, ordering_type: str = "METIS", save_iteration_visualization: bool = False, robust_noise_basin: float = 1.345,
                 use_karcher_mean_factor: bool = True, use_pose_prior: bool = False, use_calibration_prior: bool = True, use_first_point_prior: bool = False,
                 use_gnc: bool = False, gnc_loss="GMC", factor_weight_outlier_threshold: float = 0.0, min_track_length: int = 2, device=None, **solver_options) -> None:
        mode = RobustBAMode(getattr(robust_ba_mode, "value", robust_ba_mode))
        if mode not in (RobustBAMode.HUBER, RobustBAMode.NONE):
            raise NotImplementedError(f"robust_ba_mode {mode.name}: the device bundle adjustment has HUBER and NONE only")
        if use_gnc:
            raise NotImplementedError("use_gnc: graduated non-convexity is not implemented in the device bundle adjustment")
        if shared_calib:
            raise NotImplementedError("shared_calib: calibrations are held fixed per camera in the device bundle adjustment")
        if use_pose_prior:
            raise NotImplementedError("use_pose_prior: absolute pose priors are not implemented in the device bundle adjustment (one camera is held fixed)")
        if use_first_point_prior:
            raise NotImplementedError("use_first_point_prior: a prior on the first point is not implemented in the device bundle adjustment")
        thresholds = list(reproj_error_thresholds)
        if not thresholds:
            raise ValueError("reproj_error_thresholds must have at least one entry")
        unknown = set(solver_options) - {"cg_forcing", "max_inner", "rel_tol", "abs_tol"}
        if unknown:
            raise TypeError(f"unknown options {sorted(unknown)}")
        self._reproj_error_thresholds = thresholds
        self._reproj_error_threshold = math.inf if thresholds[-1] is None else float(thresholds[-1])
        self._robust_ba_mode = mode
        self._huber_k = float(robust_noise_basin) if mode is RobustBAMode.HUBER else math.inf
        self._max_iterations = 100 if max_iterations is None else int(max_iterations)  # gtsam's LevenbergMarquardtParams default
        self._measurement_sigma = float(measurement_noise_sigma)
        self._min_track_length = int(min_track_length)
        self._solver_options = dict(solver_options)
        self._device = device
        self._engine = None

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_engine"] = None
        return state

    def options(self):
        from gtsfm_amd.runtime.global_ba_engine import GlobalBAOptions

        return GlobalBAOptions(measurement_sigma=self._measurement_sigma, huber_k=self._huber_k, reproj_error_threshold=self._reproj_error_threshold,
                               min_track_length=self._min_track_length, max_iterations=self._max_iterations, **self._solver_options)

    def engine(self, device=None):
        if self._engine is None:
            from gtsfm_amd.runtime.global_ba_engine import GlobalBAEngine

            self._engine = GlobalBAEngine(device if device is not None else self._device)
        return self._engine

    def run_ba_device(self, cameras, track_off, image, uv, point, track_enable=None, meas_enable=None, anchor: int = -1) -> Dict[str, object]:
        """The adjustment on device tensors where they lie (``GlobalBAEngine.adjust``'s arguments and result, one problem)."""
        return self.engine(cameras.device).adjust(cameras, track_off, image, uv, point, track_enable, meas_enable, anchor=anchor, options=self.options())

    def run_ba_arrays(self, cameras, track_off, image, uv, point, track_enable=None, meas_enable=None) -> Dict[str, object]:
        """Host arrays in (the camera table [N, 17], the track CSR, the points, the two masks or None), host arrays out: ``cameras`` [N, 17],
        ``point`` [T, 3], ``reproj_error`` [S], ``track_valid`` [T], ``camera_kept`` [N], ``node_valid`` [N + T], ``counters`` [8], ``costs`` [4],
        ``status``."""
        engine = self.engine()
        out = engine.adjust(*engine.upload(cameras, track_off, image, uv, point, track_enable, meas_enable), options=self.options())
        res = {k: out[k].cpu().numpy() for k in ("point", "reproj_error", "track_valid")}
        res.update({k: out[k][0].cpu().numpy() for k in ("cameras", "camera_kept", "node_valid")})
        res.update(counters=out["counters"][0], costs=out["costs"][0], status=out["status"][0])
        return res

    def run_ba(self, cameras: Dict[int, object], tracks: Sequence[object], absolute_pose_priors=None, relative_pose_priors=None) -> Tuple[Dict[int, object], List[object], List[bool]]:
        """``cameras``: ``{image: PinholeCamera}`` (anything with ``pose()`` and ``calibration()``); ``tracks``: ``SfmTrack``s (``point3()``,
        ``numberMeasurements()``, ``measurement(k)``). Returns (the optimised cameras of the adjusted component and the optimised tracks, as
        ``run_ba``'s unfiltered data; the cameras and tracks that pass the filter, as its filtered data; the tracks' valid mask)."""
        from gtsfm_amd.common.calibration import PinholeCamera
        from gtsfm_amd.data_association.point3d_initializer import SfmTrack
        from gtsfm_amd.runtime.triangulation_engine import pack_cameras

        if absolute_pose_priors and any(p is not None for p in (absolute_pose_priors.values() if isinstance(absolute_pose_priors, dict) else absolute_pose_priors)):
            raise NotImplementedError("absolute_pose_priors: absolute pose priors are not implemented in the device bundle adjustment")
        if relative_pose_priors:
            raise NotImplementedError("relative_pose_priors: relative pose priors (BetweenFactorPose3) are not implemented in the device bundle adjustment")
        table = pack_cameras(cameras)  # a calibration that is not a pure pinhole raises NotImplementedError naming it
        lengths = [t.numberMeasurements() for t in tracks]
        track_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        meas = [t.measurement(k) for t in tracks for k in range(t.numberMeasurements())]
        image = np.asarray([int(i) for i, _ in meas], np.int32)
        uv = np.asarray([np.asarray(x, np.float32).reshape(2) for _, x in meas], np.float32).reshape(-1, 2)
        point = np.asarray([np.asarray(t.point3(), np.float64).reshape(3) for t in tracks], np.float64).reshape(-1, 3)
        res = self.run_ba_arrays(table, track_off, image, uv, point)

        def camera(i):
            return PinholeCamera(res["cameras"][i, 5:14].reshape(3, 3).copy(), res["cameras"][i, 14:17].copy(), cameras[i].calibration())

        def track(j):
            out = SfmTrack(res["point"][j].copy())
            for k in range(tracks[j].numberMeasurements()):
                out.addMeasurement(*tracks[j].measurement(k))
            return out

        in_problem = [j for j in range(len(tracks)) if res["node_valid"][len(table) + j]]
        optimized = ({int(i): camera(int(i)) for i in cameras if cameras[i] is not None and res["node_valid"][int(i)]}, [track(j) for j in in_problem])
        filtered = ({i: c for i, c in optimized[0].items() if res["camera_kept"][i]}, [track(j) for j in in_problem if res["track_valid"][j]])
        return optimized, filtered, [bool(res["track_valid"][j]) for j in in_problem]
