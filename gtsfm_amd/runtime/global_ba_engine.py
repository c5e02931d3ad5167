"""Host side of the device's global bundle adjustment: ``gtsfm_global_ba_f64`` runs what ``BundleAdjustmentOptimizer.run_ba`` does after the
triangulation (``gtsfm/bundle/bundle_adjustment.py``, called from ``gtsfm/multi_view_optimizer.py:215-221``) on the arrays
``gtsfm_triangulate_tracks_f64`` reads and writes: the camera table, the track CSR, the points, the exit codes and the inlier mask.
PyTorch provides device memory and streams only."""

from __future__ import annotations

import dataclasses
from typing import Dict

import numpy as np

from gtsfm_amd.runtime.engine_base import EngineBase, merge_options

COUNTER_FIELDS = ("status", "anchor", "cameras", "points", "valid_measurements", "accepted_steps", "solves_tried", "cg_iterations")
COST_FIELDS = ("init_cost", "final_cost", "gradient_inf_norm", "lambda")
STATUS_NAMES = ("CONVERGED", "MAX_ITERATIONS", "NO_VALID_ROW", "NON_FINITE", "LAMBDA_BOUND")
CONVERGED, MAX_ITERATIONS, NO_VALID_ROW, NON_FINITE, LAMBDA_BOUND = 0, 1, 2, 3, 4
# measurement_sigma, huber_k and the last reprojection threshold are unified.yaml's; rel_tol and abs_tol gtsam's documented LM defaults;
# cg_forcing and max_inner (0: six per camera) were chosen on the restatement (tests/global_ba_reference.py)
DEFAULTS = dict(measurement_sigma=1.0, huber_k=1.345, reproj_error_threshold=3.0, min_track_length=2, rel_tol=1e-5, abs_tol=1e-5, cg_forcing=1e-2, max_iterations=100,
                max_inner=0)


@dataclasses.dataclass(frozen=True)
class GlobalBAOptions:
    """The options of ``gtsfm_global_ba_f64``; ``huber_k`` = inf is ``RobustBAMode.NONE``, ``reproj_error_threshold`` = inf no filter."""

    measurement_sigma: float = 1.0
    huber_k: float = 1.345
    reproj_error_threshold: float = 3.0
    min_track_length: int = 2
    rel_tol: float = 1e-5
    abs_tol: float = 1e-5
    cg_forcing: float = 1e-2
    max_iterations: int = 100
    max_inner: int = 0

    def as_dict(self) -> Dict[str, object]:
        return dataclasses.asdict(self)


class GlobalBAEngine(EngineBase):
    def adjust(self, cameras, track_off, image, uv, point, track_enable=None, meas_enable=None, *, anchor: int = -1, problem_off=None, options: GlobalBAOptions = None,
               **overrides) -> Dict[str, object]:
        """Device tensors as in include/gtsfm_amd.h: ``cameras`` [N, 17] float64, ``track_off`` [T + 1] int64, ``image`` [S] int32, ``uv`` [S, 2]
        float32, ``point`` [T, 3] float64, ``track_enable`` [T] / ``meas_enable`` [S] uint8 or None. ``problem_off`` [P + 1] over the tracks, a HOST
        array (the widest problem sizes the outputs) or None: one problem over everything. ``options``: a ``GlobalBAOptions``, ``overrides`` its
        fields by name. Returns device tensors ``cameras`` [P, N, 17], ``point`` [T, 3], ``reproj_error`` [S], ``track_valid`` [T], ``camera_kept``
        [P, N], ``node_valid`` [P, N + the most tracks of a problem] and, read back, ``counters`` [P, 8] int32, ``costs`` [P, 4] float64 and
        ``status`` (a list of names). The inputs are not changed."""
        torch = self._torch
        dev = self.device
        o = merge_options(DEFAULTS if options is None else options.as_dict(), overrides)
        n, t, s = int(cameras.shape[0]), int(track_off.shape[0]) - 1, int(image.shape[0])
        if t < 0:
            raise ValueError("track_off must be [T + 1]")
        off_dev, p, t_max = None, 1, t
        if problem_off is not None:
            off = np.ascontiguousarray(np.asarray(problem_off.cpu() if isinstance(problem_off, torch.Tensor) else problem_off, dtype=np.int64).reshape(-1))
            p = len(off) - 1
            if p < 1:
                raise ValueError("problem_off must be [P + 1] with P >= 1")
            t_max = int(min(max(int(np.diff(off).max()), 0), t))
            off_dev = torch.from_numpy(off).to(dev)
        spec = (("cameras", cameras, torch.float64, 17 * n), ("track_off", track_off, torch.int64, t + 1), ("image", image, torch.int32, s), ("uv", uv, torch.float32, 2 * s),
                ("point", point, torch.float64, 3 * t), ("track_enable", track_enable, torch.uint8, t), ("meas_enable", meas_enable, torch.uint8, s))
        self._check_tensors(spec, optional={"track_enable", "meas_enable"})
        ws = self._sized_workspace("gtsfm_global_ba_workspace_bytes", s, n, t, t_max, p)
        m = n + t_max
        out = {"cameras": torch.empty((p, n, 17), dtype=torch.float64, device=dev), "point": torch.empty((t, 3), dtype=torch.float64, device=dev),
               "reproj_error": torch.empty(s, dtype=torch.float64, device=dev), "track_valid": torch.empty(t, dtype=torch.uint8, device=dev),
               "camera_kept": torch.empty((p, n), dtype=torch.uint8, device=dev), "node_valid": torch.empty((p, m), dtype=torch.uint8, device=dev)}
        counters = torch.empty((p, 8), dtype=torch.int32, device=dev)
        costs = torch.empty((p, 4), dtype=torch.float64, device=dev)
        q = self._ptr
        rc = self._lib.gtsfm_global_ba_f64(
            q(cameras), n, q(track_off) if t > 0 else None, q(image), q(uv), q(point), q(track_enable), q(meas_enable), t, s, q(off_dev), p, t_max, int(anchor),
            int(o["min_track_length"]), float(o["measurement_sigma"]), float(o["huber_k"]), float(o["reproj_error_threshold"]), float(o["rel_tol"]), float(o["abs_tol"]),
            float(o["cg_forcing"]), int(o["max_iterations"]), int(o["max_inner"]), ws.data_ptr(), ws.numel(), q(out["cameras"]), q(out["point"]), q(out["reproj_error"]),
            q(out["track_valid"]), q(out["camera_kept"]), q(out["node_valid"]), counters.data_ptr(), costs.data_ptr(), self._stream())
        self._L.check(rc, "gtsfm_global_ba_f64")
        c = counters.cpu().numpy()
        return {**out, "counters": c, "costs": costs.cpu().numpy(), "status": [STATUS_NAMES[int(k)] for k in c[:, 0]]}

    def upload(self, cameras, track_off, image, uv, point, track_enable=None, meas_enable=None):
        """Host arrays -> the seven device tensors ``adjust`` takes, in its order (None stays None)."""
        up = self._up
        return (up(cameras, np.float64, (-1, 17)), up(track_off, np.int64, (-1,)), up(image, np.int32, (-1,)), up(uv, np.float32, (-1, 2)), up(point, np.float64, (-1, 3)),
                up(track_enable, np.uint8, (-1,)), up(meas_enable, np.uint8, (-1,)))
