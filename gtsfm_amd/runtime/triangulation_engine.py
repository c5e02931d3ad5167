"""Host side of the device triangulation: ``gtsfm_triangulate_tracks_f64`` triangulates every feature track of a scene in one call,
replacing the per-track loop of ``gtsfm/data_association/data_assoc.py:205-273`` over ``point3d_initializer.py``. PyTorch provides
device memory and copies only."""

from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from gtsfm_amd.runtime.engine_base import EngineBase

MODES = ("NO_RANSAC", "RANSAC_SAMPLE_UNIFORM", "RANSAC_SAMPLE_BIASED_BASELINE", "RANSAC_TOPK_BASELINES")
MAX_HYPOTHESES = (1 << 31) - 1  # a track has fewer pairs than this (at most 65535 measurements)
CAMERA_FIELDS = 17  # valid, fx, fy, cx, cy, wRc row-major, wtc


def pack_cameras(cameras: Dict[int, object], num_images: Optional[int] = None) -> np.ndarray:
    """[num_images, 17] float64 from ``{image: camera}``; a camera is anything with ``pose()`` (``rotation().matrix()``,
    ``translation()``) and ``calibration()``, ``None`` or a missing key an image without an estimate. A calibration that is not pure
    pinhole raises ``NotImplementedError``: its distortion must not be dropped silently."""
    from gtsfm_amd.common.calibration import pinhole_parameters

    keys = [int(i) for i in cameras]
    if any(i < 0 for i in keys):
        raise ValueError("negative image index in the camera dictionary")
    n = (max(keys) + 1 if keys else 0) if num_images is None else int(num_images)
    table = np.zeros((n, CAMERA_FIELDS), dtype=np.float64)
    for i, cam in cameras.items():
        if cam is None or int(i) >= n:
            continue
        cal = cam.calibration()
        fx, fy, cx, cy, pure = pinhole_parameters(cal)
        if not pure:
            raise NotImplementedError(f"camera {i}: calibration {type(cal).__name__} is not a pure pinhole; the device triangulation has no distortion model")
        pose = cam.pose()
        table[int(i), 0] = 1.0
        table[int(i), 1:5] = fx, fy, cx, cy
        table[int(i), 5:14] = np.asarray(pose.rotation().matrix(), dtype=np.float64).reshape(9)
        table[int(i), 14:17] = np.asarray(pose.translation(), dtype=np.float64).reshape(3)
    return table


class TriangulationEngine(EngineBase):
    def triangulate(self, track_off, image, uv, cameras, mode="NO_RANSAC", reproj_error_threshold: float = float("inf"),
                    min_triangulation_angle_deg: float = 0.0, num_hypotheses: int = 2749, seed: int = 0) -> Dict[str, object]:
        """``track_off`` [T + 1] int64, ``image`` [S] int32, ``uv`` [S, 2] float32: device tensors (used where they lie) or host arrays;
        ``cameras`` [num_images, 17] float64 (``pack_cameras``). Returns device tensors ``point`` [T, 3] / ``avg_error`` [T] float64,
        ``exit_code`` [T] int32, ``inlier_mask`` [S] uint8, ``stats`` [T, 4] int32."""
        torch = self._torch
        mode_id = MODES.index(getattr(mode, "name", mode)) if not isinstance(mode, int) else int(mode)
        off = self._dev(track_off, torch.int64)
        img = self._dev(image, torch.int32)
        xy = self._dev(uv, torch.float32).reshape(-1, 2)
        cams = self._dev(cameras, torch.float64).reshape(-1, CAMERA_FIELDS)
        num_tracks, total = int(off.numel()) - 1, int(img.numel())
        if num_tracks < 0 or int(xy.shape[0]) != total:
            raise ValueError(f"track_off has {off.numel()} entries; image has {total} and uv {xy.shape[0]} measurements")
        max_hyp = 0 if mode_id == 0 else max(0, min(int(num_hypotheses), MAX_HYPOTHESES))
        out = {"point": torch.full((num_tracks, 3), float("nan"), dtype=torch.float64, device=self.device),
               "avg_error": torch.full((num_tracks,), float("nan"), dtype=torch.float64, device=self.device),
               "exit_code": torch.zeros(num_tracks, dtype=torch.int32, device=self.device),
               "inlier_mask": torch.zeros(total, dtype=torch.uint8, device=self.device),
               "stats": torch.zeros((num_tracks, 4), dtype=torch.int32, device=self.device)}
        if num_tracks == 0:
            return out
        ws = self._sized_workspace("gtsfm_triangulate_workspace_bytes", num_tracks, total, max_hyp)
        ptr = self._ptr
        rc = self._lib.gtsfm_triangulate_tracks_f64(
            off.data_ptr(), ptr(img), ptr(xy), num_tracks, total, ptr(cams), int(cams.shape[0]),
            mode_id, float(reproj_error_threshold), float(min_triangulation_angle_deg), max_hyp, int(seed) & ((1 << 64) - 1), ws.data_ptr(), ws.numel(),
            out["point"].data_ptr(), out["avg_error"].data_ptr(), out["exit_code"].data_ptr(), ptr(out["inlier_mask"]), out["stats"].data_ptr(),
            self._stream())
        self._L.check(rc, "gtsfm_triangulate_tracks_f64")
        return out
