"""Drop-in for ``gtsfm/data_association/point3d_initializer.py``: landmark initialisation from feature tracks at known cameras, with or
without RANSAC over measurement pairs, for a whole list of tracks in one device launch.

PARITY UNPINNED towards gtsam: ``gtsam.triangulatePoint3`` and ``np.random.choice`` are restated (tests/triangulation_reference.py is
the specification, the reference's known answers and the Lund door expectations are pinned there). Measurements are read as float32
pixels, the precision of GTSfM's keypoint coordinates.

Where GTSfM is importable, ``TriangulationExitCode``, ``TriangulationSamplingMode`` and ``TriangulationOptions`` are the reference's own
classes, and a calibration that is not a pure pinhole goes to the reference's ``Point3dInitializer``; elsewhere it raises
``NotImplementedError`` naming the calibration -- distortion is never ignored."""

from __future__ import annotations

import sys
from enum import Enum
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from gtsfm_amd.common.sfm_track import SfmTrack2d

NUM_SAMPLES_PER_RANSAC_HYPOTHESIS = 2

try:  # pragma: no cover - exercised only where GTSfM is installed
    from gtsfm.data_association.point3d_initializer import Point3dInitializer as _ReferenceInitializer  # type: ignore
    from gtsfm.data_association.point3d_initializer import TriangulationExitCode, TriangulationOptions, TriangulationSamplingMode  # type: ignore  # noqa: F401
except Exception:  # noqa: BLE001 - any import failure (cv2, gtsam, ...) selects the restated classes
    _ReferenceInitializer = None

    class TriangulationExitCode(Enum):  # type: ignore[no-redef]
        SUCCESS = 0
        CHEIRALITY_FAILURE = 1
        INLIERS_UNDERCONSTRAINED = 2
        POSES_UNDERCONSTRAINED = 3
        EXCEEDS_REPROJ_THRESH = 4
        LOW_TRIANGULATION_ANGLE = 5

    class TriangulationSamplingMode(str, Enum):  # type: ignore[no-redef]
        NO_RANSAC = "NO_RANSAC"
        RANSAC_SAMPLE_UNIFORM = "RANSAC_SAMPLE_UNIFORM"
        RANSAC_SAMPLE_BIASED_BASELINE = "RANSAC_SAMPLE_BIASED_BASELINE"
        RANSAC_TOPK_BASELINES = "RANSAC_TOPK_BASELINES"

    class TriangulationOptions(NamedTuple):  # type: ignore[no-redef]
        """``point3d_initializer.py:61-112``."""

        mode: TriangulationSamplingMode
        reproj_error_threshold: float = np.inf
        min_triangulation_angle: float = 0.0
        min_inlier_ratio: float = 0.1
        confidence: float = 0.9999
        dyn_num_hypotheses_multiplier: float = 3.0
        min_num_hypotheses: int = 0
        max_num_hypotheses: int = sys.maxsize

        def num_ransac_hypotheses(self) -> int:
            assert self.reproj_error_threshold > 0
            assert 0 < self.min_inlier_ratio < 1
            assert 0 < self.confidence < 1
            assert self.dyn_num_hypotheses_multiplier > 0
            assert 0 <= self.min_num_hypotheses < self.max_num_hypotheses
            dyn = int((np.log(1 - self.confidence) / np.log(1 - self.min_inlier_ratio**NUM_SAMPLES_PER_RANSAC_HYPOTHESIS)) * self.dyn_num_hypotheses_multiplier)
            return max(min(self.max_num_hypotheses, dyn), self.min_num_hypotheses)


try:  # pragma: no cover - exercised only where gtsam is installed
    from gtsam import SfmTrack  # type: ignore
except Exception:  # noqa: BLE001

    class SfmTrack:  # type: ignore[no-redef]
        """The part of ``gtsam.SfmTrack`` the pipeline reads: a landmark and its (image, uv) measurements."""

        def __init__(self, point3: np.ndarray):
            self._p = np.asarray(point3, dtype=np.float64).reshape(3)
            self._m: List[Tuple[int, np.ndarray]] = []

        def point3(self) -> np.ndarray:
            return self._p

        def numberMeasurements(self) -> int:  # noqa: N802 - gtsam's name
            return len(self._m)

        def measurement(self, k: int) -> Tuple[int, np.ndarray]:
            return self._m[k]

        def addMeasurement(self, i: int, uv: np.ndarray) -> None:  # noqa: N802
            self._m.append((int(i), np.asarray(uv)))


def tracks_to_csr(tracks_2d: Sequence[SfmTrack2d]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    lengths = np.fromiter((len(t.measurements) for t in tracks_2d), dtype=np.int64, count=len(tracks_2d))
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    image = np.fromiter((m.i for t in tracks_2d for m in t.measurements), dtype=np.int32, count=int(off[-1]))
    uv = np.array([np.asarray(m.uv, dtype=np.float32).reshape(2) for t in tracks_2d for m in t.measurements], dtype=np.float32).reshape(-1, 2)
    return off, image, uv


class Point3dInitializer:
    """``Point3dInitializer(track_camera_dict, options)``; ``triangulate(track_2d)`` has the reference's signature and return triple,
    ``triangulate_batch(tracks_2d)`` returns the list of those triples from one launch. ``seed`` keys the sampler of tracks with more
    measurement pairs than hypotheses."""

    def __init__(self, track_camera_dict: Dict[int, object], options, seed: int = 0, device=None) -> None:
        if len(track_camera_dict) == 0:
            raise ValueError("No camera positions were estimated, so triangulation is not feasible.")
        self.track_camera_dict = track_camera_dict
        self.options = options
        self.seed = int(seed)
        self._device = device
        self._engine = None  # lazy: the object must pickle before first use (Dask scatter)
        self._table = None
        self._reference = None
        from gtsfm_amd.runtime.triangulation_engine import pack_cameras

        try:
            self._table = pack_cameras(track_camera_dict)
        except NotImplementedError:
            if _ReferenceInitializer is None:
                raise
            self._reference = _ReferenceInitializer(track_camera_dict, options)  # pragma: no cover

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_engine"] = None
        return state

    def triangulate_arrays(self, track_off, image, uv) -> Dict[str, object]:
        """CSR tracks (host arrays or device tensors) -> the device call's outputs as device tensors."""
        if self._table is None:
            raise NotImplementedError("the cameras are not pure pinholes; only triangulate / triangulate_batch reach the reference's class")
        if self._engine is None:
            from gtsfm_amd.runtime.triangulation_engine import TriangulationEngine

            self._engine = TriangulationEngine(self._device)
        o = self.options
        mode = getattr(o.mode, "name", str(o.mode))
        return self._engine.triangulate(track_off, image, uv, self._table, mode=mode, reproj_error_threshold=float(o.reproj_error_threshold),
                                        min_triangulation_angle_deg=float(o.min_triangulation_angle),
                                        num_hypotheses=0 if mode == "NO_RANSAC" else o.num_ransac_hypotheses(), seed=self.seed)

    def triangulate_batch(self, tracks_2d: Sequence[SfmTrack2d]) -> List[Tuple[Optional[SfmTrack], Optional[float], TriangulationExitCode]]:
        if self._reference is not None:  # pragma: no cover
            return [self._reference.triangulate(t) for t in tracks_2d]
        if len(tracks_2d) == 0:
            return []
        off, image, uv = tracks_to_csr(tracks_2d)
        out = self.triangulate_arrays(off, image, uv)
        point, avg, code, mask = (out[k].cpu().numpy() for k in ("point", "avg_error", "exit_code", "inlier_mask"))
        results = []
        for j, track in enumerate(tracks_2d):
            exit_code = TriangulationExitCode(int(code[j]))
            error = None if np.isnan(avg[j]) else float(avg[j])
            track_3d = None
            if exit_code == TriangulationExitCode.SUCCESS:
                track_3d = SfmTrack(point[j].copy())
                for k, (i, m_uv) in enumerate(track.measurements):
                    if mask[off[j] + k]:
                        track_3d.addMeasurement(int(i), m_uv)
            results.append((track_3d, error, exit_code))
        return results

    def triangulate(self, track_2d: SfmTrack2d) -> Tuple[Optional[SfmTrack], Optional[float], TriangulationExitCode]:
        return self.triangulate_batch([track_2d])[0]
