"""Rotation averaging as a stage of the planted chain of tests/multi_view_scene.py: the rows ``VerifiedScene.rotation_averaging`` assembles (the
two-view rotations, weight = the square of the count of valid correspondences, enabled where the edge has a model and the view graph kept
it), the restatement on them, the alignment of its gauge to the planted rotations, and the stages after it fed the averaged rotations."""

from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np

from tests import multi_view_scene as M
from tests import rotation_averaging_reference as ra_ref
from tests import triangulation_reference as tri


def rotation_rows(rows: Sequence, enable: np.ndarray, counts: Sequence[int], edges_in: Iterable) -> Dict[str, np.ndarray]:
    """weight [E] and enable [E] of the rotation-averaging rows: ``counts`` is ``stats[:, 0]`` after ``two_view`` per row."""
    wanted = set(edges_in)
    c = np.asarray(counts, np.float64)
    return {"weight": c * c, "enable": np.array([bool(k) and n > 0 and e in wanted for e, k, n in zip(rows, enable, counts)], np.uint8)}


def rotation_stage(rows: Sequence, rotation: np.ndarray, weight: np.ndarray, enable: np.ndarray) -> Dict[str, object]:
    return ra_ref.solve(np.asarray(rows, np.int64).reshape(-1, 2), rotation, weight, enable, num_images=M.NUM_IMAGES)


def aligned_to_planted(scene: Dict[str, object], wri: Sequence[Optional[np.ndarray]], anchor: int) -> List[Optional[np.ndarray]]:
    """The averaged rotations (anchor = I) in the planted gauge: planted wR_anchor . averaged R_k."""
    return [None if r is None or not np.isfinite(r).all() else scene["wRi"][anchor] @ np.asarray(r, np.float64).reshape(3, 3) for r in wri]


def worst_input_error_deg(scene: Dict[str, object], rows: Sequence, rotation: np.ndarray, enable: np.ndarray) -> float:
    """The largest relative-rotation error among the rows given to the stage."""
    return max(M.pose_errors(scene, tuple(e), np.asarray(r).reshape(3, 3), np.array([1.0, 0.0, 0.0]))[0] for e, r, k in zip(rows, rotation, enable) if k)


def absolute_errors_deg(scene: Dict[str, object], aligned: Sequence[Optional[np.ndarray]]) -> np.ndarray:
    return np.array([np.nan if r is None else ra_ref.angle_deg(scene["wRi"][i], r) for i, r in enumerate(aligned)])


def downstream(restated: Dict[str, object], aligned: Sequence[np.ndarray], rows, direction, enable, corr, edges_in) -> Dict[str, object]:
    """1DSfM, the tracks and the triangulation of tests/multi_view_scene.py with ``aligned`` in place of the planted rotations (the planted
    centres and intrinsics stay): the inlier edge set and the number of tracks triangulated with SUCCESS."""
    scene = dict(restated["scene"], wRi=np.stack(aligned))
    ti = M.translation_stage(scene, rows, direction, enable, corr, edges_in, restated["threshold"])
    trk = M.tracks_stage(corr, ti["edges"])
    out = M.triangulation_stage(scene, trk["track_off"], trk["image"], trk["kp"])
    return {"edges": ti["edges"], "tracks": int(len(trk["track_off"]) - 1), "success": int((np.asarray(out["exit_code"]) == tri.SUCCESS).sum())}
