"""Translation recovery as a stage of the planted chain of tests/multi_view_scene.py: the restatement (tests/translation_recovery_reference.py)
on the rows the 1DSfM rejection leaves -- the pair rows and the track CSR with their world directions and the two inlier masks --, the fit of
its gauge (anchor at 0, the scale of one row) to the planted centres, and the triangulation with the recovered cameras."""

from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from tests import multi_view_scene as M
from tests import translation_recovery_reference as tr_ref
from tests import triangulation_reference as tri

# What the device test asserts, measured on the restatements end to end (tests/test_multi_view_chain_translation_host.py prints the figures of
# profiles/multi_view_chain.txt): the largest camera-centre error after the scale-and-shift fit, relative to the scene's extent. The bound is
# 8 x the measured value: the project's standing margin for float64 stages, here over a stage fed upstream outputs that differ from the
# restatement's own in the last bits.
MEASURED_CENTRE_ERROR_REL = 2.93e-3
MARGIN = 8.0


def recovery_stage(rows: Sequence, world_pair, pair_enable, track_off, image, world_meas, meas_enable, **options) -> Dict[str, object]:
    return tr_ref.solve(np.asarray(rows, np.int64).reshape(-1, 2), world_pair, pair_enable, track_off, image, world_meas, meas_enable, num_images=M.NUM_IMAGES, **options)


def centre_errors(scene: Dict[str, object], centres: np.ndarray) -> Dict[str, object]:
    """``centres`` [N, 3] (NaN for a camera without one) fitted to the planted centres by a least-squares scale and shift: the fitted
    centres, the scale, the shift and the largest error relative to the planted centres' extent (the longest side of their bounding box)."""
    truth = np.asarray(scene["centre"], np.float64)
    fitted, s = tr_ref.fit_scale_shift(np.asarray(centres, np.float64), truth)
    ok = np.isfinite(fitted).all(1)
    extent = float((truth.max(0) - truth.min(0)).max())
    shift = (fitted[ok] - s * np.asarray(centres)[ok]).mean(0)
    return {"fitted": fitted, "scale": s, "shift": shift, "extent": extent, "relative": float(np.linalg.norm(fitted[ok] - truth[ok], axis=1).max() / extent), "cameras": int(ok.sum())}


def triangulate_with(scene: Dict[str, object], rotations: Sequence[Optional[np.ndarray]], centres: np.ndarray, track_off, image, kp) -> Dict[str, np.ndarray]:
    """tests/triangulation_reference.triangulate_tracks with the given cameras (no planted centre enters)."""
    table = np.stack([tri.pack_camera(*scene["intrinsics"][i], rotations[i], centres[i]) for i in range(M.NUM_IMAGES)])
    return tri.triangulate_tracks(table, track_off, image, scene["xy"][image, kp], **M.triangulation_options())


def on_planted_point(scene: Dict[str, object], fit: Dict[str, object], track_off, image, kp, point, exit_code) -> Dict[str, object]:
    """The triangulated points moved to the planted gauge by the centres' fit, then ``M.point_distances``."""
    moved = fit["scale"] * np.asarray(point, np.float64) + fit["shift"]
    return M.point_distances(scene, track_off, image, kp, moved, exit_code)
