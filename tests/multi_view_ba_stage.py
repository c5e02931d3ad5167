"""Global bundle adjustment as the last stage of the planted chain of tests/multi_view_scene.py: the restatement
(tests/global_ba_reference.py) on what the triangulation leaves -- the camera table, the track CSR, the points, the exit codes and the inlier
mask --, the similarity fit of its result to the planted geometry, and what the chain's tests assert about the kept tracks."""

from __future__ import annotations

from typing import Dict

import numpy as np

from tests import global_ba_reference as ba_ref
from tests import multi_view_scene as M
from tests import triangulation_reference as tri
from tests.multi_view_translation_stage import MARGIN  # noqa: F401 - the chain's standing margin for float64 stages fed upstream outputs

# What the device test asserts, measured on the restatements end to end (tests/test_multi_view_chain_ba_host.py prints the figures of
# profiles/multi_view_chain.txt): after a least-squares similarity fit of the camera centres to the planted ones, the largest centre error
# relative to the scene's extent and the median distance of a kept track's point from its planted point, BEFORE the adjustment (the recovered
# centres, the triangulated points) and AFTER it.
MEASURED_CENTRE_ERROR_REL_BEFORE = 2.82e-3  # the similarity fit; the scale-and-shift fit of the translation stage gives 2.93e-3
MEASURED_CENTRE_ERROR_REL_AFTER = 8.33e-4
MEASURED_POINT_MEDIAN_BEFORE = 0.03222
MEASURED_POINT_MEDIAN_AFTER = 0.01385
OPTIONS = dict(measurement_sigma=1.0, huber_k=1.345, reproj_error_threshold=3.0)  # unified.yaml: HUBER, sigma 1.0, the last of [10, 5, 3]


def ba_stage(table, track_off, image, uv, point, exit_code, inlier_mask, **options) -> Dict[str, object]:
    return ba_ref.solve(table, track_off, image, uv, point, (np.asarray(exit_code) == tri.SUCCESS).astype(np.uint8), inlier_mask, **dict(OPTIONS, **options))


def fit(scene: Dict[str, object], table: np.ndarray) -> Dict[str, object]:
    """The cameras' centres (rows of a camera table; valid == 0: none) fitted to the planted centres by a least-squares similarity: the largest
    error relative to the planted centres' extent, and ``move`` for the points."""
    truth = np.asarray(scene["centre"], np.float64)
    centres = np.where(table[:M.NUM_IMAGES, :1] != 0, table[:M.NUM_IMAGES, 14:17], np.nan)
    fitted, s, rot = ba_ref.fit_similarity(centres, truth)
    ok = np.isfinite(fitted).all(1)
    extent = float((truth.max(0) - truth.min(0)).max())
    mean_x, mean_t = centres[ok].mean(0), truth[ok].mean(0)
    return {"relative": float(np.linalg.norm(fitted[ok] - truth[ok], axis=1).max() / extent), "extent": extent, "scale": s, "cameras": int(ok.sum()),
            "move": lambda p: s * (np.asarray(p, np.float64) - mean_x) @ rot.T + mean_t}


def kept_tracks(scene: Dict[str, object], fitted: Dict[str, object], track_off, image, kp, point, keep) -> Dict[str, object]:
    """Of the tracks of ``keep``: how many are one planted point's, their distances from it after the fit, and how many hold a ghost keypoint."""
    which = M.track_points(scene, track_off, image, kp)
    keep = np.asarray(keep) != 0
    pure = keep & (which >= 0)
    dist = np.linalg.norm(fitted["move"](np.asarray(point)[pure]) - scene["points"][which[pure]], axis=1)
    ghosts = sum(M.ghost_measurements(scene, image[a:b], kp[a:b]) > 0 for a, b, k in zip(track_off[:-1], track_off[1:], keep) if k)
    return {"kept": int(keep.sum()), "pure": int(pure.sum()), "distance": dist, "ghost_tracks": int(ghosts)}
