"""Seeded synthetic scenes for the triangulation tests: the smallest shapes at which the kernels take another path."""

from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from tests import triangulation_reference as ref

NUM_CAMERAS = 80
INVALID = (3, 7)  # images without an estimated camera
LOOSE = dict(threshold=10.0, num_hypotheses=100)


def cameras(seed: int = 5) -> np.ndarray:
    rng = np.random.default_rng(seed)
    table = np.zeros((NUM_CAMERAS + 2, 17))  # two more rows than cameras: images 80 and 81 exist but have no estimate
    for i in range(NUM_CAMERAS):
        th = 2.0 * np.pi * i / NUM_CAMERAS * 0.6
        eye = np.array([10.0 * np.cos(th), 10.0 * np.sin(th), 0.0]) + rng.normal(0.0, 0.3, 3)
        table[i] = ref.lookat_camera(eye, rng.normal(0.0, 0.3, 3), [0.0, 0.0, 1.0], 800.0 + 3.0 * i, 640.0, 480.0)
        table[i, 2] = table[i, 1] * 1.01  # fy != fx
    for i in INVALID:
        table[i, 0] = 0.0
    return table


def _measure(table: np.ndarray, image: int, x: np.ndarray, rng, noise: float = 0.5) -> np.ndarray:
    u, v, _ = ref.project(table[image], x)
    return np.array([u, v]) + rng.normal(0.0, noise, 2)


def small_shapes(seed: int = 11) -> Dict[str, np.ndarray]:
    """CSR tracks: lengths 0, 1, 2, 3, 14, 15 and 75 (1, 3, 91 hypotheses; 105 > 100 and 2 775 > 2 749 pairs exercise the sampler), a
    first measurement without a camera, no camera at all, an image index outside the table, two measurements in one image, outliers,
    crossed measurements (a point behind the cameras), and short filler tracks up to a count that is no multiple of the 256 tracks of
    a workgroup; the hypothesis segments of the long tracks straddle wave and workgroup boundaries."""
    rng = np.random.default_rng(seed)
    table = cameras()
    valid = [i for i in range(NUM_CAMERAS) if i not in INVALID]
    tracks: List[List[Tuple[int, np.ndarray]]] = []

    def track(images, outliers=(), noise=0.5):
        x = rng.uniform(-2.0, 2.0, 3)
        meas = [(int(i), _measure(table, int(i), x, rng, noise) if table[int(i), 0] else rng.uniform(0.0, 900.0, 2)) for i in images]
        for k in outliers:
            meas[k] = (meas[k][0], meas[k][1] + rng.choice([-1.0, 1.0], 2) * rng.uniform(40.0, 80.0, 2))
        tracks.append(meas)

    for n in (2, 3, 14, 15, 14, 15, 3, 2):
        track(sorted(rng.choice(valid, n, replace=False)))
    track(sorted(rng.choice(valid, 15, replace=False)), outliers=(4,))
    track(sorted(rng.choice(valid, 14, replace=False)), outliers=(0, 13))
    track(sorted(rng.choice(valid, 6, replace=False)), outliers=(2,))
    track([3, 10, 20, 30])            # the first measurement's camera is not estimated
    track([3, 7])                     # no camera at all
    track([3, 12])                    # one camera: POSES_UNDERCONSTRAINED without RANSAC
    track([5, 81, 40])                # an image beyond the cameras that exist
    track([9, 30, 9, 50])             # two measurements in one image
    tracks.append([])                 # an empty track
    track([15])                       # a single measurement
    track([20, 21])                   # crossed: each camera gets the other's pixel, the rays meet behind the cameras
    tracks[-1] = [(20, tracks[-1][1][1]), (21, tracks[-1][0][1])]
    track([40, 41], noise=0.0)        # neighbours: a small triangulation angle
    track([0, 79], noise=0.0)         # the ends of the arc: a large one
    track([i for i in range(78) if i not in INVALID][:75], outliers=(10, 50))
    while len(tracks) < 301:
        track(sorted(rng.choice(valid, int(rng.integers(2, 5)), replace=False)), outliers=(0,) if rng.random() < 0.15 else ())
    order = rng.permutation(len(tracks))  # the long tracks do not sit at the front
    tracks = [tracks[j] for j in order]
    off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    image = np.array([m[0] for t in tracks for m in t], dtype=np.int32)
    uv = np.array([m[1] for t in tracks for m in t], dtype=np.float32).reshape(-1, 2)
    return {"cameras": table, "track_off": off, "image": image, "uv": uv}


def reversed_tracks(off: np.ndarray, image: np.ndarray, uv: np.ndarray):
    idx = np.concatenate([np.arange(a, b)[::-1] for a, b in zip(off[:-1], off[1:])] + [np.zeros(0, np.int64)]).astype(np.int64)
    return image[idx], uv[idx], idx


def reversal_tolerance(scene: Dict[str, np.ndarray], factor: float = 8.0) -> Tuple[float, float]:
    """The fixture's recipe on this scene: ``factor`` x the largest difference between the restatement on each track's measurements in
    forward and in reversed order (relative point distance, average error in px), over NO_RANSAC without a threshold and over
    RANSAC_SAMPLE_UNIFORM on the tracks whose pairs are all evaluated (a sampled track draws other pairs when reversed)."""
    off, image, uv, table = scene["track_off"], scene["image"], scene["uv"], scene["cameras"]
    rimage, ruv, idx = reversed_tracks(off, image, uv)
    rel, dif = [1e-16], [1e-16]
    for opts in (dict(mode=ref.NO_RANSAC), dict(mode=ref.RANSAC_SAMPLE_UNIFORM, **LOOSE)):
        sampled = np.array([opts["mode"] != ref.NO_RANSAC and (b - a) * (b - a - 1) // 2 > LOOSE["num_hypotheses"] for a, b in zip(off[:-1], off[1:])])
        keep = np.concatenate([[0], np.cumsum(np.where(sampled, 0, np.diff(off)))])
        sel = np.concatenate([np.arange(a, b) for a, b, s in zip(off[:-1], off[1:], sampled) if not s])
        fwd = ref.triangulate_tracks(table, keep, image[sel], uv[sel], **opts)
        rev = ref.triangulate_tracks(table, keep, rimage[sel], ruv[sel], **opts)
        same = (fwd["exit_code"] == rev["exit_code"]) & ~fwd["non_decisive"]
        ok = same & (fwd["exit_code"] == ref.SUCCESS)
        rel.append(float(np.max(np.linalg.norm(fwd["point"][ok] - rev["point"][ok], axis=1) / np.linalg.norm(fwd["point"][ok], axis=1), initial=0.0)))
        fin = same & np.isfinite(fwd["avg_error"]) & np.isfinite(rev["avg_error"])
        dif.append(float(np.max(np.abs(fwd["avg_error"][fin] - rev["avg_error"][fin]), initial=0.0)))
    return factor * max(rel), factor * max(dif)
