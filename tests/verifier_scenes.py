"""Scene catalogue of the verifier tests: named, seeded two-view inputs that drive ``oracle/verifier_oracle.py`` (and therefore
``verifier_kernels.hip``, which follows it operation for operation) through every exit of the RANSAC loop -- cameras with
fx != fy, cx != cy and K1 != K2, the widths the kernel is built around (minimum counts, 255 / 256 / 257 matches), degenerate
geometry, non-finite keypoints, seeds with the top bit set. numpy only; ``tests/test_verifier_scenes_host.py`` asserts that the
catalogue reaches the branches, ``tests/test_verifier_scenes_gpu.py`` that the device equals the oracle on all of it.

An entry is a dict: ``coordinates_i1/2`` float32 (N, 2), ``match_indices`` int32 (M, 2), ``intrinsics_i1/2`` (fx, fy, cx, cy),
``threshold_px``, ``seed``, ``modes`` (a subset of ("E", "F"): essential / fundamental matrix estimation), plus whatever the
planted geometry is known by (``i2Ri1``, ``nonfinite_rows``). Every index stays inside its keypoint table."""

from __future__ import annotations

from functools import lru_cache
from typing import Callable, Dict, List, Tuple

import numpy as np

from gtsfm_amd.utils import synthetic
from oracle import verifier_oracle as vo

K_A = (700.0, 820.0, 500.0, 530.0)  # camera 1: fx != fy, cx != cy
K_B = (910.0, 640.0, 560.0, 470.0)  # camera 2: another camera altogether
SIZE_A = (1000, 1060)  # (width, height), non-square
SIZE_B = (1120, 940)
BOTH = ("E", "F")
MIN_MATCHES = {"E": 6, "F": 8}  # below these the verifier fails without drawing a sample


def _entry(c1, c2, idx, k1, k2, thr, seed, modes=BOTH, **extra) -> Dict[str, object]:
    c1 = np.ascontiguousarray(c1, dtype=np.float32).reshape(-1, 2)
    c2 = np.ascontiguousarray(c2, dtype=np.float32).reshape(-1, 2)
    idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1, 2)
    assert c1.shape[0] > 0 and c2.shape[0] > 0
    assert idx.size == 0 or (idx.min() >= 0 and idx[:, 0].max() < c1.shape[0] and idx[:, 1].max() < c2.shape[0])
    return {"coordinates_i1": c1, "coordinates_i2": c2, "match_indices": idx, "intrinsics_i1": tuple(map(float, k1)),
            "intrinsics_i2": tuple(map(float, k2)), "threshold_px": float(thr), "seed": int(seed), "modes": tuple(modes), **extra}


def _from_synthetic(s, thr, seed, k1=None, k2=None, modes=BOTH, **extra):
    return _entry(s["coordinates_i1"], s["coordinates_i2"], s["match_indices"], k1 or s["intrinsics"], k2 or s["intrinsics"], thr, seed, modes,
                  i2Ri1=s["i2Ri1"], **extra)


def _project(points, k):
    return np.stack([points[:, 0] / points[:, 2] * k[0] + k[2], points[:, 1] / points[:, 2] * k[1] + k[3]], 1)


def _planted(points, rot, trans, k1, k2, rng, noise_px=0.0, num_outliers=0, size2=SIZE_B, num_extra=0):
    """``points`` (camera-1 frame) seen by camera 1 (K1) and by camera 2 = (rot, trans) with K2; the first ``num_outliers``
    matches re-pointed at random pixels of image 2; keypoint tables shuffled and padded so that indices are not the identity."""
    m = points.shape[0]
    uv1 = _project(points, k1) + noise_px * rng.normal(size=(m, 2))
    uv2 = _project(points @ rot.T + trans, k2) + noise_px * rng.normal(size=(m, 2))
    uv2[:num_outliers] = rng.uniform([0, 0], size2, size=(num_outliers, 2))
    extra1 = rng.uniform([0, 0], SIZE_A, size=(num_extra, 2))
    extra2 = rng.uniform([0, 0], size2, size=(num_extra, 2))
    perm1, perm2 = rng.permutation(m + num_extra), rng.permutation(m + num_extra)
    c1, c2 = np.concatenate([uv1, extra1], 0)[perm1], np.concatenate([uv2, extra2], 0)[perm2]
    order = rng.permutation(m)
    idx = np.stack([np.argsort(perm1)[:m], np.argsort(perm2)[:m]], 1)[order]
    return c1, c2, idx, (np.arange(m) >= num_outliers)[order]


def _slab(rng, m):
    return np.stack([rng.uniform(-4, 4, m), rng.uniform(-3, 3, m), rng.uniform(6, 14, m)], 1)


def _motion(rng, angle=0.25):
    rot = synthetic._rotation_about(rng.normal(size=3), angle)
    trans = rng.normal(size=3)
    return rot, trans / np.linalg.norm(trans)


def anisotropic():
    rng = np.random.default_rng(61)
    rot, trans = _motion(rng)
    c1, c2, idx, is_inlier = _planted(_slab(rng, 120), rot, trans, K_A, K_B, rng, noise_px=0.5, num_outliers=36, num_extra=11)
    return _entry(c1, c2, idx, K_A, K_B, 2.0, 4, i2Ri1=rot, is_inlier=is_inlier)


def wrong_k():
    """Coordinates projected with (800, 800, 512, 512), verified with two other cameras: no planted pose to recover, the
    normalisation alone decides the outcome."""
    return _from_synthetic(synthetic.synthetic_two_view_matches(120, 0.3, 0.5, seed=21, num_extra_keypoints=9), 2.0, 5, K_A, K_B)


def count_edge(m):
    def build():
        return _from_synthetic(synthetic.synthetic_two_view_matches(m, 0.3 if m > 20 else 0.0, 0.3, seed=100 + m, num_extra_keypoints=5), 2.0, m)

    return build


def heavy_outliers(share):
    def build():
        return _from_synthetic(synthetic.synthetic_two_view_matches(200, share, 0.5, seed=7), 1.0, 9)

    return build


def same_point_pair():
    c1 = np.array([[10.0, 20.0], [300.0, 400.0], [900.0, 50.0]])
    c2 = np.array([[350.0, 410.0], [5.0, 5.0]])
    return _entry(c1, c2, np.tile([[1, 0]], (40, 1)), K_A, K_B, 1.0, 2)


def identity_motion():
    rng = np.random.default_rng(62)
    c1, _, idx, _ = _planted(_slab(rng, 40), np.eye(3), np.zeros(3), K_A, K_A, rng, num_extra=4)
    return _entry(c1, c1.copy(), np.stack([idx[:, 0], idx[:, 0]], 1), K_A, K_A, 1.0, 3, modes=("E",))


def pure_rotation():
    rng = np.random.default_rng(63)
    rot = synthetic._rotation_about([0.2, 1.0, 0.1], 0.2)
    c1, c2, idx, _ = _planted(_slab(rng, 40), rot, np.zeros(3), K_A, K_B, rng, num_extra=3)
    return _entry(c1, c2, idx, K_A, K_B, 1.0, 4, i2Ri1=rot)


def collinear():
    rng = np.random.default_rng(64)
    s = rng.uniform(-1, 1, 40)
    points = np.array([0.3, -0.2, 9.0]) + s[:, None] * np.array([3.0, 2.0, 1.5])  # a 3-D line: a line in each image
    rot, trans = _motion(rng)
    c1, c2, idx, _ = _planted(points, rot, trans, K_A, K_B, rng, num_extra=3)
    return _entry(c1, c2, idx, K_A, K_B, 1.0, 5, i2Ri1=rot)


def one_plane():
    rng = np.random.default_rng(65)
    points = _slab(rng, 60)
    points[:, 2] = 9.0 + 0.1 * points[:, 0]
    rot, trans = _motion(rng)
    c1, c2, idx, _ = _planted(points, rot, trans, K_A, K_B, rng, noise_px=0.2, num_extra=3)
    return _entry(c1, c2, idx, K_A, K_B, 1.0, 6, i2Ri1=rot)


def non_finite():
    """Two matched keypoints of image 1 are NaN, one of image 2 is +inf (D2-Net can emit such rows); all three belong to
    planted inliers, so only their coordinates make them outliers."""
    s = synthetic.synthetic_two_view_matches(60, 0.2, 0.3, seed=33)
    rows = np.flatnonzero(s["is_inlier"])[[0, 7, 19]]
    c1, c2 = s["coordinates_i1"].copy(), s["coordinates_i2"].copy()
    c1[s["match_indices"][rows[0], 0]] = np.nan
    c1[s["match_indices"][rows[1], 0], 1] = np.nan
    c2[s["match_indices"][rows[2], 1], 0] = np.inf
    return _entry(c1, c2, s["match_indices"], s["intrinsics"], s["intrinsics"], 2.0, 33, i2Ri1=s["i2Ri1"], nonfinite_rows=np.sort(rows))


def tiny_threshold():
    return _from_synthetic(synthetic.synthetic_two_view_matches(30, 0.0, 1.0, seed=34), 1e-7, 34)


def vanishing_threshold():
    """threshold^2 underflows to zero: every model scores zero inliers, so a model is found and nothing is verified."""
    return _from_synthetic(synthetic.synthetic_two_view_matches(30, 0.0, 1.0, seed=36), 1e-200, 36)


def repeated_matches():
    s = synthetic.synthetic_two_view_matches(12, 0.0, 0.0, seed=35)
    s["match_indices"] = s["match_indices"][[0, 0, 1, 1, 2, 2, 3, 3]]
    return _from_synthetic(s, 1.0, 35)


def cheirality_sweep(k):
    def build():
        return _from_synthetic(synthetic.synthetic_two_view_matches(50, 0.2, 0.3, seed=200 + k), 2.0, k, modes=("E",))

    return build


def big_seed(seed):
    def build():
        return _from_synthetic(synthetic.synthetic_two_view_matches(60, 0.2, 0.3, seed=33), 2.0, seed, modes=("E",))

    return build


def too_few(m):
    """Below both minimum counts (m = 0: a pair without a single match): failure before any sample is drawn."""

    def build():
        s = synthetic.synthetic_two_view_matches(max(m, 1), seed=90 + m, num_extra_keypoints=2)
        s["match_indices"] = s["match_indices"][:m]
        return _from_synthetic(s, 1.0, m)

    return build


CATALOGUE: Dict[str, Callable[[], Dict[str, object]]] = {
    "anisotropic": anisotropic,
    "wrong_k": wrong_k,
    **{f"count_{m}": count_edge(m) for m in (6, 7, 8, 9, 255, 256, 257, 513)},
    **{f"outliers_{int(100 * share)}": heavy_outliers(share) for share in (0.8, 0.9, 0.95, 1.0)},
    "same_point_pair": same_point_pair,
    "identity_motion": identity_motion,
    "pure_rotation": pure_rotation,
    "collinear": collinear,
    "one_plane": one_plane,
    "non_finite": non_finite,
    "tiny_threshold": tiny_threshold,
    "vanishing_threshold": vanishing_threshold,
    "repeated_matches": repeated_matches,
    **{f"cheirality_{k}": cheirality_sweep(k) for k in range(16)},
    "seed_all_ones": big_seed(2**64 - 1),
    "seed_top_bit": big_seed(2**63),
    "seed_high_word": big_seed((7 << 32) | 3),
    "count_0": too_few(0),
    "count_5": too_few(5),
}


@lru_cache(maxsize=None)
def scene(name: str) -> Dict[str, object]:
    """The entry, built once; treat it as read-only."""
    s = CATALOGUE[name]()
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def cases() -> List[Tuple[str, str]]:
    """Every (entry, mode) of the catalogue."""
    return [(name, mode) for name in CATALOGUE for mode in scene(name)["modes"]]


def run_oracle(s: Dict[str, object], mode: str, **override) -> Dict[str, object]:
    """``vo.verify`` on an entry. A failure is told apart: ``no_model`` = no sample of the whole run produced a model (the
    device then writes NaN poses), against a model without a single inlier or a match count below the minimum."""
    a = {**s, **override}
    res = dict(vo.verify(a["coordinates_i1"], a["coordinates_i2"], a["match_indices"], a["intrinsics_i1"], a["intrinsics_i2"],
                         a["threshold_px"], seed=a["seed"], use_intrinsics_in_verification=mode == "E"))
    m = a["match_indices"].shape[0]
    res["num_matches"] = m
    if res["R"] is None:
        res["no_model"] = True
        if m >= MIN_MATCHES[mode]:
            idx = a["match_indices"].astype(np.int64)
            if mode == "E":
                x1 = vo.normalize_pinhole(a["coordinates_i1"], *a["intrinsics_i1"])[idx[:, 0]]
                x2 = vo.normalize_pinhole(a["coordinates_i2"], *a["intrinsics_i2"])[idx[:, 1]]
                raw = vo.ransac_essential(x1, x2, a["threshold_px"] / max(a["intrinsics_i1"][0], a["intrinsics_i2"][0]), a["seed"])["E"]
            else:
                p1 = np.asarray(a["coordinates_i1"], dtype=np.float64)[idx[:, 0]]
                p2 = np.asarray(a["coordinates_i2"], dtype=np.float64)[idx[:, 1]]
                raw = vo.ransac_fundamental(p1, p2, a["threshold_px"], a["seed"])["F"]
            res["no_model"] = raw is None
    return res


@lru_cache(maxsize=None)
def oracle(name: str, mode: str) -> Dict[str, object]:
    """The oracle's answer for (entry, mode), computed once per process and shared by every test; read-only."""
    return run_oracle(scene(name), mode)


def rotation_angle_deg(a: np.ndarray, b: np.ndarray) -> float:
    return float(np.degrees(np.arccos(np.clip((np.trace(a.T @ b) - 1.0) / 2.0, -1.0, 1.0))))
