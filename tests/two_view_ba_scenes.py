"""Seeded synthetic image pairs for the two-view bundle adjustment tests, and their batch in the verifier's capacity layout.

A pair: points 4 - 9 units deep in front of camera 1, baseline 1, f = 800, 0.5 px noise, 10 % of the matches displaced by sigma = 2.5 px (so
both Huber branches occur), pixel coordinates rounded to float32, the starting pose off the true one by 0.02 rad."""

from __future__ import annotations

import zlib
from typing import Dict, List, Optional

import numpy as np

F, CX, CY = 800.0, 320.0, 240.0
BATCH_COUNTS = (0, 5, 15, 16, 255, 256, 257, 600)  # below the minimum, the lane-count boundaries, a third stride with a ragged tail


def _rot(w: np.ndarray) -> np.ndarray:
    theta = float(np.linalg.norm(w))
    if theta == 0.0:
        return np.eye(3)
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / theta
    return np.eye(3) + np.sin(theta) * k + (1.0 - np.cos(theta)) * (k @ k)


def make_pair(seed: int, n: int, noise: float = 0.5, outliers: float = 0.1, perturb: float = 0.02, baseline: float = 1.0, fy_ratio: float = 1.0) -> Dict[str, np.ndarray]:
    """``k1``, ``k2`` (fx, fy, cx, cy); ``uv1``, ``uv2`` [n, 2] float32; ``R`` / ``t``: the starting i2Ri1 and unit i2Ui1; ``R_true`` / ``t_true``."""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4.0, 9.0, n)], axis=1)
    r_true = _rot(rng.normal(0.0, 0.05, 3) + np.array([0.0, -0.1, 0.0]))
    direction = np.array([1.0, 0.0, 0.0]) + rng.normal(0.0, 0.1, 3)
    t_true = -baseline * direction / np.linalg.norm(direction)  # i2ti1: camera 2 sits at +direction in camera 1's frame, about
    k1 = np.array([F, F * fy_ratio, CX, CY])
    k2 = np.array([F * 1.01, F * 1.01 * fy_ratio, CX + 3.0, CY - 2.0])

    def project(k, x):
        return np.stack([k[0] * x[:, 0] / x[:, 2] + k[2], k[1] * x[:, 1] / x[:, 2] + k[3]], axis=1)

    uv1 = project(k1, pts) + rng.normal(0.0, noise, (n, 2))
    uv2 = project(k2, pts @ r_true.T + t_true) + rng.normal(0.0, noise, (n, 2))
    bad = rng.random(n) < outliers
    uv2[bad] += rng.normal(0.0, 2.5, (int(bad.sum()), 2))
    r0 = _rot(rng.normal(0.0, perturb / np.sqrt(3.0), 3)) @ r_true
    t0 = _rot(rng.normal(0.0, perturb / np.sqrt(3.0), 3)) @ t_true
    t0 = t0 / np.linalg.norm(t0) if baseline > 0 else t0
    return {"k1": k1, "k2": k2, "uv1": uv1.astype(np.float32), "uv2": uv2.astype(np.float32), "R": r0, "t": t0, "R_true": r_true,
            "t_true": t_true / max(np.linalg.norm(t_true), 1e-300)}


def exact_pair(seed: int = 3, n: int = 40) -> Dict[str, np.ndarray]:
    """Noise-free, started at the true pose: the first step leaves."""
    return make_pair(seed, n, noise=0.0, outliers=0.0, perturb=0.0)


def nan_pose_pair(seed: int = 4, n: int = 30) -> Dict[str, np.ndarray]:
    pair = make_pair(seed, n)
    pair["R"], pair["t"] = np.full((3, 3), np.nan), np.full(3, np.nan)
    return pair


def flipped_pair(seed: int = 5, n: int = 30) -> Dict[str, np.ndarray]:
    """The translation flipped: every triangulation fails cheirality."""
    pair = make_pair(seed, n, perturb=0.0)
    pair["t"] = -pair["t"]
    return pair


def rotation_pair(seed: int = 6, n: int = 40) -> Dict[str, np.ndarray]:
    """Nearly a pure rotation (baseline 1e-9 of the depth): the depths, hence the system, are all but indeterminate."""
    return make_pair(seed, n, baseline=1e-9, perturb=0.0, outliers=0.0)


def behind_pair(seed: int = 7, n: int = 30) -> Dict[str, np.ndarray]:
    """One match whose second pixel is far off: its point triangulates just in front of the cameras and the adjustment pushes it about."""
    pair = make_pair(seed, n)
    pair["uv2"][3] = pair["uv2"][3] + np.float32(60.0)
    return pair


def door_pair(door: Dict[str, np.ndarray], i1: int, i2: int, perturb: float = 0.02, seed: int = 8) -> Optional[Dict[str, np.ndarray]]:
    """The two-image tracks of cameras (i1, i2) of tests/golden/triangulation_lund_door.npz, and their relative pose perturbed."""
    off, image, uv, cams = door["track_off"], door["image"], door["uv"], door["cameras"]
    uv1, uv2 = [], []
    for j in range(len(off) - 1):
        a, b = int(off[j]), int(off[j + 1])
        if b - a == 2 and sorted(image[a:b].tolist()) == sorted((i1, i2)):
            first = a if image[a] == i1 else a + 1
            uv1.append(uv[first])
            uv2.append(uv[2 * a + 1 - first])
    if not uv1:
        return None
    c1, c2 = cams[i1], cams[i2]
    r1, r2 = c1[5:14].reshape(3, 3), c2[5:14].reshape(3, 3)
    r = r2.T @ r1  # i2Ri1
    t = r2.T @ (c1[14:17] - c2[14:17])
    rng = np.random.default_rng(seed)
    r0 = _rot(rng.normal(0.0, perturb / np.sqrt(3.0), 3)) @ r
    t0 = _rot(rng.normal(0.0, perturb / np.sqrt(3.0), 3)) @ (t / np.linalg.norm(t))
    return {"k1": c1[1:5].copy(), "k2": c2[1:5].copy(), "uv1": np.asarray(uv1, np.float32), "uv2": np.asarray(uv2, np.float32), "R": r0, "t": t0,
            "R_true": r, "t_true": t / np.linalg.norm(t)}


def batch_pairs(seed: int = 100) -> List[Dict[str, np.ndarray]]:
    return [make_pair(seed + i, n) for i, n in enumerate(BATCH_COUNTS)]


def special_pairs() -> Dict[str, Dict[str, np.ndarray]]:
    return {"exact": exact_pair(), "nan_pose": nan_pose_pair(), "flipped": flipped_pair(), "rotation": rotation_pair(), "behind": behind_pair()}


def capacity_layout(pairs: List[Dict[str, np.ndarray]], seed: int = 1, slack: int = 7, unverified: float = 0.3) -> Dict[str, np.ndarray]:
    """The verifier's arrays for a batch: every pair gets keypoint tables of its own (shuffled), a slice of ``match_idx`` longer than its
    ``match_count``, and unverified rows (mask 0) interleaved with the verified ones (the same way for the same pair and ``seed``,
    whatever the batch). ``rows[p]``: the rows of pair p's verified
    correspondences, in order. Rows past ``match_count`` hold indices that must never be read (-1) and a mask of 1."""
    kp, off1, off2, idx, mask, moff, count, rows, intr, rot, trans = [], [], [], [], [], [0], [], [], [], [], []
    base = 0
    for pair in pairs:
        n = len(pair["uv1"])
        # seeded by the pair itself: the same pair gets the same slice (which rows are verified decides which lane owns a point, hence the
        # order of the device's sums) wherever it stands in whatever batch
        rng = np.random.default_rng([seed, n, zlib.crc32(np.ascontiguousarray(pair["uv1"]).tobytes())])
        extra = int(np.ceil(unverified * n)) + 1
        m = n + extra
        verified = np.zeros(m, bool)
        verified[np.sort(rng.choice(m, n, replace=False))] = True
        uv1 = np.zeros((m, 2), np.float32)
        uv2 = np.zeros((m, 2), np.float32)
        uv1[verified], uv2[verified] = pair["uv1"], pair["uv2"]
        uv1[~verified] = rng.uniform(0.0, 600.0, (extra, 2)).astype(np.float32)
        uv2[~verified] = rng.uniform(0.0, 600.0, (extra, 2)).astype(np.float32)
        p1, p2 = rng.permutation(m), rng.permutation(m)  # row j uses keypoint p1[j] of image 1
        t1, t2 = np.zeros((m, 2), np.float32), np.zeros((m, 2), np.float32)
        t1[p1], t2[p2] = uv1, uv2
        off1.append(base)
        off2.append(base + m)
        kp += [t1, t2]
        base += 2 * m
        cap = m + slack
        block = np.full((cap, 2), -1, np.int32)
        block[:m, 0], block[:m, 1] = p1, p2
        idx.append(block)
        mask.append(np.concatenate([verified.astype(np.uint8), np.ones(slack, np.uint8)]))
        rows.append(moff[-1] + np.flatnonzero(verified))
        moff.append(moff[-1] + cap)
        count.append(m)
        intr.append(np.concatenate([pair["k1"], pair["k2"]]))
        rot.append(pair["R"].reshape(9))
        trans.append(pair["t"])
    return {"kp_xy": np.concatenate(kp), "kp_off1": np.asarray(off1, np.int64), "kp_off2": np.asarray(off2, np.int64), "match_idx": np.concatenate(idx),
            "match_off": np.asarray(moff, np.int64), "match_count": np.asarray(count, np.int32), "inlier_mask": np.concatenate(mask),
            "intrinsics": np.asarray(intr, np.float64), "rotation": np.asarray(rot, np.float64), "translation": np.asarray(trans, np.float64), "rows": rows}


def verified_scene_arrays(pairs: List[Dict[str, np.ndarray]], **layout_options) -> Dict[str, object]:
    """The same batch as a scene of 2 P images in the generators' layout (one feature table [2 P, cap, 2], pair p = images (2 p, 2 p + 1)):
    ``xy``, one verifier launch's host arrays (``match_idx``, ``match_off``, ``match_count``, ``mask``, ``R``, ``t``, ``stats``, ``pairs``),
    and the host dictionaries ``putative`` / ``verified`` of ``generate_correspondences_and_verify``. A pair without a pose is what the
    verifier leaves of it: no inliers, NaN matrices, the failure tuple."""
    lay = capacity_layout(pairs, **layout_options)
    num = len(pairs)
    counts = lay["match_count"]
    cap = int(max(counts.max(initial=0), 1))
    xy = np.zeros((2 * num, cap, 2), np.float32)
    mask = lay["inlier_mask"].copy()
    stats = np.zeros((num, 8), np.int32)
    putative, verified = {}, {}
    for p, pair in enumerate(pairs):
        m, a = int(counts[p]), int(lay["match_off"][p])
        xy[2 * p, :m] = lay["kp_xy"][lay["kp_off1"][p]:lay["kp_off1"][p] + m]
        xy[2 * p + 1, :m] = lay["kp_xy"][lay["kp_off2"][p]:lay["kp_off2"][p] + m]
        rows = lay["match_idx"][a:a + m].astype(np.int64)
        putative[(2 * p, 2 * p + 1)] = rows
        keep = mask[a:a + m].astype(bool)
        if np.isfinite(pair["R"]).all() and keep.any():
            stats[p, 0] = int(keep.sum())
            verified[(2 * p, 2 * p + 1)] = (pair["R"], pair["t"], rows[keep], float(keep.mean()))
        else:
            mask[a:int(lay["match_off"][p + 1])] = 0
            verified[(2 * p, 2 * p + 1)] = (None, None, np.array([], dtype=np.uint64), 0.0)
    rot = np.where(stats[:, :1, None] > 0, lay["rotation"].reshape(num, 3, 3), np.nan)
    trans = np.where(stats[:, :1] > 0, lay["translation"], np.nan)
    return {"xy": xy, "launch": {"match_idx": lay["match_idx"], "match_off": lay["match_off"].tolist(), "match_count": counts, "mask": mask, "R": rot, "t": trans,
                                 "stats": stats, "pairs": [(2 * p, 2 * p + 1) for p in range(num)]},
            "putative": putative, "verified": verified, "intrinsics": lay["intrinsics"], "layout": lay}
