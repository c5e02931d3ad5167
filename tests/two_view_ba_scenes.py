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


def make_general_pair(seed: int, n: int, rotvec=(0.0, -0.1, 0.0), centre=(1.0, 0.0, 0.0), focal: float = F, principal=(CX, CY), depth=(4.0, 9.0),
                      planar: bool = False, translation_scale: float = 1.0, noise: float = 0.5, outliers: float = 0.1, perturb: float = 0.02) -> Dict[str, np.ndarray]:
    """``make_pair`` with the geometry open: ``rotvec`` is the rotation vector of i2Ri1, camera 2's centre lies at ``centre`` (made unit:
    the baseline is 1) in camera 1's frame, both cameras have the focal length ``focal`` (camera 2's 1 % longer) and the principal point
    ``principal``; the points lie ``depth`` deep in front of camera 1 (``planar``: on one slanted plane through that range) and at least
    0.5 deep in front of camera 2; the starting translation is the perturbed unit one times ``translation_scale``."""
    rng = np.random.default_rng(seed)
    r_true = _rot(np.asarray(rotvec, np.float64))
    c = np.asarray(centre, np.float64) / np.linalg.norm(centre)
    t_true = -r_true @ c
    pts = np.zeros((0, 3))
    while len(pts) < n:
        cand = np.stack([rng.uniform(-2.0, 2.0, 4 * n), rng.uniform(-1.5, 1.5, 4 * n), rng.uniform(depth[0], depth[1], 4 * n)], axis=1)
        if planar:
            cand[:, 2] = 0.5 * (depth[0] + depth[1]) + 0.25 * (depth[1] - depth[0]) * (0.5 * cand[:, 0] + 0.3 * cand[:, 1])
        pts = np.concatenate([pts, cand[(cand @ r_true.T + t_true)[:, 2] > 0.5]])
    pts = pts[:n]
    k1 = np.array([focal, focal, principal[0], principal[1]])
    k2 = np.array([focal * 1.01, focal * 1.01, principal[0] + 3.0, principal[1] - 2.0])

    def project(k, x):
        return np.stack([k[0] * x[:, 0] / x[:, 2] + k[2], k[1] * x[:, 1] / x[:, 2] + k[3]], axis=1)

    uv1 = project(k1, pts) + rng.normal(0.0, noise, (n, 2))
    uv2 = project(k2, pts @ r_true.T + t_true) + rng.normal(0.0, noise, (n, 2))
    bad = rng.random(n) < outliers
    uv2[bad] += rng.normal(0.0, 2.5, (int(bad.sum()), 2))
    r0 = _rot(rng.normal(0.0, perturb / np.sqrt(3.0), 3)) @ r_true
    t0 = _rot(rng.normal(0.0, perturb / np.sqrt(3.0), 3)) @ t_true
    return {"k1": k1, "k2": k2, "uv1": uv1.astype(np.float32), "uv2": uv2.astype(np.float32), "R": r0, "t": translation_scale * t0 / np.linalg.norm(t0),
            "R_true": r_true, "t_true": t_true}


def displaced_pair(seed: int, n: int, every: int = 3, by: float = 40.0, **kw) -> Dict[str, np.ndarray]:
    """Every ``every``-th second pixel moved by ``by`` px in both coordinates: gross outliers that the Huber loss must carry."""
    pair = make_pair(seed, n, **kw)
    pair["uv2"][::every] += np.float32(by)
    return pair


def late_first_pair(seed: int, n: int = 300, late: int = 270) -> Dict[str, np.ndarray]:
    """The first ``late`` correspondences cannot be triangulated (their second pixel is 400 px off: behind the cameras), so the first
    triangulated one, which carries the point prior, is correspondence ``late``."""
    pair = make_pair(seed, n)
    pair["uv2"][:late, 0] += np.float32(400.0)
    return pair


HARD_FAMILIES = ("rejections", "step_limit", "late_first", "triangulation_options", "geometry", "loss", "strides", "non_finite", "non_decisive")
DECISIVE_FAMILIES = HARD_FAMILIES[:-1]


def hard_pairs() -> Dict[str, List[Dict[str, object]]]:
    """The catalogue of hard pairs: family -> entries ``{"name", "pair", "options"}`` (``options``: what differs from the defaults of
    tests/two_view_ba_reference.py). What every family must contain is asserted on the restatement by tests/test_two_view_ba_host.py; every
    family but ``non_decisive`` holds decisive pairs only (the seeds were chosen for it)."""
    def entry(name, pair, **options):
        return {"name": name, "pair": pair, "options": options}

    inf = float("inf")
    out = {
        # far starts and gross outliers: the fidelity test rejects trials, lambda climbs and comes back
        "rejections": [entry("far_23", make_pair(23, 24, perturb=0.1)), entry("farther_506", make_pair(506, 24, perturb=0.2)),
                       entry("farther_502", make_pair(502, 48, perturb=0.2)), entry("displaced_505", displaced_pair(505, 24)),
                       entry("displaced_534", displaced_pair(534, 24)),
                       entry("far_n300", make_pair(81, 300, perturb=0.1)), entry("far_n600", make_pair(81, 600, perturb=0.1))],
        # the limit counts ACCEPTED steps: it cuts runs whose first solves were rejected, and a run with more than 100 solves at 100 steps
        "step_limit": [entry(f"limit_{k}", make_pair(315, 24, perturb=0.1), max_iterations=k) for k in (1, 2, 3, 4)]  # left alone it stops by tolerance after 5 steps
                      + [entry("behind_limit_5", behind_pair(), max_iterations=5), entry("displaced_100", displaced_pair(42, 24))],
        # the point that carries the prior in a second stride (slice row >= 256), and in a lane other than 0 of the first
        "late_first": [entry("second_stride_91", late_first_pair(91)), entry("second_stride_92", late_first_pair(92)),
                       entry("other_lane", late_first_pair(91, n=150, late=100))],
        "triangulation_options": [entry("threshold_2", make_pair(93, 40, outliers=0.3), triangulation_threshold=2.0),
                                  entry("min_angle_1", make_pair(93, 40, outliers=0.3), triangulation_min_angle_deg=1.0),
                                  # 20 - 120 deep at baseline 1: parallax 0.5 - 2.9 degrees, so one degree divides the points
                                  entry("deep_min_angle_1", make_general_pair(602, 40, depth=(20.0, 120.0), outliers=0.3), triangulation_min_angle_deg=1.0),
                                  entry("min_angle_8", make_pair(94, 40, outliers=0.3), triangulation_min_angle_deg=8.0)],
        "geometry": [entry("planar", make_general_pair(61, 40, planar=True)), entry("wide_rotation", make_general_pair(62, 40, rotvec=(0.0, 0.9, 0.0))),
                     entry("roll", make_general_pair(63, 40, rotvec=(0.0, 0.0, 3.1))),
                     entry("long_focal", make_general_pair(64, 40, focal=3000.0, principal=(2000.0, 1500.0))),
                     entry("translation_x5", make_general_pair(65, 40, translation_scale=5.0)),
                     entry("translation_x1e-3", make_general_pair(95, 40, translation_scale=1e-3))],
        "loss": [entry("no_robust_loss", make_pair(71, 40), huber_k=inf), entry("huber_0.1", make_pair(72, 40), huber_k=0.1),
                 entry("sigma_0.5", make_pair(73, 40), measurement_sigma=0.5), entry("no_filter", make_pair(74, 40), reproj_error_threshold=inf)],
        "strides": [entry("n1100", make_pair(99, 1100))],
        # every scaled residual overflows: the initial cost is inf, every trial is rejected, lambda runs into its bound. The threshold of
        # 4.2 px splits the entering points' reprojection errors (2.2 .. 5.9 px, none within 0.1 px of it): the filter's mask is neither
        # empty nor full where the pair is let through, and empty only because the pair is given up where it is not
        "non_finite": [entry("given_up", make_pair(400, 20, outliers=0.0), measurement_sigma=1e-160, reproj_error_threshold=4.2),
                       entry("allowed", make_pair(400, 20, outliers=0.0), measurement_sigma=1e-160, reproj_error_threshold=4.2, allow_indeterminate=True)],
        # honestly non-decisive: the undamped system's pivots are rounding-level by nature
        "non_decisive": [entry("forward", make_general_pair(66, 40, centre=(0.05, 0.02, 1.0))),
                         entry("translation_x1e3", make_general_pair(67, 40, translation_scale=1e3)), entry("rotation", rotation_pair())],
    }
    assert tuple(out) == HARD_FAMILIES
    return out


def dud_row_layouts(pair: Dict[str, np.ndarray], **layout_options):
    """Three layouts of one pair that differ in one row below ``match_count``: (its mask at 0, the row verified with ``match_idx`` -1, the
    row verified with a NaN pixel in its first keypoint), and the row. A verified row that cannot be triangulated counts as verified and
    changes nothing else."""
    base = capacity_layout([pair], **layout_options)
    unverified = np.flatnonzero(base["inlier_mask"][:int(base["match_count"][0])] == 0)
    row = int(unverified[len(unverified) // 2])
    no_index, nan_pixel = ({k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in base.items()} for _ in range(2))
    no_index["inlier_mask"][row] = nan_pixel["inlier_mask"][row] = 1
    no_index["match_idx"][row] = -1
    nan_pixel["kp_xy"][int(base["kp_off1"][0]) + int(base["match_idx"][row, 0]), 0] = np.nan
    return base, no_index, nan_pixel, row
