"""CPU restatement of track triangulation (numpy, float64): the specification of gtsfm_amd/csrc/triangulation_kernels.hip.

PARITY UNPINNED towards gtsam
-----------------------------
Restated from ``gtsfm/data_association/point3d_initializer.py``, ``gtsfm/utils/reprojection.py``, ``gtsfm/utils/tracks.py:83-103`` and
``gtsfm/densify/mvs_utils.py:23-52``. gtsam cannot be imported where this suite runs, so
``gtsam.triangulatePoint3(cameras, measurements, rank_tol=1e-9, optimize=True)`` is restated from its documented behaviour:

* DLT: rows ``u P[2] - P[0]`` and ``v P[2] - P[1]`` with ``P = K [wRc^T | -wRc^T wtc]``; fewer than 3 singular values above
  ``rank_tol`` is "underconstrained"; otherwise the last right singular vector, dehomogenised. Here numpy's SVD; the device reduces
  the rows to a 4 x 4 triangle by Givens rotations in measurement order and runs a one-sided Jacobi on it.
* Refinement: damped Gauss-Newton on the pixel reprojection error of the three point coordinates, ``GN_STEPS`` steps, always.
  gtsam's Levenberg-Marquardt stops by a data-dependent rule ("decrease < 1e-5, absolute or relative"); on the Lund door tracks that
  rule lands up to 4.2e-5 (relative point) / 0.0062 px (average error) away from the converged point, while 6 and 10 fixed steps
  agree to every printed digit. A step that raises the cost is discarded and costs one of the steps (the damping grows tenfold), so
  ``GN_STEPS`` = 8 = the 6 measured to suffice plus two discarded ones. The fixed count lets every lane of a wave run the same loop.
  A non-positive pivot or a non-finite step fails the hypothesis.
* Cheirality: depth <= 0 in any camera used fails the call (gtsam's ``RuntimeError``).

Sampling when a track has more measurement pairs than hypotheses cannot be pinned to ``np.random.choice``: the pairs (in
``itertools.combinations`` order) get a key from a counter-based generator, the verifier's splitmix64 of (seed, track key, pair index),
and the ``num_hypotheses`` smallest keys are taken: the hashed integer itself (uniform), an exponential clock ``-log(u) / baseline``
(biased baseline: successive weighted draws without replacement), or ``-baseline`` with ties to the larger index, which is a stable
ascending argsort's tail (top-k). The track key hashes the track's first measurement (image, float32 bits of u and v), so a track
draws the same pairs wherever it stands in a batch. When ``num_hypotheses`` equals the number of pairs every pair is evaluated and the
reference's permutation only reorders them; exact ties go to the lowest pair index, one of the reference's own possible outcomes.

Sums over a track's measurements run in measurement order.

Validity domain
---------------
``dlt`` (numpy's SVD) resolves a singular value to about eps x sigma_max ABSOLUTE, so on badly scaled scenes it is less accurate than
the device, whose Givens / one-sided Jacobi keeps small singular values to relative accuracy. ``dlt_jacobi`` is a float64 port of the
device's solve; ``triangulate_point(..., solver="jacobi")`` uses it. The default stays numpy: the Lund door fixture was recorded with
it. Measured against the high-precision arbiter (tests/triangulation_arbiter.py; figures in profiles/triangulation_hard_scenes.txt):
with the numpy solver the restatement agrees with the arbiter on the synthetic scenes and the Lund door (point 1.1e-8 relative, average
error 4.6e-7 px at worst, inside the tolerances those scenes use) and is a valid specification within about 1e3 units of the origin. On
the 8-camera circle at world offset (5e5, 4e6, 100) its DLT point for a neighbour pair is 3.3e-3 units off (6.4e-10 with the port) and
it reports rank 3 for a facing pair whose exact sigma_3 is 4e-15; near rank deficiency (sigma_3 <= 1e-6) its points are up to 0.55
relative off where the port's are 8e-9. With EITHER solver the fixed ``GN_STEPS`` hold the cost within 1e-5 max(1, cost) of the minimum
down to baseline / depth 1e-5 near the origin, but not at baseline / depth 1e-3 with a world offset of 1e5 or more: the homogeneous DLT
is not invariant under translation and starts too far away (gap 9.5e-5, or another winning pair). No test compares the device there.
"""

from __future__ import annotations

import itertools
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

GN_STEPS = 8
JACOBI_SWEEPS = 10
RANK_TOL = 1e-9
LAMBDA_INITIAL, LAMBDA_FACTOR, LAMBDA_FLOOR = 1e-5, 10.0, 1e-20
MAX_TRACK_REPROJ_ERROR = float(np.finfo(np.float32).max)

SUCCESS, CHEIRALITY_FAILURE, INLIERS_UNDERCONSTRAINED, POSES_UNDERCONSTRAINED, EXCEEDS_REPROJ_THRESH, LOW_TRIANGULATION_ANGLE = range(6)
NO_RANSAC, RANSAC_SAMPLE_UNIFORM, RANSAC_SAMPLE_BIASED_BASELINE, RANSAC_TOPK_BASELINES = range(4)
MODE_NAMES = ("NO_RANSAC", "RANSAC_SAMPLE_UNIFORM", "RANSAC_SAMPLE_BIASED_BASELINE", "RANSAC_TOPK_BASELINES")

_M64 = (1 << 64) - 1


def pack_camera(fx: float, fy: float, cx: float, cy: float, wRc: np.ndarray, wtc: np.ndarray) -> np.ndarray:
    """One row of the device's camera table: valid, fx, fy, cx, cy, wRc row-major, wtc."""
    return np.concatenate([[1.0, fx, fy, cx, cy], np.asarray(wRc, np.float64).reshape(9), np.asarray(wtc, np.float64).reshape(3)])


def camera_table(cameras: Dict[int, np.ndarray], num_images: Optional[int] = None) -> np.ndarray:
    n = (max(cameras) + 1 if cameras else 0) if num_images is None else num_images
    table = np.zeros((n, 17))
    for i, c in cameras.items():
        if c is not None:
            table[i] = c
    return table


def _camera(table: np.ndarray, i: int) -> Optional[np.ndarray]:
    return table[i] if 0 <= i < len(table) and table[i, 0] != 0.0 else None


def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def track_key(image0: int, uv0: np.ndarray) -> int:
    bits = np.asarray(uv0, np.float32).view(np.uint32)
    k = splitmix64(((int(image0) & 0xFFFFFFFF) << 32) ^ int(bits[0]))
    return splitmix64(k ^ int(bits[1]))


def pair_hash(seed: int, tkey: int, p: int) -> int:
    return splitmix64((seed & _M64) ^ splitmix64(tkey ^ p))


def baseline(c1: Optional[np.ndarray], c2: Optional[np.ndarray]) -> float:
    """|wRc1^T (wtc2 - wtc1)|, the reference's ``wTc1.inverse().compose(wTc2).translation()``; 0 with a camera missing."""
    if c1 is None or c2 is None:
        return 0.0
    r, d = c1[5:14], c2[14:17] - c1[14:17]
    x = float(r[0]) * float(d[0]) + float(r[3]) * float(d[1]) + float(r[6]) * float(d[2])
    y = float(r[1]) * float(d[0]) + float(r[4]) * float(d[1]) + float(r[7]) * float(d[2])
    z = float(r[2]) * float(d[0]) + float(r[5]) * float(d[1]) + float(r[8]) * float(d[2])
    return math.sqrt(x * x + y * y + z * z)


def select_pairs(table: np.ndarray, images: Sequence[int], uv: np.ndarray, mode: int, num_hypotheses: int, seed: int) -> List[int]:
    """Indices (ascending) of the evaluated pairs in ``itertools.combinations`` order."""
    n = len(images)
    total = n * (n - 1) // 2
    h = min(int(num_hypotheses), total)
    if h >= total:
        return list(range(total))
    pairs = list(itertools.combinations(range(n), 2))
    tkey = track_key(images[0], uv[0])
    keys = np.empty(total)
    for p, (k1, k2) in enumerate(pairs):
        if mode == RANSAC_SAMPLE_UNIFORM:
            keys[p] = float(pair_hash(seed, tkey, p) >> 11)
        else:
            w = baseline(_camera(table, images[k1]), _camera(table, images[k2]))
            if mode == RANSAC_TOPK_BASELINES:
                keys[p] = -w
            else:
                u = (float(pair_hash(seed, tkey, p) >> 11) + 0.5) * 2.0**-53
                keys[p] = -math.log(u) / w if w > 0.0 else math.inf
    tie = -np.arange(total) if mode == RANSAC_TOPK_BASELINES else np.arange(total)
    order = np.lexsort((tie, keys))
    return sorted(int(p) for p in order[:h])


def project(cam: np.ndarray, x: np.ndarray) -> Tuple[float, float, float]:
    r, d = cam[5:14], x - cam[14:17]
    p0 = r[0] * d[0] + r[3] * d[1] + r[6] * d[2]
    p1 = r[1] * d[0] + r[4] * d[1] + r[7] * d[2]
    p2 = r[2] * d[0] + r[5] * d[1] + r[8] * d[2]
    return cam[1] * p0 / p2 + cam[3], cam[2] * p1 / p2 + cam[4], p2


def dlt(cams: Sequence[np.ndarray], uvs: Sequence[np.ndarray]) -> Optional[np.ndarray]:
    rows = []
    for cam, uv in zip(cams, uvs):
        rt = cam[5:14].reshape(3, 3).T
        m = -(rt @ cam[14:17])
        p = np.hstack([rt, m[:, None]])
        p0, p1, p2 = cam[1] * p[0] + cam[3] * p[2], cam[2] * p[1] + cam[4] * p[2], p[2]
        rows += [uv[0] * p2 - p0, uv[1] * p2 - p1]
    _, s, vt = np.linalg.svd(np.array(rows))
    if int((s > RANK_TOL).sum()) < 3:
        return None
    v = vt[-1]
    return v[:3] / v[3]


def givens_row(r: List[List[float]], a: List[float]) -> None:
    """Rotates one row into the 4 x 4 upper triangle ``r`` (the device's ``tri_givens_row``)."""
    for j in range(4):
        h = math.sqrt(r[j][j] * r[j][j] + a[j] * a[j])
        if a[j] == 0.0 or not h > 0.0:
            continue
        c, s = r[j][j] / h, a[j] / h
        for k in range(j, 4):
            t = c * r[j][k] + s * a[k]
            a[k] = c * a[k] - s * r[j][k]
            r[j][k] = t


def jacobi_triangle(g: List[List[float]], sweeps: int = JACOBI_SWEEPS) -> Tuple[List[float], List[List[float]]]:
    """One-sided Jacobi (Hestenes) on the columns of ``g`` (destroyed): the column norms and V (the device's ``tri_dlt_solve``)."""
    v = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(sweeps):
        for p in range(3):
            for q in range(p + 1, 4):
                alpha = beta = gamma = 0.0
                for i in range(4):
                    alpha += g[i][p] * g[i][p]
                    beta += g[i][q] * g[i][q]
                    gamma += g[i][p] * g[i][q]
                if not abs(gamma) > 1.0e-17 * math.sqrt(alpha * beta):
                    continue
                zeta = (beta - alpha) / (2.0 * gamma)
                t = (1.0 if zeta >= 0.0 else -1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
                c = 1.0 / math.sqrt(1.0 + t * t)
                s = c * t
                for i in range(4):
                    gp, gq = g[i][p], g[i][q]
                    g[i][p], g[i][q] = c * gp - s * gq, s * gp + c * gq
                    vp, vq = v[i][p], v[i][q]
                    v[i][p], v[i][q] = c * vp - s * vq, s * vp + c * vq
    sigma = [math.sqrt(g[0][j] * g[0][j] + g[1][j] * g[1][j] + g[2][j] * g[2][j] + g[3][j] * g[3][j]) for j in range(4)]
    return sigma, v


def dlt_jacobi(cams: Sequence[np.ndarray], uvs: Sequence[np.ndarray]) -> Optional[np.ndarray]:
    """Float64 port of the device's DLT: Givens row insertion in measurement order, ``JACOBI_SWEEPS`` Hestenes sweeps with the 1e-17
    skip test, rank against ``RANK_TOL``, the column of the smallest norm (the first one among equals)."""
    r = [[0.0] * 4 for _ in range(4)]
    with np.errstate(all="ignore"):
        for cam, uv in zip(cams, uvs):
            cam = [float(c) for c in cam]
            rot, t = cam[5:14], cam[14:17]
            p = [[rot[j], rot[3 + j], rot[6 + j], -(rot[j] * t[0] + rot[3 + j] * t[1] + rot[6 + j] * t[2])] for j in range(3)]
            u, w = float(uv[0]), float(uv[1])
            a = [u * p[2][k] - (cam[1] * p[0][k] + cam[3] * p[2][k]) for k in range(4)]
            b = [w * p[2][k] - (cam[2] * p[1][k] + cam[4] * p[2][k]) for k in range(4)]
            givens_row(r, a)
            givens_row(r, b)
        try:
            sigma, v = jacobi_triangle(r)
        except (OverflowError, ValueError):
            return None
        if sum(1 for s in sigma if s > RANK_TOL) < 3:
            return None
        last, smallest = 0, math.inf
        for j in range(4):
            if sigma[j] < smallest:
                smallest, last = sigma[j], j
        return np.array([v[0][last], v[1][last], v[2][last]]) / np.float64(v[3][last])


SOLVERS = {"numpy": dlt, "jacobi": dlt_jacobi}


def _normal_equations(cams, uvs, x):
    """cost = 1/2 sum r^2, H = J^T J (upper triangle as 6 numbers), g = J^T r; sums in measurement order."""
    cost, h, g = 0.0, [0.0] * 6, [0.0] * 3
    for cam, uv in zip(cams, uvs):
        r, d = cam[5:14], x - cam[14:17]
        p0 = r[0] * d[0] + r[3] * d[1] + r[6] * d[2]
        p1 = r[1] * d[0] + r[4] * d[1] + r[7] * d[2]
        p2 = r[2] * d[0] + r[5] * d[1] + r[8] * d[2]
        ru, rv = cam[1] * p0 / p2 + cam[3] - uv[0], cam[2] * p1 / p2 + cam[4] - uv[1]
        a, b0, b1 = 1.0 / p2, cam[1] * p0 / (p2 * p2), cam[2] * p1 / (p2 * p2)
        ju = [cam[1] * a * r[0] - b0 * r[2], cam[1] * a * r[3] - b0 * r[5], cam[1] * a * r[6] - b0 * r[8]]
        jv = [cam[2] * a * r[1] - b1 * r[2], cam[2] * a * r[4] - b1 * r[5], cam[2] * a * r[7] - b1 * r[8]]
        cost += 0.5 * (ru * ru + rv * rv)
        k = 0
        for i in range(3):
            g[i] += ju[i] * ru + jv[i] * rv
            for j in range(i, 3):
                h[k] += ju[i] * ju[j] + jv[i] * jv[j]
                k += 1
    return cost, h, g


def _cost(cams, uvs, x) -> float:
    cost = 0.0
    for cam, uv in zip(cams, uvs):
        u, v, _ = project(cam, x)
        cost += 0.5 * ((u - uv[0]) * (u - uv[0]) + (v - uv[1]) * (v - uv[1]))
    return cost


def _solve_spd3(h, g, lam) -> Optional[np.ndarray]:
    """(H + lam I) d = -g by elimination without pivoting; None for a pivot that is not positive."""
    a00, a01, a02, a11, a12, a22 = h[0] + lam, h[1], h[2], h[3] + lam, h[4], h[5] + lam
    b0, b1, b2 = -g[0], -g[1], -g[2]
    if not a00 > 0.0:
        return None
    l10, l20 = a01 / a00, a02 / a00
    a11, a12, a22 = a11 - l10 * a01, a12 - l10 * a02, a22 - l20 * a02
    b1, b2 = b1 - l10 * b0, b2 - l20 * b0
    if not a11 > 0.0:
        return None
    l21 = a12 / a11
    a22, b2 = a22 - l21 * a12, b2 - l21 * b1
    if not a22 > 0.0:
        return None
    d2 = b2 / a22
    d1 = (b1 - a12 * d2) / a11
    d0 = (b0 - a01 * d1 - a02 * d2) / a00
    d = np.array([d0, d1, d2])
    return d if np.all(np.isfinite(d)) else None


def refine(cams, uvs, x: np.ndarray, steps: int = GN_STEPS) -> Optional[np.ndarray]:
    lam = LAMBDA_INITIAL
    with np.errstate(all="ignore"):
        for _ in range(steps):
            e, h, g = _normal_equations(cams, uvs, x)
            d = _solve_spd3(h, g, lam)
            if d is None:
                return None
            xn = x + d
            en = _cost(cams, uvs, xn)
            if math.isfinite(en) and not en > e:
                x, lam = xn, max(lam / LAMBDA_FACTOR, LAMBDA_FLOOR)
            else:
                lam = lam * LAMBDA_FACTOR
    return x


def triangulate_point(cams, uvs, steps: int = GN_STEPS, solver: str = "numpy") -> Optional[np.ndarray]:
    """gtsam.triangulatePoint3(..., rank_tol=1e-9, optimize=True); None where it raises. ``solver``: "numpy" (LAPACK's SVD) or
    "jacobi" (the float64 port of the device's solve, see the validity domain above)."""
    with np.errstate(all="ignore"):
        x = SOLVERS[solver](cams, uvs)
        if x is None or not np.all(np.isfinite(x)):
            return None
        x = refine(cams, uvs, x, steps)
        if x is None:
            return None
        for cam in cams:
            if not project(cam, x)[2] > 0.0:
                return None
    return x


def reprojection_errors(table: np.ndarray, x: np.ndarray, images: Sequence[int], uv: np.ndarray) -> np.ndarray:
    out = np.full(len(images), np.nan)
    with np.errstate(all="ignore"):
        for k, i in enumerate(images):
            cam = _camera(table, i)
            if cam is None:
                continue
            u, v, z = project(cam, x)
            if z > 0.0:
                du, dv = u - uv[k][0], v - uv[k][1]
                out[k] = math.sqrt(du * du + dv * dv)
    return out


def max_triangulation_angle_deg(table: np.ndarray, x: np.ndarray, images: Sequence[int]) -> float:
    rays = []
    for i in images:
        d = x - table[i, 14:17]
        rays.append(d / math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
    best = -math.inf
    for a, b in itertools.combinations(rays, 2):
        dot = min(1.0, max(-1.0, a[0] * b[0] + a[1] * b[1] + a[2] * b[2]))
        best = max(best, math.degrees(math.acos(dot)))
    return best


def triangulate_track(table: np.ndarray, images: Sequence[int], uv: np.ndarray, mode: int = NO_RANSAC, threshold: float = math.inf,
                      min_angle_deg: float = 0.0, num_hypotheses: int = 2749, seed: int = 0, steps: int = GN_STEPS, detail: Optional[dict] = None,
                      solver: str = "numpy"):
    """One track: (point [3] or NaNs, average error or NaN, exit code, inlier mask [n], stats [4]). ``uv`` float64 (n, 2); ``detail``
    receives the per-hypothesis (votes, mean error, inlier mask) of a RANSAC run, for the fixture's decisiveness test."""
    images = [int(i) for i in images]
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    n = len(images)
    nan3 = np.full(3, np.nan)
    stats = np.array([0, 0, -1, 0], np.int32)
    inl = np.ones(n, bool)
    if n < 2:
        return nan3, math.nan, INLIERS_UNDERCONSTRAINED, np.zeros(n, bool) if mode != NO_RANSAC else inl, stats
    if mode != NO_RANSAC:
        pairs = list(itertools.combinations(range(n), 2))
        chosen = select_pairs(table, images, uv, mode, num_hypotheses, seed)
        best_votes, best_err, inl = 0, MAX_TRACK_REPROJ_ERROR, np.zeros(n, bool)
        stats[0] = len(chosen)
        for p in chosen:
            k1, k2 = pairs[p]
            c1, c2 = _camera(table, images[k1]), _camera(table, images[k2])
            x = None if c1 is None or c2 is None else triangulate_point([c1, c2], [uv[k1], uv[k2]], steps, solver)
            if x is None:
                stats[1] += 1
                continue
            err = reprojection_errors(table, x, images, uv)
            ok = err < threshold
            votes = int(ok.sum())
            if detail is not None:
                detail.setdefault("hyp", []).append((p, votes, ok.copy(), err.copy()))
            if votes > 0:
                mean = 0.0
                for k in range(n):
                    if ok[k]:
                        mean += err[k]
                mean /= votes
                if votes > best_votes or (votes == best_votes and mean < best_err):
                    best_votes, best_err, inl = votes, mean, ok
                    stats[2], stats[3] = p, votes
    idx = [k for k in range(n) if inl[k]]
    if len(idx) < 2:
        return nan3, math.nan, INLIERS_UNDERCONSTRAINED, inl, stats
    used = [k for k in idx if _camera(table, images[k]) is not None]
    if len(used) < 2:
        return nan3, math.nan, POSES_UNDERCONSTRAINED, inl, stats
    x = triangulate_point([table[images[k]] for k in used], [uv[k] for k in used], steps, solver)
    if x is None:
        return nan3, math.nan, CHEIRALITY_FAILURE, inl, stats
    err = reprojection_errors(table, x, [images[k] for k in idx], uv[idx])
    good = err[~np.isnan(err)]
    avg = math.nan
    if good.size:
        avg = 0.0
        for e in good:
            avg += e
        avg /= good.size
    if detail is not None:
        detail["final_err"] = err
    if not np.all(err < threshold):
        return nan3, avg, EXCEEDS_REPROJ_THRESH, inl, stats
    if min_angle_deg > 0.0 and max_triangulation_angle_deg(table, x, [images[k] for k in idx]) < min_angle_deg:
        return nan3, avg, LOW_TRIANGULATION_ANGLE, inl, stats
    return x, avg, SUCCESS, inl, stats


def non_decisive(detail: dict, threshold: float, margin: float = 1e-6) -> bool:
    """A track whose inlier mask or exit code a rounding difference may flip: some hypothesis's (or the final point's) error lies
    within ``margin`` px of the threshold, or a rival hypothesis with another inlier set lies within ``margin`` px of the winner's mean
    error at equal votes."""
    errs = [h[3] for h in detail.get("hyp", [])] + ([detail["final_err"]] if "final_err" in detail else [])
    for err in errs:
        e = err[np.isfinite(err)]
        if e.size and math.isfinite(threshold) and np.any(np.abs(e - threshold) < margin):
            return True
    scored = [(votes, float(err[ok].mean()), ok) for _, votes, ok, err in detail.get("hyp", []) if votes > 0]
    if scored:
        top = max(s[0] for s in scored)
        best = min((s for s in scored if s[0] == top), key=lambda s: s[1])
        for votes, mean, ok in scored:
            if votes == top and abs(mean - best[1]) < margin and not np.array_equal(ok, best[2]):
                return True
    return False


def triangulate_tracks(table: np.ndarray, track_off: np.ndarray, image: np.ndarray, uv: np.ndarray, **options) -> Dict[str, np.ndarray]:
    """The device call's outputs for CSR tracks (``uv`` float32, as the device reads it), and ``non_decisive`` per track."""
    t = len(track_off) - 1
    out = {"point": np.full((t, 3), np.nan), "avg_error": np.full(t, np.nan), "exit_code": np.zeros(t, np.int32),
           "inlier_mask": np.zeros(len(image), np.uint8), "stats": np.zeros((t, 4), np.int32), "non_decisive": np.zeros(t, bool)}
    for j in range(t):
        a, b = int(track_off[j]), int(track_off[j + 1])
        detail: dict = {}
        x, avg, code, inl, stats = triangulate_track(table, image[a:b], np.asarray(uv[a:b], np.float32).astype(np.float64), detail=detail, **options)
        out["non_decisive"][j] = non_decisive(detail, options.get("threshold", math.inf))
        out["point"][j], out["avg_error"][j], out["exit_code"][j], out["stats"][j] = x, avg, code, stats
        out["inlier_mask"][a:b] = inl
    return out


def lookat_camera(eye: np.ndarray, target: np.ndarray, up: np.ndarray, f: float, cx: float = 0.0, cy: float = 0.0) -> np.ndarray:
    """gtsam's ``PinholeCamera.Lookat``: z towards the target, x = z cross (-up)... i.e. x = (-up) x z normalised, y = z x x."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(-up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return pack_camera(f, f, cx, cy, np.stack([x, y, z], axis=1), eye)
