"""High-precision arbiter of track triangulation (mpmath, ``DIGITS`` digits): what the device, the host build of its kernels and the
float64 restatement (tests/triangulation_reference.py) are all measured against on hard geometry.

Per track, from the camera table and the float32 pixels as the device reads them:

* DLT: the exact singular values (``mp.svd_r``), the rank against ``ref.RANK_TOL`` and the null vector, dehomogenised.
* The TRUE minimiser of 1/2 sum r^2 (pixel reprojection residuals): damped Newton with the exact Hessian from the DLT point, iterated
  until the step is below ``STEP_RTOL`` relative. ``no finite minimiser`` when the iterate leaves ``BOUND`` x the scene's extent or
  does not settle in ``MAX_ITERATIONS`` (rays that do not meet: the infimum lies at infinity).
* Cheirality, reprojection errors, mean inlier error and the largest triangulation angle at that minimiser.
* The per-track procedure of ``ref.triangulate_track``: selected pairs (``ref.select_pairs``: integer and hash logic, no numerics),
  votes, the key (votes descending, mean error ascending, pair index ascending), the final n-view solve and the exit code.
* ``non_decisive``: the restatement's rule at its 1e-6 px margin, evaluated in high precision, and two more: a sigma_3 of any solve
  within a factor 10 of ``RANK_TOL``, and a smallest depth within 1e-6 relative of 0.

The acceptance rule for anything compared with the arbiter (``accept``): discrete outputs equal; cost(x) - cost(minimiser) <=
1e-5 max(1, cost(minimiser)) in high precision, gtsam's stopping rule as the repository's documents cite it; point and average error
within a per-family bound.
"""

from __future__ import annotations

import itertools
import math
from typing import Dict, List, Optional, Sequence, Tuple

import mpmath as mp
import numpy as np

from tests import triangulation_reference as ref

DIGITS = 60
STEP_RTOL = mp.mpf(10) ** -30
BOUND = mp.mpf(10) ** 30
MAX_ITERATIONS = 300
MARGIN_PX = 1e-6
SIGMA_BAND = 10.0
DEPTH_MARGIN = 1e-6
COST_RTOL = 1e-5
FLOAT64_MAX = mp.mpf(1.7976931348623157e308)

mp.mp.dps = DIGITS


class Cam:
    """One camera row in high precision."""

    def __init__(self, row: np.ndarray):
        v = [mp.mpf(float(c)) for c in row]
        self.key = np.asarray(row, np.float64).tobytes()
        self.fx, self.fy, self.cx, self.cy = v[1:5]
        self.r = v[5:14]
        self.t = v[14:17]

    def to_camera(self, x):
        d = [x[k] - self.t[k] for k in range(3)]
        r = self.r
        return [r[0] * d[0] + r[3] * d[1] + r[6] * d[2], r[1] * d[0] + r[4] * d[1] + r[7] * d[2], r[2] * d[0] + r[5] * d[1] + r[8] * d[2]]

    def residual(self, x, uv):
        p = self.to_camera(x)
        return self.fx * p[0] / p[2] + self.cx - uv[0], self.fy * p[1] / p[2] + self.cy - uv[1], p


def _mp_uv(uv) -> List:
    return [mp.mpf(float(uv[0])), mp.mpf(float(uv[1]))]


def dlt_matrix(cams: Sequence[Cam], uvs) -> mp.matrix:
    rows = []
    for c, uv in zip(cams, uvs):
        p = [[c.r[j], c.r[3 + j], c.r[6 + j], -(c.r[j] * c.t[0] + c.r[3 + j] * c.t[1] + c.r[6 + j] * c.t[2])] for j in range(3)]
        rows.append([uv[0] * p[2][k] - (c.fx * p[0][k] + c.cx * p[2][k]) for k in range(4)])
        rows.append([uv[1] * p[2][k] - (c.fy * p[1][k] + c.cy * p[2][k]) for k in range(4)])
    return mp.matrix(rows)


def dlt(cams: Sequence[Cam], uvs) -> Tuple[List, Optional[List]]:
    """(singular values, descending; the DLT point, or None: rank below 3 or a point that float64 cannot hold)."""
    _, s, v = mp.svd_r(dlt_matrix(cams, uvs))
    sigma = [s[i] for i in range(4)]
    if sum(1 for x in sigma if x > ref.RANK_TOL) < 3 or v[3, 3] == 0:
        return sigma, None
    x = [v[3, k] / v[3, 3] for k in range(3)]
    return sigma, (x if all(abs(c) <= FLOAT64_MAX for c in x) else None)


def cost(cams: Sequence[Cam], uvs, x):
    total = mp.mpf(0)
    for c, uv in zip(cams, uvs):
        ru, rv, _ = c.residual(x, uv)
        total += (ru * ru + rv * rv) / 2
    return total


def _derivatives(cams: Sequence[Cam], uvs, x):
    """cost, gradient [3], exact Hessian [3][3] (J^T J plus the residual-weighted second derivatives of the projection), J^T J."""
    zero = mp.mpf(0)
    total, g = zero, [zero] * 3
    h, jtj = [[zero] * 3 for _ in range(3)], [[zero] * 3 for _ in range(3)]
    for c, uv in zip(cams, uvs):
        ru, rv, p = c.residual(x, uv)
        total += (ru * ru + rv * rv) / 2
        z = p[2]
        # in camera coordinates: d(f p_a / z) = f (e_a / z - p_a e_2 / z^2); second derivatives (a, 2): -f / z^2, (2, 2): 2 f p_a / z^3
        ju = [c.fx / z, zero, -c.fx * p[0] / (z * z)]
        jv = [zero, c.fy / z, -c.fy * p[1] / (z * z)]
        gc = [ju[k] * ru + jv[k] * rv for k in range(3)]
        jc = [[ju[k] * ju[l] + jv[k] * jv[l] for l in range(3)] for k in range(3)]
        hc = [[jc[k][l] for l in range(3)] for k in range(3)]
        hc[0][2] = hc[2][0] = hc[0][2] - ru * c.fx / (z * z)
        hc[1][2] = hc[2][1] = hc[1][2] - rv * c.fy / (z * z)
        hc[2][2] = hc[2][2] + 2 * (ru * c.fx * p[0] + rv * c.fy * p[1]) / (z * z * z)
        # p_k = sum_i r[3 i + k] d_i: gradient R gc, Hessians R (.) R^T
        r = c.r
        for i in range(3):
            g[i] = g[i] + r[3 * i] * gc[0] + r[3 * i + 1] * gc[1] + r[3 * i + 2] * gc[2]
        for m, mc in ((h, hc), (jtj, jc)):
            half = [[r[3 * i] * mc[0][l] + r[3 * i + 1] * mc[1][l] + r[3 * i + 2] * mc[2][l] for l in range(3)] for i in range(3)]
            for i in range(3):
                for j in range(3):
                    m[i][j] = m[i][j] + half[i][0] * r[3 * j] + half[i][1] * r[3 * j + 1] + half[i][2] * r[3 * j + 2]
    return total, g, h, jtj


def _solve_spd3(h, g, lam) -> Optional[List]:
    a00, a01, a02, a11, a12, a22 = h[0][0] + lam, h[0][1], h[0][2], h[1][1] + lam, h[1][2], h[2][2] + lam
    b0, b1, b2 = -g[0], -g[1], -g[2]
    if not a00 > 0:
        return None
    l10, l20 = a01 / a00, a02 / a00
    a11, a12, a22 = a11 - l10 * a01, a12 - l10 * a02, a22 - l20 * a02
    b1, b2 = b1 - l10 * b0, b2 - l20 * b0
    if not a11 > 0:
        return None
    l21 = a12 / a11
    a22, b2 = a22 - l21 * a12, b2 - l21 * b1
    if not a22 > 0:
        return None
    d2 = b2 / a22
    d1 = (b1 - a12 * d2) / a11
    return [(b0 - a01 * d1 - a02 * d2) / a00, d1, d2]


def _norm(v):
    return mp.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def minimise(cams: Sequence[Cam], uvs, x0) -> Optional[List]:
    """The local minimiser of the cost reached from ``x0`` by steps that never raise the cost and never cross a camera's principal
    plane (the cost has a pole there): the full Newton step where the exact Hessian is positive definite and the step is acceptable,
    a Levenberg-Marquardt step on J^T J otherwise. Converged when a full Newton step is below ``STEP_RTOL``; None without a finite
    minimiser."""
    x = list(x0)
    extent = max([_norm([x[k] - c.t[k] for k in range(3)]) for c in cams] + [_norm([c.t[k] - cams[0].t[k] for k in range(3)]) for c in cams])
    lam = None

    def acceptable(xn, e) -> bool:
        return all((c.to_camera(xn)[2] > 0) == (c.to_camera(x)[2] > 0) for c in cams) and cost(cams, uvs, xn) <= e

    for _ in range(MAX_ITERATIONS):
        e, g, h, jtj = _derivatives(cams, uvs, x)
        d = _solve_spd3(h, g, mp.mpf(0))
        xn = None
        if d is not None:
            xn = [x[k] + d[k] for k in range(3)]
            if _norm(d) <= STEP_RTOL * max(_norm(xn), _norm([xn[k] - cams[0].t[k] for k in range(3)])):
                return xn
            if not acceptable(xn, e):
                xn = None
        if xn is None:
            trace = jtj[0][0] + jtj[1][1] + jtj[2][2]
            lam = trace * mp.mpf(10) ** -5 if lam is None else lam
            for _ in range(400):
                d = _solve_spd3(jtj, g, lam)
                if d is not None:
                    xn = [x[k] + d[k] for k in range(3)]
                    if acceptable(xn, e):
                        break
                xn, lam = None, max(lam * 10, mp.mpf(10) ** -300)
            if xn is None:
                return None
            lam = lam / 10
        x = xn
        if max(_norm(x), _norm([x[k] - cams[0].t[k] for k in range(3)])) > BOUND * extent:
            return None
    return None


class Solve:
    """One triangulation (a hypothesis or the final n-view solve)."""

    _memo: Dict[bytes, "Solve"] = {}

    @classmethod
    def of(cls, cams: Sequence[Cam], uvs) -> "Solve":
        """Memoised by the inputs' bits: a two-measurement track's hypothesis is its final solve, and option sets share solves."""
        key = b"".join(c.key for c in cams) + np.array([[float(u), float(v)] for u, v in uvs]).tobytes()
        if key not in cls._memo:
            cls._memo[key] = cls(cams, uvs)
        return cls._memo[key]

    def __init__(self, cams: Sequence[Cam], uvs):
        self.sigma, x0 = dlt(cams, uvs)
        self.status, self.x, self.cost, self.depth_ratio = "rank", None, None, None
        if x0 is None:
            return
        x = minimise(cams, uvs, x0)
        if x is None:
            self.status = "no finite minimiser"
            return
        depths = [c.to_camera(x)[2] for c in cams]
        self.depth_ratio = min(depths[j] / _norm([x[k] - c.t[k] for k in range(3)]) if any(x[k] != c.t[k] for k in range(3)) else mp.mpf(0)
                               for j, c in enumerate(cams))
        self.cost = cost(cams, uvs, x)
        if min(depths) > 0:
            self.status, self.x = "ok", x
        else:
            self.status = "cheirality"

    def fragile(self) -> Optional[str]:
        if ref.RANK_TOL / SIGMA_BAND < self.sigma[2] < ref.RANK_TOL * SIGMA_BAND:
            return f"sigma_3 {float(self.sigma[2]):.2e} within a factor {SIGMA_BAND:g} of rank_tol"
        if self.depth_ratio is not None and abs(self.depth_ratio) < DEPTH_MARGIN:
            return f"smallest depth {float(self.depth_ratio):.2e} relative, within {DEPTH_MARGIN:g} of 0"
        return None


def errors(cams: Sequence[Optional[Cam]], uvs, x) -> List:
    """Reprojection error per measurement; None for a missing camera or depth <= 0."""
    out = []
    for c, uv in zip(cams, uvs):
        if c is None:
            out.append(None)
            continue
        ru, rv, p = c.residual(x, uv)
        out.append(mp.sqrt(ru * ru + rv * rv) if p[2] > 0 else None)
    return out


def max_angle_deg(cams: Sequence[Cam], x):
    rays = []
    for c in cams:
        d = [x[k] - c.t[k] for k in range(3)]
        n = _norm(d)
        rays.append([v / n for v in d])
    best = -mp.inf
    for a, b in itertools.combinations(rays, 2):
        dot = min(mp.mpf(1), max(mp.mpf(-1), a[0] * b[0] + a[1] * b[1] + a[2] * b[2]))
        best = max(best, mp.degrees(mp.acos(dot)))
    return best


def _camera(table: np.ndarray, i: int) -> Optional[Cam]:
    return Cam(table[i]) if 0 <= i < len(table) and table[i, 0] != 0.0 else None


def triangulate_track(table: np.ndarray, images: Sequence[int], uv: np.ndarray, mode: int = ref.NO_RANSAC, threshold: float = math.inf,
                      min_angle_deg: float = 0.0, num_hypotheses: int = 2749, seed: int = 0) -> Dict[str, object]:
    """``ref.triangulate_track`` in high precision. Returns point [3] / avg_error (rounded to float64), exit_code, inlier_mask, stats,
    cost_min (the final solve's cost at its minimiser, NaN without one), non_decisive (a reason or "") and no_minimiser (bool: some
    solve had no finite minimiser, so the track has no arbiter answer)."""
    images = [int(i) for i in images]
    uv32 = np.asarray(uv, np.float32).reshape(-1, 2)
    uvs = [_mp_uv(p) for p in uv32]
    n = len(images)
    cams = [_camera(table, i) for i in images]
    thr = mp.inf if math.isinf(threshold) else mp.mpf(float(threshold))
    out = {"point": np.full(3, np.nan), "avg_error": math.nan, "exit_code": ref.INLIERS_UNDERCONSTRAINED, "inlier_mask": np.ones(n, bool),
           "stats": np.array([0, 0, -1, 0], np.int32), "cost_min": math.nan, "non_decisive": "", "no_minimiser": False}
    reasons: List[str] = []

    def near_threshold(errs) -> None:
        if thr != mp.inf and any(e is not None and abs(e - thr) < MARGIN_PX for e in errs):
            reasons.append(f"an error within {MARGIN_PX:g} px of the threshold")

    def note(solve: Solve) -> None:
        if solve.status == "no finite minimiser":
            out["no_minimiser"] = True
        why = solve.fragile()
        if why:
            reasons.append(why)

    def finish():
        out["non_decisive"] = "; ".join(dict.fromkeys(reasons))
        return out

    if n < 2:
        if mode != ref.NO_RANSAC:
            out["inlier_mask"] = np.zeros(n, bool)
        return finish()
    inl = [True] * n
    if mode != ref.NO_RANSAC:
        pairs = list(itertools.combinations(range(n), 2))
        chosen = ref.select_pairs(table, images, uv32, mode, num_hypotheses, seed)
        out["stats"][0] = len(chosen)
        inl = [False] * n
        scored = []  # (votes, mean, pair, mask)
        for p in chosen:
            k1, k2 = pairs[p]
            if cams[k1] is None or cams[k2] is None:
                out["stats"][1] += 1
                continue
            solve = Solve.of([cams[k1], cams[k2]], [uvs[k1], uvs[k2]])
            note(solve)
            if solve.x is None:
                out["stats"][1] += 1
                continue
            errs = errors(cams, uvs, solve.x)
            near_threshold(errs)
            ok = [e is not None and e < thr for e in errs]
            votes = sum(ok)
            if votes > 0:
                scored.append((votes, sum(e for e, o in zip(errs, ok) if o) / votes, p, ok))
        if scored:
            best = min(scored, key=lambda s: (-s[0], s[1], s[2]))
            inl, out["stats"][2], out["stats"][3] = best[3], best[2], best[0]
            for s in scored:
                if s[0] == best[0] and abs(s[1] - best[1]) < MARGIN_PX and s[3] != best[3]:
                    reasons.append(f"a rival inlier set within {MARGIN_PX:g} px of the winner's mean error")
    out["inlier_mask"] = np.array(inl, bool)
    idx = [k for k in range(n) if inl[k]]
    if len(idx) < 2:
        return finish()
    used = [k for k in idx if cams[k] is not None]
    if len(used) < 2:
        out["exit_code"] = ref.POSES_UNDERCONSTRAINED
        return finish()
    solve = Solve.of([cams[k] for k in used], [uvs[k] for k in used])
    note(solve)
    if solve.x is None:
        out["exit_code"] = ref.CHEIRALITY_FAILURE
        return finish()
    out["cost_min"] = float(solve.cost)
    errs = errors([cams[k] for k in idx], [uvs[k] for k in idx], solve.x)
    near_threshold(errs)
    good = [e for e in errs if e is not None]
    if good:
        out["avg_error"] = float(sum(good) / len(good))
    if not all(e is not None and e < thr for e in errs):
        out["exit_code"] = ref.EXCEEDS_REPROJ_THRESH
        return finish()
    if min_angle_deg > 0.0 and max_angle_deg([cams[k] for k in idx], solve.x) < min_angle_deg:
        out["exit_code"] = ref.LOW_TRIANGULATION_ANGLE
        return finish()
    out["point"] = np.array([float(c) for c in solve.x])
    out["exit_code"] = ref.SUCCESS
    return finish()


def final_cost(table: np.ndarray, images: Sequence[int], uv: np.ndarray, mask: np.ndarray, x: np.ndarray) -> float:
    """The final solve's cost at a float64 point ``x``, in high precision: over the inliers whose camera is estimated."""
    uv32 = np.asarray(uv, np.float32).reshape(-1, 2)
    cams, uvs = [], []
    for k, i in enumerate(images):
        c = _camera(table, int(i))
        if mask[k] and c is not None:
            cams.append(c)
            uvs.append(_mp_uv(uv32[k]))
    return cost(cams, uvs, [mp.mpf(float(v)) for v in x])


def cost_gap(table, images, uv, mask, x, cost_min: float) -> Tuple[float, float]:
    """(cost(x) - cost(minimiser), the allowance ``COST_RTOL`` max(1, cost(minimiser)))."""
    gap = final_cost(table, images, uv, mask, x) - mp.mpf(cost_min)
    return float(gap), COST_RTOL * max(1.0, cost_min)


def triangulate_tracks(table: np.ndarray, track_off: np.ndarray, image: np.ndarray, uv: np.ndarray, tracks: Optional[Sequence[int]] = None,
                       **options) -> Dict[str, np.ndarray]:
    """The device call's outputs from the arbiter, with cost_min, non_decisive (reason strings) and no_minimiser per track. With
    ``tracks``, only those rows are computed (the others keep their initial values)."""
    t = len(track_off) - 1
    out = {"point": np.full((t, 3), np.nan), "avg_error": np.full(t, np.nan), "exit_code": np.zeros(t, np.int32),
           "inlier_mask": np.zeros(len(image), np.uint8), "stats": np.zeros((t, 4), np.int32), "cost_min": np.full(t, np.nan),
           "non_decisive": np.array([""] * t, dtype=object), "no_minimiser": np.zeros(t, bool)}
    for j in range(t) if tracks is None else tracks:
        a, b = int(track_off[j]), int(track_off[j + 1])
        row = triangulate_track(table, image[a:b], uv[a:b], **options)
        for k in ("point", "avg_error", "exit_code", "stats", "cost_min", "non_decisive", "no_minimiser"):
            out[k][j] = row[k]
        out["inlier_mask"][a:b] = row["inlier_mask"]
    return out


DISCRETE = ("exit_code", "inlier_mask", "stats")


def accept(scene: Dict[str, np.ndarray], arb: Dict[str, np.ndarray], out: Dict[str, np.ndarray], tracks: Optional[Sequence[int]] = None) -> Dict[str, object]:
    """Compares outputs ``out`` (of the port, the host build or the device) with the arbiter's ``arb`` on ``scene``. Returns per track
    a list of failures of the discrete and the cost criterion (``failures[j]``: strings), and the measured figures: the relative point
    distance and the average error's difference per track (NaN where not defined), the cost gap and its allowance."""
    off = scene["track_off"]
    t = len(off) - 1
    res = {"failures": [[] for _ in range(t)], "point_rel": np.full(t, np.nan), "avg_dif": np.full(t, np.nan), "gap": np.full(t, np.nan), "allowed": np.full(t, np.nan)}
    for j in range(t) if tracks is None else tracks:
        a, b = int(off[j]), int(off[j + 1])
        fail = res["failures"][j]
        if out["exit_code"][j] != arb["exit_code"][j]:
            fail.append(f"exit code {int(out['exit_code'][j])}, arbiter {int(arb['exit_code'][j])}")
        if not np.array_equal(np.asarray(out["inlier_mask"][a:b]) != 0, np.asarray(arb["inlier_mask"][a:b]) != 0):
            fail.append("inlier mask")
        if not np.array_equal(out["stats"][j], arb["stats"][j]):
            fail.append(f"stats {out['stats'][j].tolist()}, arbiter {arb['stats'][j].tolist()}")
        if not np.array_equal(np.isnan(out["point"][j]), np.isnan(arb["point"][j])) or np.isnan(out["avg_error"][j]) != np.isnan(arb["avg_error"][j]):
            fail.append("NaN pattern")
        if fail:
            continue
        if arb["exit_code"][j] == ref.SUCCESS:
            gap, allowed = cost_gap(scene["cameras"], scene["image"][a:b], scene["uv"][a:b], arb["inlier_mask"][a:b], out["point"][j], float(arb["cost_min"][j]))
            res["gap"][j], res["allowed"][j] = gap, allowed
            if not gap <= allowed:
                fail.append(f"cost gap {gap:.3e} above {allowed:.3e}")
            res["point_rel"][j] = np.linalg.norm(out["point"][j] - arb["point"][j]) / np.linalg.norm(arb["point"][j])
        if np.isfinite(arb["avg_error"][j]):
            res["avg_dif"][j] = abs(out["avg_error"][j] - arb["avg_error"][j])
    return res
