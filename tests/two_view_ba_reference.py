"""The specification of the device two-view bundle adjustment (gtsfm_two_view_ba_f64): numpy, float64, and np.longdouble on request.

It restates what ``TwoViewEstimator.bundle_adjust`` does for one image pair (gtsfm/two_view_estimator.py:212-288) with the graph that
``TwoViewEstimator.__init__`` configures (gtsfm/bundle/two_view_ba.py, bundle_adjustment.py): triangulate the verified correspondences
at the verifier's pose, refine both poses and the points by a robust Levenberg-Marquardt, filter by reprojection error. gtsam is not
available where this project is developed, so this file, not gtsam, is what the kernels are held to.

PARITY UNPINNED towards gtsam -- every item below is restated from gtsam's documentation and source, none was observed running:
  * the Levenberg-Marquardt path: lambda_0 = 1e-5, factor 10, upper bound 1e5, lambda * I damping on every variable (no diagonal scaling),
    a step accepted when model fidelity > 1e-3, lambda / 10 on acceptance and * 10 on rejection; stop when the absolute or the relative
    decrease of the robust cost is < 1e-5, when lambda exceeds its bound, or after ``max_iterations`` accepted steps. A linear system that
    cannot be factored counts as a rejected step. The model decrease is -g.d / 2 + lambda |d|^2 / 2, which equals
    -g.d - d.H d / 2 when (H + lambda I) d = -g; H is the Gauss-Newton matrix of the re-weighted residuals.
  * the retraction: a pose (R, t), world from camera, tangent (omega, v) rotation first, moves to (R Exp(omega), t + R v) -- gtsam's
    first-order chart, not the full SE(3) exponential. Both have the same Jacobians at the origin.
  * the cheirality convention: a measurement whose point has depth <= 0 in its camera contributes zero residual and zero Jacobian
    (GeneralSFMFactor2's catch of CheiralityException).
  * Huber on the NORM of the pixel residual, k = 1.345: loss e^2 / 2 up to k, k (e - k / 2) above, weight 1 or k / e.
  * the pivot thresholds of the indeterminate-system test: here a pivot <= 0 or not finite, in a point's 3 x 3 block or in the reduced
    12 x 12 camera system, of the UNDAMPED system at the final values.
  * calibrations are HELD FIXED (pinhole fx, fy, cx, cy). The reference gives them priors of sigma 1e-5, which fixes them for every
    practical purpose.
  * priors: PriorFactorPose3 on camera 0 at the identity (isotropic sigma 0.1; residual (Log R0, t0) / sigma in the chart above) and
    PriorFactorPoint3 on the first triangulated point at its initial value (sigma 0.1). Nothing else fixes the scale. There are no
    relative pose priors.

Linear algebra, in an order the device can follow: each point's 3 x 3 block is eliminated (elimination without pivoting, written out)
into the 12 x 12 Schur complement of the cameras, which is factored by a Cholesky written out below; no LAPACK.

A pair is marked NON-DECISIVE when one of its own decisions (a fidelity test, a stopping test, a pivot sign -- of every system factored,
the damped ones of the loop included --, a reprojection error against the filter threshold) lies within ``sensitivity`` of its threshold:
another rounding path may decide otherwise. A decision with an operand that is not finite (an infinite cost, a NaN pivot) has no margin: no
rounding path turns it.

``two_view_ba`` also reports how the loop went: ``stop`` (one of STOP_REASONS) and ``rejected``, the number of trials rejected by each of
REJECT_ROUTES.
"""

from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np

from tests import triangulation_reference as tri

OK, SKIPPED, NO_INITIAL_POSE, NONE_TRIANGULATED, INDETERMINATE = range(5)
STATUS_NAMES = ("OK", "SKIPPED", "NO_INITIAL_POSE", "NONE_TRIANGULATED", "INDETERMINATE")
STATS_FIELDS = ("status", "verified", "triangulated", "valid", "accepted_steps", "solves_tried", "spare0", "spare1")

LAMBDA_INITIAL = 1e-5
LAMBDA_FACTOR = 10.0
LAMBDA_UPPER = 1e5
MIN_FIDELITY = 1e-3
ABS_TOL = 1e-5
REL_TOL = 1e-5
FILTER_MARGIN_PX = 1e-6  # as the triangulation restatement
STOP_REASONS = ("tolerance", "lambda_bound", "step_limit")
# why a trial was rejected, in the order the tests are made: a point block's pivot, a pivot of the reduced camera system, a step that is
# not finite, a trial cost that is not finite, a model decrease <= 0 (or NaN), a fidelity <= MIN_FIDELITY
REJECT_ROUTES = ("point_pivot", "camera_pivot", "step_not_finite", "cost_not_finite", "model_not_positive", "fidelity")

DEFAULTS = dict(max_iterations=100, reproj_error_threshold=0.5, huber_k=1.345, measurement_sigma=1.0, pose_prior_sigma=0.1, point_prior_sigma=0.1,
                min_verified=15, allow_indeterminate=False, triangulation_threshold=math.inf, triangulation_min_angle_deg=0.0)


def exp_so3(w):
    """Rodrigues; the series below theta = 1e-4 (its error there is ~1e-18)."""
    dt = w.dtype.type
    t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    theta = np.sqrt(t2)
    if theta < dt(1e-4):
        a, b = dt(1) - t2 / dt(6), dt(0.5) - t2 / dt(24)
    else:
        a, b = np.sin(theta) / theta, (dt(1) - np.cos(theta)) / t2
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=w.dtype)
    return np.eye(3, dtype=w.dtype) + a * k + b * (k @ k)


def log_so3(r):
    dt = r.dtype.type
    v = np.array([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]], dtype=r.dtype) * dt(0.5)
    s = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    c = (r[0, 0] + r[1, 1] + r[2, 2] - dt(1)) * dt(0.5)
    f = dt(1) + s * s / dt(6) if s < dt(1e-4) else np.arctan2(s, c) / s
    return v * f


def right_jacobian_inverse(w):
    """d Log(R Exp(delta)) / d delta at delta = 0, with w = Log R."""
    dt = w.dtype.type
    t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    theta = np.sqrt(t2)
    if theta < dt(1e-3):
        c = dt(1) / dt(12) + t2 / dt(720)
    else:
        c = dt(1) / t2 - (dt(1) + np.cos(theta)) / (dt(2) * theta * np.sin(theta))
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=w.dtype)
    return np.eye(3, dtype=w.dtype) + dt(0.5) * k + c * (k @ k)


class _State:
    def __init__(self, r0, t0, r1, t1, pts):
        self.r = [r0, r1]
        self.t = [t0, t1]
        self.pts = pts


def _measure(state: _State, cam: int, k, uv):
    """Camera coordinates q [n, 3], residual r [n, 2], cheirality ok [n] of every point in one camera."""
    q = (state.pts - state.t[cam]) @ state.r[cam]  # rows: R^T (P - t)
    ok = q[:, 2] > 0
    z = np.where(ok, q[:, 2], 1)
    res = np.stack([k[0] * q[:, 0] / z + k[2] - uv[:, 0], k[1] * q[:, 1] / z + k[3] - uv[:, 1]], axis=1)
    res = np.where(ok[:, None], res, 0)
    return q, z, res, ok


def _huber(res, kh):
    dt = res.dtype.type
    with np.errstate(over="ignore"):  # a scaled residual may overflow: e = inf, loss = inf, weight = k / inf = 0
        e = np.sqrt(res[:, 0] * res[:, 0] + res[:, 1] * res[:, 1])
        small = e <= kh
        loss = np.where(small, e * e * dt(0.5), kh * (e - kh * dt(0.5)))
    w = np.where(small, 1, kh / np.where(small, 1, e))
    return e, loss, w.astype(res.dtype)


def _pose_prior(state: _State, sigma):
    """Residual [6] and Jacobian [6, 6] of the prior on camera 0 at the identity."""
    dt = state.pts.dtype
    w = log_so3(state.r[0])
    res = np.concatenate([w, state.t[0]]) / sigma
    jac = np.zeros((6, 6), dtype=dt)
    jac[:3, :3] = right_jacobian_inverse(w) / sigma
    jac[3:, 3:] = state.r[0] / sigma
    return res, jac


def cost(state: _State, k1, k2, uv1, uv2, p0_init, opt) -> "float":
    dt = state.pts.dtype.type
    kh, sm = dt(opt["huber_k"]), dt(opt["measurement_sigma"])
    per_point = np.zeros(len(state.pts), dtype=state.pts.dtype)
    for cam, (k, uv) in enumerate(((k1, uv1), (k2, uv2))):
        _, _, res, _ = _measure(state, cam, k, uv)
        _, loss, _ = _huber(res / sm, kh)
        per_point = per_point + loss
    d = (state.pts[0] - p0_init) / dt(opt["point_prior_sigma"])
    per_point[0] = per_point[0] + dt(0.5) * (d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    total = dt(0)
    for v in per_point:  # index order
        total = total + v
    res, _ = _pose_prior(state, dt(opt["pose_prior_sigma"]))
    return total + dt(0.5) * (res @ res)


def residual_jacobians(state: _State, cam: int, k, uv):
    """Unweighted residual [n, 2], its Jacobians towards the camera's tangent [n, 2, 6] and the point [n, 2, 3] (zero behind the camera)."""
    dt = state.pts.dtype
    n = len(state.pts)
    q, z, res, ok = _measure(state, cam, k, uv)
    d = np.zeros((n, 2, 3), dtype=dt)
    d[:, 0, 0] = k[0] / z
    d[:, 0, 2] = -k[0] * q[:, 0] / (z * z)
    d[:, 1, 1] = k[1] / z
    d[:, 1, 2] = -k[1] * q[:, 1] / (z * z)
    d = np.where(ok[:, None, None], d, 0)
    skew = np.zeros((n, 3, 3), dtype=dt)  # [q]x
    skew[:, 0, 1], skew[:, 0, 2] = -q[:, 2], q[:, 1]
    skew[:, 1, 0], skew[:, 1, 2] = q[:, 2], -q[:, 0]
    skew[:, 2, 0], skew[:, 2, 1] = -q[:, 1], q[:, 0]
    jc = np.concatenate([d @ skew, -d], axis=2)
    jp = d @ state.r[cam].T
    return res, jc, jp


def linearise(state: _State, k1, k2, uv1, uv2, p0_init, opt):
    """Gauss-Newton blocks of the re-weighted problem: V [n, 3, 3], W [n, 12, 3], gp [n, 3], U [12, 12], gc [12]."""
    dt = state.pts.dtype
    n = len(state.pts)
    kh, sm = dt.type(opt["huber_k"]), dt.type(opt["measurement_sigma"])
    v = np.zeros((n, 3, 3), dtype=dt)
    w = np.zeros((n, 12, 3), dtype=dt)
    gp = np.zeros((n, 3), dtype=dt)
    u_pts = np.zeros((n, 12, 12), dtype=dt)
    gc_pts = np.zeros((n, 12), dtype=dt)
    for cam, (k, uv) in enumerate(((k1, uv1), (k2, uv2))):
        res, jc, jp = residual_jacobians(state, cam, k, uv)
        res, jc, jp = res / sm, jc / sm, jp / sm
        _, _, wt = _huber(res, kh)
        jcw, jpw = jc * wt[:, None, None], jp * wt[:, None, None]
        s = slice(6 * cam, 6 * cam + 6)
        v = v + np.swapaxes(jpw, 1, 2) @ jp
        w[:, s, :] = np.swapaxes(jcw, 1, 2) @ jp
        gp = gp + np.einsum("nij,ni->nj", jpw, res)
        u_pts[:, s, s] = np.swapaxes(jcw, 1, 2) @ jc
        gc_pts[:, s] = np.einsum("nij,ni->nj", jcw, res)
    inv = dt.type(1) / (dt.type(opt["point_prior_sigma"]) * dt.type(opt["point_prior_sigma"]))
    v[0] = v[0] + inv * np.eye(3, dtype=dt)
    gp[0] = gp[0] + inv * (state.pts[0] - p0_init)
    u = np.zeros((12, 12), dtype=dt)
    gc = np.zeros(12, dtype=dt)
    for j in range(n):  # index order
        u = u + u_pts[j]
        gc = gc + gc_pts[j]
    res, jac = _pose_prior(state, dt.type(opt["pose_prior_sigma"]))
    u[:6, :6] = u[:6, :6] + jac.T @ jac
    gc[:6] = gc[:6] + jac.T @ res
    return v, w, gp, u, gc


def overflowed_points(state: _State, k1, k2, uv1, uv2, opt):
    """[n] bool: points with a measurement whose scaled residual norm is not finite (see pivot_margin)."""
    dt = state.pts.dtype.type
    out = np.zeros(len(state.pts), bool)
    for cam, (k, uv) in enumerate(((k1, uv1), (k2, uv2))):
        _, _, res, _ = _measure(state, cam, k, uv)
        with np.errstate(over="ignore", invalid="ignore"):
            e, _, _ = _huber(res / dt(opt["measurement_sigma"]), dt(opt["huber_k"]))
        out |= ~np.isfinite(e)
    return out


def solve_point_blocks(v, lam, rhs):
    """(V_j + lam I)^-1 rhs_j for every point, rhs [n, 3, m]: elimination without pivoting, written out. Returns (x, pivots [n, 3])."""
    a00, a01, a02 = v[:, 0, 0] + lam, v[:, 0, 1], v[:, 0, 2]
    a11, a12, a22 = v[:, 1, 1] + lam, v[:, 1, 2], v[:, 2, 2] + lam
    with np.errstate(all="ignore"):
        l10, l20 = a01 / a00, a02 / a00
        a11 = a11 - l10 * a01
        a12 = a12 - l10 * a02
        a22 = a22 - l20 * a02
        l21 = a12 / a11
        a22 = a22 - l21 * a12
        b0 = rhs[:, 0, :]
        b1 = rhs[:, 1, :] - l10[:, None] * b0
        b2 = rhs[:, 2, :] - l20[:, None] * b0 - l21[:, None] * b1
        x2 = b2 / a22[:, None]
        x1 = (b1 - a12[:, None] * x2) / a11[:, None]
        x0 = (b0 - a01[:, None] * x1 - a02[:, None] * x2) / a00[:, None]
    return np.stack([x0, x1, x2], axis=1), np.stack([a00, a11, a22], axis=1)


def cholesky_solve(s, b):
    """S x = b by a Cholesky written out (lower triangle, row by row). Returns (x or None, pivots [12]): a pivot <= 0 or not finite fails."""
    n = len(b)
    dt = s.dtype
    low = np.zeros((n, n), dtype=dt)
    piv = np.full(n, np.nan, dtype=dt)
    for i in range(n):
        for j in range(i + 1):
            acc = s[i, j]
            for k in range(j):
                acc = acc - low[i, k] * low[j, k]
            if i == j:
                piv[i] = acc
                if not (acc > 0) or not np.isfinite(acc):
                    return None, piv
                low[i, i] = np.sqrt(acc)
            else:
                low[i, j] = acc / low[j, j]
    y = np.zeros(n, dtype=dt)
    for i in range(n):
        acc = b[i]
        for k in range(i):
            acc = acc - low[i, k] * y[k]
        y[i] = acc / low[i, i]
    x = np.zeros(n, dtype=dt)
    for i in range(n - 1, -1, -1):
        acc = y[i]
        for k in range(i + 1, n):
            acc = acc - low[k, i] * x[k]
        x[i] = acc / low[i, i]
    return x, piv


def pivot_margin(ppiv, cpiv, u, sensitivity, overflowed=None):
    """The margin entry of one factorisation's pivot signs, or None when no pivot is finite. The band scales with the largest FINITE
    diagonal entry of the cameras' block: an entry that is not finite must not make every pivot look rounding-level.
    ``overflowed`` [n]: points with a measurement whose scaled residual norm is not finite. Its weight is k / inf = 0 exactly, so its blocks
    are exact zeros here and 0 x inf = NaN where the weight is applied last (the device): a pivot of 0 there is no rounding-level value,
    it fails on every path. Such points' pivots, and the pivots of a camera system that such a point entered, get no margin."""
    ppiv, cpiv = np.asarray(ppiv), np.asarray(cpiv)
    if overflowed is not None and overflowed.any():
        ppiv, cpiv = ppiv[~overflowed], cpiv[:0]
    piv = np.concatenate([ppiv.reshape(-1), cpiv.reshape(-1)]).astype(np.float64)
    piv = piv[np.isfinite(piv)]
    if not piv.size:
        return None
    diag = np.abs(np.diagonal(u).astype(np.float64))
    diag = diag[np.isfinite(diag)]
    scale = float(max(diag.max(initial=0.0), 1.0))
    return ("pivot", float(np.min(np.abs(piv))), sensitivity * scale)


def schur_solve(v, w, gp, u, gc, lam):
    """The damped step: (dc [12], dp [n, 3]) or None, the pivots (points [n, 3], cameras [12]), and why there is no step (None, or one
    of the first three REJECT_ROUTES)."""
    dt = v.dtype
    n = len(v)
    rhs = np.concatenate([np.swapaxes(w, 1, 2), gp[:, :, None]], axis=2)  # [n, 3, 13]
    y, ppiv = solve_point_blocks(v, lam, rhs)
    bad = ~(np.isfinite(ppiv).all() and (ppiv > 0).all())
    s = u + lam * np.eye(12, dtype=dt)
    b = -gc
    if not bad:
        contrib = w @ y  # [n, 12, 13]
        for j in range(n):  # index order
            s = s - contrib[j, :, :12]
            b = b + contrib[j, :, 12]
    dc, cpiv = (None, np.full(12, np.nan, dtype=dt)) if bad else cholesky_solve(s, b)
    if dc is None:
        return None, None, ppiv, cpiv, "point_pivot" if bad else "camera_pivot"
    if not np.isfinite(dc).all():
        return None, None, ppiv, cpiv, "step_not_finite"
    dp = -(y[:, :, 12] + y[:, :, :12] @ dc)
    return dc, dp, ppiv, cpiv, None


def retract(state: _State, dc, dp) -> _State:
    r, t = [], []
    for cam in range(2):
        r.append(state.r[cam] @ exp_so3(dc[6 * cam:6 * cam + 3]))
        t.append(state.t[cam] + state.r[cam] @ dc[6 * cam + 3:6 * cam + 6])
    return _State(r[0], t[0], r[1], t[1], state.pts + dp)


def optimise(state: _State, k1, k2, uv1, uv2, opt, abs_tol=ABS_TOL, rel_tol=REL_TOL, trace: Optional[list] = None, sensitivity: float = 0.0,
             report: Optional[dict] = None):
    """Levenberg-Marquardt as the header states it. Returns (state, initial cost, final cost, accepted, solves, margins): ``margins`` holds
    (name, |value - threshold|, band) of every fidelity, stopping and pivot-sign decision taken; within the band the decision is not
    decisive. ``report`` receives ``stop`` and ``rejected`` (see the header)."""
    dt = state.pts.dtype.type
    p0 = state.pts[0].copy()
    cur = cost(state, k1, k2, uv1, uv2, p0, opt)
    first = cur
    lam = dt(LAMBDA_INITIAL)
    accepted = solves = 0
    margins = []
    rejected = dict.fromkeys(REJECT_ROUTES, 0)
    reason = None
    stop = False
    while accepted < opt["max_iterations"] and not stop:
        v, w, gp, u, gc = linearise(state, k1, k2, uv1, uv2, p0, opt)
        overflowed = overflowed_points(state, k1, k2, uv1, uv2, opt)
        while True:
            solves += 1
            dc, dp, ppiv, cpiv, why = schur_solve(v, w, gp, u, gc, lam)
            entry = pivot_margin(ppiv, cpiv, u, sensitivity, overflowed)
            if entry is not None:
                margins.append(entry)
            ok = False
            if dc is not None:
                trial = retract(state, dc, dp)
                new = cost(trial, k1, k2, uv1, uv2, p0, opt)
                gtd = gc @ dc
                dd = dc @ dc
                for j in range(len(dp)):
                    gtd = gtd + gp[j] @ dp[j]
                    dd = dd + dp[j] @ dp[j]
                model = -dt(0.5) * gtd + dt(0.5) * lam * dd
                if not np.isfinite(new):
                    why = "cost_not_finite"
                elif not model > 0:
                    why = "model_not_positive"
                else:
                    fidelity = (cur - new) / model
                    if np.isfinite(fidelity):  # an infinite current cost: no rounding path turns the test
                        margins.append(("fidelity", abs(float(fidelity) - MIN_FIDELITY), sensitivity))
                    ok = bool(fidelity > MIN_FIDELITY)
                    why = None if ok else "fidelity"
            if ok:
                dec = cur - new
                rel = dec / cur
                margins.append(("abs", abs(float(dec) - abs_tol), sensitivity * float(cur)))
                margins.append(("rel", abs(float(rel) - rel_tol), sensitivity))
                state, cur = trial, new
                accepted += 1
                lam = lam / dt(LAMBDA_FACTOR)
                if trace is not None:
                    trace.append((float(cur), float(lam), float(dec)))
                if dec < abs_tol or rel < rel_tol:
                    stop, reason = True, "tolerance"
                break
            rejected[why] += 1
            lam = lam * dt(LAMBDA_FACTOR)
            if lam > LAMBDA_UPPER:
                stop, reason = True, "lambda_bound"
                break
    if report is not None:
        report["stop"] = reason if stop else "step_limit"
        report["rejected"] = rejected
    return state, first, cur, accepted, solves, margins


def reprojection_errors(state: _State, cam: int, k, uv):
    """Pixels; NaN for depth <= 0."""
    q, z, res, ok = _measure(state, cam, k, uv)
    e = np.sqrt(res[:, 0] * res[:, 0] + res[:, 1] * res[:, 1])
    return np.where(ok, e, np.nan)


def two_view_ba(k1, k2, uv1, uv2, i2Ri1, i2Ui1, dtype=np.float64, order=None, sensitivity: float = 1e-10, initial_points=None, abs_tol=ABS_TOL,
                rel_tol=REL_TOL, trace: Optional[list] = None, **options) -> Dict[str, object]:
    """One pair. ``k1``, ``k2``: (fx, fy, cx, cy); ``uv1``, ``uv2`` [n, 2]: the VERIFIED correspondences' pixels (float32 values, as the
    device reads them); ``i2Ri1`` [3, 3], ``i2Ui1`` [3]: the verifier's pose (NaN: none). ``order``: a permutation of the triangulated
    points applied before the optimisation (the first stays first), for the sensitivity measurement.
    Returns ``status``, ``rotation`` [3, 3] / ``translation`` [3] (NaN where the reference returns None), ``valid`` [n] bool,
    ``points`` [n, 3] (NaN where not triangulated), ``cost`` (initial, final), ``stats`` [8], ``non_decisive``, ``triangulated`` [n] bool, and
    for a pair that reaches the optimisation ``stop``, ``rejected`` and ``margins``."""
    unknown = set(options) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown options {sorted(unknown)}")
    opt = {**DEFAULTS, **options}
    uv1 = np.asarray(uv1, np.float32).astype(np.float64).reshape(-1, 2)
    uv2 = np.asarray(uv2, np.float32).astype(np.float64).reshape(-1, 2)
    n = len(uv1)
    r_in, t_in = np.asarray(i2Ri1, np.float64).reshape(3, 3), np.asarray(i2Ui1, np.float64).reshape(3)
    out = {"status": OK, "rotation": np.full((3, 3), np.nan), "translation": np.full(3, np.nan), "valid": np.zeros(n, bool), "points": np.full((n, 3), np.nan),
           "cost": np.full(2, np.nan), "stats": np.zeros(8, np.int32), "non_decisive": False, "triangulated": np.zeros(n, bool)}
    out["stats"][1] = n

    def done(status):
        out["status"] = out["stats"][0] = status
        out["stats"][3] = int(out["valid"].sum())
        return out

    if n < opt["min_verified"]:
        out["rotation"], out["translation"], out["valid"][:] = r_in, t_in, True
        return done(SKIPPED)
    if not (np.isfinite(r_in).all() and np.isfinite(t_in).all()):
        out["valid"][:] = True
        return done(NO_INITIAL_POSE)
    w_r1, w_t1 = r_in.T, -r_in.T @ t_in  # camera 1 = the inverse of Pose3(i2Ri1, i2Ui1)
    if initial_points is None:
        table = np.stack([tri.pack_camera(*k1, np.eye(3), np.zeros(3)), tri.pack_camera(*k2, w_r1, w_t1)])
        pts = np.full((n, 3), np.nan)
        for j in range(n):
            x, _, code, _, _ = tri.triangulate_track(table, [0, 1], np.stack([uv1[j], uv2[j]]), mode=tri.NO_RANSAC, threshold=opt["triangulation_threshold"],
                                                     min_angle_deg=opt["triangulation_min_angle_deg"], solver="jacobi")
            if code == tri.SUCCESS:
                pts[j] = x
    else:
        pts = np.asarray(initial_points, np.float64).reshape(n, 3).copy()
    ok = np.isfinite(pts).all(axis=1)
    out["triangulated"] = ok
    out["stats"][2] = int(ok.sum())
    if not ok.any():
        out["rotation"], out["translation"] = r_in, t_in
        return done(NONE_TRIANGULATED)
    idx = np.flatnonzero(ok)
    if order is not None:
        idx = idx[np.asarray(order)]
    cast = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
    ka, kb, ua, ub = cast(k1), cast(k2), cast(uv1[idx]), cast(uv2[idx])
    state = _State(cast(np.eye(3)), cast(np.zeros(3)), cast(w_r1), cast(w_t1), cast(pts[idx]))
    p0 = state.pts[0].copy()
    state, first, last, accepted, solves, margins = optimise(state, ka, kb, ua, ub, opt, abs_tol, rel_tol, trace, sensitivity, report=out)
    out["cost"] = np.array([float(first), float(last)])
    out["stats"][4], out["stats"][5] = accepted, solves
    out["points"][idx] = state.pts.astype(np.float64)
    out["state"] = state

    # the undamped system at the final values
    v, w, gp, u, gc = linearise(state, ka, kb, ua, ub, p0, opt)
    _, _, ppiv, cpiv, why = schur_solve(v, w, gp, u, gc, dtype(0))
    entry = pivot_margin(ppiv, cpiv, u, sensitivity, overflowed_points(state, ka, kb, ua, ub, opt))
    if entry is not None:
        margins.append(entry)
    out["margins"] = margins
    # the header's test: a PIVOT that is not positive or not finite. A solution that is not finite over pivots that are fine (a right-hand
    # side that overflows) is not part of it, and the device, which factors without a right-hand side here, never sees one.
    indeterminate = why in ("point_pivot", "camera_pivot")
    if indeterminate and not opt["allow_indeterminate"]:
        out["non_decisive"] = any(m <= band for _, m, band in margins)
        return done(INDETERMINATE)

    thr = opt["reproj_error_threshold"]
    e1, e2 = reprojection_errors(state, 0, ka, ua).astype(np.float64), reprojection_errors(state, 1, kb, ub).astype(np.float64)
    with np.errstate(invalid="ignore"):
        out["valid"][idx] = (e1 < thr) & (e2 < thr)
    errs = np.concatenate([e1, e2])
    errs = errs[np.isfinite(errs)]
    if errs.size and math.isfinite(thr):
        margins.append(("filter", float(np.min(np.abs(errs - thr))), FILTER_MARGIN_PX))
    r_rel = state.r[1].T @ state.r[0]  # wTi2.between(wTi1)
    t_rel = state.r[1].T @ (state.t[0] - state.t[1])
    out["rotation"] = r_rel.astype(np.float64)
    out["translation"] = (t_rel / np.sqrt(t_rel @ t_rel)).astype(np.float64)
    out["non_decisive"] = any(m <= band for _, m, band in margins)
    return done(INDETERMINATE if indeterminate else OK)


def reference_check_options(robust_ba_mode="HUBER", relative_pose_prior=None, use_gnc=False, use_karcher_mean_factor=False, shared_calib=False,
                            ba_reproj_error_thresholds=(0.5,), calibration=None) -> None:
    """What the restatement does not cover raises NotImplementedError naming itself."""
    if calibration is not None and not (isinstance(calibration, (tuple, list, np.ndarray)) and len(calibration) == 4):
        raise NotImplementedError(f"calibration {type(calibration).__name__}: only a pinhole (fx, fy, cx, cy) is restated, held fixed")
    if relative_pose_prior is not None:
        raise NotImplementedError("a relative pose prior (BetweenFactorPose3) is not restated")
    if getattr(robust_ba_mode, "name", robust_ba_mode) not in ("HUBER", "NONE"):
        raise NotImplementedError(f"robust_ba_mode {robust_ba_mode} is not restated (HUBER / NONE only)")
    if use_gnc:
        raise NotImplementedError("GNC is not restated")
    if use_karcher_mean_factor:
        raise NotImplementedError("a Karcher mean factor is not restated")
    if shared_calib:
        raise NotImplementedError("shared calibration is not restated")
    if len(list(ba_reproj_error_thresholds)) != 1:
        raise NotImplementedError("more than one entry in ba_reproj_error_thresholds is not restated")
