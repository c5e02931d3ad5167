"""The specification of ``gtsfm_global_ba_f64`` (gtsfm_amd/csrc/global_ba_kernels.hip): a numpy restatement that does the same float64
operations in the same order, so that the device's bytes can be held to it. It restates what ``BundleAdjustmentOptimizer.run_ba`` does after
the triangulation (gtsfm/bundle/bundle_adjustment.py, called from gtsfm/multi_view_optimizer.py:215-221): refine every camera pose and every
track's point by a robust Levenberg-Marquardt on the reprojection errors, then filter the tracks by reprojection error. gtsam is not available
where this project is developed, so this file, not gtsam, is what the kernels are held to.

PARITY UNPINNED towards gtsam -- every item is restated from gtsam's and the reference's source, none was observed running:
  * gtsam's Levenberg-Marquardt path (here: the two-view stage's scalar rules around an INEXACT step), its elimination ordering (here: every
    point eliminated, the reduced camera system solved matrix-free by preconditioned conjugate gradients) and its retraction (here Cayley);
  * the Karcher-mean factor and the soft prior (sigma 0.1) on the first camera: here ONE HARD ANCHOR, a camera whose pose is not an unknown;
    the scale is left to the damping, as the reference's own graph leaves it;
  * calibration variables and their priors, and ``shared_calib``: calibrations are HELD FIXED (pinhole fx, fy, cx, cy), as in the two-view stage;
  * GNC / GMC / TLS (HUBER and NONE only);
  * relative and absolute pose priors;
  * the marginals check;
  * ``select_largest_connected_component``: here the ANCHOR'S connected component of the camera-point graph is the problem;
  * the metrics group.

INPUTS. ``cameras`` [N][17], the triangulation's rows: valid, fx, fy, cx, cy, wRc row-major, wtc. The track CSR ``track_off`` [T + 1] int64,
``image`` [S] int32, ``uv`` [S][2] float32; ``point`` [T][3] float64; optional ``track_enable`` [T] and ``meas_enable`` [S] uint8 (in the chain:
``exit_code == SUCCESS`` and the triangulation's ``inlier_mask``). A measurement is VALID when it is enabled, its camera id lies in 0 .. N - 1
with ``valid != 0`` and its pixel is finite; a track is valid when it is enabled, its point is finite and it has at least ``min_track_length``
valid measurements; a measurement counts only in a valid track. A camera id outside the table counts as not estimated, as in the
triangulation: it is not a refusal. Offsets that are not ascending are refused (ValueError here, GTSFM_ERR_INVALID there, nothing written).

THE PROBLEM. Nodes are the cameras 0 .. N - 1, then the tracks N + j. ``anchor`` is a camera; -1 means the smallest camera id that has a valid
measurement. The problem is the anchor's connected component over the valid measurements; every camera and point outside it is copied
through unchanged with ``node_valid`` 0 (valid cameras without a measurement, a second component, disabled tracks). Without a valid
measurement (or none at a given anchor): NO_VALID_ROW.

THE COST. f = sum_m rho_k(|proj(cam_i, p_j) - uv_m| / sigma), rho_k gtsam's Huber on the NORM of the scaled residual: e^2 / 2 up to k,
k (e - k / 2) above, weight 1 or k / e (k <= 0 or inf: always the half square, RobustBAMode.NONE). q = wRc^T (p - wtc), the pixel is
(fx q0 / q2 + cx, fy q1 / q2 + cy). The cheirality convention: a measurement whose point has depth q2 <= 0 in its camera contributes zero
residual and zero Jacobian (GeneralSFMFactor2's catch of CheiralityException). The anchor's pose is held fixed exactly.

THE UPDATE. A pose (R, t), world from camera, with the tangent (omega, v), moves to (R Cay(omega), t + R v), Cay(omega) = I + s (H + H H),
H = [omega / 2]x, s = 2 / (1 + |omega / 2|^2); a point moves by its 3-vector. Nothing but + - * / sqrt and comparisons is used.

THE ARITHMETIC. Products of short vectors sum left to right: ((a0 b0 + a1 b1) + a2 b2) + ... Every node has the list of its valid
measurements, a camera's in ascending (track, measurement) order, a track's in ascending (camera, measurement) order, and sums over it in
that order. The component's nodes are numbered 0 .. n - 1 in ascending node id (the compact index: its cameras, then its tracks); every
global scalar is the pairwise tree over the per-node values in compact order, padded with zeros to a power of two; a cost is half the tree of
the per-node sums of rho (every measurement is in two lists).

LINEARISATION at the values held, per list entry: the scaled residual r [2], the weight w, the Jacobians Jc [2][6] = [D [q]x, -D] / sigma and
Jp [2][3] = D wRc^T / sigma with D = [[fx / q2, 0, -fx q0 / q2^2], [0, fy / q2, -fy q1 / q2^2]]. Per camera g = sum (w Jc)^T r and the lower
triangle of U = sum (w Jc)^T Jc; per point g = sum (w Jp)^T r and V = sum (w Jp)^T Jp; W = (w Jc)^T Jp is never formed: W y = (w Jc)^T (Jp y)
and W^T d = (w Jp)^T (Jc d).

THE STEP at a damping lambda (lambda I on every variable): every point's damped 3 x 3 block is eliminated (elimination without pivoting,
written out); the reduced camera system (U + lambda I - W (V + lambda I)^-1 W^T) dc = -g_c + W (V + lambda I)^-1 g_p is applied matrix-free
-- one pass over the tracks, one over the cameras -- and solved by conjugate gradients from 0, preconditioned by the inverse of every
camera's damped 6 x 6 block (Cholesky, written out), the anchor's entries zero throughout. CG stops at |r| <= cg_forcing |r0| or at r.M^-1 r <= 0 (or NaN: nothing is left to
precondition), both tested before every iteration, or after ``max_inner`` iterations (<= 0: six per camera of the problem). The points follow by back-substitution,
dp = -(V + lambda I)^-1 (g_p + W^T dc). Because the step is inexact its model decrease is computed from the step itself by one more pass:
-(g.d + (1 / 2) sum_m w |Jc dc + Jp dp|^2).

THE OUTER LOOP, the two-view stage's rules: lambda starts at 1e-5; a trial is ACCEPTED when its cost is finite, the model decrease is > 0 and
(f - f_new) / model > 1e-3; then lambda / 10, else lambda * 10. The loop ends when an accepted step lowered the cost by less than ``abs_tol``
or relatively by less than ``rel_tol`` (CONVERGED; gtsam's 1e-5 both), when lambda exceeds 1e5 (LAMBDA_BOUND), after ``max_iterations``
accepted steps (MAX_ITERATIONS; also after 2 max_iterations + 16 linear solves, which the other rules make unreachable). A first cost that is
NaN: NON_FINITE. On NO_VALID_ROW and NON_FINITE the outputs are the inputs, ``track_valid`` and ``camera_kept`` are zero.

OUTPUTS. ``cameras_out`` [N][17], ``point_out`` [T][3]; ``reproj_error`` [S] in pixels at the final values: NaN where the measurement is not a
valid one of the problem (its camera not estimated, its track not in the problem) or the point is behind the camera; ``track_valid`` [T]:
the track is in the problem and every one of its valid measurements has a finite error < ``reproj_error_threshold``
(GtsfmData.__validate_track); ``camera_kept`` [N]: the camera has a valid measurement in a kept track (what filter_landmarks retains);
``node_valid`` [N + T]; ``counters`` (COUNTER_FIELDS), ``costs`` (COST_FIELDS).

THE THRESHOLD LIST. The reference restarts every entry of ``reproj_error_thresholds`` from the same ``initial_data``
(bundle_adjustment.py:617-625): the stages are identical optimisations and only the last threshold shapes the result. The drop-in therefore
runs the optimisation once and filters at the last threshold.
"""

from __future__ import annotations

from typing import Dict

import numpy as np

CONVERGED, MAX_ITERATIONS, NO_VALID_ROW, NON_FINITE, LAMBDA_BOUND = 0, 1, 2, 3, 4
STATUS_NAMES = ("CONVERGED", "MAX_ITERATIONS", "NO_VALID_ROW", "NON_FINITE", "LAMBDA_BOUND")
COUNTER_FIELDS = ("status", "anchor", "cameras", "points", "valid_measurements", "accepted_steps", "solves_tried", "cg_iterations")
COST_FIELDS = ("init_cost", "final_cost", "gradient_inf_norm", "lambda")
DEFAULTS = dict(measurement_sigma=1.0, huber_k=1.345, reproj_error_threshold=3.0, min_track_length=2, rel_tol=1e-5, abs_tol=1e-5, cg_forcing=1e-2,
                max_iterations=100, max_inner=0)
LAMBDA_INITIAL, LAMBDA_FACTOR, LAMBDA_UPPER, MIN_FIDELITY = 1e-5, 10.0, 1e5, 1e-3
FILTER_MARGIN_PX = 1e-6  # as the triangulation restatement


def chain(terms):
    """((t0 + t1) + t2) + ..."""
    s = terms[0]
    for t in terms[1:]:
        s = s + t
    return s


def tree(values, op=np.add):
    n = len(values)
    p2 = 1
    while p2 < n:
        p2 *= 2
    t = np.zeros(p2, dtype=np.float64)
    t[:n] = values
    while len(t) > 1:
        t = op(t[0::2], t[1::2])
    return t[0]


def pick_max(x, y):
    return np.where(x > y, x, y)


def validity(cameras, track_off, image, uv, point, track_enable, meas_enable, min_track_length):
    """(valid [S] bool, track_ok [T] bool). Refuses offsets that are not ascending from 0 to S."""
    t, s, n = len(track_off) - 1, len(image), len(cameras)
    if t < 0 or track_off[0] != 0 or track_off[-1] != s or (np.diff(track_off) < 0).any():
        raise ValueError("track_off is not ascending from 0 to the number of measurements")
    en_m = np.ones(s, bool) if meas_enable is None else np.asarray(meas_enable).reshape(-1) != 0
    en_t = np.ones(t, bool) if track_enable is None else np.asarray(track_enable).reshape(-1) != 0
    inside = (image >= 0) & (image < n)
    cam_ok = np.zeros(s, bool)
    cam_ok[inside] = cameras[image[inside], 0] != 0
    meas_ok = en_m & cam_ok & np.isfinite(uv).all(1)
    track = np.repeat(np.arange(t), np.diff(track_off))
    count = np.bincount(track[meas_ok], minlength=t) if t else np.zeros(0, np.int64)
    track_ok = en_t & np.isfinite(point).all(1) & (count >= min_track_length)
    return meas_ok & track_ok[track], track_ok


class Graph:
    """The anchor's component with the nodes' lists in compact numbering."""

    def __init__(self, cameras, track_off, image, uv, valid, anchor):
        n_cam, t = len(cameras), len(track_off) - 1
        track = np.repeat(np.arange(t), np.diff(track_off))
        rows = np.flatnonzero(valid)
        self.num_valid = len(rows)
        a, b = image.astype(np.int64), n_cam + track
        if anchor < 0:
            anchor = int(a[rows].min()) if len(rows) else -1
        elif not (a[rows] == anchor).any():
            anchor = -1
        self.anchor = anchor
        reach = np.zeros(n_cam + t, bool)
        if anchor >= 0:
            reach[anchor] = True
            ra, rb = a[rows], b[rows]
            while True:
                grow = reach.copy()
                grow[ra[reach[rb]]] = True
                grow[rb[reach[ra]]] = True
                if (grow == reach).all():
                    break
                reach = grow
        self.nodes = np.flatnonzero(reach)
        self.n = len(self.nodes)
        self.nc = int(reach[:n_cam].sum())
        cid = np.full(n_cam + t, -1, np.int64)
        cid[self.nodes] = np.arange(self.n)
        self.anchor_c = int(cid[anchor]) if anchor >= 0 else -1
        inside = rows[reach[a[rows]]] if len(rows) else rows
        ent = np.concatenate([np.stack([cid[a[inside]], cid[b[inside]], inside, np.ones_like(inside)], 1), np.stack([cid[b[inside]], cid[a[inside]], inside, np.zeros_like(inside)], 1)])
        ent = ent[np.lexsort((ent[:, 2], ent[:, 1], ent[:, 0]))].reshape(-1, 4)
        self.node, self.nbr, self.row, self.is_cam = ent[:, 0], ent[:, 1], ent[:, 2], ent[:, 3] == 1
        start = np.searchsorted(self.node, self.node, side="left")
        rank = np.arange(len(ent)) - start
        self.by_rank = [np.flatnonzero(rank == r) for r in range(int(rank.max()) + 1 if len(rank) else 0)]
        self.ci, self.pj = np.where(self.is_cam, self.node, self.nbr), np.where(self.is_cam, self.nbr, self.node)
        self.cam_entries, self.pt_entries = np.flatnonzero(self.is_cam), np.flatnonzero(~self.is_cam)
        k = cameras[a[self.row]]
        self.fx, self.fy, self.cx, self.cy = k[:, 1], k[:, 2], k[:, 3], k[:, 4]
        self.u, self.v = uv[self.row, 0].astype(np.float64), uv[self.row, 1].astype(np.float64)

    def gather_sum(self, terms, shape):
        """Per node, over its list in order."""
        out = np.zeros((self.n,) + shape)
        for idx in self.by_rank:
            k = self.node[idx]
            out[k] = out[k] + terms[idx]
        return out

    def measure(self, x):
        """Per entry: q [m, 3], ok [m], the unscaled residual [m, 2] (zero behind the camera)."""
        r, t, p = x[self.ci, :9].reshape(-1, 3, 3), x[self.ci, 9:12], x[self.pj, :3]
        dv = p - t
        q = np.stack([(r[:, 0, k] * dv[:, 0] + r[:, 1, k] * dv[:, 1]) + r[:, 2, k] * dv[:, 2] for k in range(3)], 1)
        ok = q[:, 2] > 0
        z = np.where(ok, q[:, 2], 1.0)
        res = np.stack([(self.fx * (q[:, 0] / z) + self.cx) - self.u, (self.fy * (q[:, 1] / z) + self.cy) - self.v], 1)
        return q, ok, np.where(ok[:, None], res, 0.0), r


def huber(r, k):
    """Per entry of the scaled residual: (rho, w)."""
    e = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])
    on = bool(k > 0 and np.isfinite(k))
    beyond = (e > k) if on else np.zeros(e.shape, bool)
    kk = np.float64(k)
    return np.where(beyond, kk * (e - 0.5 * kk), 0.5 * (e * e)), np.where(beyond, kk / np.where(beyond, e, 1.0), 1.0)


def cost(g: Graph, x, sigma, k):
    _, _, res, _ = g.measure(x)
    rho, _ = huber(res / sigma, k)
    return 0.5 * tree(g.gather_sum(rho, ()))


def entries_at(g: Graph, x, sigma, k):
    """Per list entry: r [m, 2], w [m], rho [m], Jc [m, 2, 6], Jp [m, 2, 3] (scaled by 1 / sigma; zero behind the camera)."""
    q, ok, res, rot = g.measure(x)
    m = len(q)
    z = q[:, 2]
    zero = np.zeros(m)
    with np.errstate(all="ignore"):
        d00, d02 = g.fx / z, -((g.fx * q[:, 0]) / (z * z))
        d11, d12 = g.fy / z, -((g.fy * q[:, 1]) / (z * z))
        jc = np.stack([np.stack([-(d02 * q[:, 1]), d02 * q[:, 0] - d00 * q[:, 2], d00 * q[:, 1], -d00, zero, -d02], 1),
                       np.stack([d11 * q[:, 2] - d12 * q[:, 1], d12 * q[:, 0], -(d11 * q[:, 0]), zero, -d11, -d12], 1)], 1)
        jp = np.stack([np.stack([d00 * rot[:, kk, 0] + d02 * rot[:, kk, 2] for kk in range(3)], 1),
                       np.stack([d11 * rot[:, kk, 1] + d12 * rot[:, kk, 2] for kk in range(3)], 1)], 1)
        jc, jp = jc / sigma, jp / sigma
    jc, jp = np.where(ok[:, None, None], jc, 0.0), np.where(ok[:, None, None], jp, 0.0)
    r = res / sigma
    rho, w = huber(r, k)
    return r, w, rho, jc, jp


LOWER = [(a, b) for a in range(6) for b in range(a + 1)]  # the order the device stores a camera's block in


def linearise(g: Graph, x, sigma, k):
    """(f, grad [n, 6], U [nc, 6, 6] symmetric, V [n - nc, 6] = (v00, v10, v11, v20, v21, v22), entries)."""
    r, w, rho, jc, jp = entries_at(g, x, sigma, k)
    f = 0.5 * tree(g.gather_sum(rho, ()))
    jcw, jpw = w[:, None, None] * jc, w[:, None, None] * jp
    gterm = np.zeros((len(r), 6))
    gterm[:, :6] = np.where(g.is_cam[:, None], jcw[:, 0, :] * r[:, 0:1] + jcw[:, 1, :] * r[:, 1:2], 0.0)
    gterm[:, :3] = np.where(g.is_cam[:, None], gterm[:, :3], jpw[:, 0, :] * r[:, 0:1] + jpw[:, 1, :] * r[:, 1:2])
    grad = g.gather_sum(gterm, (6,))
    grad[g.anchor_c] = 0.0
    ut = np.zeros((len(r), 6, 6))
    for a, b in LOWER:
        ut[:, a, b] = jcw[:, 0, a] * jc[:, 0, b] + jcw[:, 1, a] * jc[:, 1, b]
        ut[:, b, a] = ut[:, a, b]
    u = g.gather_sum(np.where(g.is_cam[:, None, None], ut, 0.0), (6, 6))[:g.nc]
    vt = np.stack([jpw[:, 0, a] * jp[:, 0, b] + jpw[:, 1, a] * jp[:, 1, b] for a, b in LOWER[:6]], 1)
    v = g.gather_sum(np.where(g.is_cam[:, None], 0.0, vt), (6,))[g.nc:]
    return f, grad, u, v, (r, w, jc, jp, jcw, jpw)


def point_solve(v, lam, b):
    """(V + lam I)^-1 b per point, elimination without pivoting, written out."""
    with np.errstate(all="ignore"):
        a00, a01, a02 = v[:, 0] + lam, v[:, 1], v[:, 3]
        a11, a12, a22 = v[:, 2] + lam, v[:, 4], v[:, 5] + lam
        l10, l20 = a01 / a00, a02 / a00
        a11 = a11 - l10 * a01
        a12 = a12 - l10 * a02
        a22 = a22 - l20 * a02
        l21 = a12 / a11
        a22 = a22 - l21 * a12
        b0 = b[:, 0]
        b1 = b[:, 1] - l10 * b0
        b2 = (b[:, 2] - l20 * b0) - l21 * b1
        x2 = b2 / a22
        x1 = (b1 - a12 * x2) / a11
        x0 = ((b0 - a01 * x1) - a02 * x2) / a00
    return np.stack([x0, x1, x2], 1)


def camera_factor(u, lam):
    """The Cholesky factor of U + lam I per camera, row by row; a pivot that is not positive gives NaN, which ends in a rejected trial."""
    low = np.zeros_like(u)
    with np.errstate(all="ignore"):
        for i in range(6):
            for j in range(i + 1):
                acc = u[:, i, j] + lam if i == j else u[:, i, j]
                for k in range(j):
                    acc = acc - low[:, i, k] * low[:, j, k]
                low[:, i, j] = np.sqrt(acc) if i == j else acc / low[:, j, j]
    return low


def camera_solve(low, b, anchor_c):
    with np.errstate(all="ignore"):
        y = np.zeros_like(b)
        for i in range(6):
            acc = b[:, i]
            for k in range(i):
                acc = acc - low[:, i, k] * y[:, k]
            y[:, i] = acc / low[:, i, i]
        x = np.zeros_like(b)
        for i in range(5, -1, -1):
            acc = y[:, i]
            for k in range(i + 1, 6):
                acc = acc - low[:, k, i] * x[:, k]
            x[:, i] = acc / low[:, i, i]
    x[anchor_c] = 0.0
    return x


def dot6(a, b):
    return chain([a[:, i] * b[:, i] for i in range(6)])


def w_times(g: Graph, ent, y):
    """Per camera: sum over its list of W y_point = (w Jc)^T (Jp y); y [n, 3+] by compact node."""
    _, _, _, jp, jcw, _ = ent
    yy = y[g.nbr]
    tmp = [(jp[:, a, 0] * yy[:, 0] + jp[:, a, 1] * yy[:, 1]) + jp[:, a, 2] * yy[:, 2] for a in range(2)]
    term = jcw[:, 0, :] * tmp[0][:, None] + jcw[:, 1, :] * tmp[1][:, None]
    return g.gather_sum(np.where(g.is_cam[:, None], term, 0.0), (6,))[:g.nc]


def wt_times(g: Graph, ent, d):
    """Per point: sum over its list of W^T d_camera = (w Jp)^T (Jc d); d [nc, 6]."""
    _, _, jc, _, _, jpw = ent
    dd = d[np.where(g.is_cam, 0, g.nbr)]
    tmp = [chain([jc[:, a, b] * dd[:, b] for b in range(6)]) for a in range(2)]
    term = jpw[:, 0, :] * tmp[0][:, None] + jpw[:, 1, :] * tmp[1][:, None]
    return g.gather_sum(np.where(g.is_cam[:, None], 0.0, term), (3,))[g.nc:]


def nodes_tree(g: Graph, cam_values):
    t = np.zeros(g.n)
    t[:g.nc] = cam_values
    return tree(t)


def schur_apply(g: Graph, ent, u, v, lam, d):
    """S d with S = U + lam I - W (V + lam I)^-1 W^T; the anchor's row zero."""
    tp = np.zeros((g.n, 3))
    tp[g.nc:] = point_solve(v, lam, wt_times(g, ent, d))
    ud = np.stack([chain([(u[:, a, b] + lam if a == b else u[:, a, b]) * d[:, b] for b in range(6)]) for a in range(6)], 1)
    sd = ud - w_times(g, ent, tp)
    sd[g.anchor_c] = 0.0
    return sd


def step(g: Graph, ent, grad, u, v, lam, forcing, inner_cap):
    """The inexact damped step: (dx [n, 6], model decrease, CG iterations)."""
    nc, ac = g.nc, g.anchor_c
    y = np.zeros((g.n, 3))
    y[nc:] = point_solve(v, lam, grad[nc:, :3])
    rhs = w_times(g, ent, y) - grad[:nc]
    rhs[ac] = 0.0
    low = camera_factor(u, lam)
    xc, r = np.zeros((nc, 6)), rhs.copy()
    z = camera_solve(low, r, ac)
    d = z.copy()
    with np.errstate(all="ignore"):
        rz, rr = nodes_tree(g, dot6(r, z)), nodes_tree(g, dot6(r, r))
        target = forcing * np.sqrt(rr)
        its = 0
        while its < inner_cap and not np.sqrt(rr) <= target and rz > 0:
            sd = schur_apply(g, ent, u, v, lam, d)
            alpha = rz / nodes_tree(g, dot6(d, sd))
            xc = xc + alpha * d
            r = r - alpha * sd
            rr = nodes_tree(g, dot6(r, r))
            z = camera_solve(low, r, ac)
            rz_new = nodes_tree(g, dot6(r, z))
            beta = rz_new / rz
            d = z + beta * d
            rz = rz_new
            its += 1
        dx = np.zeros((g.n, 6))
        dx[:nc] = xc
        dx[nc:, :3] = -point_solve(v, lam, grad[nc:, :3] + wt_times(g, ent, xc))
        # the model decrease of this very step
        _, w, jc, jp, _, _ = ent
        dc, dp = dx[g.ci], dx[g.pj]
        jd = [chain([jc[:, a, b] * dc[:, b] for b in range(6)]) + ((jp[:, a, 0] * dp[:, 0] + jp[:, a, 1] * dp[:, 1]) + jp[:, a, 2] * dp[:, 2]) for a in range(2)]
        hs = g.gather_sum(w * (jd[0] * jd[0] + jd[1] * jd[1]), ())
        gd = np.where(np.arange(g.n) < nc, dot6(grad, dx), (grad[:, 0] * dx[:, 0] + grad[:, 1] * dx[:, 1]) + grad[:, 2] * dx[:, 2])
        model = -tree(gd + 0.25 * hs)
    return dx, model, its


def mm3(a, b):
    """[m, 3, 3] products, each entry (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j."""
    return np.stack([np.stack([(a[:, i, 0] * b[:, 0, j] + a[:, i, 1] * b[:, 1, j]) + a[:, i, 2] * b[:, 2, j] for j in range(3)], 1) for i in range(3)], 1)


def retract(g: Graph, x, dx):
    nc = g.nc
    out = x.copy()
    r, t, om, v = x[:nc, :9].reshape(-1, 3, 3), x[:nc, 9:12], dx[:nc, :3], dx[:nc, 3:6]
    with np.errstate(all="ignore"):
        h = 0.5 * om
        s = 2.0 / (1.0 + ((h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1]) + h[:, 2] * h[:, 2]))
        zero = np.zeros(nc)
        hh = np.stack([np.stack([zero, -h[:, 2], h[:, 1]], 1), np.stack([h[:, 2], zero, -h[:, 0]], 1), np.stack([-h[:, 1], h[:, 0], zero], 1)], 1)
        q = np.eye(3)[None] + s[:, None, None] * (hh + mm3(hh, hh))
        out[:nc, :9] = mm3(r, q).reshape(-1, 9)
        out[:nc, 9:12] = t + np.stack([(r[:, i, 0] * v[:, 0] + r[:, i, 1] * v[:, 1]) + r[:, i, 2] * v[:, 2] for i in range(3)], 1)
        out[nc:, :3] = x[nc:, :3] + dx[nc:, :3]
    out[g.anchor_c] = x[g.anchor_c]
    return out


def inf_norm(g: Graph, grad):
    a = np.abs(grad)
    m = a[:, 0]
    for i in range(1, 6):
        m = pick_max(m, a[:, i])
    return tree(m, pick_max)


def solve(cameras, track_off, image, uv, point, track_enable=None, meas_enable=None, *, anchor: int = -1, measurement_sigma=DEFAULTS["measurement_sigma"],
          huber_k=DEFAULTS["huber_k"], reproj_error_threshold=DEFAULTS["reproj_error_threshold"], min_track_length=DEFAULTS["min_track_length"],
          rel_tol=DEFAULTS["rel_tol"], abs_tol=DEFAULTS["abs_tol"], cg_forcing=DEFAULTS["cg_forcing"], max_iterations=DEFAULTS["max_iterations"],
          max_inner=DEFAULTS["max_inner"]) -> Dict[str, object]:
    """One problem. Returns the outputs the header lists, ``log`` (one dict per linear solve) and ``graph``."""
    cameras = np.ascontiguousarray(np.asarray(cameras, np.float64).reshape(-1, 17))
    track_off = np.asarray(track_off, np.int64).reshape(-1)
    image = np.asarray(image, np.int32).reshape(-1)
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    point = np.ascontiguousarray(np.asarray(point, np.float64).reshape(-1, 3))
    n_cam, t, s = len(cameras), len(track_off) - 1, len(image)
    if not (anchor >= -1 and anchor < max(n_cam, 1)):
        raise ValueError("anchor outside -1 .. N - 1")
    sigma = np.float64(measurement_sigma)
    if not (np.isfinite(sigma) and sigma > 0 and not np.isnan(huber_k) and reproj_error_threshold > 0 and min_track_length >= 1):
        raise ValueError("measurement_sigma must be positive and finite, huber_k not NaN, the threshold and min_track_length positive")
    valid, _ = validity(cameras, track_off, image, uv, point, track_enable, meas_enable, min_track_length)
    g = Graph(cameras, track_off, image, uv, valid, anchor)
    counters = dict.fromkeys(COUNTER_FIELDS, 0)
    costs = dict.fromkeys(COST_FIELDS, float("nan"))
    counters.update(status=NO_VALID_ROW, anchor=anchor, valid_measurements=g.num_valid)
    out = {"cameras": cameras.copy(), "point": point.copy(), "reproj_error": np.full(s, np.nan), "track_valid": np.zeros(t, np.uint8), "camera_kept": np.zeros(n_cam, np.uint8),
           "node_valid": np.zeros(n_cam + t, np.uint8), "counters": counters, "costs": costs, "log": [], "graph": g, "valid": valid}
    if g.anchor < 0:
        return out
    n, nc = g.n, g.nc
    counters.update(anchor=g.anchor, cameras=nc, points=n - nc)
    x = np.zeros((n, 12))
    x[:nc] = cameras[g.nodes[:nc], 5:17]
    x[nc:, :3] = point[g.nodes[nc:] - n_cam]
    with np.errstate(all="ignore"):
        f, grad, u, v, ent = linearise(g, x, sigma, huber_k)
        costs["init_cost"] = f if not np.isnan(f) else float("nan")  # one NaN: a computed one may differ in its sign bit
        out["initial_weights"], out["initial_behind"] = ent[1][g.cam_entries], int((~g.measure(x)[1][g.cam_entries]).sum())  # for the scenes' checks
        if np.isnan(f):
            counters["status"] = NON_FINITE
            return out
        inner_cap = max_inner if max_inner > 0 else 6 * nc
        lam, status, accepted, solves, cg_total, fresh = np.float64(LAMBDA_INITIAL), MAX_ITERATIONS, 0, 0, 0, True
        while status == MAX_ITERATIONS and accepted < max_iterations and solves < 2 * max_iterations + 16:
            if not fresh:
                _, grad, u, v, ent = linearise(g, x, sigma, huber_k)
                fresh = True
            solves += 1
            dx, model, its = step(g, ent, grad, u, v, lam, np.float64(cg_forcing), inner_cap)
            cg_total += its
            x_new = retract(g, x, dx)
            f_new = cost(g, x_new, sigma, huber_k)
            ok = bool(np.isfinite(f_new) and model > 0 and (f - f_new) / model > MIN_FIDELITY)
            out["log"].append({"cost": f, "trial_cost": f_new, "model": model, "lambda": lam, "cg": its, "accepted": ok})
            if ok:
                dec = f - f_new
                rel = dec / f
                x, f, fresh = x_new, f_new, False
                accepted += 1
                lam = lam / LAMBDA_FACTOR
                if dec < abs_tol or rel < rel_tol:
                    status = CONVERGED
            else:
                lam = lam * LAMBDA_FACTOR
                if lam > LAMBDA_UPPER:
                    status = LAMBDA_BOUND
        if not fresh:
            _, grad, u, v, ent = linearise(g, x, sigma, huber_k)
        costs.update(final_cost=f, gradient_inf_norm=inf_norm(g, grad), **{"lambda": lam})
        counters.update(status=status, accepted_steps=accepted, solves_tried=solves, cg_iterations=cg_total)
        out["cameras"][g.nodes[:nc], 5:17] = x[:nc]
        out["point"][g.nodes[nc:] - n_cam] = x[nc:, :3]
        out["node_valid"][g.nodes] = 1
        _, ok, res, _ = g.measure(x)
        err = np.where(ok, np.sqrt(res[:, 0] * res[:, 0] + res[:, 1] * res[:, 1]), np.nan)
        pe = g.pt_entries
        out["reproj_error"][g.row[pe]] = err[pe]
        good = np.ones(n, bool)
        np.logical_and.at(good, g.node[pe], err[pe] < reproj_error_threshold)
        out["track_valid"][g.nodes[nc:] - n_cam] = good[nc:]
        ce = g.cam_entries
        kept = np.zeros(n, bool)
        np.logical_or.at(kept, g.node[ce], good[g.nbr[ce]])
        out["camera_kept"][g.nodes[:nc]] = kept[:nc]
        out["x"] = x
    return out


def problem_arrays(track_off, image, uv, point, track_enable, meas_enable, problem_off, p):
    """Problem p of a batch as arrays of its own: the six arrays ``solve`` takes after the cameras."""
    tlo, thi = int(problem_off[p]), int(problem_off[p + 1])
    track_off = np.asarray(track_off, np.int64)
    mlo, mhi = int(track_off[tlo]), int(track_off[thi])
    cut = lambda a, lo, hi: None if a is None else np.asarray(a)[lo:hi]  # noqa: E731
    return track_off[tlo:thi + 1] - mlo, cut(image, mlo, mhi), cut(uv, mlo, mhi), cut(point, tlo, thi), cut(track_enable, tlo, thi), cut(meas_enable, mlo, mhi)


def filter_margin(result, threshold):
    """The smallest distance of a finite reprojection error from the threshold (inf when there is none)."""
    e = result["reproj_error"]
    e = e[np.isfinite(e)]
    return float(np.min(np.abs(e - threshold))) if e.size and np.isfinite(threshold) else float("inf")


def fit_similarity(x, truth):
    """Least-squares s, R, t with s R x + t ~ truth (Umeyama) over finite rows; returns the mapped x."""
    ok = np.isfinite(x).all(1) & np.isfinite(truth).all(1)
    mx, mt = x[ok].mean(0), truth[ok].mean(0)
    xc, tc = x[ok] - mx, truth[ok] - mt
    uu, dd, vt = np.linalg.svd(tc.T @ xc)
    sgn = np.diag([1.0, 1.0, np.sign(np.linalg.det(uu @ vt))])
    rot = uu @ sgn @ vt
    s = float((dd * np.diag(sgn)).sum() / (xc * xc).sum())
    return s * (x - mx) @ rot.T + mt, s, rot
