"""A 60-digit arbiter for the two-view bundle adjustment: the minimiser of the cost that tests/two_view_ba_reference.py states, found by other
means, for pairs of at most 16 points (as tests/triangulation_arbiter.py is for the triangulation).

It shares no code with the restatement: the residuals are written out in mpmath, every Jacobian is a central difference of those residuals
(h = 1e-25 at 60 digits: truncation ~1e-50, rounding ~1e-35), and the minimiser is a Gauss-Newton iteration on the re-weighted residuals
with step halving on the cost -- no damping schedule, no model-fidelity test, no stopping tolerance but the step's own size. The certificate
is the gradient of the robust cost, sum of w J^T r over all factors, at the point it returns: its largest entry is reported, and a point
with a gradient of 1e-25 in a cost whose Gauss-Newton matrix is positive definite (the Cholesky of every block succeeds) is a local
minimiser to far more digits than float64 holds. The Huber cost is once differentiable, so that gradient is exact also at the kink."""

from __future__ import annotations

from typing import Dict, List

import mpmath
from mpmath import mp, mpf

DIGITS = 60
H = mpf(10) ** -25


def _skew(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def _exp(w):
    t2 = w[0] ** 2 + w[1] ** 2 + w[2] ** 2
    if t2 == 0:
        return mp.eye(3)
    t = mp.sqrt(t2)
    k = _skew(w)
    return mp.eye(3) + (mp.sin(t) / t) * k + ((1 - mp.cos(t)) / t2) * (k * k)


def _log(r):
    v = [(r[2, 1] - r[1, 2]) / 2, (r[0, 2] - r[2, 0]) / 2, (r[1, 0] - r[0, 1]) / 2]
    s = mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
    if s == 0:
        return v
    f = mp.atan2(s, (r[0, 0] + r[1, 1] + r[2, 2] - 1) / 2) / s
    return [x * f for x in v]


def _moved(r, t, d):
    """(R Exp(omega), t + R v)."""
    return r * _exp(d[:3]), t + r * mp.matrix(d[3:6])


def _residual(r, t, k, p, uv):
    """Pixel residual of one measurement, or None behind the camera."""
    q = r.T * (p - t)
    if not q[2] > 0:
        return None
    return [k[0] * q[0] / q[2] + k[2] - uv[0], k[1] * q[1] / q[2] + k[3] - uv[1]]


def _huber(res, kh):
    e = mp.sqrt(res[0] ** 2 + res[1] ** 2)
    return (e * e / 2, mpf(1)) if e <= kh else (kh * (e - kh / 2), kh / e)


class Problem:
    def __init__(self, k1, k2, uv1, uv2, i2Ri1, i2Ui1, points, huber_k=1.345, sigma=1.0, pose_sigma=0.1, point_sigma=0.1):
        mp.dps = DIGITS
        m = lambda a: mp.matrix([[mpf(float(x)) for x in row] for row in a])  # noqa: E731
        v = lambda a: mp.matrix([mpf(float(x)) for x in a])  # noqa: E731
        self.k = [[mpf(float(x)) for x in k1], [mpf(float(x)) for x in k2]]
        self.uv = [[[mpf(float(x)) for x in row] for row in uv1], [[mpf(float(x)) for x in row] for row in uv2]]
        rin, tin = m(i2Ri1), v(i2Ui1)
        self.r, self.t = [mp.eye(3), rin.T], [mp.zeros(3, 1), -(rin.T * tin)]
        self.p = [v(x) for x in points]
        self.p0 = self.p[0].copy()
        self.kh, self.sigma, self.pose_sigma, self.point_sigma = mpf(huber_k), mpf(sigma), mpf(pose_sigma), mpf(point_sigma)
        self.n = len(self.p)

    def _prior_pose(self, r, t):
        return [x / self.pose_sigma for x in _log(r)] + [t[i] / self.pose_sigma for i in range(3)]

    def cost(self, r=None, t=None, p=None):
        r, t, p = r or self.r, t or self.t, p or self.p
        total = mpf(0)
        for c in range(2):
            for j in range(self.n):
                res = _residual(r[c], t[c], self.k[c], p[j], self.uv[c][j])
                if res is not None:
                    total += _huber([x / self.sigma for x in res], self.kh)[0]
        total += sum(x * x for x in self._prior_pose(r[0], t[0])) / 2
        d = p[0] - self.p0
        return total + (d[0] ** 2 + d[1] ** 2 + d[2] ** 2) / (2 * self.point_sigma ** 2)

    def system(self):
        """Gauss-Newton blocks from central differences: hcc [12, 12], hcp [n] of [12, 3], hpp [n] of [3, 3], gc [12], gp [n] of [3]."""
        n = self.n
        hcc, gc = mp.zeros(12, 12), mp.zeros(12, 1)
        hcp, hpp, gp = [mp.zeros(12, 3) for _ in range(n)], [mp.zeros(3, 3) for _ in range(n)], [mp.zeros(3, 1) for _ in range(n)]
        unit = lambda i, size: [H if a == i else mpf(0) for a in range(size)]  # noqa: E731
        for c in range(2):
            plus = [_moved(self.r[c], self.t[c], unit(a, 6)) for a in range(6)]
            minus = [_moved(self.r[c], self.t[c], [-x for x in unit(a, 6)]) for a in range(6)]
            for j in range(n):
                res = _residual(self.r[c], self.t[c], self.k[c], self.p[j], self.uv[c][j])
                if res is None:
                    continue
                res = [x / self.sigma for x in res]
                _, w = _huber(res, self.kh)
                jc = mp.zeros(2, 6)
                jp = mp.zeros(2, 3)
                for a in range(6):
                    hi = _residual(*plus[a], self.k[c], self.p[j], self.uv[c][j])
                    lo = _residual(*minus[a], self.k[c], self.p[j], self.uv[c][j])
                    for row in range(2):
                        jc[row, a] = (hi[row] - lo[row]) / (2 * H) / self.sigma
                for a in range(3):
                    step = mp.matrix(unit(a, 3))
                    hi = _residual(self.r[c], self.t[c], self.k[c], self.p[j] + step, self.uv[c][j])
                    lo = _residual(self.r[c], self.t[c], self.k[c], self.p[j] - step, self.uv[c][j])
                    for row in range(2):
                        jp[row, a] = (hi[row] - lo[row]) / (2 * H) / self.sigma
                rv = mp.matrix(res)
                s = slice(6 * c, 6 * c + 6)
                hcc[s, s] += w * (jc.T * jc)
                gc[s, 0] += w * (jc.T * rv)
                hcp[j][s, :] = w * (jc.T * jp)
                hpp[j] += w * (jp.T * jp)
                gp[j] += w * (jp.T * rv)
        base = self._prior_pose(self.r[0], self.t[0])
        jac = mp.zeros(6, 6)
        for a in range(6):
            hi = self._prior_pose(*_moved(self.r[0], self.t[0], unit(a, 6)))
            lo = self._prior_pose(*_moved(self.r[0], self.t[0], [-x for x in unit(a, 6)]))
            for row in range(6):
                jac[row, a] = (hi[row] - lo[row]) / (2 * H)
        hcc[0:6, 0:6] += jac.T * jac
        gc[0:6, 0] += jac.T * mp.matrix(base)
        inv = 1 / self.point_sigma ** 2
        hpp[0] += inv * mp.eye(3)
        gp[0] += inv * (self.p[0] - self.p0)
        return hcc, hcp, hpp, gc, gp

    def gradient_max(self, blocks=None):
        _, _, _, gc, gp = blocks or self.system()
        return max([abs(x) for x in gc] + [abs(x) for g in gp for x in g])

    def minimise(self, max_iterations: int = 400, step_tol=mpf(10) ** -32) -> Dict[str, object]:
        cost = self.cost()
        history: List[str] = []
        for it in range(max_iterations):
            hcc, hcp, hpp, gc, gp = self.system()
            s, b = hcc.copy(), -gc
            inv = []
            for j in range(self.n):
                mpmath.cholesky(hpp[j])  # raises unless positive definite
                vi = hpp[j] ** -1
                inv.append(vi)
                s -= hcp[j] * vi * hcp[j].T
                b += hcp[j] * vi * gp[j]
            mpmath.cholesky(s)
            dc = mp.lu_solve(s, b)
            dp = [-(inv[j] * (gp[j] + hcp[j].T * dc)) for j in range(self.n)]
            size = max([abs(x) for x in dc] + [abs(x) for d in dp for x in d])
            scale = mpf(1)
            while True:  # step halving on the cost
                r = [_moved(self.r[c], self.t[c], [scale * dc[6 * c + a] for a in range(6)]) for c in range(2)]
                p = [self.p[j] + scale * dp[j] for j in range(self.n)]
                new = self.cost([x[0] for x in r], [x[1] for x in r], p)
                if new <= cost or scale < mpf(2) ** -40:
                    break
                scale /= 2
            if new <= cost:
                self.r, self.t, self.p, cost = [x[0] for x in r], [x[1] for x in r], p, new
            history.append(mp.nstr(cost, 25))
            if size * scale < step_tol or new > cost:
                break
        rel = self.r[1].T * self.r[0]
        tr = self.r[1].T * (self.t[0] - self.t[1])
        norm = mp.sqrt(tr[0] ** 2 + tr[1] ** 2 + tr[2] ** 2)
        return {"cost": cost, "gradient_max": self.gradient_max(), "iterations": it + 1, "rotation": [[float(rel[i, j]) for j in range(3)] for i in range(3)],
                "translation": [float(tr[i] / norm) for i in range(3)], "history": history}
