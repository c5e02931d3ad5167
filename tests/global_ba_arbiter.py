"""An arbiter for the global bundle adjustment's restatement (tests/global_ba_reference.py) that shares no code with it: the same cost
minimised by a DENSE Levenberg-Marquardt in np.longdouble -- the residuals of all measurements as one vector function of all unknowns
(six per camera but the anchor, three per point), its Jacobian by the complex-step derivative in np.clongdouble (exact to rounding: the
residual is a rational function of the unknowns), the Huber weights applied to rows, the damped normal equations solved exactly by
Gaussian elimination with partial pivoting. A step is kept when it lowers the cost; the loop ends when twenty damping levels in a row
bring no decrease. Poses move along the same Cayley chart, so that the minimiser is parametrised alike; nothing else is shared."""

import numpy as np

LD, CLD = np.longdouble, np.clongdouble


def cayley(w):
    h = w / 2
    s = 2 / (1 + h[0] * h[0] + h[1] * h[1] + h[2] * h[2])
    k = np.array([[0 * h[0], -h[2], h[1]], [h[2], 0 * h[0], -h[0]], [-h[1], h[0], 0 * h[0]]])
    return np.eye(3, dtype=w.dtype) + s * (k + k @ k)


class Problem:
    def __init__(self, cameras, image, track, uv, points, anchor, sigma, huber_k):
        self.intr = np.asarray(cameras[:, 1:5], LD)
        self.rot = [np.asarray(c[5:14], LD).reshape(3, 3) for c in cameras]
        self.trans = [np.asarray(c[14:17], LD) for c in cameras]
        self.points = np.asarray(points, LD)
        self.image, self.track, self.uv = np.asarray(image), np.asarray(track), np.asarray(uv, np.float32).astype(LD)
        self.free = [i for i in sorted(set(self.image.tolist())) if i != anchor]
        self.sigma, self.k = LD(sigma), huber_k
        self.num = 6 * len(self.free) + 3 * len(self.points)

    def residuals(self, delta):
        """[S, 2] scaled residuals at the values held moved by ``delta`` (longdouble or clongdouble)."""
        dt = delta.dtype
        rot, trans = [r.astype(dt) for r in self.rot], [t.astype(dt) for t in self.trans]
        for n, i in enumerate(self.free):
            d = delta[6 * n:6 * n + 6]
            rot[i], trans[i] = self.rot[i].astype(dt) @ cayley(d[:3]), self.trans[i].astype(dt) + self.rot[i].astype(dt) @ d[3:]
        pts = self.points.astype(dt) + delta[6 * len(self.free):].reshape(-1, 3)
        q = np.einsum("sji,sj->si", np.stack(rot)[self.image], pts[self.track] - np.stack(trans)[self.image])
        ok = q[:, 2].real > 0
        z = np.where(ok, q[:, 2], 1)
        k = self.intr[self.image]
        out = np.stack([(k[:, 0] * q[:, 0] / z + k[:, 2] - self.uv[:, 0]) / self.sigma, (k[:, 1] * q[:, 1] / z + k[:, 3] - self.uv[:, 1]) / self.sigma], axis=1)
        return np.where(ok[:, None], out, 0)

    def cost_weights(self, r):
        e = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])
        robust = np.isfinite(self.k) and self.k > 0
        beyond = (e > self.k) if robust else np.zeros(len(e), bool)
        k = LD(self.k) if robust else LD(0)
        rho = np.where(beyond, k * (e - k / 2), e * e / 2)
        return rho.sum(), np.where(beyond, k / np.where(beyond, e, 1), LD(1))

    def jacobian(self):
        step = LD(1e-30)
        jac = np.zeros((2 * len(self.image), self.num), dtype=LD)
        for k in range(self.num):
            d = np.zeros(self.num, dtype=CLD)
            d[k] = 1j * step
            jac[:, k] = (self.residuals(d).imag / step).reshape(-1)
        return jac

    def move(self, delta):
        delta = np.asarray(delta, LD)
        for n, i in enumerate(self.free):
            d = delta[6 * n:6 * n + 6]
            self.rot[i], self.trans[i] = self.rot[i] @ cayley(d[:3]), self.trans[i] + self.rot[i] @ d[3:]
        self.points = self.points + delta[6 * len(self.free):].reshape(-1, 3)


def solve_dense(a, b):
    """a x = b by Gaussian elimination with partial pivoting, in the arrays' own precision."""
    a, b = a.copy(), b.copy()
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        if p != k:
            a[[k, p]], b[[k, p]] = a[[p, k]], b[[p, k]]
        f = a[k + 1:, k] / a[k, k]
        a[k + 1:, k:] -= f[:, None] * a[k, k:][None, :]
        b[k + 1:] -= f * b[k]
    x = np.zeros(n, dtype=a.dtype)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - a[k, k + 1:] @ x[k + 1:]) / a[k, k]
    return x


def minimise(cameras, track_off, image, uv, point, valid, node_valid, anchor, sigma=1.0, huber_k=1.345, max_steps=60):
    """The minimum reached from the given start over the valid measurements of the problem's nodes. Returns cost, steps, gradient norm."""
    n_cam = len(cameras)
    track_all = np.repeat(np.arange(len(track_off) - 1), np.diff(track_off))
    rows = np.flatnonzero(valid & (node_valid[n_cam + track_all] != 0))
    ids = np.flatnonzero(node_valid[n_cam:])
    renum = np.full(len(track_off) - 1, -1)
    renum[ids] = np.arange(len(ids))
    pr = Problem(np.asarray(cameras, np.float64), np.asarray(image)[rows], renum[track_all[rows]], np.asarray(uv)[rows], np.asarray(point)[ids], anchor, sigma, huber_k)
    zero = np.zeros(pr.num, dtype=LD)
    f, w = pr.cost_weights(pr.residuals(zero))
    lam, steps, idle, grad = LD(1e-5), 0, 0, LD(0)
    while steps < max_steps and idle < 20:
        r = pr.residuals(zero)
        f, w = pr.cost_weights(r)
        jac = pr.jacobian()
        jw = jac * np.repeat(w, 2)[:, None]
        h, g = jw.T @ jac, jw.T @ r.reshape(-1)
        grad = np.abs(g).max()
        moved = False
        while idle < 20:
            d = solve_dense(h + lam * np.eye(pr.num, dtype=LD), -g)
            f_new, _ = pr.cost_weights(pr.residuals(d))
            if np.isfinite(f_new) and f_new < f:
                pr.move(d)
                lam, idle, moved = lam / 10, 0, True
                steps += 1
                f = f_new
                break
            lam, idle = lam * 10, idle + 1
        if not moved:
            break
    return {"cost": f, "steps": steps, "gradient": grad}
