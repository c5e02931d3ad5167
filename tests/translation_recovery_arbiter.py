"""The arbiter of the translation-recovery restatement: a dense ``np.longdouble`` damped Newton iteration on the stated cost, sharing no code
with tests/translation_recovery_reference.py. The rows, the anchor's component and the cost f(x) = sum_e rho(|unit(x_b - x_a) - z_e| / sigma) +
rho(|(x_b - x_a) - scale z_e0| / sigma) are written out from the scene's arrays; the gradient is assembled row by row from
d|r|/dx_b = P_u r / (|d| |r|), the matrix is the Gauss-Newton one with the Huber weights plus a Levenberg damping lambda diag(H), solved by
Gaussian elimination with partial pivoting in longdouble (numpy's solvers stop at float64). A step is kept when the cost falls; lambda
shrinks by 10 then and grows by 10 otherwise; the tolerances are 0: the iteration ends when lambda passes 1e12 or after MAX_STEPS."""

from __future__ import annotations

import numpy as np

LD = np.longdouble
MAX_STEPS = 80
MAX_NODES = 130  # the dense system is O(n^3) in longdouble


def rows_of(sc):
    e, n = len(sc["pair_images"]), sc["num_images"]
    track = np.repeat(np.arange(len(sc["track_off"]) - 1), np.diff(sc["track_off"]))
    a = np.concatenate([np.asarray(sc["pair_images"], np.int64).reshape(-1, 2)[:, 1], np.asarray(sc["image"], np.int64)])
    b = np.concatenate([np.asarray(sc["pair_images"], np.int64).reshape(-1, 2)[:, 0], n + track])
    z = np.concatenate([np.asarray(sc["world_pair"], np.float64).reshape(-1, 3), np.asarray(sc["world_meas"], np.float64).reshape(-1, 3)])
    on = np.concatenate([np.ones(e, bool) if sc["pair_enable"] is None else np.asarray(sc["pair_enable"]) != 0,
                         np.ones(len(track), bool) if sc["meas_enable"] is None else np.asarray(sc["meas_enable"]) != 0])
    return a, b, z, on & np.isfinite(z).all(1)


def component(a, b, valid, anchor):
    seen, grew = {int(anchor)}, True
    while grew:
        grew = False
        for i, j in zip(a[valid], b[valid]):
            if (int(i) in seen) != (int(j) in seen):
                seen.update((int(i), int(j)))
                grew = True
    return seen


def rho_and_weight(s, k):
    if k > 0 and np.isfinite(k):
        beyond = s > LD(k)
        return np.where(beyond, LD(k) * (s - LD(k) / 2), s * s / 2), np.where(beyond, LD(k) / np.where(beyond, s, LD(1)), LD(1))
    return s * s / 2, np.ones_like(s)


class Problem:
    def __init__(self, sc, anchor, scale, sigma, k):
        a, b, z, valid = rows_of(sc)
        inside = component(a, b, valid, anchor)
        keep = valid & np.array([int(i) in inside for i in a])
        self.a, self.b, self.z = a[keep], b[keep], z[keep].astype(LD)
        self.e0 = 0  # the first valid row of the component
        self.anchor, self.scale, self.sigma, self.k = int(anchor), LD(scale), LD(sigma), k
        self.free = sorted(inside - {int(anchor)})
        self.col = {node: 3 * i for i, node in enumerate(self.free)}

    def parts(self, x):
        d = x[self.b] - x[self.a]
        nrm = np.sqrt((d * d).sum(1))
        u = d / nrm[:, None]
        r = u - self.z
        rn = np.sqrt((r * r).sum(1))
        rho, w = rho_and_weight(rn / self.sigma, self.k)
        rs = d[self.e0] - self.scale * self.z[self.e0]
        rho_s, w_s = rho_and_weight(np.sqrt((rs * rs).sum())[None] / self.sigma, self.k)
        return d, nrm, u, r, rho, w, rs, rho_s[0], w_s[0]

    def cost(self, x):
        p = self.parts(x)
        return p[4].sum() + p[7]

    def system(self, x):
        d, nrm, u, r, rho, w, rs, rho_s, w_s = self.parts(x)
        m = 3 * len(self.free)
        g, h = np.zeros(m, LD), np.zeros((m, m), LD)
        eye = np.eye(3, dtype=LD)
        for e in range(len(self.a)):
            proj = eye - np.outer(u[e], u[e])
            ge = (w[e] / (nrm[e] * self.sigma * self.sigma)) * (proj @ r[e])
            he = (w[e] / (nrm[e] * self.sigma) ** 2) * proj
            if e == self.e0:
                ge = ge + (w_s / self.sigma ** 2) * rs
                he = he + (w_s / self.sigma ** 2) * eye
            ca, cb = self.col.get(int(self.a[e])), self.col.get(int(self.b[e]))
            if cb is not None:
                g[cb:cb + 3] += ge
                h[cb:cb + 3, cb:cb + 3] += he
            if ca is not None:
                g[ca:ca + 3] -= ge
                h[ca:ca + 3, ca:ca + 3] += he
            if ca is not None and cb is not None:
                h[ca:ca + 3, cb:cb + 3] -= he
                h[cb:cb + 3, ca:ca + 3] -= he
        return g, h


def solve_dense(h, g):
    """h y = g by Gaussian elimination with partial pivoting, in the arrays' own precision."""
    n = len(g)
    m = np.concatenate([h, g[:, None]], axis=1).copy()
    for c in range(n):
        p = c + int(np.argmax(np.abs(m[c:, c])))
        if p != c:
            m[[c, p]] = m[[p, c]]
        m[c + 1:] -= np.outer(m[c + 1:, c] / m[c, c], m[c])
    y = np.zeros(n, m.dtype)
    for c in range(n - 1, -1, -1):
        y[c] = (m[c, n] - m[c, c + 1:n] @ y[c + 1:]) / m[c, c]
    return y


def refine(sc, result, scale, sigma, k):
    """From the restatement's ``result`` on ``sc``: {"cost", "x", "steps", "gradient"} at the point the damped Newton iteration ends."""
    prob = Problem(sc, result["counters"]["anchor"], scale, sigma, k)
    x = np.nan_to_num(np.asarray(result["translation"], np.float64)).astype(LD)
    f, lam, steps = prob.cost(x), LD(1e-6), 0
    g, h = prob.system(x)
    while steps < MAX_STEPS and lam <= 1e12 and len(prob.free):
        step = solve_dense(h + lam * np.diag(np.diag(h)), -g)
        trial = x.copy()
        for node, c in prob.col.items():
            trial[node] += step[c:c + 3]
        f_trial = prob.cost(trial)
        steps += 1
        if f_trial < f:
            x, f, lam = trial, f_trial, lam / 10
            g, h = prob.system(x)
        else:
            lam = lam * 10
    return {"cost": f, "x": x, "steps": steps, "gradient": float(np.abs(g).max()) if len(g) else 0.0}
