"""The arbiters of the rotation-averaging restatement: how far is the float64 answer from the critical point it stands for?

UP TO 65 NODES: ``mp_arbiter``, 60-digit mpmath, sharing no code with the restatement. The cost is written out from the scene's rows,
f = sum kappa |R_i2 M - R_i1|_F^2. The restatement's rotations are first made orthonormal to 60 digits (Newton's polar iteration), and stay so:
every update is R_k <- R_k exp(hat d_k) by Rodrigues' formula. On rotations the cost of a row is kappa (|M|^2 + 3 - 2 tr(R_i1^T R_i2 M)); its
derivatives along the exponential map are written from that trace form: with P = R_i1^T R_i2 M, N = M R_i1^T R_i2 and
w(X) = (X21 - X12, X02 - X20, X10 - X01) the gradient blocks are -2 kappa w(P) and 2 kappa w(N), the Hessian blocks
-2 kappa (sym P - tr P I), -2 kappa (sym N - tr N I) and 2 kappa [tr(E_i R_i1^T R_i2 E_j M)]_ij. That is another derivation than the
restatement's W / Lambda / vee form, another retraction (exp, not Cayley) and no trust region: a plain Newton iteration on the reduced dense
system (the anchor's three rows and columns removed) until |g|_inf <= 1e-40. The GRADIENT is evaluated in mpmath and is the certificate; the
dense Hessian is assembled and factored in float64 (numpy) from the rounded point, so each step is Newton's up to a relative 1e-10 or so and
the iteration contracts by that factor per step instead of quadratically: four to six steps from the restatement's answer. ``distance`` is
the restatement's largest per-node angle from that point in degrees (anchor at I in both) and its relative cost gap.

LARGER SCENES: ``arbiter``, the restatement's own scheme continued in ``np.longdouble`` (64 bits of mantissa where float64 has 53) from its
answer with the gradient tolerance seven orders lower. It is not independent of the restatement; it shows where the same scheme ends when run
on, which is what bounds a float64 run of it.

A scene that stopped at ``MAX_ITERATIONS`` is not near a critical point, so no arbiter is asked about it. The second measure is the
restatement's own difference between forward and reversed row order (the anchor held): only a pair listed more than once changes a sum's
order, so it is zero on most scenes. ``sensitivity(name)`` is the larger of the two, the figure the device tests multiply by the project's
standing factor 8."""

from __future__ import annotations

import functools

import numpy as np

from tests import rotation_averaging_reference as ref
from tests import rotation_averaging_scenes as scenes

ARBITER_GRADIENT_TOL = 1e-16
ARBITER_MAX_OUTER = 40
MP_DIGITS = 60
MP_MAX_NODES = 65
MP_GRADIENT_TOL = 1e-40
MP_MAX_STEPS = 16


def angle_deg(ra, rb):
    """The angle of ra^T rb in degrees, in the arrays' own precision, exact for tiny angles (atan2 of the vee norm and the trace)."""
    m = np.swapaxes(ra, -1, -2) @ rb
    v = np.stack([m[..., 2, 1] - m[..., 1, 2], m[..., 0, 2] - m[..., 2, 0], m[..., 1, 0] - m[..., 0, 1]], -1)
    return np.degrees(np.arctan2(np.sqrt((v * v).sum(-1)), m[..., 0, 0] + m[..., 1, 1] + m[..., 2, 2] - 1.0))


def max_angle_deg(a, b) -> float:
    """Largest per-node angle between two [N, 9] outputs over the rows finite in both (0.0 when there is none)."""
    a, b = np.asarray(a).reshape(-1, 3, 3), np.asarray(b).reshape(-1, 3, 3)
    on = np.isfinite(a).all((1, 2)) & np.isfinite(b).all((1, 2))
    return float(angle_deg(a[on].astype(np.longdouble), b[on].astype(np.longdouble)).max()) if on.any() else 0.0


def arbiter(sc, result):
    """The extended-precision continuation from ``result`` (a restatement's output on scene ``sc``)."""
    start = np.nan_to_num(result["wRi"].reshape(-1, 3, 3))
    opts = {k: v for k, v in scenes.options_of(sc).items() if k in ("delta0", "kappa_cg", "theta", "max_inner")}
    return ref.solve(sc["pair_images"], sc["rotation"], sc["weight"], sc["pair_enable"], num_images=sc["num_images"], anchor=result["counters"]["anchor"], start=start,
                     dtype=np.longdouble, gradient_tol=ARBITER_GRADIENT_TOL, max_outer=ARBITER_MAX_OUTER, **opts)


# ---- the mpmath arbiter: 3 x 3 matrices as lists of lists of mpf ----


def _mm(a, b):
    return [[a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j] for j in range(3)] for i in range(3)]


def _t(a):
    return [[a[j][i] for j in range(3)] for i in range(3)]


def _w(x):
    return [x[2][1] - x[1][2], x[0][2] - x[2][0], x[1][0] - x[0][1]]


def _mp_exp(d):
    from mpmath import mp, mpf

    t2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    k = [[mpf(0), -d[2], d[1]], [d[2], mpf(0), -d[0]], [-d[1], d[0], mpf(0)]]
    if t2 == 0:
        return [[mpf(i == j) for j in range(3)] for i in range(3)]
    t = mp.sqrt(t2)
    a, b, k2 = mp.sin(t) / t, (1 - mp.cos(t)) / t2, _mm(k, k)
    return [[mpf(i == j) + a * k[i][j] + b * k2[i][j] for j in range(3)] for i in range(3)]


def _mp_orthonormal(x):
    """Newton's polar iteration X <- (X + X^-T) / 2: from a float64 rotation, three steps reach 60 digits."""
    from mpmath import mp

    m = mp.matrix(x)
    for _ in range(4):
        m = (m + (m ** -1).T) / 2
    return [[m[i, j] for j in range(3)] for i in range(3)]


def _mp_angle_deg(a, b):
    from mpmath import mp

    m = _mm(_t(a), b)
    v = _w(m)
    return mp.degrees(mp.atan2(mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2), m[0][0] + m[1][1] + m[2][2] - 1))


def mp_edges(sc, result):
    """The valid rows of the solved component as (compact i1, compact i2, M, kappa) in mpmath, from the scene's arrays."""
    from mpmath import mpf

    g = result["graph"]
    rot, wgt = np.asarray(sc["rotation"], np.float64).reshape(-1, 3, 3), np.asarray(sc["weight"], np.float64).reshape(-1)
    return [(int(k), int(j), [[mpf(float(rot[e, a, b])) for b in range(3)] for a in range(3)], mpf(float(wgt[e]))) for k, j, e, o in zip(g.node, g.nbr, g.row, g.orient) if o == 1]


def mp_cost(edges, r):
    """f = sum kappa |R_i2 M - R_i1|_F^2, written out."""
    total = 0
    for i1, i2, m, kappa in edges:
        d = _mm(r[i2], m)
        total += kappa * sum((d[a][b] - r[i1][a][b]) ** 2 for a in range(3) for b in range(3))
    return total


def mp_gradient(edges, r, n):
    """The gradient of f along R_k exp(hat x_k) at x = 0, for orthonormal R: [n][3]."""
    from mpmath import mpf

    g = [[mpf(0)] * 3 for _ in range(n)]
    for i1, i2, m, kappa in edges:
        a = _mm(_t(r[i1]), r[i2])
        wp, wn = _w(_mm(a, m)), _w(_mm(m, a))
        g[i1] = [g[i1][c] - 2 * kappa * wp[c] for c in range(3)]
        g[i2] = [g[i2][c] + 2 * kappa * wn[c] for c in range(3)]
    return g


def dense_hessian(edges, r64, n):
    """The Hessian of f along the exponential map at the rounded point, float64, [3 n, 3 n], from the trace form of the module's docstring."""
    gen = np.zeros((3, 3, 3))
    gen[0, 1, 2], gen[0, 2, 1], gen[1, 0, 2], gen[1, 2, 0], gen[2, 0, 1], gen[2, 1, 0] = -1, 1, 1, -1, -1, 1
    h = np.zeros((3 * n, 3 * n))
    for i1, i2, m, kappa in edges:
        m64, k64 = np.array([[float(x) for x in row] for row in m]), float(kappa)
        a = r64[i1].T @ r64[i2]
        p, q = a @ m64, m64 @ a
        s1, s2 = slice(3 * i1, 3 * i1 + 3), slice(3 * i2, 3 * i2 + 3)
        h[s1, s1] += -2 * k64 * (0.5 * (p + p.T) - np.trace(p) * np.eye(3))
        h[s2, s2] += -2 * k64 * (0.5 * (q + q.T) - np.trace(q) * np.eye(3))
        c = 2 * k64 * np.array([[np.trace(gen[i] @ a @ gen[j] @ m64) for j in range(3)] for i in range(3)])
        h[s1, s2] += c
        h[s2, s1] += c.T
    return h


def mp_arbiter(sc, result):
    """Newton on the reduced dense system from the restatement's answer until |g|_inf <= 1e-40. Returns the rotations (compact order, mpmath),
    the cost there, the final |g|_inf, the steps taken, and the restatement's distance: degrees per node (the largest) and the relative cost gap."""
    import mpmath
    from mpmath import mp, mpf

    g = result["graph"]
    n, anchor = g.n, g.anchor_c
    with mp.workdps(MP_DIGITS):
        edges = mp_edges(sc, result)
        start = result["wRi"].reshape(-1, 3, 3)[g.nodes]
        r = [_mp_orthonormal([[mpf(float(x)) for x in row] for row in start[k]]) for k in range(n)]
        keep = np.array([3 * k + c for k in range(n) if k != anchor for c in range(3)], dtype=np.int64)
        steps, gnorm = 0, None
        while True:
            grad = mp_gradient(edges, r, n)
            grad[anchor] = [mpf(0)] * 3
            gnorm = max(abs(x) for row in grad for x in row) if n else mpf(0)
            if gnorm <= MP_GRADIENT_TOL or steps >= MP_MAX_STEPS or len(keep) == 0:
                break
            r64 = np.array([[[float(x) for x in row] for row in rk] for rk in r])
            h = dense_hessian(edges, r64, n)[np.ix_(keep, keep)]
            scaled = np.array([float(x / gnorm) for row in grad for x in row])[keep]  # the solve sees numbers of size 1, whatever |g| is
            step = np.zeros(3 * n)
            step[keep] = np.linalg.solve(h, -scaled)
            r = [_mm(r[k], _mp_exp([gnorm * mpf(float(step[3 * k + c])) for c in range(3)])) for k in range(n)]
            steps += 1
        cost = mp_cost(edges, r)
        deg = max([_mp_angle_deg([[mpf(float(x)) for x in row] for row in start[k]], r[k]) for k in range(n)] or [mpf(0)])
        f = mpf(float(result["costs"]["final_cost"]))
        return {"R": r, "cost": cost, "gradient": float(gnorm), "steps": steps, "deg": float(deg), "cost_rel": float(abs(f - cost) / max(abs(f), mpf(1))),
                "converged": bool(gnorm <= MP_GRADIENT_TOL), "digits": mpmath.mp.dps}


def reversed_rows(sc, result):
    """The restatement on the rows in reversed order, the anchor held."""
    enable = None if sc["pair_enable"] is None else sc["pair_enable"][::-1]
    return ref.solve(sc["pair_images"][::-1], sc["rotation"][::-1], sc["weight"][::-1], enable, num_images=sc["num_images"], anchor=result["counters"]["anchor"],
                     **scenes.options_of(sc))


@functools.lru_cache(maxsize=None)
def sensitivity(name):
    """``sensitivity_of`` a named scene and its restatement, once per process."""
    return sensitivity_of(scenes.get(name), scenes.expected(name))


def sensitivity_of(sc, res):
    """{"rotation_deg", "cost_rel"} and the parts they are the larger of; zeros for a scene without a solved component."""
    out = {"arbiter_deg": 0.0, "arbiter_cost_rel": 0.0, "order_deg": 0.0, "order_cost_rel": 0.0, "arbiter_gradient": float("nan"), "arbiter_status": None}
    out["arbiter"] = None
    if res["counters"]["status"] in (ref.CONVERGED, ref.MAX_ITERATIONS):
        f = res["costs"]["final_cost"]
        if res["counters"]["status"] == ref.MAX_ITERATIONS:
            pass  # not near a critical point: no arbiter has anything to say; the row order alone (and hence the bytes) binds the device
        elif sc["num_images"] <= MP_MAX_NODES:
            arb = mp_arbiter(sc, res)
            out.update(arbiter="mpmath", arbiter_deg=arb["deg"], arbiter_cost_rel=arb["cost_rel"], arbiter_gradient=arb["gradient"],
                       arbiter_status=ref.CONVERGED if arb["converged"] else ref.MAX_ITERATIONS, arbiter_steps=arb["steps"])
        else:
            arb = arbiter(sc, res)
            fa = arb["costs"]["final_cost"]
            out.update(arbiter="longdouble", arbiter_deg=max_angle_deg(res["wRi"], arb["wRi"]), arbiter_cost_rel=float(abs(np.longdouble(f) - fa) / max(abs(f), 1.0)),
                       arbiter_gradient=float(arb["costs"]["gradient_inf_norm"]), arbiter_status=arb["counters"]["status"])
        rev = reversed_rows(sc, res)
        out.update(order_deg=max_angle_deg(res["wRi"], rev["wRi"]), order_cost_rel=float(abs(f - rev["costs"]["final_cost"]) / max(abs(f), 1.0)))
    out["rotation_deg"] = max(out["arbiter_deg"], out["order_deg"])
    out["cost_rel"] = max(out["arbiter_cost_rel"], out["order_cost_rel"])
    return out
