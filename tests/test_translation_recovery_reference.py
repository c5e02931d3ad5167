"""CPU: the restatement of the translation recovery (tests/translation_recovery_reference.py) against what it stands for.

- On the noise-free scenes it recovers the planted positions after a least-squares scale and shift, within the reference's own thresholds
  (relative 3e-2, absolute 3e-1: tests/averaging/translation/test_averaging_1dsfm.py); the achieved distance is printed (measured: 2.7e-6 of
  the extent at the worst, what the 1e-5 stopping rule leaves).
- Its gradient equals 60-digit mpmath differences of f, and its Gauss-Newton Hessian-vector product equals mpmath second differences of f at
  a zero-residual point (there the Gauss-Newton matrix is the Hessian).
- The arbiter (tests/translation_recovery_arbiter.py: dense longdouble damped Newton, no shared code, tolerances 0), started from the
  restatement's answer at tolerances 0, ends at a cost within 8 x the restatement's own sensitivity (the larger of reversed summation order,
  longdouble arithmetic, and the rounding of a sum of that many rows); what the default 1e-5 stopping rule leaves above the arbiter is
  measured per scene and printed (profiles/translation_recovery_reference.txt).
- With 8 wrong rows and Huber on, the cameras stay near those of the same scene without the wrong rows; a landmark seen through a wrong row
  can fly off, so only cameras are asserted."""

import mpmath
import numpy as np
import pytest

from tests import translation_recovery_arbiter as arbiter
from tests import translation_recovery_reference as ref
from tests import translation_recovery_scenes as scenes

MARGIN = 8.0
REL_TOL, ABS_TOL = 3e-2, 3e-1  # the reference's thresholds on positions
ARBITER_SCENES = ("circle4_all_edges", "circle8_two_edges", "door12_exhaustive", "planted_noise_free", "planted_noise", "planted_wrong_huber", "pairs_only", "tracks_only",
                  "leaves", "masked_rows", "gaps", "scale_2_5", "sigma_0_5")
# the cameras of planted_wrong_huber against those of planted_noise, after the fit, relative to the extent: measured 6.85e-3 on the restatement
# (8 of 410 rows are wrong); the bound is 8 x that
MEASURED_WRONG_ROW_SHIFT = 6.85e-3


def fitted_error(sc, res, nodes=None):
    ok = res["node_valid"] == 1
    if nodes is not None:
        ok[nodes:] = False
    truth = np.where(ok[:, None], sc["truth"], np.nan)
    fit, _ = ref.fit_scale_shift(np.where(ok[:, None], res["translation"], np.nan), truth)
    extent = float((np.nanmax(truth, 0) - np.nanmin(truth, 0)).max())
    return float(np.abs(fit[ok] - truth[ok]).max()), extent


@pytest.mark.parametrize("name", scenes.NOISE_FREE)
def test_noise_free_scenes_recover_the_planted_positions(name):
    sc, res = scenes.get(name), scenes.expected(name)
    assert res["counters"]["status"] == ref.CONVERGED and res["node_valid"].all()
    err, extent = fitted_error(sc, res)
    print(f"\ntranslation_recovery_reference {name}: largest position error {err:.3e} (extent {extent:.3f}, relative {err / extent:.3e}), cost {res['costs']['final_cost']:.3e}")
    assert err <= ABS_TOL and err <= REL_TOL * extent


def mp_cost(sc, x, scale, sigma, k):
    a, b, z, valid = arbiter.rows_of(sc)
    total, first = mpmath.mpf(0), True
    for e in np.flatnonzero(valid):
        d = [x[int(b[e])][i] - x[int(a[e])][i] for i in range(3)]
        nrm = mpmath.sqrt(sum(v * v for v in d))
        r = [d[i] / nrm - mpmath.mpf(float(z[e][i])) for i in range(3)]
        terms = [mpmath.sqrt(sum(v * v for v in r)) / sigma]
        if first:
            terms.append(mpmath.sqrt(sum((d[i] - scale * mpmath.mpf(float(z[e][i]))) ** 2 for i in range(3))) / sigma)
            first = False
        for s in terms:
            total += k * (s - k / 2) if k > 0 and s > k else s * s / 2
    return total


def test_gradient_and_hessian_vector_against_mpmath_differences():
    mpmath.mp.dps = 60
    # the gradient at a point with residuals on both sides of Huber's k: the restatement's answer after one iteration
    sc = scenes.get("leaves")
    res = scenes.solve(sc, max_outer=1)
    g = res["graph"]
    with np.errstate(all="ignore"):
        f, grad, m, entries = g.model(res["x"], 1.0, 0.01, 1.3)
    x = [[mpmath.mpf(float(v)) for v in row] for row in np.nan_to_num(res["translation"])]
    assert abs(mp_cost(sc, x, mpmath.mpf(1), mpmath.mpf("0.01"), mpmath.mpf("1.3")) - mpmath.mpf(float(f))) <= 1e-12 * f
    h = mpmath.mpf(10) ** -25
    worst = 0.0
    scale = float(np.abs(grad).max())
    for c in range(g.n):
        for i in range(3):
            if c == g.anchor_c:
                continue
            node = int(g.nodes[c])
            x[node][i] += h
            up = mp_cost(sc, x, mpmath.mpf(1), mpmath.mpf("0.01"), mpmath.mpf("1.3"))
            x[node][i] -= 2 * h
            down = mp_cost(sc, x, mpmath.mpf(1), mpmath.mpf("0.01"), mpmath.mpf("1.3"))
            x[node][i] += h
            worst = max(worst, abs(float((up - down) / (2 * h)) - float(grad[c, i])))
    print(f"\ntranslation_recovery_reference gradient: largest difference from mpmath {worst:.3e} at |g|_inf {scale:.3e}")
    # a node's gradient is a sum of at most 12 terms of the size of |g|_inf, each a dozen float64 operations: 2^-52 * 12 * 12 * |g|_inf, times the margin
    assert worst <= MARGIN * 144 * 2.0 ** -52 * scale
    # the Hessian-vector product at a zero-residual point: the planted positions of a noise-free scene, anchor moved to 0, the scale row's length kept
    sc = scenes.get("planted_noise_free")
    base = scenes.expected("planted_noise_free")
    g = base["graph"]
    a0, b0 = int(sc["pair_images"][0][1]), int(sc["pair_images"][0][0])
    s = 1.0 / np.linalg.norm(sc["truth"][b0] - sc["truth"][a0])
    xt = ((sc["truth"] - sc["truth"][a0]) * s)[g.nodes]
    with np.errstate(all="ignore"):
        _, _, _, entries = g.model(xt, 1.0, 0.01, 1.3)
    rng = np.random.default_rng(0)
    v, w = rng.normal(size=xt.shape), rng.normal(size=xt.shape)
    v[g.anchor_c] = w[g.anchor_c] = 0.0
    got = float((w * g.hessian(entries, v)).sum())
    h = mpmath.mpf(10) ** -15

    def at(sv, sw):
        pts = [[mpmath.mpf(float(xt[c, i])) + h * (sv * mpmath.mpf(float(v[c, i])) + sw * mpmath.mpf(float(w[c, i]))) for i in range(3)] for c in range(g.n)]
        return mp_cost(sc, pts, mpmath.mpf(1), mpmath.mpf("0.01"), mpmath.mpf("1.3"))

    want = float((at(1, 1) - at(1, -1) - at(-1, 1) + at(-1, -1)) / (4 * h * h))
    print(f"translation_recovery_reference Hessian-vector: w.Hv {got:.12e}, mpmath second difference {want:.12e}")
    # the residuals at the planted point are the rounding of the unit vectors (1e-16): the Gauss-Newton matrix is the Hessian to that relative size, the
    # difference quotient to h^2 = 1e-30; what is left is float64 rounding of a sum of 410 rows
    assert abs(got - want) <= MARGIN * 410 * 2.0 ** -52 * max(abs(want), 1.0) * 16


@pytest.mark.parametrize("name", ARBITER_SCENES)
def test_cost_against_the_arbiter(name):
    sc = scenes.get(name)
    opts = scenes.options_of(sc)
    tight = dict(rel_tol=0.0, abs_tol=0.0, gradient_tol=0.0, max_outer=60)
    res = scenes.solve(sc, **tight)
    rev = scenes.solve(sc, reverse=True, **tight)
    ld = scenes.solve(sc, dtype=np.longdouble, **tight)
    f = float(res["costs"]["final_cost"])
    rows = res["counters"]["valid_rows"]
    sens = max(abs(f - float(rev["costs"]["final_cost"])), abs(f - float(ld["costs"]["final_cost"]))) / max(f, 1.0)
    floor = rows * 2.0 ** -53
    arb = arbiter.refine(sc, res, opts["scale_factor"], opts["sigma"], opts["huber_k"])
    gap = (f - float(arb["cost"])) / max(f, 1.0)
    default = float(scenes.expected(name)["costs"]["final_cost"])
    left = (default - float(arb["cost"])) / max(float(arb["cost"]), 1.0)
    print(f"\ntranslation_recovery_reference {name}: cost {f:.12e} at tolerances 0, arbiter {float(arb['cost']):.12e} after {arb['steps']} steps (|g|_inf {arb['gradient']:.2e}), "
          f"gap {gap:.3e}; sensitivity {sens:.3e} (floor {floor:.3e}); the 1e-5 stopping rule leaves {left:.3e}")
    assert abs(gap) <= MARGIN * max(sens, floor)


def test_wrong_rows_with_huber_leave_the_cameras_in_place():
    clean, wrong = scenes.get("planted_noise"), scenes.get("planted_wrong_huber")
    n = clean["num_images"]
    a, b = scenes.expected("planted_noise"), scenes.expected("planted_wrong_huber")
    fit, _ = ref.fit_scale_shift(b["translation"][:n], a["translation"][:n])
    extent = float((a["translation"][:n].max(0) - a["translation"][:n].min(0)).max())
    shift = float(np.linalg.norm(fit - a["translation"][:n], axis=1).max() / extent)
    off = scenes.expected("planted_wrong_no_huber")
    fit_off, _ = ref.fit_scale_shift(off["translation"][:n], a["translation"][:n])
    shift_off = float(np.linalg.norm(fit_off - a["translation"][:n], axis=1).max() / extent)
    print(f"\ntranslation_recovery_reference wrong rows {wrong['wrong_rows'].tolist()}: cameras move by {shift:.3e} of the extent with Huber on, {shift_off:.3e} with Huber off")
    assert b["counters"]["status"] == ref.CONVERGED and shift <= MARGIN * MEASURED_WRONG_ROW_SHIFT
