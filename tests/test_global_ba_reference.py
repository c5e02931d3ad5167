"""CPU: the restatement of the global bundle adjustment (tests/global_ba_reference.py) held to what it must be.

* The residual and both Jacobian blocks against 60-digit ``mpmath`` central differences along the retraction (h = 1e-20: the differences'
  own error is ~1e-40). The float64 blocks are a dozen operations on numbers of the block's size, with one cancelling difference per
  rotation column: the bound is 1e-12 of the block's largest entry, a few hundred roundings.
* The cost does not rise over the accepted steps of any scene; the scenes' own checks hold (the planted answers among them).
* The final cost against the dense longdouble arbiter (tests/global_ba_arbiter.py, no shared code) on the small scenes, with the
  restatement's tolerances at 0 and cg_forcing = 0: the relative difference was measured per scene (profiles/global_ba_reference.txt) and
  is asserted at MARGIN = 8 x the largest measured value, the project's customary margin over its own sensitivity. What the 1e-5 stopping
  rule and cg_forcing's default leave above that minimum is measured and printed, and asserted only not to lie below it by more than the
  same bound.
``-s`` prints the lines of profiles/global_ba_reference.txt."""

import numpy as np
import pytest

from tests import global_ba_arbiter as arbiter
from tests import global_ba_reference as ref
from tests import global_ba_scenes as scenes

MARGIN = 8
MEASURED_ARBITER_RELATIVE = 1.8e-12  # the largest |restatement - arbiter| / arbiter over scenes.SMALL (long_track; the others 3e-15 .. 2.2e-13)
MEASURED_NOISE_FREE_ABSOLUTE = 6.1e-18  # planted_noise_free ends at a cost of 8.9e-9 px^2, the float32 rounding of its pixels: a sum of squares of residuals of 1e-5 px,
# each known to ~1e-13 px in float64; there the difference is measured absolutely


def test_residual_and_jacobians_against_mpmath():
    import mpmath as mp  # a missing library is a failure here, not a skip: nothing else holds the derivatives to an outside standard

    mp.mp.dps = 60
    sc = scenes.get("anisotropic")
    valid, _ = ref.validity(sc["cameras"], sc["track_off"], sc["image"], sc["uv"], sc["point"], None, None, 2)
    g = ref.Graph(sc["cameras"], sc["track_off"], sc["image"], sc["uv"], valid, -1)
    x = np.zeros((g.n, 12))
    x[:g.nc], x[g.nc:, :3] = sc["cameras"][g.nodes[:g.nc], 5:17], sc["point"][g.nodes[g.nc:] - len(sc["cameras"])]
    sigma = 0.7
    r, _, _, jc, jp = ref.entries_at(g, x, np.float64(sigma), 1.345)

    def residual(e, d_pose, d_point):
        i, j = int(g.ci[e]), int(g.pj[e])
        rot = mp.matrix(3, 3)
        for a in range(3):
            for b in range(3):
                rot[a, b] = mp.mpf(float(x[i, 3 * a + b]))
        t = mp.matrix([mp.mpf(float(v)) for v in x[i, 9:12]])
        p = mp.matrix([mp.mpf(float(v)) for v in x[j, :3]]) + mp.matrix(d_point)
        h = mp.matrix(d_pose[:3]) / 2
        k = mp.matrix([[0, -h[2], h[1]], [h[2], 0, -h[0]], [-h[1], h[0], 0]])
        cay = mp.eye(3) + (2 / (1 + h[0] ** 2 + h[1] ** 2 + h[2] ** 2)) * (k + k * k)
        t = t + rot * mp.matrix(d_pose[3:])
        rot = rot * cay
        q = rot.T * (p - t)
        return [(mp.mpf(float(g.fx[e])) * q[0] / q[2] + mp.mpf(float(g.cx[e])) - mp.mpf(float(g.u[e]))) / mp.mpf(sigma),
                (mp.mpf(float(g.fy[e])) * q[1] / q[2] + mp.mpf(float(g.cy[e])) - mp.mpf(float(g.v[e]))) / mp.mpf(sigma)]

    h = mp.mpf(10) ** -20
    worst = 0.0
    for e in list(g.cam_entries[:6]) + list(g.pt_entries[-6:]):
        zero6, zero3 = [mp.mpf(0)] * 6, [mp.mpf(0)] * 3
        r0 = residual(e, zero6, zero3)
        scale = max(float(np.abs(jc[e]).max()), float(np.abs(jp[e]).max()))
        assert max(abs(float(r0[a] - mp.mpf(float(r[e, a])))) for a in range(2)) <= 1e-12 * max(1.0, float(np.abs(r[e]).max()))
        for k in range(9):
            dp, dq = list(zero6), list(zero3)
            if k < 6:
                dp[k] = h
            else:
                dq[k - 6] = h
            up = residual(e, dp, dq)
            down = residual(e, [-v for v in dp], [-v for v in dq])
            for a in range(2):
                want = (up[a] - down[a]) / (2 * h)
                got = jc[e, a, k] if k < 6 else jp[e, a, k - 6]
                worst = max(worst, abs(float(want - mp.mpf(float(got)))) / scale)
    print(f"\nglobal_ba_reference Jacobians: largest difference from mpmath {worst:.3e} of the block's largest entry")
    assert worst <= 1e-12


@pytest.mark.parametrize("name", scenes.SCENE_NAMES)
def test_scene_holds_and_cost_is_monotone(name):
    sc, res = scenes.get(name), scenes.expected(name)
    assert sc["check"](res), "the scene does not contain what it is named for"
    costs = [e["cost"] for e in res["log"] if e["accepted"]] + [res["costs"]["final_cost"]]
    assert all(b <= a for a, b in zip(costs, costs[1:])), "the cost rose over an accepted step"
    assert all(e["trial_cost"] < e["cost"] for e in res["log"] if e["accepted"])
    if res["log"]:
        assert res["costs"]["final_cost"] <= res["costs"]["init_cost"]
    assert res["counters"]["solves_tried"] == len(res["log"]) and res["counters"]["accepted_steps"] == sum(e["accepted"] for e in res["log"])


@pytest.mark.parametrize("name", scenes.SMALL)
def test_final_cost_against_the_arbiter(name):
    sc = scenes.get(name)
    opts = scenes.options_of(sc)
    tight = scenes.solve(sc, rel_tol=0.0, abs_tol=0.0, cg_forcing=0.0, max_inner=60, max_iterations=60)
    usual = scenes.expected(name)
    arb = arbiter.minimise(sc["cameras"], sc["track_off"], sc["image"], sc["uv"], sc["point"], tight["valid"], tight["node_valid"], tight["counters"]["anchor"],
                           sigma=opts["measurement_sigma"], huber_k=opts["huber_k"])
    f, fa, fu = float(tight["costs"]["final_cost"]), float(arb["cost"]), float(usual["costs"]["final_cost"])
    print(f"\nglobal_ba_reference {name}: cost {f:.12e} at tolerances 0 ({ref.STATUS_NAMES[tight['counters']['status']]}, {tight['counters']['accepted_steps']} steps), arbiter {fa:.12e} "
          f"after {arb['steps']} steps (|g|_inf {float(arb['gradient']):.2e}), relative difference {abs(f - fa) / fa:.3e}; the usual stopping rule ends at {fu:.12e}: "
          f"{(fu - fa) / fa:.3e} above the minimum")
    bound = MARGIN * MEASURED_NOISE_FREE_ABSOLUTE if name == "planted_noise_free" else MARGIN * MEASURED_ARBITER_RELATIVE * fa
    assert abs(f - fa) <= bound
    assert fu >= fa - bound
