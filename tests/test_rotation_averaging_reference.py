"""CPU: the rotation-averaging restatement (tests/rotation_averaging_reference.py) against what does not depend on it: the reference's known
answers, the dense optimality check S = L - blockdiag(Lambda) per scene, a monotone cost over the accepted steps, the gradient and the exact
Hessian against mpmath differences of f along the Cayley retraction, and the arbiters (60-digit mpmath up to 65 nodes, np.longdouble beyond)."""

import pickle

import numpy as np
import pytest

from tests import rotation_averaging_arbiter as arbiter
from tests import rotation_averaging_reference as ref
from tests import rotation_averaging_scenes as scenes

SOLVED = [n for n in scenes.SCENE_NAMES if n not in ("empty", "non_finite")]


@pytest.mark.parametrize("name", scenes.SCENE_NAMES)
def test_scene_contains_what_it_is_named_for(name):
    sc, res = scenes.get(name), scenes.expected(name)
    assert sc["check"](res), (res["counters"], res["costs"])
    assert res["counters"]["hessian_applications"] == sum(e["inner"] for e in res["log"])
    assert res["counters"]["accepted_steps"] == sum(e["accepted"] for e in res["log"]) and res["counters"]["outer_iterations"] == len(res["log"])


@pytest.mark.parametrize("name", [n for n in scenes.SCENE_NAMES if scenes.get(n)["known_tol_deg"] is not None])
def test_known_answers(name):
    """The reference's expected rotations, compared as it compares them: up to one common rotation (here: relative to the anchor)."""
    sc, res = scenes.get(name), scenes.expected(name)
    a = res["counters"]["anchor"]
    for k in np.flatnonzero(res["node_valid"]):
        assert ref.angle_deg(res["wRi"][k], sc["truth"][a].T @ sc["truth"][k]) <= sc["known_tol_deg"], k
    assert np.array_equal(res["wRi"][a], np.eye(3).reshape(9))


@pytest.mark.parametrize("name", SOLVED)
def test_dense_check_verdict(name):
    """Every scene but two reaches the certified global minimum; ``not_global`` provably does not; ``max_iterations`` is not at a critical point."""
    res = scenes.expected(name)
    g = res["graph"]
    lam = ref.dense_certificate(res)
    degree = max(len(np.flatnonzero(g.node == k)) for k in range(g.n)) if len(g.node) else 1
    rounding = 1e-12 * max(float(g.kappa.max()) if len(g.kappa) else 1.0, 1.0) * degree  # eigvalsh's error: a few thousand eps |S|, |S| <= 2 max kappa . degree
    print(f"{name}: lambda_min(S) = {lam:.3e} (rounding allowance {rounding:.1e}), cost {res['costs']['final_cost']:.6g}")
    if name == "not_global":
        assert lam < 100 * ref.GTSAM_OPTIMALITY_THRESHOLD
    elif name != "max_iterations":
        assert lam >= -rounding


@pytest.mark.parametrize("name", SOLVED)
def test_cost_is_monotone_over_accepted_steps(name):
    res = scenes.expected(name)
    for e in res["log"]:
        if e["accepted"]:
            assert e["trial_cost"] <= e["cost"] + ref.RHO_REG * max(1.0, abs(e["cost"])), e
    assert res["counters"]["status"] != ref.CONVERGED or res["costs"]["final_cost"] <= res["costs"]["chordal_cost"]


def mp_cayley_cost(sc, res, r64, xi, t):
    """f(R_k cayley(t xi_k)) in mpmath, from the scene's rows (arbiter.mp_cost) and Cayley's map in its other form, (I - hat h)^-1 (I + hat h)
    with h = t xi / 2: nothing of the restatement is used."""
    from mpmath import mp, mpf

    r = []
    for k in range(len(r64)):
        h = [t * mpf(float(x)) / 2 for x in xi[k]]
        hh = mp.matrix([[0, -h[2], h[1]], [h[2], 0, -h[0]], [-h[1], h[0], 0]])
        q = (mp.eye(3) - hh) ** -1 * (mp.eye(3) + hh)
        m = mp.matrix([[mpf(float(x)) for x in row] for row in r64[k]]) * q
        r.append([[m[a, b] for b in range(3)] for a in range(3)])
    return arbiter.mp_cost(arbiter.mp_edges(sc, res), r)


@pytest.mark.parametrize("name", ["gaps", "duplicate_pairs", "weights_span", "masked_rows", "two_components", "ring65"])
def test_gradient_and_hessian_against_mpmath_differences_along_the_retraction(name):
    """f(R cayley(t xi)) = f + t <g, xi> + t^2 / 2 <xi, H xi> + O(t^3) at a point that is not critical (Lambda matters there): the restatement's
    float64 gradient and Hessian against central differences of f evaluated in 60-digit mpmath, t = 1e-12. The differences are exact to
    O(t^2) = 1e-24 relative (rounding 1e-60 / t^2 = 1e-36), so what is measured is the float64 evaluation of <g, xi> and <xi, H xi>: sums of
    terms of size kappa |xi_i| |xi_j|, a few hundred float64 operations deep with the 3 x 3 products, hence 1024 eps times the sum of those
    sizes over the rows (`scale`), not times the result, which may be smaller by cancellation."""
    from mpmath import mp, mpf

    sc, res = scenes.get(name), scenes.expected(name)
    g = res["graph"]
    rng = np.random.default_rng(3)
    r = np.stack([scenes.rodrigues(0.3 * rng.standard_normal(3)) for _ in range(g.n)])
    w, _ = g.pass_w(r)
    aa = ref.mTm(r, w)
    lam, grad = 0.5 * (aa + np.swapaxes(aa, 1, 2)), ref.vee4(aa)
    xi = rng.standard_normal((g.n, 3))
    xi[g.anchor_c] = 0
    h = g.hessian(r, lam, xi)
    norm = np.abs(xi).sum(1)
    scale = float(sum(k * (norm[a] + norm[b]) ** 2 for a, b, k, o in zip(g.node, g.nbr, g.kappa, g.orient) if o == 1))
    with mp.workdps(arbiter.MP_DIGITS):
        t = mpf(10) ** -12
        f0, fp, fm = (mp_cayley_cost(sc, res, r, xi, x) for x in (mpf(0), t, -t))
        first, second = (fp - fm) / (2 * t), (fp - 2 * f0 + fm) / (t * t)
        g_xi, xi_h_xi = float((grad * xi).sum()), float((xi * h).sum())
        d1, d2 = float(abs(first - mpf(g_xi))), float(abs(second - mpf(xi_h_xi)))
    bound = 1024 * 2.0 ** -52 * scale
    print(f"{name}: <g, xi> {g_xi:.15e} off by {d1:.2e}; <xi, H xi> {xi_h_xi:.15e} off by {d2:.2e}; allowed {bound:.2e} (relative {bound / abs(xi_h_xi):.1e})")
    assert d1 <= bound and d2 <= bound


@pytest.mark.parametrize("name", [n for n in SOLVED if n not in ("max_iterations",)])
def test_arbiter_agreement(name):
    """Up to 65 nodes the 60-digit mpmath Newton iteration, which shares no code with the restatement, ends at |g|_inf <= 1e-40 within a few
    steps of the restatement's answer; beyond, the extended-precision continuation converges seven orders deeper. Either way the restatement
    stands where the gradient tolerance lets it: far below a thousandth of a degree."""
    s = arbiter.sensitivity(name)
    res, sc = scenes.expected(name), scenes.get(name)
    print(f"{name}: {s['arbiter']} arbiter: restatement off by {s['arbiter_deg']:.3e} deg, cost {s['arbiter_cost_rel']:.3e} rel; forward-reversed {s['order_deg']:.3e} deg; arbiter |g| {s['arbiter_gradient']:.2e}")
    assert s["arbiter"] == ("mpmath" if sc["num_images"] <= arbiter.MP_MAX_NODES else "longdouble")
    assert s["arbiter_status"] == ref.CONVERGED
    if s["arbiter"] == "mpmath":
        assert s["arbiter_gradient"] <= arbiter.MP_GRADIENT_TOL and s["arbiter_steps"] <= 8
    else:
        assert s["arbiter_gradient"] <= 1e-6 * ref.DEFAULTS["gradient_tol"] * float(res["graph"].kappa.max())
    assert s["arbiter_deg"] < 1e-3 and s["arbiter_cost_rel"] < 1e-9


@pytest.mark.parametrize("name", ["ring64", "gaps", "duplicate_pairs", "weights_span", "unweighted"])
def test_the_two_arbiters_agree_where_both_run(name):
    """The extended-precision continuation, which the larger scenes rely on, against the independent mpmath arbiter on scenes small enough for
    both: they name the same critical point, to far below the distance either measures."""
    sc, res = scenes.get(name), scenes.expected(name)
    exact, ld = arbiter.mp_arbiter(sc, res), arbiter.arbiter(sc, res)
    deg = arbiter.max_angle_deg(res["wRi"], ld["wRi"])
    print(f"{name}: restatement off by {exact['deg']:.6e} deg (mpmath), {deg:.6e} deg (longdouble)")
    assert exact["converged"] and abs(exact["deg"] - deg) <= 1e-3 * exact["deg"] + 1e-14


def test_max_iterations_scene_has_no_arbiter():
    s = arbiter.sensitivity("max_iterations")
    assert s["arbiter"] is None and s["rotation_deg"] == 0.0 and s["cost_rel"] == 0.0  # the device is held to the restatement's bytes there


def test_refusals_and_options():
    eye = np.eye(3).reshape(1, 9)
    for pairs in ([(0, 0)], [(0, 3)], [(-1, 1)]):
        with pytest.raises(ValueError):
            ref.solve(pairs, eye, [1.0], num_images=3)
    with pytest.raises(ValueError):
        ref.solve([(0, 1)], eye, [1.0], num_images=3, theta=0.75)
    with pytest.raises(ValueError):
        ref.solve([(0, 1)], eye, [1.0], num_images=3, anchor=3)
    assert ref.solve([(0, 0)], eye, [1.0], [0], num_images=3)["counters"]["status"] == ref.NO_VALID_ROW  # a disabled row is not looked at


def test_drop_in_host_logic():
    """The reference's host logic without a GPU: the rows it builds, quirks included; pickling; the random start is refused."""
    from gtsfm_amd.averaging.rotation import RotationAveragingBase, ShonanRotationAveraging

    obj = ShonanRotationAveraging()
    assert isinstance(obj, RotationAveragingBase) and pickle.loads(pickle.dumps(obj))._weight_by_inliers is True
    with pytest.raises(NotImplementedError):
        ShonanRotationAveraging(use_chordal_init=False)
    assert obj.run_rotation_averaging(4, {}, {}, {}) == [None] * 4
    m = scenes.ry(30)

    class Prior:
        value = scenes.rx(30)
        covariance = np.eye(6) * 1e-5

    i2Ri1 = {(0, 1): m, (1, 2): None, (2, 3): m, (0, 3): m}
    corr = {(0, 1): np.zeros((0, 2)), (1, 2): np.zeros((9, 2)), (2, 3): np.zeros((5, 2)), (0, 3): np.zeros((0, 2))}
    pairs, rotation, weight = obj.measurement_rows(i2Ri1, {(0, 2): Prior()}, corr)
    assert pairs.tolist() == [[0, 1], [2, 3], [0, 3], [2, 0]]
    # zero correspondences first: the default sigma 1; then 1 / 5; zero again: the entry before it is carried over; the prior: sqrt(1e-5)
    np.testing.assert_allclose(weight, [1.0, 25.0, 25.0, 1e5], rtol=1e-12)
    assert rotation[3].tobytes() == scenes.rx(30).reshape(9).tobytes()
    # the one retry: a status other than CONVERGED with weights on -> once more unweighted, and the object stays unweighted
    calls = []
    retried = ShonanRotationAveraging()
    assert retried.solve_with_retry(lambda weighted: (calls.append(weighted), ("MAX_ITERATIONS" if weighted else "CONVERGED", len(calls)))[1]) == 2
    assert calls == [True, False] and retried._weight_by_inliers is False and retried._device is None
    assert retried.solve_with_retry(lambda weighted: (calls.append(weighted), ("NON_FINITE", 7))[1]) == 7 and calls == [True, False, False]
    assert ShonanRotationAveraging(two_view_rotation_sigma=0.5, weight_by_inliers=False).measurement_rows(i2Ri1, {}, corr)[2].tolist() == [4.0, 4.0, 4.0]


def test_rotation_config_instantiates():
    import yaml

    from gtsfm_amd.averaging.rotation import ShonanRotationAveraging
    from tests.conftest import REPO
    from tests.test_config_hook import instantiate

    node = yaml.safe_load((REPO / "gtsfm_amd" / "configs" / "deep_front_end_amd_rotation.yaml").read_text())
    translation = yaml.safe_load((REPO / "gtsfm_amd" / "configs" / "deep_front_end_amd_translation.yaml").read_text())
    assert {k: v for k, v in node.items() if k != "rot_avg_module"} == translation
    obj = instantiate(node["rot_avg_module"])
    assert isinstance(obj, ShonanRotationAveraging) and obj._weight_by_inliers is True and obj._two_view_rotation_sigma == 1.0 and obj._use_chordal_init is True
