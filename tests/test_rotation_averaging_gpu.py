"""GPU: ``gtsfm_rotation_averaging_f64`` on every scene of tests/rotation_averaging_scenes.py against the restatement
(tests/rotation_averaging_reference.py). Status, mask, anchor, component size and valid rows are equal; on DECISIVE scenes (no accept /
radius / stopping decision of the restatement was close) the outer-iteration and accepted-step counts too. Rotations are compared in degrees
per node and the final cost relative to max(cost, 1); both sit within 8 x the restatement's own measured sensitivity
(tests/rotation_averaging_arbiter.py: the larger of its distance from the extended-precision arbiter and its difference between forward and
reversed row order; 8 is the project's standing margin for float64 stages; a scene stopped by its iteration cap has no arbiter and is
held to the row order alone). On top of that bound the device's rotations and costs are ASSERTED to be the restatement's bytes on every scene: the
stage is float64 + - * / sqrt in one stated order, and that is the contract the documents state. Equal bytes run to run, alone against batched (P = 3, the problem in the middle) and under a row permutation with the anchor
given; inputs untouched; invalid input refused with nothing written. ``-s`` prints the lines of profiles/rotation_averaging_gpu_tests.txt."""

import numpy as np
import pytest

from tests import rotation_averaging_arbiter as arbiter
from tests import rotation_averaging_reference as ref
from tests import rotation_averaging_scenes as scenes

pytestmark = pytest.mark.gpu

MARGIN = 8.0


@pytest.fixture(scope="module")
def engine(gpu_device):
    from gtsfm_amd.runtime.rotation_averaging_engine import RotationAveragingEngine

    return RotationAveragingEngine(gpu_device)


def run_device(engine, sc, **override):
    opts = dict(sc["options"], **override)
    anchor = opts.pop("anchor", sc["anchor"])
    dev = engine.upload(sc["pair_images"], sc["rotation"], sc["weight"], sc["pair_enable"])
    keep = [None if t is None else t.clone() for t in dev]
    out = engine.average(*dev[:4], num_images=sc["num_images"], anchor=anchor, **opts)
    for before, after in zip(keep, dev):
        assert before is None or bytes(before.cpu().numpy().tobytes()) == bytes(after.cpu().numpy().tobytes()), "an input was changed"
    return {"wRi": out["wRi"].cpu().numpy()[0], "node_valid": out["node_valid"].cpu().numpy()[0], "counters": out["counters"][0], "costs": out["costs"][0]}


def same_bytes(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("wRi", "node_valid", "counters", "costs"))


@pytest.mark.parametrize("name", scenes.SCENE_NAMES)
def test_device_against_the_restatement(engine, name):
    sc, want, sens = scenes.get(name), scenes.expected(name), arbiter.sensitivity(name)
    assert sc["check"](want), "the scene does not contain what it is named for"
    got = run_device(engine, sc)
    assert same_bytes(got, run_device(engine, sc)), "two runs differ"
    c = dict(zip(ref.COUNTER_FIELDS, (int(x) for x in got["counters"])))
    wc = want["counters"]
    rot = arbiter.max_angle_deg(got["wRi"], want["wRi"])
    f, wf = float(got["costs"][2]), want["costs"]["final_cost"]
    cost = abs(f - wf) / max(abs(wf), 1.0) if np.isfinite(wf) else 0.0
    equal = got["wRi"].tobytes() == want["wRi"].tobytes() and got["costs"].tobytes() == np.array([want["costs"][k] for k in ref.COST_FIELDS]).tobytes()
    print(f"\nrotation_averaging {name}: status {ref.STATUS_NAMES[c['status']]} n {c['component_size']} outer {c['outer_iterations']} (restatement {wc['outer_iterations']}) "
          f"accepted {c['accepted_steps']} ({wc['accepted_steps']}) hessian {c['hessian_applications']} ({wc['hessian_applications']}) decisive {want['decisive']} | "
          f"device-restatement {rot:.3e} deg, cost {cost:.3e} rel, bytes equal {equal} | sensitivity {sens['rotation_deg']:.3e} deg (arbiter {sens['arbiter_deg']:.3e}, "
          f"order {sens['order_deg']:.3e}), cost {sens['cost_rel']:.3e}")
    for k in ("status", "anchor", "component_size", "valid_rows"):
        assert c[k] == wc[k], k
    assert np.array_equal(got["node_valid"], want["node_valid"])
    assert np.array_equal(np.isnan(got["wRi"]), np.isnan(want["wRi"]))
    if want["decisive"]:
        assert (c["outer_iterations"], c["accepted_steps"]) == (wc["outer_iterations"], wc["accepted_steps"])
    if wc["status"] in (ref.CONVERGED, ref.MAX_ITERATIONS):
        assert np.array_equal(got["wRi"][wc["anchor"]], np.eye(3).reshape(9)), "the gauge"
        assert rot <= MARGIN * sens["rotation_deg"], (rot, sens)
        assert cost <= MARGIN * sens["cost_rel"], (cost, sens)
        assert equal, "the device's bytes are not the restatement's"
        assert [c[k] for k in ref.COUNTER_FIELDS] == [wc[k] for k in ref.COUNTER_FIELDS]
        if sc["known_tol_deg"] is not None:  # the reference's known answers, gauge removed
            a = wc["anchor"]
            truth = np.stack([sc["truth"][a].T @ r for r in sc["truth"]]).reshape(-1, 9)
            truth[got["node_valid"] == 0] = np.nan
            assert arbiter.max_angle_deg(got["wRi"], truth) <= sc["known_tol_deg"]
    else:
        assert np.isnan(got["wRi"]).all() and not got["node_valid"].any()


def test_batch_equals_alone(engine):
    """P = 3 over row ranges of the same arrays: every problem, the middle one too, gives the bytes it gives alone."""
    parts = [scenes.get(n) for n in ("ring65", "gaps", "duplicate_pairs")]
    n = max(x["num_images"] for x in parts)
    row_off = np.concatenate([[0], np.cumsum([len(x["pair_images"]) for x in parts])])
    dev = engine.upload(np.concatenate([x["pair_images"] for x in parts]), np.concatenate([x["rotation"] for x in parts]), np.concatenate([x["weight"] for x in parts]), None, row_off)
    out = engine.average(*dev[:4], num_images=n, problem_row_off=dev[4])
    wri, valid = out["wRi"].cpu().numpy(), out["node_valid"].cpu().numpy()
    for p, sc in enumerate(parts):
        alone = run_device(engine, dict(sc, num_images=n))
        assert same_bytes(alone, {"wRi": wri[p], "node_valid": valid[p], "counters": out["counters"][p], "costs": out["costs"][p]}), f"problem {p}"


@pytest.mark.parametrize("name", ["ring65", "gaps", "window120x6_outliers", "two_components"])
def test_row_permutation(engine, name):
    """No pair is listed twice: with the anchor given, the order of the rows changes no byte."""
    sc = scenes.get(name)
    anchor = scenes.expected(name)["counters"]["anchor"]
    perm = np.random.default_rng(5).permutation(len(sc["pair_images"]))
    moved = dict(sc, pair_images=sc["pair_images"][perm], rotation=sc["rotation"][perm], weight=sc["weight"][perm],
                 pair_enable=None if sc["pair_enable"] is None else sc["pair_enable"][perm])
    a, b = run_device(engine, sc, anchor=anchor), run_device(engine, moved, anchor=anchor)
    assert same_bytes(a, b)


@pytest.mark.parametrize("case", ["self_pair", "out_of_range", "negative", "offsets", "theta", "anchor"])
def test_invalid_input_is_refused_with_nothing_written(engine, case):
    import torch

    from gtsfm_amd.runtime import lib as L

    pairs = {"self_pair": [(0, 1), (2, 2)], "out_of_range": [(0, 1), (1, 5)], "negative": [(-1, 1), (1, 2)]}.get(case, [(0, 1), (1, 2)])
    row_off = [0, 3] if case == "offsets" else [0, 2]
    dev = engine.upload(np.asarray(pairs), np.tile(np.eye(3).reshape(9), (2, 1)), np.ones(2), None, row_off)
    lib = L.load()
    ws = torch.zeros(int(lib.gtsfm_rotation_averaging_workspace_bytes(2, 3, 1)) + 256, dtype=torch.uint8, device=engine.device)
    wri = torch.full((3, 9), 7.0, dtype=torch.float64, device=engine.device)
    valid = torch.full((3,), 7, dtype=torch.uint8, device=engine.device)
    counters = torch.full((8,), 7, dtype=torch.int32, device=engine.device)
    costs = torch.full((4,), 7.0, dtype=torch.float64, device=engine.device)
    o = ref.DEFAULTS
    rc = lib.gtsfm_rotation_averaging_f64(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), None, 2, 3, dev[4].data_ptr(), 1, 5 if case == "anchor" else -1, o["chordal_tol"],
                                          o["chordal_max_iterations"], o["delta0"], o["kappa_cg"], 0.75 if case == "theta" else o["theta"], o["gradient_tol"], o["max_outer"],
                                          o["max_inner"], ws.data_ptr(), ws.numel(), wri.data_ptr(), valid.data_ptr(), counters.data_ptr(), costs.data_ptr(),
                                          torch.cuda.current_stream(engine.device).cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and lib.gtsfm_last_error()
    assert (wri == 7.0).all() and (valid == 7).all() and (counters == 7).all() and (costs == 7.0).all(), "an output was written"


def test_drop_in_known_answers(gpu_device):
    """ShonanRotationAveraging.run_rotation_averaging on the reference's known answers (tests/averaging/rotation/test_shonan.py), to its 2 degrees
    (0.1 for the graph with an orphan), compared as the reference compares: relative to a common image."""
    from gtsfm_amd.averaging.rotation import ShonanRotationAveraging

    for name in ("simple", "nonconsecutive", "circle_two_edges", "circle_all_edges", "line_large_edges", "panorama"):
        sc = scenes.get(name)
        i2Ri1 = {(int(a), int(b)): m.reshape(3, 3) for (a, b), m in zip(sc["pair_images"], sc["rotation"])}
        corr = {k: np.zeros((k[0] + k[1], 2), np.int64) for k in i2Ri1}
        obj = ShonanRotationAveraging()
        wRi = obj.run_rotation_averaging(sc["num_images"], i2Ri1, {}, corr)
        assert len(wRi) == sc["num_images"]
        on = [k for k, r in enumerate(wRi) if r is not None]
        assert on == np.flatnonzero(scenes.expected(name)["node_valid"]).tolist()
        for k in on:
            assert ref.angle_deg(wRi[on[0]].T @ wRi[k], sc["truth"][on[0]].T @ sc["truth"][k]) <= sc["known_tol_deg"]
    # the prior becomes a row (i2, i1, i1Ri2) with sigma = sqrt(mean diagonal covariance)
    sc = scenes.get("simple_with_prior")

    class Prior:
        value = sc["rotation"][1].reshape(3, 3)  # i1Ri2 of the prior (0, 2): the row (2, 0)'s rotation
        covariance = np.eye(6) * 1e-5

    wRi = ShonanRotationAveraging().run_rotation_averaging(3, {(1, 0): sc["rotation"][0].reshape(3, 3)}, {(0, 2): Prior()}, {(1, 0): np.zeros((1, 2), np.int64)})
    for k in range(3):
        assert ref.angle_deg(wRi[0].T @ wRi[k], sc["truth"][k]) <= 2.0
    assert ShonanRotationAveraging().run_rotation_averaging(3, {}, {}, {}) == [None] * 3
