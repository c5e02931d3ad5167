"""CPU: rotation averaging as the missing link of the planted chain (tests/multi_view_scene.py), on the restatements: the view graph's edges
with the two-view rotations and weights -> tests/rotation_averaging_reference.py -> 1DSfM, tracks and triangulation with the AVERAGED rotations
in place of the planted ones. This is the host twin of tests/test_multi_view_chain_rotation_gpu.py: what holds here is what that test asserts
on the device."""

import numpy as np
import pytest

from tests import multi_view_rotation_stage as RS
from tests import multi_view_scene as M
from tests import rotation_averaging_reference as ra_ref
from tests import triangulation_reference as tri


@pytest.fixture(scope="module")
def stage():
    r = M.restated_chain()
    rows = r["scene"]["rows"]
    rr = RS.rotation_rows(rows, r["enable"], [r["two_view"][e]["stats0"] for e in rows], r["view_graph"]["edges"])
    res = RS.rotation_stage(rows, r["rotation"], rr["weight"], rr["enable"])
    return r, rows, rr, res


def test_the_stage_solves_the_view_graph_to_the_certified_global_minimum(stage):
    r, rows, rr, res = stage
    assert [e for e, k in zip(rows, rr["enable"]) if k] == r["view_graph"]["edges"] and M.WRONG_ROTATION not in r["view_graph"]["edges"]
    c = res["counters"]
    assert c["status"] == ra_ref.CONVERGED and c["component_size"] == M.NUM_IMAGES and c["valid_rows"] == len(r["view_graph"]["edges"]) and res["node_valid"].all()
    assert c["anchor"] == r["view_graph"]["edges"][0][1]
    lam = ra_ref.dense_certificate(res)
    print(f"counters {c}, costs {res['costs']}, lambda_min(S) {lam:.3e}")
    assert lam > -1e-6 * max(rr["weight"].max(), 1.0)  # rounding of the dense check at these weights


def test_every_averaged_rotation_is_within_the_worst_input_edge_error(stage):
    r, rows, rr, res = stage
    sc = r["scene"]
    aligned = RS.aligned_to_planted(sc, list(res["wRi"]), res["counters"]["anchor"])
    err, worst = RS.absolute_errors_deg(sc, aligned), RS.worst_input_error_deg(sc, rows, r["rotation"], rr["enable"])
    print(f"absolute rotation errors {np.round(err, 4).tolist()} deg, worst input edge {worst:.4f} deg")
    assert err.max() <= worst


def test_the_stages_after_it_do_not_change_with_the_averaged_rotations(stage):
    r, rows, rr, res = stage
    aligned = RS.aligned_to_planted(r["scene"], list(res["wRi"]), res["counters"]["anchor"])
    down = RS.downstream(r, aligned, rows, r["direction"], r["enable"], r["corr"], r["view_graph"]["edges"])
    planted_success = int((np.asarray(r["triangulation"]["exit_code"]) == tri.SUCCESS).sum())
    print(f"inlier edges {len(down['edges'])} (planted rotations {len(r['translation']['edges'])}), tracks {down['tracks']}, triangulated {down['success']} (planted {planted_success})")
    assert down["edges"] == r["translation"]["edges"]
    assert down["tracks"] == len(r["tracks"]["track_off"]) - 1 and down["success"] == planted_success
