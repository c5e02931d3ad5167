"""GPU: the planted scene of tests/multi_view_scene.py through ``two_view`` -> ``view_graph`` -> ``rotation_averaging`` on one scene object, and
then ``translation_inliers`` -> ``tracks`` -> ``triangulate`` with the AVERAGED rotations in place of the planted ones: the chain runs without
being handed a rotation. The stage is held to its restatement (tests/rotation_averaging_reference.py) FED THE DEVICE'S OWN UPSTREAM OUTPUT, by
the rule of tests/test_rotation_averaging_gpu.py (8 x the restatement's measured sensitivity on these very rows). After aligning the anchor,
every averaged rotation lies no further from the planted one than the worst relative-rotation error among the input edges it was given. The
host twin (tests/test_multi_view_chain_rotation_host.py) shows that the inlier edge set and the triangulated-track count equal those with the
planted rotations, so both are asserted here."""

import numpy as np
import pytest

from tests import multi_view_rotation_stage as RS
from tests import multi_view_scene as M
from tests import rotation_averaging_arbiter as arbiter
from tests import rotation_averaging_reference as ra_ref
from tests import rotation_averaging_scenes as ra_scenes
from tests import triangulation_reference as tri

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def restated():
    return M.restated_chain()


@pytest.fixture(scope="module")
def chain(gpu_device, restated):
    from gtsfm_amd.bundle.two_view_ba import TwoViewOptions
    from gtsfm_amd.common.calibration import PinholeCamera, PinholeIntrinsics
    from gtsfm_amd.data_association.point3d_initializer import TriangulationOptions, TriangulationSamplingMode
    from gtsfm_amd.frontend.correspondence_generator import batched_twoway_correspondence_generator as module
    from gtsfm_amd.frontend.verifier.ransac import Ransac
    from tests.test_multi_view_chain_gpu import planted_generator, two_view_rows
    from tests.test_translation_inliers_gpu import ShortAveraging

    sc = restated["scene"]
    cals = [PinholeIntrinsics(k[0], k[2], k[3], fy=k[1]) for k in sc["intrinsics"]]
    with pytest.MonkeyPatch.context() as patch:
        patch.setattr(module, "MAX_VERIFY_PAIRS", M.LAUNCH_PAIRS)
        scene = planted_generator(sc, gpu_device).generate_verified_scene(None, [None] * M.NUM_IMAGES, sc["edges"], cals, Ransac(True, M.VERIFY_THRESHOLD_PX))
    new = scene.two_view(TwoViewOptions(min_num_inliers_est_model=M.MIN_INLIERS, min_inlier_ratio_est_model=M.MIN_RATIO), cals)
    vg = new.view_graph()
    ra = new.rotation_averaging(edges=vg.edges)
    again = new.rotation_averaging(edges=vg.edges)
    anchor = ra.counters["anchor"]
    aligned = RS.aligned_to_planted(sc, ra.wRi_list, anchor)
    averaging = ShortAveraging()
    averaging._outlier_weight_threshold = restated["threshold"]
    ti = new.translation_inliers(aligned, cals, edges=vg.edges, averaging=averaging)
    ti_planted = new.translation_inliers([sc["wRi"][i] for i in range(M.NUM_IMAGES)], cals, edges=vg.edges, averaging=averaging)
    options = TriangulationOptions(mode=TriangulationSamplingMode.NO_RANSAC, reproj_error_threshold=M.TRIANGULATION_THRESHOLD_PX)
    tri_avg = new.triangulate({i: PinholeCamera(aligned[i], sc["centre"][i], cals[i]) for i in range(M.NUM_IMAGES)}, options, edges=ti.edges)
    tri_planted = new.triangulate({i: PinholeCamera(sc["wRi"][i], sc["centre"][i], cals[i]) for i in range(M.NUM_IMAGES)}, options, edges=ti_planted.edges)
    return {"new": new, "vg": vg, "ra": ra, "again": again, "aligned": aligned, "ti": ti, "ti_planted": ti_planted, "tri": tri_avg, "tri_planted": tri_planted,
            "rows": two_view_rows(new)}


def test_rotation_averaging_on_the_view_graph_edges_equals_the_restatement(chain, restated):
    new, vg, ra = chain["new"], chain["vg"], chain["ra"]
    rows, rotation, _, enable, corr = chain["rows"]
    assert ra.pairs == rows
    counts = [len(corr[e]) if k else 0 for e, k in zip(rows, enable)]  # stats[:, 0] after two_view: the count of the valid mask
    rr = RS.rotation_rows(rows, enable, counts, vg.edges)
    np.testing.assert_array_equal(ra.enabled, rr["enable"])
    np.testing.assert_array_equal(ra.weight[rr["enable"] > 0], rr["weight"][rr["enable"] > 0])
    want = RS.rotation_stage(rows, rotation, rr["weight"], rr["enable"])
    sc = ra_scenes.scene("chain", rows, rotation, rr["weight"], M.NUM_IMAGES, enable=rr["enable"])
    sens = arbiter.sensitivity_of(sc, want)
    got = np.stack([np.full(9, np.nan) if r is None else r.reshape(9) for r in ra.wRi_list])
    rot = arbiter.max_angle_deg(got, want["wRi"])
    f, wf = ra.costs["final_cost"], want["costs"]["final_cost"]
    cost = abs(f - wf) / max(abs(wf), 1.0)
    print(f"chain rotation averaging: {ra.status}, counters {ra.counters} (restatement {want['counters']}, decisive {want['decisive']}), device-restatement {rot:.3e} deg, "
          f"cost {cost:.3e} rel; sensitivity {sens['rotation_deg']:.3e} deg, cost {sens['cost_rel']:.3e}")
    assert ra.status == "CONVERGED" == ra_ref.STATUS_NAMES[want["counters"]["status"]]
    for k in ("anchor", "component_size", "valid_rows"):
        assert ra.counters[k] == want["counters"][k], k
    assert [r is not None for r in ra.wRi_list] == want["node_valid"].astype(bool).tolist() == [True] * M.NUM_IMAGES
    if want["decisive"]:
        assert (ra.counters["outer_iterations"], ra.counters["accepted_steps"]) == (want["counters"]["outer_iterations"], want["counters"]["accepted_steps"])
    assert rot <= 8.0 * sens["rotation_deg"] and cost <= 8.0 * sens["cost_rel"]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ra.wRi_list, chain["again"].wRi_list)) and ra.counters == chain["again"].counters


def test_every_averaged_rotation_is_within_the_worst_input_edge_error(chain, restated):
    sc, ra = restated["scene"], chain["ra"]
    rows, rotation, _, _, _ = chain["rows"]
    err, worst = RS.absolute_errors_deg(sc, chain["aligned"]), RS.worst_input_error_deg(sc, rows, rotation, ra.enabled)
    print(f"absolute rotation errors {np.round(err, 4).tolist()} deg, worst input edge {worst:.4f} deg")
    assert np.isfinite(err).all() and err.max() <= worst


def test_the_chain_runs_on_the_averaged_rotations(chain, restated):
    ti, ti_planted, out, out_planted = chain["ti"], chain["ti_planted"], chain["tri"], chain["tri_planted"]
    success, success_planted = int((out["exit_code"] == tri.SUCCESS).sum()), int((out_planted["exit_code"] == tri.SUCCESS).sum())
    print(f"inlier edges {len(ti.edges)} (planted rotations {len(ti_planted.edges)}), triangulated tracks {success} of {len(out['track_off']) - 1} (planted {success_planted})")
    assert ti.edges == ti_planted.edges and set(ti.edges) == set(M.window_edges()) - {M.WRONG_ROTATION, M.WRONG_TRANSLATION}
    assert len(out["track_off"]) == len(out_planted["track_off"]) and success == success_planted
    res = M.point_distances(restated["scene"], out["track_off"], out["image"], out["kp"], out["point"], out["exit_code"])
    assert res["pure"] == res["success"] == success
