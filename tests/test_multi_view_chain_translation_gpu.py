"""GPU: the planted scene of tests/multi_view_scene.py through ``two_view`` -> ``view_graph`` -> ``rotation_averaging`` ->
``translation_averaging`` -> ``tracks`` -> ``triangulate`` on one scene object: the chain runs from the verified matches to the points without
being handed a rotation or a position -- the triangulation's cameras are the averaged rotations and the RECOVERED centres. The recovery is
held to its restatement (tests/translation_recovery_reference.py) FED THE DEVICE'S OWN READ-BACK rows (world directions, masks, track CSR):
byte equality. After a least-squares scale-and-shift fit the largest camera-centre error, relative to the scene's extent, stays within
8 x what the host twin (tests/test_multi_view_chain_translation_host.py) measures on the restatements; every triangulated track lies on one
planted point and their count equals that with the planted cameras; the inlier edge set equals that with planted rotations."""

import numpy as np
import pytest

from tests import multi_view_rotation_stage as RS
from tests import multi_view_scene as M
from tests import multi_view_translation_stage as TS
from tests import translation_recovery_reference as tr_ref
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
    from tests.test_multi_view_chain_gpu import planted_generator
    from tests.test_translation_inliers_gpu import ShortAveraging

    sc = restated["scene"]
    cals = [PinholeIntrinsics(k[0], k[2], k[3], fy=k[1]) for k in sc["intrinsics"]]
    with pytest.MonkeyPatch.context() as patch:
        patch.setattr(module, "MAX_VERIFY_PAIRS", M.LAUNCH_PAIRS)
        scene = planted_generator(sc, gpu_device).generate_verified_scene(None, [None] * M.NUM_IMAGES, sc["edges"], cals, Ransac(True, M.VERIFY_THRESHOLD_PX))
    new = scene.two_view(TwoViewOptions(min_num_inliers_est_model=M.MIN_INLIERS, min_inlier_ratio_est_model=M.MIN_RATIO), cals)
    vg = new.view_graph()
    ra = new.rotation_averaging(edges=vg.edges)
    aligned = RS.aligned_to_planted(sc, ra.wRi_list, ra.counters["anchor"])
    averaging = ShortAveraging(translation_recovery="device")
    averaging._outlier_weight_threshold = restated["threshold"]
    ta = new.translation_averaging(aligned, cals, edges=vg.edges, averaging=averaging)
    again = new.translation_averaging(aligned, cals, edges=vg.edges, averaging=averaging)
    ti_planted = new.translation_inliers([sc["wRi"][i] for i in range(M.NUM_IMAGES)], cals, edges=vg.edges, averaging=averaging)
    options = TriangulationOptions(mode=TriangulationSamplingMode.NO_RANSAC, reproj_error_threshold=M.TRIANGULATION_THRESHOLD_PX)
    out = new.triangulate(ta.cameras(cals), options, edges=ta.inliers.edges)
    out_planted = new.triangulate({i: PinholeCamera(sc["wRi"][i], sc["centre"][i], cals[i]) for i in range(M.NUM_IMAGES)}, options, edges=ti_planted.edges)
    return {"ta": ta, "again": again, "ti_planted": ti_planted, "tri": out, "tri_planted": out_planted, "vg": vg}


def test_the_recovery_equals_the_restatement_on_the_devices_own_rows(chain):
    ta = chain["ta"]
    rows = ta.read_back()
    want = TS.recovery_stage(rows["pair_images"], rows["world_pair"], rows["pair_enable"], rows["track_off"], rows["image"], rows["world_meas"], rows["meas_enable"])
    got = np.stack([np.full(3, np.nan) if t is None else t for t in ta.wti_list])
    print(f"chain translation recovery: {ta.status}, counters {ta.counters}, costs {ta.costs}")
    assert ta.status == "CONVERGED" == tr_ref.STATUS_NAMES[want["counters"]["status"]]
    assert ta.counters == want["counters"]
    assert np.array([ta.costs[k] for k in tr_ref.COST_FIELDS]).tobytes() == np.array([want["costs"][k] for k in tr_ref.COST_FIELDS], np.float64).tobytes()
    assert got.tobytes() == want["translation"][:M.NUM_IMAGES].tobytes() and ta.landmarks.tobytes() == want["translation"][M.NUM_IMAGES:].tobytes()
    assert all(t is not None for t in ta.wti_list) and all(p is not None for p in ta.wTi_list)
    assert ta.counters["valid_rows"] == int(rows["pair_enable"].sum()) + int(rows["meas_enable"].sum())
    assert np.stack(chain["again"].wti_list).tobytes() == got.tobytes() and chain["again"].counters == ta.counters


def test_the_recovered_centres_are_the_planted_ones_up_to_scale_and_shift(chain, restated):
    fit = TS.centre_errors(restated["scene"], np.stack(chain["ta"].wti_list))
    print(f"centre error {fit['relative']:.3e} of the extent {fit['extent']:.3f} after the fit (scale {fit['scale']:.6f}); host twin {TS.MEASURED_CENTRE_ERROR_REL:.3e}")
    assert fit["cameras"] == M.NUM_IMAGES and fit["relative"] <= TS.MARGIN * TS.MEASURED_CENTRE_ERROR_REL


def test_the_chain_triangulates_with_recovered_cameras_only(chain, restated):
    sc, ta, out, out_planted = restated["scene"], chain["ta"], chain["tri"], chain["tri_planted"]
    assert ta.inliers.edges == chain["ti_planted"].edges and set(ta.inliers.edges) == set(M.window_edges()) - {M.WRONG_ROTATION, M.WRONG_TRANSLATION}
    success, success_planted = int((out["exit_code"] == tri.SUCCESS).sum()), int((out_planted["exit_code"] == tri.SUCCESS).sum())
    fit = TS.centre_errors(sc, np.stack(ta.wti_list))
    res = TS.on_planted_point(sc, fit, out["track_off"], out["image"], out["kp"], out["point"], out["exit_code"])
    print(f"triangulated tracks {success} of {len(out['track_off']) - 1} (planted cameras {success_planted}), on one planted point {res['pure']}, largest distance "
          f"{res['distance'].max():.4f}, median {np.median(res['distance']):.4f}")
    assert len(out["track_off"]) == len(out_planted["track_off"]) and success == success_planted
    assert res["pure"] == res["success"] == success
