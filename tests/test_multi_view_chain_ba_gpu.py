"""GPU: the planted scene of tests/multi_view_scene.py through ``two_view`` -> ``view_graph`` -> ``rotation_averaging`` ->
``translation_averaging`` -> ``bundle_adjust`` (tracks -> triangulate -> global bundle adjustment on the device arrays where they lie) on one
scene object. The adjustment is held to its restatement (tests/global_ba_reference.py) FED THE DEVICE'S OWN READ-BACK triangulation (the
camera table, the track CSR, the points, the exit codes, the inlier mask): byte equality. It converges with a final cost <= the initial one;
no track with a ghost keypoint is kept; every kept track lies on one planted point; and after a similarity fit the camera-centre error relative
to the extent and the median point distance, before and after the adjustment, stay within MARGIN x what the host twin
(tests/test_multi_view_chain_ba_host.py) measures on the restatements, exactly as the translation stage is held."""

import numpy as np
import pytest

from tests import global_ba_reference as ba_ref
from tests import multi_view_ba_stage as BS
from tests import multi_view_rotation_stage as RS
from tests import multi_view_scene as M
from tests import triangulation_reference as tri

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def restated():
    return M.restated_chain()


@pytest.fixture(scope="module")
def chain(gpu_device, restated):
    from gtsfm_amd.bundle.bundle_adjustment import BundleAdjustmentOptimizer, RobustBAMode
    from gtsfm_amd.bundle.two_view_ba import TwoViewOptions
    from gtsfm_amd.common.calibration import PinholeIntrinsics
    from gtsfm_amd.data_association.point3d_initializer import TriangulationOptions, TriangulationSamplingMode
    from gtsfm_amd.frontend.correspondence_generator import batched_twoway_correspondence_generator as module
    from gtsfm_amd.frontend.verifier.ransac import Ransac
    from gtsfm_amd.runtime.triangulation_engine import pack_cameras
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
    options = TriangulationOptions(mode=TriangulationSamplingMode.NO_RANSAC, reproj_error_threshold=M.TRIANGULATION_THRESHOLD_PX)
    optimizer = BundleAdjustmentOptimizer(reproj_error_thresholds=[10, 5, 3], robust_ba_mode=RobustBAMode.HUBER, measurement_noise_sigma=1.0)
    cameras = ta.cameras(cals)
    ba = new.bundle_adjust(cameras, options, optimizer=optimizer, edges=ta.inliers.edges)
    again = new.bundle_adjust(cameras, options, optimizer=optimizer, edges=ta.inliers.edges)
    return {"ba": ba, "again": again, "tri": new.triangulate(cameras, options, edges=ta.inliers.edges), "uv": new.tracks(edges=ta.inliers.edges)["track_uv"],
            "table": pack_cameras(cameras, num_images=M.NUM_IMAGES)}


def test_the_adjustment_equals_the_restatement_on_the_devices_own_triangulation(chain):
    ba, t = chain["ba"], chain["tri"]
    assert ba["track_off"].tobytes() == t["track_off"].tobytes() and ba["image"].tobytes() == t["image"].tobytes() and ba["exit_code"].tobytes() == t["exit_code"].tobytes()
    want = BS.ba_stage(chain["table"], t["track_off"], t["image"], chain["uv"], t["point"], t["exit_code"], t["inlier_mask"])
    print(f"chain bundle adjustment: {ba['status']}, counters {ba['counters']}, costs {ba['costs']}")
    assert ba["status"] == "CONVERGED" == ba_ref.STATUS_NAMES[want["counters"]["status"]] and ba["costs"]["final_cost"] <= ba["costs"]["init_cost"]
    assert ba["counters"] == want["counters"]
    assert np.array([ba["costs"][k] for k in ba_ref.COST_FIELDS]).tobytes() == np.array([want["costs"][k] for k in ba_ref.COST_FIELDS], np.float64).tobytes()
    for k in ("cameras", "point", "reproj_error", "track_valid", "camera_kept"):
        assert ba[k].tobytes() == want[k].tobytes(), k
        assert chain["again"][k].tobytes() == ba[k].tobytes(), f"two runs differ in {k}"
    assert ba_ref.filter_margin(want, BS.OPTIONS["reproj_error_threshold"]) > ba_ref.FILTER_MARGIN_PX
    assert ba["counters"]["points"] == int((t["exit_code"] == tri.SUCCESS).sum()) and ba["counters"]["cameras"] == M.NUM_IMAGES


def test_the_kept_tracks_are_planted_points_and_the_geometry_is_refined(chain, restated):
    sc, ba, t = restated["scene"], chain["ba"], chain["tri"]
    success = (t["exit_code"] == tri.SUCCESS).astype(np.uint8)
    before_fit, after_fit = BS.fit(sc, chain["table"]), BS.fit(sc, ba["cameras"])
    before = BS.kept_tracks(sc, before_fit, t["track_off"], t["image"], t["kp"], t["point"], success)
    after = BS.kept_tracks(sc, after_fit, ba["track_off"], ba["image"], ba["kp"], ba["point"], ba["track_valid"])
    print(f"centre error {before_fit['relative']:.3e} -> {after_fit['relative']:.3e} of the extent (host twin {BS.MEASURED_CENTRE_ERROR_REL_BEFORE:.3e} -> "
          f"{BS.MEASURED_CENTRE_ERROR_REL_AFTER:.3e}); tracks {before['kept']} -> {after['kept']} kept, on one planted point {after['pure']}, median distance "
          f"{np.median(before['distance']):.5f} -> {np.median(after['distance']):.5f} (host twin {BS.MEASURED_POINT_MEDIAN_BEFORE} -> {BS.MEASURED_POINT_MEDIAN_AFTER}), ghost tracks "
          f"kept {after['ghost_tracks']}")
    assert after["ghost_tracks"] == 0, "a track with a ghost keypoint passed the filter"
    assert after["pure"] == after["kept"] > 0, "a kept track is not one planted point's"
    assert ba["camera_kept"].all() and after_fit["cameras"] == M.NUM_IMAGES
    assert before_fit["relative"] <= BS.MARGIN * BS.MEASURED_CENTRE_ERROR_REL_BEFORE and after_fit["relative"] <= BS.MARGIN * BS.MEASURED_CENTRE_ERROR_REL_AFTER
    assert np.median(before["distance"]) <= BS.MARGIN * BS.MEASURED_POINT_MEDIAN_BEFORE and np.median(after["distance"]) <= BS.MARGIN * BS.MEASURED_POINT_MEDIAN_AFTER

