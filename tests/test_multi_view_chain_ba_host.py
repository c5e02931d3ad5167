"""CPU: global bundle adjustment as the last link of the planted chain (tests/multi_view_scene.py), on the restatements end to end: the 1DSfM
rejection's rows -> the recovered centres -> tracks and triangulation with them -> tests/global_ba_reference.py. The host twin of
tests/test_multi_view_chain_ba_gpu.py: it measures what that test asserts (after a similarity fit, the largest camera-centre error relative to
the scene's extent and the median distance of a kept point from its planted point, before and after the adjustment) and asserts that the
recorded constants have not moved, and calls ``VerifiedScene.bundle_adjust`` on a scene without rows; ``-s`` prints the lines appended to profiles/multi_view_chain.txt."""

import numpy as np
import pytest

from tests import global_ba_reference as ba_ref
from tests import multi_view_ba_stage as BS
from tests import multi_view_scene as M
from tests import multi_view_translation_stage as TS
from tests import triangulation_reference as tri


@pytest.fixture(scope="module")
def stage():
    r = M.restated_chain()
    sc, t, trk = r["scene"], r["translation"], r["tracks"]
    rec = TS.recovery_stage(sc["rows"], t["world_pair"], t["pair_inlier"], t["tracks"]["track_off"], t["tracks"]["image"], t["world_meas"], t["meas_inlier"])
    centres = rec["translation"][:M.NUM_IMAGES]
    table = np.stack([tri.pack_camera(*sc["intrinsics"][i], sc["wRi"][i], centres[i]) for i in range(M.NUM_IMAGES)])
    uv = sc["xy"][trk["image"], trk["kp"]]
    tr = tri.triangulate_tracks(table, trk["track_off"], trk["image"], uv, **M.triangulation_options())
    ba = BS.ba_stage(table, trk["track_off"], trk["image"], uv, tr["point"], tr["exit_code"], tr["inlier_mask"])
    return sc, trk, table, tr, ba


def test_the_adjustment_converges_and_refines_the_chain(stage):
    sc, trk, table, tr, ba = stage
    c, k = ba["counters"], ba["costs"]
    assert c["status"] == ba_ref.CONVERGED and k["final_cost"] <= k["init_cost"]
    assert c["cameras"] == M.NUM_IMAGES and c["points"] == int((np.asarray(tr["exit_code"]) == tri.SUCCESS).sum())
    assert ba_ref.filter_margin(ba, BS.OPTIONS["reproj_error_threshold"]) > ba_ref.FILTER_MARGIN_PX
    success = (np.asarray(tr["exit_code"]) == tri.SUCCESS).astype(np.uint8)
    before_fit, after_fit = BS.fit(sc, table), BS.fit(sc, ba["cameras"])
    before = BS.kept_tracks(sc, before_fit, trk["track_off"], trk["image"], trk["kp"], tr["point"], success)
    after = BS.kept_tracks(sc, after_fit, trk["track_off"], trk["image"], trk["kp"], ba["point"], ba["track_valid"])
    print(f"\nglobal bundle adjustment (restatement): counters {c}, cost {k['init_cost']:.6e} -> {k['final_cost']:.6e}, |g|_inf {k['gradient_inf_norm']:.3e}; centre error "
          f"{before_fit['relative']:.3e} -> {after_fit['relative']:.3e} of the extent {after_fit['extent']:.3f}; tracks {before['kept']} triangulated -> {after['kept']} kept, on one "
          f"planted point {before['pure']} -> {after['pure']}, median distance {np.median(before['distance']):.5f} -> {np.median(after['distance']):.5f}, largest "
          f"{before['distance'].max():.4f} -> {after['distance'].max():.4f}, kept tracks with a ghost keypoint {after['ghost_tracks']}")
    assert after["ghost_tracks"] == 0 and after["pure"] == after["kept"] > 0
    for got, want in ((before_fit["relative"], BS.MEASURED_CENTRE_ERROR_REL_BEFORE), (after_fit["relative"], BS.MEASURED_CENTRE_ERROR_REL_AFTER),
                      (float(np.median(before["distance"])), BS.MEASURED_POINT_MEDIAN_BEFORE), (float(np.median(after["distance"])), BS.MEASURED_POINT_MEDIAN_AFTER)):
        assert got <= want * 1.0001 and got >= want * 0.99, "a MEASURED_* constant of tests/multi_view_ba_stage.py is no longer what the restatement gives"


def test_a_scene_without_rows_gives_the_empty_result():
    """``VerifiedScene.bundle_adjust`` on a scene without a feature table: no device is touched, every array is empty, the status NO_VALID_ROW."""
    from gtsfm_amd.frontend.correspondence_generator.verified_scene import VerifiedScene

    out = VerifiedScene([], {}, {}, None, [], {}).bundle_adjust({}, None)
    assert out["status"] == "NO_VALID_ROW" and out["counters"]["status"] == ba_ref.NO_VALID_ROW and out["counters"]["anchor"] == -1
    assert out["track_off"].tolist() == [0] and out["point"].shape == (0, 3) and out["cameras"].shape == (0, 17)
    assert all(len(out[k]) == 0 for k in ("image", "kp", "track_valid", "camera_kept", "reproj_error", "exit_code"))
    assert all(np.isnan(v) for v in out["costs"].values())
