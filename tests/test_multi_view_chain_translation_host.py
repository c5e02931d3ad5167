"""CPU: translation recovery as the link of the planted chain (tests/multi_view_scene.py) that produces the camera positions, on the
restatements end to end: the 1DSfM rejection's rows -> tests/translation_recovery_reference.py -> tracks and triangulation with the RECOVERED
centres in place of the planted ones. The host twin of tests/test_multi_view_chain_translation_gpu.py: it measures what that test asserts
(the largest camera-centre error after a scale-and-shift fit, relative to the scene's extent; the count of tracks triangulated onto their
planted point); ``-s`` prints the lines appended to profiles/multi_view_chain.txt."""

import numpy as np
import pytest

from tests import multi_view_scene as M
from tests import multi_view_translation_stage as TS
from tests import translation_recovery_reference as tr_ref
from tests import triangulation_reference as tri


@pytest.fixture(scope="module")
def stage():
    r = M.restated_chain()
    t = r["translation"]
    res = TS.recovery_stage(r["scene"]["rows"], t["world_pair"], t["pair_inlier"], t["tracks"]["track_off"], t["tracks"]["image"], t["world_meas"], t["meas_inlier"])
    return r, res


def test_the_stage_recovers_the_planted_centres(stage):
    r, res = stage
    c = res["counters"]
    assert c["status"] == tr_ref.CONVERGED and res["node_valid"][:M.NUM_IMAGES].all()
    assert c["anchor"] == r["translation"]["edges"][0][1]
    assert c["valid_rows"] == int(r["translation"]["pair_inlier"].sum()) + int(r["translation"]["meas_inlier"].sum())
    fit = TS.centre_errors(r["scene"], res["translation"][:M.NUM_IMAGES])
    line = (f"translation recovery (restatement): counters {c}, cost {res['costs']['init_cost']:.6e} -> {res['costs']['final_cost']:.6e}, centre error {fit['relative']:.3e} of the "
            f"extent {fit['extent']:.3f} after the fit (scale {fit['scale']:.6f})")
    print(line)
    assert fit["relative"] <= TS.MEASURED_CENTRE_ERROR_REL * 1.0001, "MEASURED_CENTRE_ERROR_REL is no longer what the restatement gives"


def test_triangulation_with_the_recovered_cameras(stage):
    r, res = stage
    sc = r["scene"]
    fit = TS.centre_errors(sc, res["translation"][:M.NUM_IMAGES])
    trk = r["tracks"]
    out = TS.triangulate_with(sc, sc["wRi"], res["translation"][:M.NUM_IMAGES], trk["track_off"], trk["image"], trk["kp"])
    got = TS.on_planted_point(sc, fit, trk["track_off"], trk["image"], trk["kp"], out["point"], out["exit_code"])
    planted = M.point_distances(sc, trk["track_off"], trk["image"], trk["kp"], r["triangulation"]["point"], r["triangulation"]["exit_code"])
    line = (f"triangulation with recovered centres (restatement): {got['success']} of {len(trk['track_off']) - 1} tracks (planted centres {planted['success']}), on one planted point "
            f"{got['pure']} ({planted['pure']}), largest distance {got['distance'].max():.4f} ({planted['distance'].max():.4f}), median {np.median(got['distance']):.4f}")
    print(line)
    assert got["pure"] == got["success"]
    assert (np.asarray(out["exit_code"]) == tri.SUCCESS).sum() > 0
