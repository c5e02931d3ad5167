"""CPU: the planted scene of tests/multi_view_scene.py under the restated chain, each stage fed the previous restatement's output -- so that
tests/test_multi_view_chain_gpu.py, which runs the same scene through ``VerifiedScene`` on the device, is not vacuous. What the scene is built
for is asserted here: every edge verifies, the good edges recover the true relative poses, the view graph drops exactly the wrong-rotation
edge, 1DSfM gives the wrong-translation edge the largest mean outlier weight and (with the threshold halfway to the next one) rejects exactly
it, the tracks of the surviving edges hold no ghost keypoint, and their triangulated points are the planted ones. The measured figures the
device results are held to (twice each) are printed and must not have moved from what tests/multi_view_scene.py records. None of it needs a GPU."""

import numpy as np
import pytest

from tests import multi_view_scene as M
from tests import translation_inliers_reference as ti_ref
from tests import translation_inliers_scenes, view_graph_scenes


@pytest.fixture(scope="module")
def chain():
    return M.restated_chain()


def test_scene_layout_is_the_generators(chain):
    sc = chain["scene"]
    assert len(sc["edges"]) == 26 and len(sc["device_edges"]) == 24 == 2 * M.LAUNCH_PAIRS and sc["rows"] == sc["device_edges"] + list(M.FALLBACK)
    assert sc["edges"] == sorted(M.window_edges() + [M.LOSES_SUPPORT, M.NO_MODEL]) and len(M.window_edges()) == 24
    assert sc["device_edges"].index(M.LOSES_SUPPORT) < M.LAUNCH_PAIRS <= sc["device_edges"].index(M.NO_MODEL)  # one in each launch
    assert sc["xy"].dtype == np.float32 and sc["xy"].shape == (M.NUM_IMAGES, M.CAP, 2)
    k = sc["intrinsics"]
    assert len({tuple(r) for r in k.tolist()}) == M.NUM_IMAGES and (np.abs(k[:, 0] - k[:, 1]) > 20).all()  # different and anisotropic
    assert all(np.ptp(sc["centre"][:, a]) > 2.0 for a in range(3))  # spread in x, y and z
    count, off = sc["match_count"], np.asarray(sc["match_off"])
    assert (count < np.diff(off)).all() and (np.diff(off) == M.CAP).all()
    beyond = np.concatenate([sc["match_idx"][off[p] + count[p]:off[p + 1]] for p in range(len(count))])
    assert (np.abs(beyond.astype(np.int64)) >= 1 << 20).all()  # the rows beyond the count: out of range on both sides
    for p, e in enumerate(sc["device_edges"]):
        rows = sc["putative"][e]
        assert rows.dtype == np.uint32 and (np.diff(rows[:, 0].astype(np.int64)) > 0).all() and np.array_equal(sc["match_idx"][off[p]:off[p] + count[p]], rows.astype(np.int32))
    for e in (M.WRONG_ROTATION, M.WRONG_TRANSLATION):  # the planted edges match true keypoints of i to ghosts of j; no other edge touches a ghost
        assert sum((e[1], int(k2)) in sc["ghosts"] for k2 in sc["putative"][e][:, 1]) > 0.7 * M.PER_EDGE
    assert all(not any((e[1], int(k2)) in sc["ghosts"] for k2 in sc["putative"][e][:, 1]) for e in M.good_edges(sc))
    # every window edge lies in a triplet, the planted ones included: an edge without one would be kept by the filter untested
    first = chain["view_graph"]["passes"][0]
    assert all((n > 0) == (e not in (M.LOSES_SUPPORT, M.NO_MODEL)) for e, n in zip(sc["rows"], first["num_triplets"]))


def test_verifier_and_bundle_adjustment_recover_the_true_poses(chain):
    sc, oracle, two_view = chain["scene"], chain["oracle"], chain["two_view"]
    # every window edge gets a model, the planted ones too: they are consistent. NO_MODEL has too few matches for one
    assert all((r["R"] is not None) == (e != M.NO_MODEL) for e, r in oracle.items()) and oracle[M.NO_MODEL]["hypotheses"] == 0
    worst = np.zeros(2)
    for e in M.good_edges(sc):
        for rot, direction in ((oracle[e]["R"], oracle[e]["t"]), (two_view[e]["R"], two_view[e]["t"])):
            worst = np.maximum(worst, M.pose_errors(sc, e, rot, direction))
    print(f"good edges: rotation error <= {worst[0]:.4f} deg (recorded {M.MEASURED_ROTATION_DEG}, bound {M.ROTATION_BOUND_DEG}), "
          f"direction error <= {worst[1]:.4f} deg (recorded {M.MEASURED_DIRECTION_DEG}, bound {M.DIRECTION_BOUND_DEG})")
    assert 0.9 * M.MEASURED_ROTATION_DEG < worst[0] <= M.MEASURED_ROTATION_DEG and 0.9 * M.MEASURED_DIRECTION_DEG < worst[1] <= M.MEASURED_DIRECTION_DEG
    for stage in (oracle, two_view):
        rot_err, _ = M.pose_errors(sc, M.WRONG_ROTATION, stage[M.WRONG_ROTATION]["R"], stage[M.WRONG_ROTATION]["t"])
        _, dir_err = M.pose_errors(sc, M.WRONG_TRANSLATION, stage[M.WRONG_TRANSLATION]["R"], stage[M.WRONG_TRANSLATION]["t"])
        print(f"planted: rotation edge {M.WRONG_ROTATION} off by {rot_err:.3f} deg, translation edge {M.WRONG_TRANSLATION} off by {dir_err:.3f} deg")
        assert abs(rot_err - M.ROLL_DEG) < M.ROTATION_BOUND_DEG and rot_err > M.PLANTED_ROTATION_MIN_DEG > 10 * M.ROTATION_BOUND_DEG
        assert dir_err > M.PLANTED_DIRECTION_MIN_DEG > 10 * M.DIRECTION_BOUND_DEG
    # the standing cap of tests/test_two_view_ba_gpu.py, met by the restatement alone
    non_decisive = [e for e, r in two_view.items() if r["ba"]["non_decisive"]]
    assert len(non_decisive) <= len(two_view) // 16, non_decisive
    window = {e: two_view[e] for e in M.window_edges()}
    assert all(r["supported"] and r["ba"]["status"] == 0 and M.MIN_INLIERS <= r["stats0"] <= len(chain["verified"][e][2]) for e, r in window.items())
    assert any(r["stats0"] < len(chain["verified"][e][2]) for e, r in window.items())  # the adjustment's filter removes correspondences
    # the two routes out of the chain: the adjustment runs and its filter leaves too few; nothing to adjust
    lost, none = two_view[M.LOSES_SUPPORT], two_view[M.NO_MODEL]
    print(f"{M.LOSES_SUPPORT}: {len(chain['verified'][M.LOSES_SUPPORT][2])} verified, {int(lost['valid'].sum())} valid after the adjustment, supported {lost['supported']}")
    assert lost["ba"]["status"] == 0 and len(chain["verified"][M.LOSES_SUPPORT][2]) >= M.MIN_INLIERS and 0 < lost["valid"].sum() < M.MIN_INLIERS and not lost["ba"]["non_decisive"]
    assert not lost["supported"] and lost["stats0"] == 0 and lost["R"] is None and len(lost["corr"]) == 0 and np.isfinite(lost["ba"]["rotation"]).all()
    assert none["ba"]["status"] == 1 and not none["supported"] and none["stats0"] == 0 and none["R"] is None


def test_view_graph_drops_exactly_the_wrong_rotation_edge(chain):
    sc, vg = chain["scene"], chain["view_graph"]
    first, second = vg["passes"]
    for k, out in enumerate(vg["passes"]):
        print(f"pass {k}: smallest margin {out['margin'].min():.4f} deg, aggregate of {M.WRONG_ROTATION} {out['aggregate_error'][sc['rows'].index(M.WRONG_ROTATION)]:.4f}")
        assert out["margin"].min() > view_graph_scenes.MARGIN_DEG
    dropped = [e for e, i, k in zip(sc["rows"], first["input"], first["keep"]) if i and not k]
    assert dropped == [M.WRONG_ROTATION] and [e for e, i in zip(sc["rows"], first["input"]) if not i] == [M.LOSES_SUPPORT, M.NO_MODEL]
    assert not second["input"][sc["rows"].index(M.WRONG_ROTATION)] and np.array_equal(second["keep"], first["keep"])  # absent from the second pass: dropped in both
    assert set(vg["edges"]) == set(M.window_edges()) - {M.WRONG_ROTATION} and vg["pruned_edges"] == vg["edges"]


def test_translation_inliers_reject_exactly_the_wrong_translation_edge(chain):
    sc, out = chain["scene"], chain["translation"]
    first, second = chain["top_weights"]
    print(f"largest mean outlier weight {first:.6f} at {sc['rows'][chain['top_row']]}, next {second:.6f}, threshold {chain['threshold']:.6f} "
          f"(the default is {ti_ref.OUTLIER_WEIGHT_THRESHOLD})")
    assert sc["rows"][chain["top_row"]] == M.WRONG_TRANSLATION and first > 1.5 * second
    rejected = [e for e, on, k in zip(sc["rows"], out["enable"], out["pair_inlier"]) if on and not k]
    assert rejected == [M.WRONG_TRANSLATION] and set(out["edges"]) == set(M.window_edges()) - {M.WRONG_ROTATION, M.WRONG_TRANSLATION}
    weights = np.concatenate([out["pair_weight"], out["meas_weight"]])
    assert np.nanmin(np.abs(weights - chain["threshold"])) > translation_inliers_scenes.THRESHOLD_MARGIN
    assert np.isnan(out["pair_weight"][sc["rows"].index(M.WRONG_ROTATION)]) and out["counts"][1] > 0  # the view graph's edge took no part; tracks did
    assert out["camera_inlier"].all()


def test_tracks_of_the_surviving_edges_hold_no_ghost(chain):
    sc, tracks, everything = chain["scene"], chain["tracks"], chain["tracks_all"]
    ghosts, ghosts_all = M.ghost_measurements(sc, tracks["image"], tracks["kp"]), M.ghost_measurements(sc, everything["image"], everything["kp"])
    print(f"surviving edges: {tracks['tracks']} tracks, {tracks['discarded']} discarded, {ghosts} ghost measurements; all edges: {everything['tracks']} tracks, "
          f"{everything['discarded']} discarded, {ghosts_all} ghost measurements")
    assert ghosts == 0 and ghosts_all > 50
    assert tracks["discarded"] < everything["discarded"] and tracks["tracks"] > 400 and tracks["longest"] == M.NUM_IMAGES


def test_triangulated_points_are_the_planted_ones(chain):
    sc, tracks, out = chain["scene"], chain["tracks"], chain["triangulation"]
    res = M.point_distances(sc, tracks["track_off"], tracks["image"], tracks["kp"], out["point"], out["exit_code"])
    print(f"{tracks['tracks']} tracks, exit codes {np.bincount(out['exit_code'], minlength=6).tolist()}, {res['pure']} of {res['success']} triangulated tracks are one planted "
          f"point's ({res['points']} of {M.NUM_POINTS} points), distance <= {res['distance'].max():.4f} (recorded {M.MEASURED_POINT_DISTANCE}, bound {M.POINT_BOUND}), "
          f"median {np.median(res['distance']):.4f}")
    assert res["pure"] == res["success"] > 0.95 * tracks["tracks"] and res["points"] > 0.9 * M.NUM_POINTS
    assert 0.9 * M.MEASURED_POINT_DISTANCE < res["distance"].max() <= M.MEASURED_POINT_DISTANCE
    assert 0.9 * M.MEASURED_POINT_MEDIAN < np.median(res["distance"]) <= M.MEASURED_POINT_MEDIAN
    assert not out["non_decisive"].any()
