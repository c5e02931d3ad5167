"""CPU: the specification of the device's 1DSfM outlier rejection (tests/translation_inliers_reference.py) against what it restates -- the
reference's known answers (``tests/averaging/translation/test_averaging_1dsfm.py``: the five-camera outlier case, the track selection, the
landmark direction, the measurement keys), a brute-force MFAS that recomputes every sum at every step, and two synthetic scenes with known
truth. gtsam cannot be imported here, so parity towards gtsam's own MFAS is not observed: its choice among several roots or tied scores
follows the hash order of an ``unordered_map`` (PARITY UNPINNED by nature), as do ``Unit3``'s last bits."""

import numpy as np
import pytest

from tests import translation_inliers_reference as ref
from tests import translation_inliers_scenes as scenes

EXACT_SUMS = ("empty", "one_edge", "axis_aligned")  # weights in {0, +-1} or a single edge: recomputed and decremented sums cannot differ


def test_five_camera_known_answer():
    """Test1dsfmAllOutliers: exactly the four edges that touch camera 4 are rejected; the ten mean weights are recorded."""
    sc, out = scenes.get("five_cameras"), scenes.expected("five_cameras")
    golden = np.load(scenes.GOLDEN)
    assert len(sc["directions"]) == 2000
    rejected = [tuple(p) for p, k in zip(sc["pair_images"].tolist(), out["pair_inlier"]) if not k]
    assert rejected == [(0, 4), (1, 4), (2, 4), (3, 4)]
    assert out["pair_weight"].tobytes() == golden["mean_weight"].tobytes() and out["pair_inlier"].tobytes() == golden["pair_inlier"].tobytes()
    assert np.round(out["pair_weight"][[3, 6, 8, 9]], 3).tolist() == [0.220, 0.219, 0.219, 0.241]
    others = out["pair_weight"][[0, 1, 2, 4, 5, 7]]
    assert 0.0003 < others.min() and others.max() < 0.086
    # camera 4 keeps no edge: its translation cannot be recovered, as the reference's test expects (wTi_computed[-1] is None)
    assert out["camera_inlier"].tolist() == [1, 1, 1, 1, 0]


def test_select_tracks_known_answer():
    """test_select_tracks_for_averaging: 7 tracks, measurements_per_camera = 3 -> 4 selected, each among the five listed camera lists."""
    cameras = [[0, 1, 2, 3, 5, 6], [1, 2, 3], [0, 1, 3, 4], [0, 2], [0, 1, 2], [2, 3, 4], [0, 3, 1, 5]]
    track_off = np.concatenate([[0], np.cumsum([len(c) for c in cameras])])
    image = np.concatenate(cameras)
    track_enable, meas_enable, chosen = ref.select_tracks(track_off, image, {0, 1, 2, 3}, measurements_per_camera=3)
    assert len(chosen) == 4 and track_enable.sum() == 4 and chosen[0] == 0 and 3 not in chosen and 5 not in chosen
    listed = [[0, 1, 2, 3], [1, 2, 3], [0, 1, 3], [0, 1, 2], [0, 3, 1]]
    for j in chosen:
        kept = [int(c) for c, ok in zip(cameras[j], meas_enable[track_off[j]:track_off[j + 1]]) if ok]
        assert kept in listed
    every, _, order = ref.select_tracks(track_off, image, {0, 1, 2, 3}, use_all_tracks=True)
    assert order == [0, 1, 2, 4, 6] and every.tolist() == [1, 1, 1, 0, 1, 0, 1]


def test_landmark_direction_known_answer():
    """test_get_landmark_directions: uv = (20, 20), f = 20, wRi = diag(1, -1, 1) -> (1, -1, 1) / sqrt(3). Unit3's last bits are unpinned."""
    w, valid = ref.world_landmark_directions([0, 1], [0], [[20.0, 20.0]], [1], None, np.diag([1.0, -1.0, 1.0]).reshape(1, 9), [1], [[20.0, 20.0, 0.0, 0.0]])
    assert valid.tolist() == [True]
    np.testing.assert_allclose(w[0], np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0), rtol=4e-16, atol=0)
    with pytest.raises(ValueError, match="valid rotation"):
        ref.world_landmark_directions([0, 1], [0], [[20.0, 20.0]], [1], None, np.zeros((1, 9)), [0], [[20.0, 20.0, 0.0, 0.0]])


def test_measurement_keys_known_answer():
    """test_binary_measurements_from_dict: (C(i2), C(i1)) per pair and (C(i), L(j)) per track measurement (j, i); C(i) -> i, L(j) -> N + j."""
    pairs = [(0, 1), (0, 2), (1, 2)]
    eye = np.eye(3)
    g = ref.build_edges(pairs, eye, np.ones(3, bool), [0, 2, 3], [1, 2, 2], eye, np.ones(3, bool), 3)  # tracks (0, 1), (0, 2), (1, 2) as (j, i)
    assert set(zip(g["key1"].tolist(), g["key2"].tolist())) == {(i2, i1) for i1, i2 in pairs} | {(i, 3 + j) for j, i in pairs}
    assert list(zip(g["key1"].tolist(), g["key2"].tolist())) == sorted(zip(g["key1"].tolist(), g["key2"].tolist()))  # gtsam's key order C(i) < L(j)
    with pytest.raises(ValueError, match="twice"):
        ref.build_edges([(0, 1), (0, 1)], eye[:2], np.ones(2, bool), [0], [], np.zeros((0, 3)), np.zeros(0, bool), 2)


def test_world_frame_quirk_and_refusals():
    rot = scenes.random_rotations(np.random.default_rng(3), 3)
    w, valid = ref.world_pair_directions([(0, 1), (1, 2), (0, 2)], np.tile([0.0, 0.6, 0.8], (3, 1)), [1, 1, 0], rot, [0, 1, 0])
    assert valid.tolist() == [True, False, False] and np.isnan(w[1:]).all()  # wRi[0] is not looked at; wRi[2] is
    np.testing.assert_allclose(w[0], rot[1].reshape(3, 3) @ [0.0, 0.6, 0.8], rtol=0, atol=3e-16)
    for bad in ([(1, 0)], [(0, 3)], [(-1, 1)]):
        with pytest.raises(ValueError):
            ref.world_pair_directions(bad, [[1.0, 0.0, 0.0]], None, rot, [1, 1, 1])
    sc = scenes.get("one_edge")
    with pytest.raises(ValueError, match="direction"):
        ref.translation_inliers(sc["pair_images"], sc["pair_direction"], None, sc["rotation"], sc["rotation_valid"], sc["intrinsics"], sc["track_off"], sc["image"], sc["uv"],
                                sc["track_enable"], None, np.zeros((0, 3)))


@pytest.mark.parametrize("name", scenes.SCENE_NAMES)
def test_brute_force_mfas(name):
    """Dict-of-dicts, every node's sums recomputed from the surviving edges at every step: equal positions where the sums are exact, equal
    violated sets everywhere."""
    sc, out = scenes.get(name), scenes.expected(name)
    g = out["graph"]
    nodes = sc["num_images"] + len(sc["track_off"]) - 1
    directions = sc["directions"] if name != "five_cameras" else sc["directions"][::40]
    positions = out["position"] if name != "five_cameras" else out["position"][::40]
    for d, position in zip(directions, positions):
        brute = ref.mfas_positions_brute_force(g["key1"], g["key2"], g["m"], d, nodes)
        if name in EXACT_SUMS:
            assert brute.tobytes() == position.tobytes()
        a, b = ref.outlier_weights(g["key1"], g["key2"], g["m"], d, brute), ref.outlier_weights(g["key1"], g["key2"], g["m"], d, position)
        assert a.tobytes() == b.tobytes()
        assert sorted(position[position >= 0].tolist()) == list(range(int(out["counts"][2])))  # a permutation of the graph's nodes


def true_scene(planted: int):
    """20 cameras with a window of 6, 60 landmarks seen by 3 cameras each, 200 directions, true world directions; ``planted`` pair rows are
    replaced by random directions."""
    rng = np.random.default_rng(7)
    n = 20
    centre = rng.uniform(-5, 5, size=(n, 3))
    point = rng.uniform(-5, 5, size=(60, 3))
    pairs = scenes.window(n, 6)
    tracks = [sorted(rng.choice(n, 3, replace=False).tolist()) for _ in range(60)]
    w_pair = ref.unit(np.array([centre[i1] - centre[i2] for i1, i2 in pairs]))
    w_meas = ref.unit(np.array([point[j] - centre[c] for j, cams in enumerate(tracks) for c in cams]))
    directions = scenes.random_units(rng, 200)
    rows = rng.choice(len(pairs), planted, replace=False) if planted else np.zeros(0, np.int64)
    w_pair[rows] = scenes.random_units(rng, planted)
    return scenes.scene(f"true_{planted}", pairs, np.zeros((len(pairs), 3)), n, directions, tracks=tracks, world=(w_pair, w_meas)), [pairs[k] for k in rows]


def test_noise_free_scene_has_no_outlier_weight():
    sc, _ = true_scene(0)
    out = scenes.restate(sc)
    assert out["counts"][:3].tolist() == [len(sc["pair_images"]), 180, 80]
    assert max(out["pair_weight"].max(), out["meas_weight"].max()) < 1e-12
    assert out["pair_inlier"].all() and out["meas_inlier"].all() and out["camera_inlier"].all()


def test_planted_outliers_are_the_only_rejections():
    """1DSfM does not find every outlier: the rejected set is non-empty and a subset of the planted rows."""
    sc, planted = true_scene(8)
    out = scenes.restate(sc)
    rejected = {tuple(p) for p, k in zip(sc["pair_images"].tolist(), out["pair_inlier"]) if not k}
    assert rejected and rejected <= set(planted), (rejected, planted)
    assert np.abs(np.concatenate([out["pair_weight"], out["meas_weight"]]) - sc["threshold"]).min() > scenes.THRESHOLD_MARGIN


def test_every_scene_holds_what_it_is_named_for():
    for name in scenes.SCENE_NAMES:
        scenes.expected(name)
