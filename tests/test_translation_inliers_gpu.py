"""GPU: ``gtsfm_translation_inliers_f64`` (gtsfm_amd/csrc/translation_kernels.hip) through ``TranslationInliersEngine`` on every scene of
tests/translation_inliers_scenes.py: ``position``, the mean weights, the three masks and the counts are byte-equal to the restatement
(tests/translation_inliers_reference.py), and so are the world directions. Should the device's float64 ``sqrt`` / ``/`` not be correctly
rounded, the MFAS comparison is NOT loosened: the device's own directions are fed to the restatement for it, and the directions are held to
8 x the restatement's measured distance from an ``np.longdouble`` evaluation (``-s`` prints both numbers:
profiles/translation_inliers_gpu_tests.txt). The bytes of one direction do not depend on its place in a batch (a workgroup's second direction
included, on either tier), on the run, or on the storage tier (2048 nodes are the last graph in LDS, 2049 the first in the workspace). The
drop-in's ``compute_inliers`` and ``VerifiedScene.translation_inliers`` on a synthetic scene in the generators' layout equal the restatement's edge list, and ``tracks(edges=result.edges)`` equals ``tracks()`` of the same list given by hand."""

import numpy as np
import pytest

from tests import tracks_reference as TR
from tests import translation_inliers_reference as ref
from tests import translation_inliers_scenes as scenes

pytestmark = pytest.mark.gpu

MFAS_KEYS = ("pair_weight", "meas_weight", "pair_inlier", "meas_inlier", "camera_inlier", "position", "counts")


@pytest.fixture(scope="module")
def engine(gpu_device):
    from gtsfm_amd.runtime.translation_engine import TranslationInliersEngine

    return TranslationInliersEngine(gpu_device)


def run_scene(engine, sc, directions=None, lds_nodes=None):
    dev = engine.upload(sc["pair_images"], sc["pair_direction"], sc["pair_enable"], sc["rotation"], sc["rotation_valid"], sc["intrinsics"], sc["track_off"], sc["image"],
                        sc["uv"], sc["track_enable"], sc["meas_enable"], sc["directions"] if directions is None else directions)
    world = None if sc["world"] is None else engine.upload_world(*sc["world"])
    out = engine.inliers(*dev, threshold=sc["threshold"], world=world, lds_nodes=sc["lds_node_limit"] if lds_nodes is None else lds_nodes, want_position=True)
    got = {k: out[k].cpu().numpy() for k in scenes.OUTPUT_KEYS if k != "counts"}
    got["counts"], got["tier"] = out["counts_raw"].astype(np.int32), out["tier"]
    return got


def longdouble_distance(sc, world_pair) -> float:
    """The largest distance of valid float64 pair directions from their np.longdouble evaluation."""
    on = np.isfinite(world_pair).all(axis=1)
    if not on.any():
        return 0.0
    exact = ref.longdouble_world_pair(sc["pair_direction"][on], sc["rotation"][sc["pair_images"][on, 1]])
    return float(np.abs(world_pair[on].astype(np.longdouble) - exact).max())


@pytest.mark.parametrize("name", scenes.SCENE_NAMES)
def test_scene_is_byte_equal_to_the_restatement(engine, name):
    held_to_the_restatement(engine, name, scenes.get(name), scenes.expected(name))


def rows_256_scene():
    """150 pair rows and 106 measurement rows: num_pairs + num_meas is exactly one workgroup of the per-row stages, and the last row is a
    measurement."""
    rng = np.random.default_rng(61)
    centre, rot, _, tracks = scenes.true_geometry(rng, 40, 53, per_landmark=2)
    pairs = scenes.window(40, 4)
    sc = scenes.scene("rows_256", pairs, scenes.pair_directions(centre, rot, pairs), 40, scenes.random_units(rng, 3), rotation=rot, tracks=tracks,
                      uv=rng.uniform(0, 100, size=(106, 2)))
    assert (len(sc["pair_images"]), len(sc["image"])) == (150, 106)
    return sc


def test_row_count_of_exactly_one_workgroup(engine):
    sc = rows_256_scene()
    exp = scenes.restate(sc)
    assert exp["counts"][0] == 150 and exp["counts"][1] == 106 and 0 < exp["counts"][3] and 0 < exp["counts"][4]  # every row is an edge, both kinds have inliers
    held_to_the_restatement(engine, sc["name"], sc, exp)


def held_to_the_restatement(engine, name, sc, exp):
    got = run_scene(engine, sc)
    limit = 2048 if sc["lds_node_limit"] < 0 else min(sc["lds_node_limit"], 2048)  # TR_LDS_NODES is the default and the most
    assert got["tier"] == ("workspace" if int(exp["counts"][2]) > limit else "lds")
    same_directions = all(got[k].tobytes() == exp[k].tobytes() for k in ("world_pair", "world_meas"))
    if same_directions:
        scenes.assert_bytes_equal(name, got, exp)
        print(f"{name}: world directions byte-equal to the restatement; position, weights, masks and counts byte-equal")
        return
    # float64 sqrt or / is not correctly rounded on this device: the MFAS comparison stays bit for bit, on the device's own directions
    measured = longdouble_distance(sc, exp["world_pair"])
    device = longdouble_distance(sc, got["world_pair"])
    print(f"{name}: world directions differ from the restatement; restatement from longdouble {measured:.3e}, device from longdouble {device:.3e}, bound {8 * measured:.3e}")
    again = ref.translation_inliers(sc["pair_images"], None, sc["pair_enable"], None, sc["rotation_valid"], None, sc["track_off"], sc["image"], None, sc["track_enable"],
                                    sc["meas_enable"], sc["directions"], sc["threshold"], world=(got["world_pair"], got["world_meas"]))
    scenes.assert_bytes_equal(name + " (on the device's directions)", got, again, MFAS_KEYS)
    assert np.array_equal(np.isfinite(got["world_pair"]), np.isfinite(exp["world_pair"])) and np.array_equal(np.isfinite(got["world_meas"]), np.isfinite(exp["world_meas"]))
    assert device <= 8 * measured
    on = np.isfinite(exp["world_meas"])
    assert np.abs(got["world_meas"][on] - exp["world_meas"][on]).max(initial=0.0) <= 8 * measured


def test_a_direction_gives_the_same_bytes_alone_and_anywhere_in_a_batch(engine):
    sc = scenes.get("directions_7")
    whole = run_scene(engine, sc)["position"]
    order = np.array([4, 0, 6, 2, 5, 1, 3])
    shuffled = run_scene(engine, sc, directions=sc["directions"][order])["position"]
    assert shuffled.tobytes() == whole[order].tobytes()
    for k in (0, 3, 6):
        assert run_scene(engine, sc, directions=sc["directions"][k:k + 1])["position"].tobytes() == whole[k:k + 1].tobytes()
    # more directions than workgroups: each workgroup walks several
    five = scenes.get("five_cameras")
    expected = scenes.expected("five_cameras")["position"]
    tail = run_scene(engine, five, directions=five["directions"][1990:])["position"]
    assert tail.tobytes() == expected[1990:].tobytes()
    # 770 directions on 768 workgroups, on the workspace tier and with more than 256 nodes on the LDS tier: the rows that workgroups 0 and 1
    # walk second (768, 769) equal the same directions run alone, as do a first row and the last workgroup's
    for name, tier in (("directions_770_workspace", "workspace"), ("tier_770", "lds")):
        sc = scenes.get(name)
        whole = run_scene(engine, sc)
        assert whole["tier"] == tier and whole["position"].tobytes() == scenes.expected(name)["position"].tobytes()
        for k in (0, 767, 768, 769):
            alone = run_scene(engine, sc, directions=sc["directions"][k:k + 1])
            assert alone["tier"] == tier and alone["position"].tobytes() == whole["position"][k:k + 1].tobytes(), f"{name}: direction {k} alone differs from its row in the batch"


def test_runs_and_storage_tiers_give_the_same_bytes(engine):
    lds, ws = run_scene(engine, scenes.get("tier_lds")), run_scene(engine, scenes.get("tier_workspace"))
    assert (lds["tier"], ws["tier"]) == ("lds", "workspace")
    scenes.assert_bytes_equal("tiers", ws, lds)
    scenes.assert_bytes_equal("rerun", run_scene(engine, scenes.get("tier_workspace")), ws)
    for name in ("hub_300", "lost_camera", "ring_513"):  # every scene's tier is a storage decision only
        sc = scenes.get(name)
        a, b = run_scene(engine, sc, lds_nodes=0), run_scene(engine, sc)
        assert (a["tier"], b["tier"]) == ("workspace", "lds")
        scenes.assert_bytes_equal(name, a, b)
    # TR_LDS_NODES nodes and one more, with the default limit: 2048 nodes are the largest LDS launch and go to the workspace when forced; 2049
    # go to the workspace by themselves, and no limit puts them into LDS (a larger one is clamped), so their other run is the limit 0
    sc = scenes.get("window_2048_2")
    a, b = run_scene(engine, sc), run_scene(engine, sc, lds_nodes=0)
    assert (a["tier"], b["tier"]) == ("lds", "workspace")
    scenes.assert_bytes_equal("window_2048_2", b, a)
    sc = scenes.get("window_2049_2")
    a, b, c = run_scene(engine, sc), run_scene(engine, sc, lds_nodes=0), run_scene(engine, sc, lds_nodes=4096)
    assert (a["tier"], b["tier"], c["tier"]) == ("workspace", "workspace", "workspace")
    scenes.assert_bytes_equal("window_2049_2", b, a)
    scenes.assert_bytes_equal("window_2049_2", c, a)


@pytest.mark.parametrize("case", ["reversed", "duplicate", "out_of_range", "duplicate_measurement", "camera_without_rotation", "no_direction"])
def test_bad_rows_are_refused(engine, case):
    pairs = {"reversed": [(0, 1), (2, 1)], "duplicate": [(0, 1), (1, 2), (0, 1)], "out_of_range": [(0, 1), (1, 5)]}.get(case, [(0, 1), (1, 2)])
    tracks = {"duplicate_measurement": [[0, 1, 1]], "camera_without_rotation": [[0, 1, 2]]}.get(case, [])
    sc = scenes.scene(case, [(0, 1)] * len(pairs), np.tile([0.0, 0.6, 0.8], (len(pairs), 1)), 3, np.zeros((0, 3)) if case == "no_direction" else [[1.0, 0.0, 0.0]], tracks=tracks,
                      rotation_valid=[1, 1, 0] if case == "camera_without_rotation" else [1, 1, 1])
    sc["pair_images"] = np.asarray(pairs, np.int32)
    with pytest.raises(RuntimeError, match="gtsfm_translation_inliers_f64"):
        run_scene(engine, sc)
    with pytest.raises(TypeError):
        dev = list(engine.upload(*[scenes.get("one_edge")[k] for k in ("pair_images", "pair_direction", "pair_enable", "rotation", "rotation_valid", "intrinsics", "track_off",
                                                                      "image", "uv", "track_enable", "meas_enable", "directions")]))
        dev[1] = dev[1].float()
        engine.inliers(*dev)


# ---- the drop-in and the scene layer ----

NUM_IMAGES, CAP, ROWS = 12, 16, 6
NO_MODEL, FALLBACK = (2, 4), (3, 5)


def scene_edges():
    return scenes.window(10, 3) + [(0, 9), (10, 11)]


@pytest.fixture(scope="module")
def built(gpu_device):
    """A scene in the generators' layout, as tests/test_view_graph_scene_gpu.py builds one: two verifier launches, one edge without a model,
    one edge through the per-pair fallback in ``extra``; unit translations from true camera centres, four of them replaced by random ones."""
    import torch

    from gtsfm_amd.frontend.correspondence_generator.verified_scene import VerifiedScene

    edges = scene_edges()
    rng = np.random.default_rng(44)
    centre, rot, _, _ = scenes.true_geometry(rng, NUM_IMAGES, 0)
    t = scenes.pair_directions(centre, rot, edges)
    planted = [3, 9, 14, 20]
    t[planted] = scenes.random_units(rng, len(planted))
    rows = {e: np.stack([np.sort(rng.choice(CAP, ROWS, replace=False))] * 2, axis=1).astype(np.int32) for e in edges}
    failure = (None, None, np.array([], dtype=np.uint64), 0.0)
    verified = {e: (np.eye(3), t[k].copy(), rows[e].astype(np.int64), 0.8) for k, e in enumerate(edges)}
    verified[NO_MODEL] = failure
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)  # noqa: E731
    launches = []
    for part in (edges[:11], edges[11:]):
        on = np.array([e not in (NO_MODEL, FALLBACK) for e in part])
        stats = np.zeros((len(part), 8), np.int32)
        stats[:, 0] = np.where(on, ROWS, 0)
        tt = np.stack([t[edges.index(e)] if ok else np.full(3, np.nan) for e, ok in zip(part, on)])
        launches.append({"pairs": list(part), "match_idx": dev(np.concatenate([rows[e] for e in part])), "match_off": [ROWS * k for k in range(len(part) + 1)],
                         "match_count": dev(np.where(on, ROWS, 0).astype(np.int32)), "mask": dev(np.repeat(on.astype(np.uint8), ROWS)),
                         "R": dev(np.tile(np.eye(3), (len(part), 1, 1))), "t": dev(tt), "stats": dev(stats)})
    xy = np.random.default_rng(22).uniform(0, 100, size=(NUM_IMAGES, CAP, 2)).astype(np.float32)
    scene = VerifiedScene([], {e: rows[e] for e in edges}, verified, {"xy": dev(xy)}, launches, {FALLBACK: rows[FALLBACK].astype(np.int64)})
    wRi = [rot[i].reshape(3, 3) for i in range(NUM_IMAGES)]  # noqa: N806
    wRi[11] = None
    return {"scene": scene, "edges": edges, "rows": rows, "t": t, "wRi": wRi, "xy": xy, "planted": [edges[k] for k in planted]}


def restated_scene(built, edges_in, method="SAMPLE_WITH_UNIFORM_DENSITY"):
    """The restatement on the arrays ``VerifiedScene.translation_inliers`` assembles: the launches' pairs, then the fallback edge."""
    from gtsfm_amd.common.calibration import PinholeIntrinsics

    edges, t, rows = built["edges"], built["t"], built["rows"]
    order = list(edges) + [FALLBACK]  # the fallback edge has a row without a model in its launch and its own row behind the launches
    model = [e not in (NO_MODEL, FALLBACK) for e in edges] + [True]
    enable = np.array([m and (edges_in is None or e in edges_in) for e, m in zip(order, model)], np.uint8)
    direction = np.stack([t[edges.index(e)] if m else np.full(3, np.nan) for e, m in zip(order, model)])
    rotation = np.stack([np.zeros(9) if r is None else r.reshape(9) for r in built["wRi"]])
    valid = np.array([r is not None for r in built["wRi"]], np.uint8)
    intrinsics = np.tile([120.0, 110.0, 50.0, 40.0], (NUM_IMAGES, 1))
    live = [e for e, on in zip(order, enable) if on]
    trk = TR.tracks_reference({e: rows[e].astype(np.int64) for e in live}, [CAP] * NUM_IMAGES)
    uv = built["xy"][trk["image"], trk["kp"]]
    cameras = {c for e, on in zip(order, enable) if on and valid[e[1]] for c in e}
    track_enable, meas_enable, _ = ref.select_tracks(trk["track_off"], trk["image"], cameras)
    np.random.seed(0)
    directions = ref.sample_uniform_directions()[:64]
    out = ref.translation_inliers(np.asarray(order), direction, enable, rotation, valid, intrinsics, trk["track_off"], trk["image"], uv, track_enable, meas_enable, directions)
    cams = [PinholeIntrinsics(120.0, 50.0, 40.0, fy=110.0)] * NUM_IMAGES
    return order, out, cams, trk


class ShortAveraging:
    """``TranslationAveraging1DSFM`` with 64 directions: the test needs seconds, not the 2000-direction default."""

    def __new__(cls, **kw):
        from gtsfm_amd.averaging.translation import TranslationAveraging1DSFM

        obj = TranslationAveraging1DSFM(**kw)
        sample = obj.sample_projection_directions
        obj.sample_projection_directions = lambda w: sample(w)[:64]
        return obj


def test_scene_layer_equals_the_restatement(built):
    scene = built["scene"]
    for edges_in in (None, [e for e in built["edges"] if e != (0, 9)]):
        order, exp, cams, trk = restated_scene(built, edges_in)
        res = scene.translation_inliers(built["wRi"], cams, edges=edges_in, averaging=ShortAveraging())
        assert res.pairs == order
        assert res.pair_weight.tobytes() == exp["pair_weight"].tobytes() and res.pair_inlier.tobytes() == exp["pair_inlier"].tobytes()
        assert res.meas_weight.tobytes() == exp["meas_weight"].tobytes() and res.meas_inlier.tobytes() == exp["meas_inlier"].tobytes()
        assert res.edges == [e for e, k in zip(order, exp["pair_inlier"]) if k] and res.inlier_cameras == set(np.flatnonzero(exp["camera_inlier"]).tolist())
        assert [res.counts[k] for k in ref.COUNT_FIELDS] == exp["counts"][:6].tolist()
        rejected = set(order) - set(res.edges) - {NO_MODEL} - ({(0, 9)} if edges_in else set())
        assert len(res.edges) == len(set(res.edges)) and res.pairs.count(FALLBACK) == 2
        assert rejected and rejected <= set(built["planted"]) | {(10, 11)}, rejected  # (10, 11): wRi[11] is missing
        assert FALLBACK in res.edges and np.isnan(res.mean_weights[NO_MODEL]) and res.counts["measurement_edges"] > 0
        # the result is the edges= argument of tracks()
        by_hand = [e for e, k in zip(order, exp["pair_inlier"]) if k]
        got, same = scene.tracks(edges=res.edges), scene.tracks(edges=by_hand)
        expect = TR.tracks_reference({e: built["rows"][e].astype(np.int64) for e in by_hand}, [CAP] * NUM_IMAGES)
        for k in ("track_off", "image", "kp"):
            np.testing.assert_array_equal(got[k], expect[k], err_msg=k)
            np.testing.assert_array_equal(got[k], same[k], err_msg=k)


def test_drop_in_compute_inliers_equals_the_restatement(built, gpu_device):
    from gtsfm_amd.averaging.translation import TranslationAveraging1DSFM, get_valid_measurements_in_world_frame

    class Direction:  # anything with .point3()
        def __init__(self, v):
            self.v = v

        def point3(self):
            return self.v

    order, exp, cams, trk = restated_scene(built, None)
    order = [e for e in order[:-1] if e != FALLBACK] + [FALLBACK]  # a dict holds the fallback edge once
    i2Ui1 = {e: (None if e == NO_MODEL else Direction(built["t"][built["edges"].index(e)])) for e in order}  # noqa: N806
    world, valid_cameras = get_valid_measurements_in_world_frame(i2Ui1, built["wRi"])
    rows = [k for k, w in enumerate(exp["pair_weight"]) if np.isfinite(w)]  # the valid rows: the launches', then the fallback edge's
    assert list(world) == [(built["edges"] + [FALLBACK])[k] for k in rows] and 11 not in valid_cameras
    assert np.stack(list(world.values())).tobytes() == exp["world_pair"][rows].tobytes()
    averaging = ShortAveraging(device=gpu_device)
    from gtsfm_amd.data_association.dsf_tracks_estimator import tracks_from_csr
    from gtsfm_amd.common.keypoints import Keypoints

    tracks_2d = tracks_from_csr(trk["track_off"], trk["image"], trk["kp"], [Keypoints(built["xy"][i].astype(np.float64)) for i in range(NUM_IMAGES)])
    selected = averaging._select_tracks_for_averaging(tracks_2d, valid_cameras, cams)
    landmarks = averaging._get_landmark_directions(selected, cams, built["wRi"])
    np.random.seed(0)
    inlier_pairs, inlier_tracks, inlier_cameras = averaging.compute_inliers(world, landmarks)
    # the landmark ids are the order of selection here and the track ids in the restatement: the pair results are compared on a restatement
    # of the same dicts
    keys = list(landmarks)
    by_track = sorted(range(len(keys)), key=lambda k: keys[k][0])
    num_tracks = max(j for j, _ in keys) + 1
    track_off = np.concatenate([[0], np.cumsum(np.bincount([keys[k][0] for k in by_track], minlength=num_tracks))])
    np.random.seed(0)
    again = ref.translation_inliers(np.asarray(list(world)), None, None, None, np.ones(NUM_IMAGES), None, track_off, np.array([keys[k][1] for k in by_track]), None,
                                    np.ones(num_tracks), None, ref.sample_uniform_directions()[:64],
                                    world=(np.stack(list(world.values())), np.stack([landmarks[keys[k]] for k in by_track])))
    assert list(inlier_pairs) == [e for e, k in zip(world, again["pair_inlier"]) if k] and inlier_cameras == set(np.flatnonzero(again["camera_inlier"]).tolist())
    assert set(inlier_tracks) == {keys[k] for k, on in zip(by_track, again["meas_inlier"]) if on} and 0 < len(inlier_pairs) < len(world)
    # run_mfas: per direction, the outlier weights whose mean the kernel thresholds
    np.random.seed(0)
    directions = ref.sample_uniform_directions()[:64]
    per_direction = TranslationAveraging1DSFM.run_mfas(world, landmarks, list(directions[:5]), device=gpu_device)
    from gtsfm_amd.averaging.translation.averaging_1dsfm import C

    g = again["graph"]
    for d, weights in zip(directions[:5], per_direction):
        position = ref.mfas_positions(g["key1"], g["key2"], g["m"], d, NUM_IMAGES + num_tracks)
        expect = ref.outlier_weights(g["key1"], g["key2"], g["m"], d, position)
        pair_rows = {int(r): x for r, x in zip(g["row"], expect) if r < len(world)}
        assert [weights[(C(i2), C(i1))] for i1, i2 in world] == [pair_rows[r] for r in range(len(world))]
