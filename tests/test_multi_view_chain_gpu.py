"""GPU: the planted scene of tests/multi_view_scene.py through the real ``generate_verified_scene`` and then, on that one scene object,
``two_view`` -> ``view_graph`` -> ``translation_inliers`` -> ``tracks`` -> ``triangulate``: every stage reads what the stage before it left
on the device, in the layout the verifier launches leave it (two launches, capacity rows with garbage beyond ``match_count``, images shared by
many edges through ``kp_off = i * cap``, ``stats[:, 0]`` rewritten by ``two_view``, two edges verified on the host and carried in ``extra``, an
edge without a model and its NaN pose, an edge whose mask ``two_view`` zeroes while its pose stays in the launch).

Each stage is held to its restatement FED THE DEVICE'S OWN UPSTREAM OUTPUT, by the rule that stage's own GPU test uses: the verifier by
``tests/test_verifier_gpu._compare``; the bundle adjustment by ``expected_and_tolerance`` / ``compare_pair`` of tests/test_two_view_ba_gpu.py
(from the device's entering points) and the inlier-support decisions, masks and ``stats[:, 0]`` exactly; the view graph by
``view_graph_scenes.check_outputs``; 1DSfM by ``assert_bytes_equal``; the tracks exactly; the triangulation by ``assert_matches`` of
tests/test_triangulation_gpu.py. Then the ground truth of tests/test_multi_view_chain_host.py on the device's results, and the invariances:
the scene before ``two_view`` is untouched, a second run gives the same bytes, and so does the chain with the two launches merged into one.

``view_graph()`` returns no triplet list and ``triangulate()`` no RANSAC statistics; ``check_outputs`` and ``assert_matches`` get the restatement's
own there, so those two fields are not compared (the triplet COUNT is, in ``counts``)."""

import numpy as np
import pytest

from tests import multi_view_scene as M
from tests import translation_inliers_reference as ti_ref
from tests import translation_inliers_scenes, triangulation_scenes, view_graph_scenes

pytestmark = pytest.mark.gpu

LAUNCH_KEYS = ("match_idx", "match_count", "mask", "R", "t", "E", "stats")


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def planted_generator(sc, device):
    """The real generator with the planted ``(keypoints_list, putative, state)`` in place of detection and matching."""
    import torch

    from gtsfm_amd.common.keypoints import Keypoints
    from gtsfm_amd.frontend.correspondence_generator.batched_twoway_correspondence_generator import BatchedTwoWayCorrespondenceGenerator
    from gtsfm_amd.frontend.detector_descriptor import SIFTDetectorDescriptor
    from gtsfm_amd.frontend.matcher.twoway_matcher import TwoWayMatcher

    class PlantedGenerator(BatchedTwoWayCorrespondenceGenerator):
        def _detect_and_match(self, client, images, visibility_graph):
            assert [tuple(e) for e in visibility_graph] == sc["edges"]
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
            feats = {"xy": dev(sc["xy"]), "count": dev(np.full(M.NUM_IMAGES, M.CAP, np.int32))}
            matched = {"pairs": list(sc["device_edges"]), "empty": [], "match_idx": dev(sc["match_idx"]), "match_off": list(sc["match_off"]),
                       "match_count": dev(sc["match_count"])}
            return [Keypoints(coordinates=sc["xy"][i].copy()) for i in range(M.NUM_IMAGES)], {e: sc["putative"][e].copy() for e in sc["edges"]}, {"feats": feats, "matched": matched}

    return PlantedGenerator(TwoWayMatcher(), SIFTDetectorDescriptor(max_keypoints=M.CAP))


def run_chain(sc, device, threshold, launch_pairs=None, other_order_first=False):
    """The whole chain on the device; ``launch_pairs``: pairs per verifier launch (None: the generator's own limit, one launch here);
    ``other_order_first``: on the scene ``two_view`` returned, ``tracks`` and then ``translation_inliers`` run once (over every edge) before
    ``view_graph``, so the columns of the scene's edge table are built in another order than the chain's."""
    from gtsfm_amd.bundle.two_view_ba import TwoViewOptions
    from gtsfm_amd.common.calibration import PinholeCamera, PinholeIntrinsics
    from gtsfm_amd.data_association.point3d_initializer import TriangulationOptions, TriangulationSamplingMode
    from gtsfm_amd.frontend.correspondence_generator import batched_twoway_correspondence_generator as module
    from gtsfm_amd.frontend.verifier.ransac import Ransac
    from tests.test_translation_inliers_gpu import ShortAveraging

    cals = [PinholeIntrinsics(k[0], k[2], k[3], fy=k[1]) for k in sc["intrinsics"]]
    cameras = {i: PinholeCamera(sc["wRi"][i], sc["centre"][i], cals[i]) for i in range(M.NUM_IMAGES)}
    gen = planted_generator(sc, device)
    with pytest.MonkeyPatch.context() as patch:
        if launch_pairs is not None:
            patch.setattr(module, "MAX_VERIFY_PAIRS", launch_pairs)
        scene = gen.generate_verified_scene(None, [None] * M.NUM_IMAGES, sc["edges"], cals, Ransac(True, M.VERIFY_THRESHOLD_PX))
    before = [{k: host(v).copy() for k, v in ver.items() if k in LAUNCH_KEYS} for ver in scene.launches] + [{"xy": host(scene.feats["xy"]).copy()}]
    new = scene.two_view(TwoViewOptions(min_num_inliers_est_model=M.MIN_INLIERS, min_inlier_ratio_est_model=M.MIN_RATIO), cals)
    rotations = [sc["wRi"][i] for i in range(M.NUM_IMAGES)]
    if other_order_first:
        new.tracks()
        early = ShortAveraging()
        early._outlier_weight_threshold = threshold
        new.translation_inliers(rotations, cals, averaging=early)
    vg = new.view_graph()
    averaging = ShortAveraging()
    assert M.NUM_DIRECTIONS == 64
    averaging._outlier_weight_threshold = threshold
    ti = new.translation_inliers(rotations, cals, edges=vg.edges, averaging=averaging)
    tracks = new.tracks(edges=ti.edges)
    options = TriangulationOptions(mode=TriangulationSamplingMode.NO_RANSAC, reproj_error_threshold=M.TRIANGULATION_THRESHOLD_PX)
    tri = new.triangulate(cameras, options, edges=ti.edges)
    after = [{k: host(v) for k, v in ver.items() if k in LAUNCH_KEYS} for ver in scene.launches] + [{"xy": host(scene.feats["xy"])}]
    return {"scene": scene, "new": new, "vg": vg, "ti": ti, "tracks": tracks, "tri": tri, "before": before, "after": after, "cals": cals}


def chain_bytes(res):
    """Every result of a chain run as bytes, the launches' arrays concatenated in launch order (so two launches compare with one)."""
    out = {}
    for name, sc in (("verified", res["scene"]), ("two_view", res["new"])):
        for k in ("R", "t", "stats", "mask", "match_count"):
            out[f"{name}.{k}"] = np.concatenate([host(ver[k]) for ver in sc.launches]).tobytes()
        out[f"{name}.pairs"] = repr([tuple(p) for ver in sc.launches for p in ver["pairs"]])
        out[f"{name}.extra"] = repr({e: np.asarray(v).tolist() for e, v in sc.extra.items()})
        out[f"{name}.host"] = repr({e: (None if v[0] is None else np.asarray(matrix(v[0])).tobytes(), None if v[1] is None else np.asarray(vector(v[1])).tobytes(),
                                        np.asarray(v[2]).tolist(), v[3]) for e, v in sc.verified.items()})
    vg, ti = res["vg"], res["ti"]
    out["vg"] = repr((vg.pairs, vg.keep.tobytes(), vg.pruned.tobytes(), vg.component, [(p["counts"], p["num_triplets"].tobytes(), p["aggregate_error"].tobytes(), p["keep"].tobytes())
                                                                                      for p in vg.passes]))
    out["ti"] = repr((ti.pairs, ti.pair_weight.tobytes(), ti.pair_inlier.tobytes(), ti.camera_inlier.tobytes(), ti.meas_weight.tobytes(), ti.meas_inlier.tobytes(), ti.counts))
    out["tracks"] = repr([res["tracks"][k].tobytes() for k in ("track_off", "image", "kp", "track_uv")] + [res["tracks"]["counts"]])
    out["tri"] = repr([res["tri"][k].tobytes() for k in ("track_off", "image", "kp", "point", "avg_error", "exit_code", "inlier_mask")])
    return out


def matrix(rot):
    from gtsfm_amd.view_graph_estimator.cycle_consistent_rotation_estimator import rotation_matrix

    return rotation_matrix(rot)


def vector(direction):
    from gtsfm_amd.averaging.translation.averaging_1dsfm import vector3

    return vector3(direction)


@pytest.fixture(scope="module")
def restated():
    return M.restated_chain()


@pytest.fixture(scope="module")
def device_chain(gpu_device, restated):
    return run_chain(restated["scene"], gpu_device, restated["threshold"], launch_pairs=M.LAUNCH_PAIRS)


def launch_rows(ver):
    """Per pair of a launch: (edge, first row, match count, the rows of its verified correspondences)."""
    count, mask = host(ver["match_count"]), host(ver["mask"]).astype(bool)
    out = []
    for p, e in enumerate(ver["pairs"]):
        lo, m = int(ver["match_off"][p]), int(count[p])
        out.append((tuple(e), lo, m, lo + np.flatnonzero(mask[lo:lo + m])))
    return out


def device_verified(scene):
    """The verifier's tuples as the device left them: per launch edge (R, t, verified rows of match_idx, ratio) from the launches' arrays, per
    fallback edge the host-verified tuple of ``verified``."""
    out = {}
    for ver in scene.launches:
        rot, trans, idx, stats = host(ver["R"]), host(ver["t"]), host(ver["match_idx"]), host(ver["stats"])
        for p, (e, lo, m, rows) in enumerate(launch_rows(ver)):
            ok = stats[p, 0] > 0
            out[e] = (rot[p] if ok else None, trans[p] if ok else None, idx[rows].astype(np.int64), len(rows) / m if ok and m else 0.0)
    for e in scene.extra:
        v = scene.verified[e]
        out[e] = (None if v[0] is None else matrix(v[0]), None if v[1] is None else vector(v[1]), np.asarray(v[2], np.int64).reshape(-1, 2), v[3])
    return out


def two_view_rows(new):
    """(rotation [E, 9], direction [E, 3], enable [E], correspondences per edge) of the scene after ``two_view``, in the scene's row order: what
    the view graph, 1DSfM and the tracks read."""
    rows, rot, direction, enable, corr = [], [], [], [], {}
    for ver in new.launches:
        r, t, idx, stats = host(ver["R"]).reshape(-1, 9), host(ver["t"]).reshape(-1, 3), host(ver["match_idx"]), host(ver["stats"])
        for p, (e, lo, m, kept) in enumerate(launch_rows(ver)):
            rows.append(e)
            rot.append(r[p])
            direction.append(t[p])
            enable.append(stats[p, 0] > 0)
            corr[e] = idx[kept].astype(np.int64)
    for e in new.extra:
        v = new.verified[e]
        if v[0] is not None:
            rows.append(e)
            rot.append(matrix(v[0]).reshape(9))
            direction.append(vector(v[1]))
            enable.append(True)
        corr[e] = np.asarray(new.extra[e], np.int64).reshape(-1, 2)
    return rows, np.asarray(rot), np.asarray(direction), np.asarray(enable, np.uint8), corr


def test_verifier_launches_in_the_generators_layout_equal_the_oracle(device_chain, restated):
    from tests.test_verifier_gpu import _compare

    sc, scene, oracle = restated["scene"], device_chain["scene"], restated["oracle"]
    assert [[tuple(p) for p in ver["pairs"]] for ver in scene.launches] == [sc["device_edges"][:M.LAUNCH_PAIRS], sc["device_edges"][M.LAUNCH_PAIRS:]]
    assert list(scene.extra) == list(M.FALLBACK) and list(scene.verified) == sc["edges"]
    for ver in scene.launches:
        mask = host(ver["mask"])
        for p, (e, lo, m, rows) in enumerate(launch_rows(ver)):
            assert m == len(sc["putative"][e]) and not mask[lo + m:int(ver["match_off"][p + 1])].any(), e  # nothing beyond the count is an inlier
            rot, direction, corr, ratio = scene.verified[e]
            if oracle[e]["R"] is None:  # too few matches: no inlier, no hypothesis, a NaN pose in the launch, the failure tuple on the host
                assert e == M.NO_MODEL and host(ver["stats"])[p, :2].tolist() == [0, oracle[e]["hypotheses"]] == [0, 0] and np.isnan(host(ver["R"])[p]).all() and np.isnan(host(ver["t"])[p]).all() and not mask[lo:lo + m].any()
                assert rot is None and direction is None and corr.shape == (0,) and ratio == 0.0
                continue
            _compare(ver, p, lo, lo + m, oracle[e])
            np.testing.assert_array_equal(corr, oracle[e]["v_corr_idxs"], err_msg=str(e))
            assert corr.dtype == np.uint32 and ratio == oracle[e]["inlier_ratio"] and matrix(rot).tobytes() == host(ver["R"])[p].tobytes(), e
    for e in M.FALLBACK:  # verified per pair on the host, from the same keypoints and putative matches
        rot, direction, corr, ratio = scene.verified[e]
        np.testing.assert_array_equal(corr, oracle[e]["v_corr_idxs"], err_msg=str(e))
        np.testing.assert_array_equal(scene.extra[e], corr)
        assert ratio == oracle[e]["inlier_ratio"], e
        np.testing.assert_allclose(matrix(rot), oracle[e]["R"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(vector(direction), oracle[e]["t"], rtol=0, atol=1e-9)


def test_two_view_on_the_launches_equals_the_restatement_and_the_support_decisions(device_chain, restated, gpu_device):
    from gtsfm_amd.runtime.two_view_ba_engine import STATUS_NAMES, TwoViewBAEngine, TwoViewBAOptions
    from tests import two_view_ba_reference as ba_ref
    from tests.test_two_view_ba_gpu import DEVICE_OUTPUTS, compare_pair, expected_and_tolerance

    sc, scene, new = restated["scene"], device_chain["scene"], device_chain["new"]
    upstream = device_verified(scene)
    engine = TwoViewBAEngine(gpu_device)
    names, left_out = [], 0
    table = scene.feats["xy"].reshape(-1, 2)
    for ver, after in zip(scene.launches, new.launches):
        edges = [tuple(p) for p in ver["pairs"]]
        layout = {"kp_xy": table, "kp_off1": [i * M.CAP for i, _ in edges], "kp_off2": [j * M.CAP for _, j in edges], "match_idx": ver["match_idx"],
                  "match_off": list(ver["match_off"]), "match_count": ver["match_count"], "inlier_mask": ver["mask"],
                  "intrinsics": [list(sc["intrinsics"][i]) + list(sc["intrinsics"][j]) for i, j in edges], "rotation": ver["R"], "translation": ver["t"]}
        entering = host(engine.run(layout, TwoViewBAOptions(max_iterations=0, min_verified=M.MIN_INLIERS))["point"])
        direct = engine.run(layout, TwoViewBAOptions(min_verified=M.MIN_INLIERS))
        out = {k: host(direct[k]) for k in DEVICE_OUTPUTS}
        out["stats"] = direct["stats"]
        # the scene call is the engine on the launch's arrays where they lie
        assert host(after["R"]).tobytes() == out["rotation"].tobytes() and host(after["t"]).tobytes() == out["translation"].tobytes()
        np.testing.assert_array_equal(after["two_view"], out["stats"])
        part = launch_rows(ver)
        part_pairs = [M.two_view_pair(sc, e, upstream[e]) for e, _, _, _ in part]
        expected, tolerance = expected_and_tolerance([str(e) for e, _, _, _ in part], part_pairs, {"rows": [r for _, _, _, r in part]}, entering)
        new_mask, new_stats = host(after["mask"]), host(after["stats"])
        for p, ((e, lo, m, kept), exp) in enumerate(zip(part, expected)):
            left_out += compare_pair(str(e), out, p, kept, exp, tolerance)
            # the inlier support, from the device's own counts: exact
            ba = {"valid": out["valid_mask"][kept].astype(bool), "rotation": out["rotation"][p], "translation": out["translation"][p]}
            want = M.after_two_view(upstream[e], ba)
            hi = int(ver["match_off"][p + 1])
            expect_mask = np.zeros(hi - lo, bool)
            expect_mask[kept - lo] = want["rows"]
            np.testing.assert_array_equal(new_mask[lo:hi].astype(bool), expect_mask, err_msg=str(e))
            assert new_stats[p, 0] == want["stats0"] and new.two_view_stats[e]["supported"] == want["supported"], e
            assert new.two_view_stats[e]["status"] == STATUS_NAMES[out["stats"][p, 0]] == ba_ref.STATUS_NAMES[exp["status"]], e
            rot, direction, corr, ratio = new.verified[e]
            np.testing.assert_array_equal(np.asarray(corr, np.int64).reshape(-1, 2), want["corr"], err_msg=str(e))
            if want["R"] is None:  # no support: the failure tuple on the host, whatever pose stays in the launch
                assert e in (M.LOSES_SUPPORT, M.NO_MODEL) and rot is None and direction is None and ratio == 0.0 and len(corr) == 0, e
            else:
                assert ratio == want["ratio"] and matrix(rot).tobytes() == out["rotation"][p].tobytes() and vector(direction).tobytes() == out["translation"][p].tobytes(), e
            names.append(e)
    assert names == sc["device_edges"] and left_out <= len(names) // 16, f"{left_out} non-decisive pairs"
    lost, none = new.two_view_stats[M.LOSES_SUPPORT], new.two_view_stats[M.NO_MODEL]
    print(f"{M.LOSES_SUPPORT}: {lost}; {M.NO_MODEL}: {none}")
    assert lost["status"] == "OK" and lost["verified"] >= M.MIN_INLIERS > lost["valid"] > 0 and not lost["supported"]  # the adjustment ran and its filter left too few
    assert none["status"] == "SKIPPED" and none["verified"] == 0 and not none["supported"]
    # The fallback edges go through the per-pair drop-in from their host-verified tuple. The same tuples as one launch of the engine here: that
    # launch is held to the restatement from ITS entering points like the others, and the drop-in's result to that launch as
    # tests/test_two_view_scene_gpu.py holds it: the same correspondences, counts and support, poses within 1e-9 (a pair alone sits in other lanes).
    fallback = list(M.FALLBACK)
    assert all(upstream[e][0] is not None for e in fallback)
    off = np.concatenate([[0], np.cumsum([len(upstream[e][2]) for e in fallback])]).astype(np.int64)
    layout = {"kp_xy": table, "kp_off1": [i * M.CAP for i, _ in fallback], "kp_off2": [j * M.CAP for _, j in fallback],
              "match_idx": np.concatenate([upstream[e][2] for e in fallback]).astype(np.int32), "match_off": off, "match_count": None, "inlier_mask": np.ones(int(off[-1]), np.uint8),
              "intrinsics": [list(sc["intrinsics"][i]) + list(sc["intrinsics"][j]) for i, j in fallback], "rotation": np.stack([upstream[e][0] for e in fallback]),
              "translation": np.stack([upstream[e][1] for e in fallback])}
    entering = host(engine.run(layout, TwoViewBAOptions(max_iterations=0, min_verified=M.MIN_INLIERS))["point"])
    direct = engine.run(layout, TwoViewBAOptions(min_verified=M.MIN_INLIERS))
    out = {k: host(direct[k]) for k in DEVICE_OUTPUTS}
    out["stats"] = direct["stats"]
    rows = [np.arange(off[k], off[k + 1]) for k in range(len(fallback))]
    expected, tolerance = expected_and_tolerance([f"{e} (fallback)" for e in fallback], [M.two_view_pair(sc, e, upstream[e]) for e in fallback], {"rows": rows}, entering)
    for p, (e, exp) in enumerate(zip(fallback, expected)):
        assert not compare_pair(f"{e} (fallback)", out, p, rows[p], exp, tolerance), f"{e}: non-decisive"
        want = M.after_two_view(upstream[e], {"valid": out["valid_mask"][rows[p]].astype(bool), "rotation": out["rotation"][p], "translation": out["translation"][p]})
        info, (rot, direction, corr, ratio) = new.two_view_stats[e], new.verified[e]
        assert info["host_fallback"] and info["supported"] == want["supported"] and ratio == want["ratio"], e
        assert [info["status"], info["verified"], info["triangulated"], info["valid"], info["accepted_steps"], info["solves_tried"]] == \
            [STATUS_NAMES[out["stats"][p, 0]]] + out["stats"][p, 1:6].tolist(), e
        np.testing.assert_array_equal(np.asarray(corr, np.int64).reshape(-1, 2), want["corr"], err_msg=str(e))
        np.testing.assert_array_equal(np.asarray(new.extra[e], np.int64).reshape(-1, 2), want["corr"], err_msg=str(e))
        np.testing.assert_allclose(matrix(rot), out["rotation"][p], rtol=0, atol=1e-9, err_msg=str(e))
        np.testing.assert_allclose(vector(direction), out["translation"][p], rtol=0, atol=1e-9, err_msg=str(e))
        print(f"{e} (host fallback) against the same tuple in a launch: rotation {np.abs(matrix(rot) - out['rotation'][p]).max():.3e}, "
              f"direction {np.abs(vector(direction) - out['translation'][p]).max():.3e} (allowed 1e-9)")


def test_view_graph_reads_the_refined_rotations_and_the_rewritten_stats(device_chain, restated):
    sc, new, vg = restated["scene"], device_chain["new"], device_chain["vg"]
    rows, rotation, _, enable, _ = two_view_rows(new)
    assert vg.pairs == rows == sc["rows"]
    exp = M.view_graph_stage(rows, rotation, enable)
    tol = view_graph_scenes.measured_tolerance()
    for k, (got, want) in enumerate(zip(vg.passes, exp["passes"])):
        counts = np.array([got["counts"][f] for f in ("input_edges", "kept_edges", "triplets", "max_triplets_per_edge")] + [0] * 4, np.int32)
        dist = view_graph_scenes.check_outputs(f"pass {k}", {"num_triplets": got["num_triplets"], "aggregate_error": got["aggregate_error"], "keep": got["keep"], "counts": counts,
                                                             "triplets": want["triplets"], "cycle_error": want["cycle_error"]}, want, tol["tolerance"])
        print(f"pass {k}: {counts[0]} input edges, {counts[1]} kept, {counts[2]} triplets, aggregate within {dist['aggregate_error']:.3e} deg (tolerance {tol['tolerance']:.3e}), "
              f"smallest margin {want['margin'].min():.4f} deg")
        assert want["margin"].min() > view_graph_scenes.MARGIN_DEG
    comp = exp["passes"][-1]["component"]
    np.testing.assert_array_equal(vg.keep, exp["keep"].astype(np.uint8))
    np.testing.assert_array_equal(vg.pruned, comp["pair_keep"])
    assert [vg.component[f] for f in ("nodes", "edges", "components")] == comp["counts"][:3].tolist()
    assert vg.edges == exp["edges"] and vg.pruned_edges == exp["pruned_edges"]


def test_translation_inliers_on_the_view_graph_edges_equal_the_restatement(device_chain, restated):
    sc, new, vg, ti = restated["scene"], device_chain["new"], device_chain["vg"], device_chain["ti"]
    rows, _, direction, enable, corr = two_view_rows(new)
    exp = M.translation_stage(sc, rows, direction, enable, corr, vg.edges, restated["threshold"])
    got = {"pair_weight": ti.pair_weight, "meas_weight": ti.meas_weight, "pair_inlier": ti.pair_inlier, "meas_inlier": ti.meas_inlier, "camera_inlier": ti.camera_inlier,
           "counts": np.array([ti.counts[k] for k in ti_ref.COUNT_FIELDS] + [0, 0], np.int32)}
    assert ti.pairs == rows
    translation_inliers_scenes.assert_bytes_equal("1DSfM on the chain", got, exp, keys=tuple(got))
    assert ti.edges == exp["edges"]
    for k in ("track_off", "image", "track_enable", "meas_enable"):  # the tracks the call built on the device, and the host's selection among them
        np.testing.assert_array_equal(ti.tracks[k], exp["tracks"][k] if k in exp["tracks"] else exp[k], err_msg=k)
    weights = np.concatenate([ti.pair_weight, ti.meas_weight])
    print(f"mean outlier weight of {M.WRONG_TRANSLATION}: {ti.mean_weights[M.WRONG_TRANSLATION]:.6f}, threshold {restated['threshold']:.6f}, "
          f"nearest weight {np.nanmin(np.abs(weights - restated['threshold'])):.3e} away; counts {ti.counts}")
    assert np.nanmin(np.abs(weights - restated["threshold"])) > translation_inliers_scenes.THRESHOLD_MARGIN


def test_tracks_and_triangulation_of_the_inlier_edges_equal_the_restatements(device_chain, restated):
    from tests.test_triangulation_gpu import assert_matches

    sc, new, ti, tracks, tri = restated["scene"], device_chain["new"], device_chain["ti"], device_chain["tracks"], device_chain["tri"]
    _, _, _, _, corr = two_view_rows(new)
    exp = M.tracks_stage(corr, ti.edges)
    c = tracks["counts"]
    print(c, "restatement:", {k: exp[k] for k in ("tracks", "measurements", "discarded", "components", "rounds")})
    assert (c["tracks"], c["measurements"], c["discarded"], c["components"], c["rounds"]) == (exp["tracks"], exp["measurements"], exp["discarded"], exp["components"], exp["rounds"] or 1)
    for k in ("track_off", "image", "kp"):
        assert tracks[k].dtype == exp[k].dtype and np.array_equal(tracks[k], exp[k]), k
        assert tri[k].tobytes() == tracks[k].tobytes(), k  # triangulate() builds the same tracks
    assert tracks["track_uv"].tobytes() == sc["xy"][tracks["image"], tracks["kp"]].tobytes()
    everything, want_all = new.tracks(), M.tracks_stage(corr, sc["rows"])  # every edge: the zeroed masks of the edges without support are honoured
    for k in ("track_off", "image", "kp"):
        assert np.array_equal(everything[k], want_all[k]), f"all edges: {k}"
    want = M.triangulation_stage(sc, tri["track_off"], tri["image"], tri["kp"])
    table = {"track_off": tri["track_off"], "image": tri["image"], "uv": want["uv"], "cameras": M.camera_table(sc)}
    out = dict(tri, stats=want["stats"])
    assert_matches(out, want, tri["track_off"], want["non_decisive"], *triangulation_scenes.reversal_tolerance(table), "chain")


def test_the_chain_recovers_what_was_planted(device_chain, restated):
    sc, scene, new, vg, ti, tracks, tri = (restated["scene"], device_chain["scene"], device_chain["new"], device_chain["vg"], device_chain["ti"], device_chain["tracks"],
                                            device_chain["tri"])
    worst = np.zeros(2)
    for stage in (device_verified(scene), device_verified(new)):
        for e in M.good_edges(sc):
            worst = np.maximum(worst, M.pose_errors(sc, e, stage[e][0], stage[e][1]))
        assert M.pose_errors(sc, M.WRONG_ROTATION, *stage[M.WRONG_ROTATION][:2])[0] > M.PLANTED_ROTATION_MIN_DEG
        assert M.pose_errors(sc, M.WRONG_TRANSLATION, *stage[M.WRONG_TRANSLATION][:2])[1] > M.PLANTED_DIRECTION_MIN_DEG
    print(f"good edges: rotation error <= {worst[0]:.4f} deg (bound {M.ROTATION_BOUND_DEG}), direction error <= {worst[1]:.4f} deg (bound {M.DIRECTION_BOUND_DEG})")
    assert worst[0] <= M.ROTATION_BOUND_DEG and worst[1] <= M.DIRECTION_BOUND_DEG
    assert set(vg.edges) == set(M.window_edges()) - {M.WRONG_ROTATION} and vg.pruned_edges == vg.edges
    dropped = [[e for e, k, n in zip(vg.pairs, p["keep"], p["num_triplets"]) if not k and n] for p in vg.passes]
    assert dropped == [[M.WRONG_ROTATION], []], dropped  # dropped by the first pass, absent from the second
    assert set(ti.edges) == set(M.window_edges()) - {M.WRONG_ROTATION, M.WRONG_TRANSLATION}
    assert max(ti.mean_weights, key=lambda e: -1.0 if np.isnan(ti.mean_weights[e]) else ti.mean_weights[e]) == M.WRONG_TRANSLATION
    everything = new.tracks()
    ghosts, ghosts_all = M.ghost_measurements(sc, tracks["image"], tracks["kp"]), M.ghost_measurements(sc, everything["image"], everything["kp"])
    print(f"inlier edges: {tracks['counts']}, {ghosts} ghost measurements; all edges: {everything['counts']}, {ghosts_all} ghost measurements")
    assert ghosts == 0 and ghosts_all > 50 and tracks["counts"]["discarded"] < everything["counts"]["discarded"]
    res = M.point_distances(sc, tri["track_off"], tri["image"], tri["kp"], tri["point"], tri["exit_code"])
    print(f"{res['pure']} of {res['success']} triangulated tracks are one planted point's ({res['points']} of {M.NUM_POINTS} points), distance <= {res['distance'].max():.4f} "
          f"(bound {M.POINT_BOUND}), median {np.median(res['distance']):.4f} (bound {M.POINT_MEDIAN_BOUND})")
    assert res["pure"] == res["success"] > 0.95 * tracks["counts"]["tracks"] and res["points"] > 0.9 * M.NUM_POINTS
    assert res["distance"].max() <= M.POINT_BOUND and np.median(res["distance"]) <= M.POINT_MEDIAN_BOUND


def test_the_scene_is_untouched_and_the_chain_repeats_and_does_not_depend_on_the_launch_split(device_chain, restated, gpu_device):
    for k, (a, b) in enumerate(zip(device_chain["before"], device_chain["after"])):
        for key in a:
            assert a[key].tobytes() == b[key].tobytes(), f"launch {k}: {key} changed under the chain"
    first = chain_bytes(device_chain)
    again = chain_bytes(run_chain(restated["scene"], gpu_device, restated["threshold"], launch_pairs=M.LAUNCH_PAIRS))
    assert [k for k in first if first[k] != again[k]] == []
    merged = run_chain(restated["scene"], gpu_device, restated["threshold"])
    assert len(merged["scene"].launches) == 1 and len(device_chain["scene"].launches) == 2
    one = chain_bytes(merged)
    assert [k for k in first if first[k] != one[k]] == []


def test_the_chain_does_not_depend_on_the_order_in_which_the_stages_first_ran(device_chain, restated, gpu_device):
    """``tracks`` first and ``translation_inliers`` before ``view_graph`` on one scene: each stage builds what it needs of the scene's edge
    table on first use, so the order of the first calls must not show in any result."""
    first = chain_bytes(device_chain)
    other = chain_bytes(run_chain(restated["scene"], gpu_device, restated["threshold"], launch_pairs=M.LAUNCH_PAIRS, other_order_first=True))
    assert [k for k in first if first[k] != other[k]] == []
