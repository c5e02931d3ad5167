"""GPU: ``VerifiedScene.two_view`` -- the rest of ``TwoViewEstimator.run_2view`` behind the verifier, for a whole scene on the device -- on a
small batched scene built from the pairs of tests/two_view_ba_scenes.py: edge by edge against the two-view bundle adjustment's engine on the
same arrays (pinned to its specification by tests/test_two_view_ba_gpu.py) followed by the InlierSupportProcessor's two tests restated here
in numpy; ``tracks()`` of the new scene against tests/tracks_reference.py on the post-ISP correspondences; pass-through with
``bundle_adjust_2view=False``; the old scene untouched."""

import numpy as np
import pytest

from tests import tracks_reference as TR
from tests import two_view_ba_scenes as scenes

pytestmark = pytest.mark.gpu

MIN_INLIERS, MIN_RATIO = 15, 0.1


@pytest.fixture(scope="module")
def built(gpu_device):
    import torch

    from gtsfm_amd.common.calibration import PinholeIntrinsics
    from gtsfm_amd.frontend.correspondence_generator.verified_scene import VerifiedScene
    from tests.test_two_view_ba_gpu import scene_pairs

    names, pairs = scene_pairs()
    pairs = pairs + [scenes.make_pair(301, 24, outliers=0.7)]  # 24 verified, few correspondences survive the filter: support is lost after the adjustment
    names = names + ["mostly_outliers"]
    arr = scenes.verified_scene_arrays(pairs)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)  # noqa: E731
    launch = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in arr["launch"].items()}
    scene = VerifiedScene([], arr["putative"], arr["verified"], {"xy": dev(arr["xy"])}, [launch], {})
    cals = []
    for row in arr["intrinsics"]:
        cals += [PinholeIntrinsics(row[0], row[2], row[3], fy=row[1]), PinholeIntrinsics(row[4], row[6], row[7], fy=row[5])]
    return {"names": names, "pairs": pairs, "arr": arr, "scene": scene, "cals": cals, "device": gpu_device}


def support(ratio, valid):
    """inlier_support_processor.py:73-95: the ratio test first, then the count of a model that has inliers."""
    return not (ratio < MIN_RATIO) and not (valid > 0 and valid < MIN_INLIERS)


def test_two_view_edge_by_edge_and_tracks(built):
    from gtsfm_amd.bundle.two_view_ba import TwoViewOptions
    from gtsfm_amd.runtime.two_view_ba_engine import STATUS_NAMES, TwoViewBAEngine, TwoViewBAOptions

    arr, scene = built["arr"], built["scene"]
    before = {k: v.clone() for k, v in scene.launches[0].items() if hasattr(v, "clone")}
    new = scene.two_view(TwoViewOptions(min_num_inliers_est_model=MIN_INLIERS, min_inlier_ratio_est_model=MIN_RATIO), built["cals"])
    assert new is not scene and new.launches[0] is not scene.launches[0]
    for k, v in before.items():  # the old scene is untouched
        assert v.cpu().numpy().tobytes() == scene.launches[0][k].cpu().numpy().tobytes(), k
    lay = arr["layout"]
    direct_launch = dict(lay, inlier_mask=arr["launch"]["mask"], rotation=arr["launch"]["R"], translation=arr["launch"]["t"])  # what the verifier leaves
    direct = TwoViewBAEngine(built["device"]).run(direct_launch, TwoViewBAOptions(min_verified=MIN_INLIERS))
    valid_mask, rot, trans = direct["valid_mask"].cpu().numpy(), direct["rotation"].cpu().numpy(), direct["translation"].cpu().numpy()
    new_mask, new_stats = new.launches[0]["mask"].cpu().numpy(), new.launches[0]["stats"].cpu().numpy()
    assert new.launches[0]["R"].cpu().numpy().tobytes() == rot.tobytes() and new.launches[0]["t"].cpu().numpy().tobytes() == trans.tobytes()
    surviving, lost = {}, []
    for p, (name, pair) in enumerate(zip(built["names"], built["pairs"])):
        edge = (2 * p, 2 * p + 1)
        a, b, m = int(lay["match_off"][p]), int(lay["match_off"][p + 1]), int(lay["match_count"][p])
        old = arr["verified"][edge]
        st = direct["stats"][p]
        ok = support(old[3], int(st[3]))  # a pair the verifier gave no model has ratio 0: a failure tuple before and after
        expect_rows = valid_mask[a:b].astype(bool) & ok
        np.testing.assert_array_equal(new_mask[a:b].astype(bool), expect_rows, err_msg=name)
        assert new_stats[p, 0] == (int(st[3]) if ok else 0), name
        info = new.two_view_stats[edge]
        assert info["status"] == STATUS_NAMES[st[0]] and info["accepted_steps"] == st[4] and info["solves_tried"] == st[5] and info["supported"] == ok, name
        r, u, corr, ratio = new.verified[edge]
        if not ok:
            lost.append(name)
            assert r is None and u is None and corr.dtype == np.uint64 and corr.shape == (0,) and ratio == 0.0, name
            continue
        assert ratio == old[3], name  # the reference's hack: the pre-adjustment ratio
        np.testing.assert_array_equal(corr, lay["match_idx"][a:a + m][expect_rows[:m]], err_msg=name)
        if np.isfinite(rot[p]).all():
            assert np.asarray(r).tobytes() == rot[p].tobytes() and np.asarray(u).tobytes() == trans[p].tobytes(), name
        else:
            assert r is None and u is None, name
        surviving[edge] = corr
    assert "mostly_outliers" in lost and "n5" in lost and "nan_pose" in lost and len(surviving) >= 10
    # the tracks of the new scene are those of the post-ISP correspondences; the old scene's are those of the verifier's
    sizes = [arr["xy"].shape[1]] * arr["xy"].shape[0]
    for sc, matches in ((new, surviving), (scene, {e: v[2] for e, v in arr["verified"].items() if v[0] is not None})):
        ref = TR.tracks_reference({e: np.asarray(c, np.int64).reshape(-1, 2) for e, c in matches.items()}, sizes)
        got = sc.tracks()
        for k in ("track_off", "image", "kp"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    assert new.tracks()["counts"]["measurements"] < scene.tracks()["counts"]["measurements"]


def test_pass_through_without_bundle_adjustment(built):
    from gtsfm_amd.bundle.two_view_ba import TwoViewOptions

    arr, scene = built["arr"], built["scene"]
    new = scene.two_view(TwoViewOptions(bundle_adjust_2view=False, min_num_inliers_est_model=MIN_INLIERS, min_inlier_ratio_est_model=MIN_RATIO))
    old_mask, new_mask = scene.launches[0]["mask"].cpu().numpy(), new.launches[0]["mask"].cpu().numpy()
    lay = arr["layout"]
    for p, name in enumerate(built["names"]):
        edge = (2 * p, 2 * p + 1)
        a, b = int(lay["match_off"][p]), int(lay["match_off"][p + 1])
        old = arr["verified"][edge]
        n = 0 if old[0] is None else len(old[2])
        ok = support(old[3], n)
        np.testing.assert_array_equal(new_mask[a:b], old_mask[a:b] * ok, err_msg=name)
        r, u, corr, ratio = new.verified[edge]
        if old[0] is None or not ok:
            assert r is None and len(corr) == 0, name
        else:
            assert np.asarray(r).tobytes() == np.asarray(old[0]).tobytes() and np.asarray(u).tobytes() == np.asarray(old[1]).tobytes(), name
            np.testing.assert_array_equal(corr, old[2], err_msg=name)
    assert not new.two_view_stats[(2, 3)]["supported"]  # n5: 5 verified correspondences, under the minimum of 15


def test_non_pinhole_calibration_is_refused_by_name(built):
    from gtsfm_amd.bundle.two_view_ba import TwoViewOptions

    class Cal3Fisheye:  # not of the pinhole family
        def K(self):  # noqa: N802
            return np.eye(3)

    cals = list(built["cals"])
    cals[5] = Cal3Fisheye()
    with pytest.raises(NotImplementedError, match="Cal3Fisheye"):
        built["scene"].two_view(TwoViewOptions(), cals)


def test_bad_offsets_come_back_as_an_error(built):
    from gtsfm_amd.runtime.two_view_ba_engine import TwoViewBAEngine

    lay = dict(scenes.capacity_layout(built["pairs"][2:4]))
    lay["match_off"] = lay["match_off"].copy()
    lay["match_off"][1] = lay["match_off"][2] + 1
    with pytest.raises(RuntimeError, match="match_off_dev is not ascending"):
        TwoViewBAEngine(built["device"]).run(lay)


def test_host_fallback_edges_go_through_the_per_pair_drop_in(built):
    """Edges of ``extra`` (count zero in their launch, correspondences on the host, as the generators leave an edge they verify per pair) get
    ``TwoViewEstimator.bundle_adjust`` and the inlier support tests: the same correspondences, support and poses (to 1e-9: a pair alone sits
    in other lanes) as the same edges adjusted inside the launch; ``tracks()`` equals the restatement on the post-ISP correspondences; a
    non-pinhole calibration on such an edge raises by name; the old scene keeps its ``extra``."""
    import torch

    from gtsfm_amd.bundle.two_view_ba import TwoViewOptions
    from gtsfm_amd.common.keypoints import Keypoints
    from gtsfm_amd.frontend.correspondence_generator.verified_scene import VerifiedScene

    arr, scene, cals, names = built["arr"], built["scene"], built["cals"], built["names"]
    opt = TwoViewOptions(min_num_inliers_est_model=MIN_INLIERS, min_inlier_ratio_est_model=MIN_RATIO)
    inside = scene.two_view(opt, cals)
    moved = [names.index(n) for n in ("n5", "n16", "one_wave", "mostly_outliers", "flipped", "nan_pose")]
    launch = dict(scene.launches[0])
    count, stats, mask = launch["match_count"].clone(), launch["stats"].clone(), launch["mask"].clone()
    for p in moved:
        count[p], stats[p, 0] = 0, 0
        mask[int(arr["layout"]["match_off"][p]):int(arr["layout"]["match_off"][p + 1])] = 0
    launch.update(match_count=count, stats=stats, mask=mask)
    extra = {(2 * p, 2 * p + 1): arr["verified"][(2 * p, 2 * p + 1)][2] for p in moved}
    keypoints = [Keypoints(x) for x in arr["xy"]]
    fallback = VerifiedScene(keypoints, arr["putative"], dict(arr["verified"]), scene.feats, [launch], extra)
    new = fallback.two_view(opt, cals)
    assert fallback.extra is extra and new.extra is not extra and set(new.extra) == set(extra)
    surviving = {}
    for p, name in enumerate(names):
        edge = (2 * p, 2 * p + 1)
        a, b = inside.verified[edge], new.verified[edge]
        assert new.two_view_stats[edge]["supported"] == inside.two_view_stats[edge]["supported"], name
        assert new.two_view_stats[edge].get("host_fallback", False) == (p in moved), name
        np.testing.assert_array_equal(np.asarray(a[2]), np.asarray(b[2]), err_msg=name)
        assert np.asarray(a[2]).shape == np.asarray(b[2]).shape and (a[0] is None) == (b[0] is None) and a[3] == b[3], name
        if a[0] is not None:
            np.testing.assert_allclose(np.asarray(b[0]), np.asarray(a[0]), rtol=0, atol=1e-9, err_msg=name)
            np.testing.assert_allclose(np.asarray(b[1]), np.asarray(a[1]), rtol=0, atol=1e-9, err_msg=name)
            if len(b[2]):
                surviving[edge] = np.asarray(b[2], np.int64).reshape(-1, 2)
        if p in moved:
            np.testing.assert_array_equal(np.asarray(new.extra[edge]), np.asarray(b[2]), err_msg=name)
    for name in ("n5", "mostly_outliers", "nan_pose"):
        p = names.index(name)
        r, u, corr, ratio = new.verified[(2 * p, 2 * p + 1)]
        assert r is None and corr.dtype == np.uint64 and corr.shape == (0,) and not new.two_view_stats[(2 * p, 2 * p + 1)]["supported"], name
    assert new.two_view_stats[(2 * names.index("flipped"), 2 * names.index("flipped") + 1)]["status"] == "NONE_TRIANGULATED"
    assert new.two_view_stats[(2 * names.index("n5"), 2 * names.index("n5") + 1)]["status"] == "SKIPPED"
    sizes = [arr["xy"].shape[1]] * arr["xy"].shape[0]
    ref = TR.tracks_reference(surviving, sizes)
    got = new.tracks()
    for k in ("track_off", "image", "kp"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)

    class Cal3Fisheye:
        def K(self):  # noqa: N802
            return np.eye(3)

    bad = list(cals)
    bad[2 * names.index("one_wave")] = Cal3Fisheye()
    with pytest.raises(NotImplementedError, match="Cal3Fisheye"):
        fallback.two_view(opt, bad)
    del torch
