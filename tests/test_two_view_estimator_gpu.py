"""GPU: the per-pair drop-in ``TwoViewEstimator.run_2view`` against ``VerifiedScene.two_view`` edge by edge on the small batched scene of
tests/test_two_view_scene_gpu.py: equal correspondence arrays and reports, poses within 1e-9 (a pair alone holds only its verified rows,
so its points sit in other lanes than inside the scene's capacity layout: another summation order, not another result); the early
returns of ``bundle_adjust``; the reference's own unit-test case in spirit (five noise-free points, identity calibration: the pose stays
within 1 degree and all five correspondences survive); pass-through with ``bundle_adjust_2view=False``."""

import pickle

import numpy as np
import pytest

from tests import two_view_ba_scenes as scenes
from tests.test_two_view_scene_gpu import MIN_INLIERS, MIN_RATIO, built  # noqa: F401 - the scene fixture

pytestmark = pytest.mark.gpu


class RecordedVerifier:
    """Returns what the scene's verifier launch holds for the pair it is asked about."""

    def __init__(self, verified):
        self.verified, self.edge = verified, None

    def verify(self, keypoints_i1, keypoints_i2, match_indices, camera_intrinsics_i1, camera_intrinsics_i2):
        return self.verified[self.edge]


def make_estimator(verifier, **kw):
    from gtsfm_amd.data_association.point3d_initializer import TriangulationOptions, TriangulationSamplingMode
    from gtsfm_amd.frontend.inlier_support_processor import InlierSupportProcessor
    from gtsfm_amd.two_view_estimator import TwoViewEstimator

    args = dict(verifier=verifier, inlier_support_processor=InlierSupportProcessor(MIN_INLIERS, MIN_RATIO), bundle_adjust_2view=True, eval_threshold_px=4,
                triangulation_options=TriangulationOptions(mode=TriangulationSamplingMode.NO_RANSAC))
    args.update(kw)
    return pickle.loads(pickle.dumps(TwoViewEstimator(**args)))  # pickles before first use


def test_run_2view_equals_the_scene_edge_by_edge(built):  # noqa: F811
    from gtsfm_amd.bundle.two_view_ba import TwoViewOptions
    from gtsfm_amd.common.keypoints import Keypoints

    arr, scene, cals = built["arr"], built["scene"], built["cals"]
    new = scene.two_view(TwoViewOptions(min_num_inliers_est_model=MIN_INLIERS, min_inlier_ratio_est_model=MIN_RATIO), cals)
    estimator = make_estimator(RecordedVerifier(arr["verified"]))
    verifier = estimator._verifier  # the pickled copy the estimator holds
    compared = 0
    for p, name in enumerate(built["names"]):
        edge = (2 * p, 2 * p + 1)
        verifier.edge = edge
        res = estimator.run_2view(Keypoints(arr["xy"][2 * p]), Keypoints(arr["xy"][2 * p + 1]), arr["putative"][edge], cals[2 * p], cals[2 * p + 1])
        r, u, corr, ratio = new.verified[edge]
        if name == "rotation":  # the restatement's one non-decisive pair (tests/test_two_view_ba_gpu.py)
            continue
        np.testing.assert_array_equal(np.asarray(res.v_corr_idxs), np.asarray(corr), err_msg=name)
        assert np.asarray(res.v_corr_idxs).dtype == np.asarray(corr).dtype and np.asarray(res.v_corr_idxs).shape == np.asarray(corr).shape, name
        assert (res.i2Ri1 is None) == (r is None) and (res.i2Ui1 is None) == (u is None), name
        if r is not None:
            np.testing.assert_allclose(np.asarray(res.i2Ri1), np.asarray(r), rtol=0, atol=1e-9, err_msg=name)
            np.testing.assert_allclose(np.asarray(res.i2Ui1), np.asarray(u), rtol=0, atol=1e-9, err_msg=name)
        info = new.two_view_stats[edge]
        assert res.post_isp_report.num_inliers_est_model == (len(corr) if info["supported"] else 0), name
        assert res.pre_ba_report.num_inliers_est_model == len(arr["verified"][edge][2]) and res.pre_ba_report.inlier_ratio_est_model == arr["verified"][edge][3], name
        assert res.post_ba_report.inlier_ratio_est_model == res.pre_ba_report.inlier_ratio_est_model, name  # the reference's hack
        if info["supported"] and arr["verified"][edge][0] is not None:
            assert res.post_isp_report.num_inliers_est_model == info["valid"] and res.post_isp_report is not res.post_ba_report, name
        compared += 1
    assert compared == len(built["names"]) - 1


def test_bundle_adjust_early_returns_and_the_five_point_case(built):  # noqa: F811
    from gtsfm_amd.common.calibration import PinholeCamera, PinholeIntrinsics
    from gtsfm_amd.common.keypoints import Keypoints
    from gtsfm_amd.two_view_estimator import compute_relative_pose_metrics

    estimator = make_estimator(None, inlier_support_processor=None, allow_indeterminate_linear_system=True)
    special = scenes.special_pairs()
    cal = lambda k: PinholeIntrinsics(k[0], k[2], k[3], fy=k[1])  # noqa: E731
    corr = lambda n: np.hstack([np.arange(n).reshape(-1, 1)] * 2)  # noqa: E731
    flipped = special["flipped"]
    args = (Keypoints(flipped["uv1"]), Keypoints(flipped["uv2"]), corr(30), cal(flipped["k1"]), cal(flipped["k2"]))
    r, u, c = estimator.bundle_adjust(*args, None, None, None)
    assert r is None and u is None and c is args[2]
    r, u, c = estimator.bundle_adjust(*args, flipped["R"], flipped["t"], None)  # nothing triangulates: the initial pose, no correspondences
    assert r is flipped["R"] and u is flipped["t"] and c.shape == (0, 2) and c.dtype == np.int32
    with pytest.raises(NotImplementedError, match="relative pose prior"):
        estimator.bundle_adjust(*args, flipped["R"], flipped["t"], object())
    strict = make_estimator(None, inlier_support_processor=None)
    rot = special["rotation"]
    r, u, c = strict.bundle_adjust(Keypoints(rot["uv1"]), Keypoints(rot["uv2"]), corr(40), cal(rot["k1"]), cal(rot["k2"]), rot["R"], rot["t"], None)
    assert r is None and u is None and c.shape == (0, 2)  # an indeterminate system that is not allowed
    # five noise-free points in normalised coordinates (f = 1), started at the true pose
    rng = np.random.default_rng(5)
    pts = np.stack([rng.uniform(-1, 1, 5), rng.uniform(-1, 1, 5), rng.uniform(4, 8, 5)], axis=1)
    r_true, t_true = scenes._rot(np.array([0.02, -0.1, 0.03])), np.array([-1.0, 0.1, 0.05])
    p2 = pts @ r_true.T + t_true
    kp1, kp2 = Keypoints((pts[:, :2] / pts[:, 2:]).astype(np.float32)), Keypoints((p2[:, :2] / p2[:, 2:]).astype(np.float32))
    unit = PinholeIntrinsics(1.0, 0.0, 0.0)
    cams = {0: PinholeCamera(np.eye(3), np.zeros(3), unit), 1: PinholeCamera(r_true.T, -r_true.T @ t_true, unit)}
    indices, tracks = estimator.triangulate_two_view_correspondences(cams, kp1, kp2, corr(5))
    assert indices == [0, 1, 2, 3, 4] and len(tracks) == 5
    r, u, c = estimator.bundle_adjust(kp1, kp2, corr(5), unit, unit, r_true, t_true / np.linalg.norm(t_true), None)
    r_err, u_err = compute_relative_pose_metrics(r, u, cams[0].pose(), cams[1].pose())
    assert r_err <= 1.0 and u_err <= 1.0
    np.testing.assert_array_equal(c, corr(5))


def test_pass_through_without_bundle_adjustment(built):  # noqa: F811
    from gtsfm_amd.common.keypoints import Keypoints

    arr, cals = built["arr"], built["cals"]
    estimator = make_estimator(RecordedVerifier(arr["verified"]), bundle_adjust_2view=False)
    verifier = estimator._verifier  # the pickled copy the estimator holds
    p = built["names"].index("n257")
    verifier.edge = (2 * p, 2 * p + 1)
    res = estimator.run_2view(Keypoints(arr["xy"][2 * p]), Keypoints(arr["xy"][2 * p + 1]), arr["putative"][verifier.edge], cals[2 * p], cals[2 * p + 1])
    old = arr["verified"][verifier.edge]
    assert np.asarray(res.i2Ri1).tobytes() == np.asarray(old[0]).tobytes() and np.asarray(res.i2Ui1).tobytes() == np.asarray(old[1]).tobytes()
    np.testing.assert_array_equal(res.v_corr_idxs, old[2])
    pre, post = res.pre_ba_report, res.post_ba_report
    assert post is not pre and post.v_corr_idxs is pre.v_corr_idxs and post.inlier_ratio_est_model == pre.inlier_ratio_est_model == old[3]
    assert post.num_inliers_est_model == pre.num_inliers_est_model == len(old[2])
    assert res.post_isp_report is not post and res.post_isp_report.num_inliers_est_model == len(old[2])
