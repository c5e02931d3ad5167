"""Verifier-stage oracle (``oracle/verifier_oracle.py``) and host logic, CPU only.

PARITY UNPINNED towards OpenCV (see the oracle's header). What can be checked without it: the restated mathematics against
independent numpy implementations (LAPACK SVD / eigenvalues / roots), the geometric definition of the solver's output, and
the reference's own verifier contract suite (``tests/frontend/verifier/test_verifier_base.py``) run on the oracle."""

import pickle

import numpy as np
import pytest

from gtsfm_amd.utils import synthetic
from oracle import verifier_oracle as vo


def _angle(r_a, r_b):
    return np.degrees(np.arccos(np.clip((np.trace(r_a.T @ r_b) - 1) / 2, -1, 1)))


def _normalised_scene(m, outliers=0.0, noise=0.0, seed=0):
    s = synthetic.synthetic_two_view_matches(m, outliers, noise, seed=seed)
    n1 = vo.normalize_pinhole(s["coordinates_i1"], *s["intrinsics"])[s["match_indices"][:, 0]]
    n2 = vo.normalize_pinhole(s["coordinates_i2"], *s["intrinsics"])[s["match_indices"][:, 1]]
    return s, n1, n2


def test_sampler_is_distinct_deterministic_and_covers_tiny_sets():
    idx = vo.sample_indices(7, np.arange(512), 50)
    assert idx.shape == (512, 5) and all(len(set(r)) == 5 for r in idx.tolist())
    np.testing.assert_array_equal(idx, vo.sample_indices(7, np.arange(512), 50))
    assert (idx != vo.sample_indices(8, np.arange(512), 50)).any()
    tiny = vo.sample_indices(0, np.arange(256), 5)  # five of five: every draw must terminate
    assert all(sorted(r) == [0, 1, 2, 3, 4] for r in tiny.tolist())
    assert np.bincount(idx.reshape(-1), minlength=50).min() > 20  # roughly uniform


def test_root_finder_against_companion_matrix_eigenvalues():
    rng = np.random.default_rng(0)
    polys = rng.normal(size=(64, 11))
    polys[:8, 10] *= 1e-3  # large roots
    roots, count = vo.real_roots_deg10(polys)
    for k in range(64):
        ref = np.roots(polys[k][::-1])
        ref = np.sort(ref[np.abs(ref.imag) < 1e-7 * np.maximum(1, np.abs(ref.real))].real)
        assert count[k] == len(ref)
        np.testing.assert_allclose(roots[k, : count[k]], ref, rtol=1e-8, atol=1e-10)


def test_five_point_solutions_satisfy_their_definition_and_contain_the_truth():
    rng = np.random.default_rng(3)  # exact double-precision projections (the float32 pixel tables of the scenes round them)
    pts = np.stack([rng.uniform(-4, 4, 200), rng.uniform(-3, 3, 200), rng.uniform(6, 14, 200)], 1)
    rot = synthetic._rotation_about(rng.normal(size=3), 0.25)
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    p2 = pts @ rot.T + t
    n1, n2 = pts[:, :2] / pts[:, 2:], p2[:, :2] / p2[:, 2:]
    idx = vo.sample_indices(0, np.arange(64), 200)
    models, count = vo.five_point_models(n1[idx], n2[idx])
    e_true = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ rot
    e_true /= np.linalg.norm(e_true)
    assert count.min() >= 1 and count.max() <= 10
    found = []
    for h in range(64):
        closest = np.inf
        for r in range(count[h]):
            e = models[h, r] / np.linalg.norm(models[h, r])
            for k in idx[h]:  # epipolar constraint on the sample
                assert abs(np.array([*n2[k], 1.0]) @ e @ np.array([*n1[k], 1.0])) < 1e-9
            assert abs(np.linalg.det(e)) < 1e-5 and np.abs(2 * e @ e.T @ e - np.trace(e @ e.T) * e).max() < 1e-5  # ill-conditioned samples
            closest = min(closest, np.abs(e - e_true).max(), np.abs(e + e_true).max())
        found.append(closest)
        assert np.isnan(models[h, count[h] :]).all()
    # accuracy profile of the solver in double precision (1024 samples: median 1e-14, 95 % below 3e-10, 0.5 % of the
    # minimal samples ill-conditioned enough to lose the true solution) -- a RANSAC hypothesis generator, not a refiner
    assert np.median(found) < 1e-10 and (np.array(found) < 1e-6).mean() >= 0.9


def test_sampson_error_against_its_textbook_form():
    rng = np.random.default_rng(1)
    f = rng.normal(size=(3, 3))
    x1, x2 = rng.normal(size=(20, 2)), rng.normal(size=(20, 2))
    h1, h2 = np.c_[x1, np.ones(20)], np.c_[x2, np.ones(20)]
    l2, l1 = h1 @ f.T, h2 @ f  # verification.py:213-220
    ref = np.square(np.sum(h1 * l1, 1)) / (np.sum(np.square(l1[:, :2]), 1) + np.sum(np.square(l2[:, :2]), 1))
    np.testing.assert_allclose(vo.sampson_sq(f, x1, x2), ref, rtol=1e-12)


def test_sampson_error_reproduces_the_references_known_answers():
    """The residual the verifier scores hypotheses with, against the numbers the REFERENCE'S OWN tests hold for
    ``compute_epipolar_distances_sq_sampson`` (tests/utils/test_verification_utils.py:81-110: a hand-computed case and an Argoverse
    fundamental matrix) -- the one golden vector the reference has on this stage."""
    f = np.array([[0.0, 1, 1], [1, 0, 0], [1, 0, 0]])
    got = vo.sampson_sq(f, np.array([[1.0, 3.5], [-2.0, 2.0]]), np.array([[2.0, -1.0], [1.0, 0.0]]))
    np.testing.assert_allclose(got, [81 / (21.25 + 4.0), 1 / (13.0 + 2.0)], rtol=1e-12)
    f = np.array([[7.41572822e-09, 4.26005557e-07, -2.61114657e-04], [-4.92270651e-07, 4.29568438e-09, 6.95083578e-04],
                  [2.89444929e-04, -1.49345006e-05, -4.01395060e-01]])
    got = vo.sampson_sq(f, np.array([[1553.0, 622], [1553, 622]]), np.array([[357.0, 662], [818, 517]]))
    np.testing.assert_allclose(got, [6.744895e-01, 2.397196e03], rtol=1e-3)  # the reference's own tolerance


def test_coordinate_normalisation_reproduces_the_references_known_answer():
    """``feature_utils.normalize_coordinates`` on a distortion-free ``Cal3Bundler(fx=100, u0=20, v0=30)``, the numbers of the reference's
    tests/utils/test_feature_utils.py:14-23 -- the first thing ``OpencvVerifierBase.verify`` does with the keypoints (opencv_verifier_base.py:74-75)."""
    got = vo.normalize_pinhole(np.array([[10.0, 20.0], [25.0, 12.0], [30.0, 33.0]]), 100.0, 100.0, 20.0, 30.0)
    np.testing.assert_allclose(got, [[-0.1, -0.1], [0.05, -0.18], [0.1, 0.03]], rtol=1e-12, atol=1e-15)


def test_sampson_error_equals_the_reference_function_run_live():
    """``gtsfm/utils/verification.py:172-220`` itself on 300 seeded correspondences under 20 seeded matrices: the oracle's explicit IEEE sequence
    agrees to 1e-9 relative. The reference's answers are recorded in ``tests/golden/reference_sampson_sq.npz``; where the reference tree is
    mounted the function also runs live (imported in a subprocess, gtsam / cv2 replaced by inert stand-ins: the function is numpy only) and
    must give the recorded answers."""
    import os
    from pathlib import Path

    from conftest import GOLDEN

    reference = Path(os.environ.get("GTSFM_REFERENCE", "/root/reference"))
    rng = np.random.default_rng(23)
    fs = rng.normal(size=(20, 3, 3))
    x1, x2 = rng.uniform(0, 1000, size=(300, 2)), rng.uniform(0, 1000, size=(300, 2))
    recorded = np.load(GOLDEN / "reference_sampson_sq.npz")["sampson_sq"]
    if not (reference / "gtsfm" / "utils" / "verification.py").exists():
        ref = recorded
    else:
        ref = _reference_sampson_run_live(reference, fs, x1, x2)
        np.testing.assert_array_equal(ref, recorded)
    # (the reference forms x1 . (F^T x2), the oracle x2 . (F x1): the same number up to cancellation in near-epipolar cases -- 4e-12 observed)
    np.testing.assert_allclose(vo.sampson_sq(fs, x1, x2), ref, rtol=1e-9)


def _reference_sampson_run_live(reference, fs, x1, x2):
    import json
    import subprocess
    import sys

    from conftest import REPO

    code = (
        "import json, sys\nimport numpy as np\n"
        f"sys.path.insert(0, {str(REPO / 'oracle')!r}); sys.path.insert(0, {str(REPO)!r})\n"
        "from validate_cache_against_reference import _AbsentPackages\n"
        "sys.meta_path.insert(0, _AbsentPackages())\n"
        f"sys.path.insert(0, {str(reference)!r})\n"
        "import gtsfm.utils.verification as V\n"
        "d = json.loads(sys.stdin.read())\n"
        "x1, x2 = np.array(d['x1']), np.array(d['x2'])\n"
        "print(json.dumps([V.compute_epipolar_distances_sq_sampson(x1, x2, np.array(f)).tolist() for f in d['fs']]))\n"
    )
    run = subprocess.run([sys.executable, "-c", code], input=json.dumps({"x1": x1.tolist(), "x2": x2.tolist(), "fs": fs.tolist()}), capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    return np.array(json.loads(run.stdout.strip().splitlines()[-1]))


def test_decomposition_against_lapack_svd():
    rng = np.random.default_rng(2)
    for _ in range(20):
        rot = synthetic._rotation_about(rng.normal(size=3), rng.uniform(0.05, 1.0))
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        e = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ rot * rng.uniform(0.1, 10)
        r1, r2, tt = vo.decompose_essential(e)
        u, sv, vt = np.linalg.svd(e)
        assert abs(sv[0] - sv[1]) < 1e-9 * sv[0] and sv[2] < 1e-9 * sv[0]
        for r in (r1, r2):
            assert abs(np.linalg.det(r) - 1) < 1e-12 and np.abs(r @ r.T - np.eye(3)).max() < 1e-12
        assert min(np.abs(r1 - rot).max(), np.abs(r2 - rot).max()) < 1e-9
        assert min(np.abs(tt - t).max(), np.abs(tt + t).max()) < 1e-9


@pytest.mark.parametrize("m,outliers,noise,thr", [(60, 0.0, 0.0, 0.5), (300, 0.4, 0.5, 2.0), (300, 0.65, 0.5, 4.0)])
def test_ransac_recovers_planted_geometry(m, outliers, noise, thr):
    s = synthetic.synthetic_two_view_matches(m, outliers, noise, seed=5, num_extra_keypoints=40)
    res = vo.verify(s["coordinates_i1"], s["coordinates_i2"], s["match_indices"], s["intrinsics"], s["intrinsics"], thr, seed=9)
    assert (res["mask"] & s["is_inlier"]).sum() >= 0.9 * s["is_inlier"].sum()
    assert (res["mask"] & ~s["is_inlier"]).sum() <= 0.05 * m
    assert _angle(res["R"], s["i2Ri1"]) < 2.0 and abs(np.linalg.det(res["R"]) - 1) < 1e-9
    assert res["hypotheses"] in (512, 768, 1024, 1280)  # 1-4 rounds + the local-optimisation round
    if outliers == 0.0:
        assert res["hypotheses"] == 512 and res["mask"].all()  # (1 - 1)^256 <= 1e-6 after the first round
    np.testing.assert_array_equal(res["v_corr_idxs"], s["match_indices"][res["mask"]])
    assert res["inlier_ratio"] == res["mask"].mean()


def test_seven_point_solutions_and_the_fundamental_mode():
    """Seven-point solver: every solution is singular and satisfies the epipolar constraint on its sample; the planted F is
    among them. Fundamental-mode RANSAC on pixel coordinates recovers the planted geometry through E = K2^T F K1."""
    s = synthetic.synthetic_two_view_matches(200, seed=1)
    p1 = s["coordinates_i1"].astype(np.float64)[s["match_indices"][:, 0]]
    p2 = s["coordinates_i2"].astype(np.float64)[s["match_indices"][:, 1]]
    idx = vo.sample_indices(0, np.arange(128), 200, 7)
    assert idx.shape == (128, 7) and all(len(set(r)) == 7 for r in idx.tolist())
    models, count = vo.seven_point_models(p1[idx], p2[idx])
    fx, fy, cx, cy = s["intrinsics"]
    k_inv = np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]))
    t = s["i2Ui1"]
    f_true = k_inv.T @ (np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ s["i2Ri1"]) @ k_inv
    f_true /= np.linalg.norm(f_true)
    found = []
    for h in range(128):
        assert 1 <= count[h] <= 3
        closest = np.inf
        for r in range(count[h]):
            f = models[h, r] / np.linalg.norm(models[h, r])
            assert abs(np.linalg.det(f)) < 1e-9
            for k in idx[h]:
                assert abs(np.array([*p2[k], 1.0]) @ f @ np.array([*p1[k], 1.0])) < 1e-7
            closest = min(closest, np.abs(f - f_true).max(), np.abs(f + f_true).max())
        found.append(closest)
    assert np.median(found) < 1e-6  # pixel coordinates rounded to float32 (3e-5 px) bound this, not the solver
    err = vo.epipolar_distance_sq_max(f_true, p1, p2)
    assert err.max() < 1e-6  # squared pixels: the planted F explains the float32-rounded projections
    for m, outliers, noise, thr in ((100, 0.0, 0.0, 0.5), (300, 0.5, 0.5, 2.0)):
        s = synthetic.synthetic_two_view_matches(m, outliers, noise, seed=4, num_extra_keypoints=20)
        res = vo.verify(s["coordinates_i1"], s["coordinates_i2"], s["match_indices"], s["intrinsics"], s["intrinsics"], thr, seed=2,
                        use_intrinsics_in_verification=False)
        assert (res["mask"] & s["is_inlier"]).sum() >= 0.9 * s["is_inlier"].sum() and (res["mask"] & ~s["is_inlier"]).sum() <= 0.05 * m
        assert _angle(res["R"], s["i2Ri1"]) < 2.0 and res["F"].shape == (3, 3)
    short = vo.verify(s["coordinates_i1"], s["coordinates_i2"], s["match_indices"][:7], s["intrinsics"], s["intrinsics"], 2.0,
                      use_intrinsics_in_verification=False)
    assert short["R"] is None and short["v_corr_idxs"].size == 0  # fewer than NUM_MATCHES_REQ_F_MATRIX = 8


def test_noise_free_winner_equals_the_eight_point_solution():
    """Independent estimator: on exact correspondences the linear eight-point solution (LAPACK SVD of the 9-column system) and
    the RANSAC winner -- a five-point solution of some minimal sample -- must be the same essential matrix."""
    rng = np.random.default_rng(12)
    pts = np.stack([rng.uniform(-4, 4, 80), rng.uniform(-3, 3, 80), rng.uniform(6, 14, 80)], 1)
    rot = synthetic._rotation_about(rng.normal(size=3), 0.3)
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    p2 = pts @ rot.T + t
    x1, x2 = pts[:, :2] / pts[:, 2:], p2[:, :2] / p2[:, 2:]
    res = vo.ransac_essential(x1, x2, 1e-6, seed=3)
    assert res["mask"].all() and res["hypotheses"] == 512
    a = np.stack([x2[:, 0] * x1[:, 0], x2[:, 0] * x1[:, 1], x2[:, 0], x2[:, 1] * x1[:, 0], x2[:, 1] * x1[:, 1], x2[:, 1], x1[:, 0], x1[:, 1], np.ones(80)], 1)
    e8 = np.linalg.svd(a)[2][-1].reshape(3, 3)
    e5 = res["E"] / np.linalg.norm(res["E"])
    assert min(np.abs(e5 - e8).max(), np.abs(e5 + e8).max()) < 1e-8
    r, tt, _ = vo.recover_pose(res["E"], x1, x2)
    assert np.abs(r - rot).max() < 1e-8 and np.abs(tt - t).max() < 1e-8


def test_polish_lowers_the_cost_and_the_pose_error():
    """Six Gauss-Newton steps on the winner's inliers: the MSAC cost over all matches never goes up (the polished pose is only
    kept when it goes down), the rotation stays a rotation, and over a dozen noisy scenes the pose error shrinks."""
    before, after = [], []
    for seed in range(12):
        s, n1, n2 = _normalised_scene(250, 0.4, 0.7, seed=seed)
        thr = 2.0 / s["intrinsics"][0]
        res = vo.ransac_essential(n1, n2, thr, seed)
        r, t, _ = vo.recover_pose(res["E"], n1[res["mask"]], n2[res["mask"]])
        r2, t2 = vo.polish_pose(r, t, n1, n2, res["mask"])
        assert abs(np.linalg.det(r2) - 1) < 1e-12 and np.abs(r2 @ r2.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.norm(t2) - 1) < 1e-12
        assert vo.msac_cost(vo._essential_from_pose(r2, t2), n1, n2, thr * thr) < res["cost"]
        before.append((_angle(r, s["i2Ri1"]), np.degrees(np.arccos(np.clip(t @ s["i2Ui1"], -1, 1)))))
        after.append((_angle(r2, s["i2Ri1"]), np.degrees(np.arccos(np.clip(t2 @ s["i2Ui1"], -1, 1)))))
        full = vo.verify(s["coordinates_i1"], s["coordinates_i2"], s["match_indices"], s["intrinsics"], s["intrinsics"], 2.0, seed=seed)
        assert full["polished"] and np.abs(full["R"] - r2).max() < 1e-12  # verify() keeps the polished pose
    before, after = np.median(before, axis=0), np.median(after, axis=0)
    assert after[0] < 0.6 * before[0] and after[1] < before[1], (before, after)  # measured: 0.26 -> 0.10 and 0.57 -> 0.50 degrees


def test_reference_contract_suite_on_the_oracle():
    """two-plane scene: pose within 2 degrees and every match verified (test_verifier_base.py:80-99); fewer than six
    matches / empty input: the failure tuple (:117-135, opencv_verifier_base.py:71-80)."""
    from tests.test_verifier_gpu import _two_planes_scene

    uv1, uv2, rot, direction = _two_planes_scene(4, 4)
    matches = np.stack([np.arange(8), np.arange(8)], 1)
    for use_intrinsics in (True, False):  # TestRansacForEssentialMatrix / TestRansacForFundamentalMatrix (test_ransac.py:12-31)
        res = vo.verify(uv1, uv2, matches, (1, 1, 0, 0), (1, 1, 0, 0), 0.5, use_intrinsics_in_verification=use_intrinsics)
        assert _angle(res["R"], rot) < 2 and np.degrees(np.arccos(np.clip(res["t"] @ direction, -1, 1))) < 2
        np.testing.assert_array_equal(res["v_corr_idxs"], matches)
    for bad in (np.zeros((0, 2), dtype=np.int32), np.array([], dtype=np.int32), matches[:5]):
        fail = vo.verify(uv1, uv2, bad, (1, 1, 0, 0), (1, 1, 0, 0), 0.5)
        assert fail["R"] is None and fail["t"] is None and fail["v_corr_idxs"].size == 0 and fail["inlier_ratio"] == 0.0


def test_plugin_constructs_pickles_and_returns_the_failure_tuple_early():
    from gtsfm_amd.common.calibration import PinholeIntrinsics, pinhole_parameters
    from gtsfm_amd.frontend.verifier.ransac import Ransac

    v = pickle.loads(pickle.dumps(Ransac(use_intrinsics_in_verification=True, estimation_threshold_px=4)))
    assert repr(v) == "Ransac__use_intrinsicsTrue_4px"  # verifier_base.py:37-41: the cache / report key of the reference
    f_mode = Ransac(use_intrinsics_in_verification=False, estimation_threshold_px=4)
    assert repr(f_mode) == "Ransac__use_intrinsicsFalse_4px" and f_mode._min_matches == 8  # NUM_MATCHES_REQ_F_MATRIX
    assert pinhole_parameters(PinholeIntrinsics(500.0, 320.0, 240.0)) == (500.0, 500.0, 320.0, 240.0, True)

    class Distorted(PinholeIntrinsics):
        def k1(self):
            return 0.1

    assert pinhole_parameters(Distorted(500.0, 320.0, 240.0))[4] is False

    class Cal3Fisheye(PinholeIntrinsics):  # gtsam's equidistant model (CALIBRATION_TYPE): never ((u - cx) / fx, .), even with k1..k4 = 0
        def k1(self):
            return 0.0

    class Cal3DS2(PinholeIntrinsics):
        def k1(self):
            return 0.0

        def p2(self):
            return self.fy - 500.0

    assert pinhole_parameters(Cal3Fisheye(500.0, 320.0, 240.0))[4] is False
    assert pinhole_parameters(Cal3DS2(500.0, 320.0, 240.0))[4] is True and pinhole_parameters(Cal3DS2(500.0, 320.0, 240.0, fy=501.0))[4] is False
    from gtsfm_amd.common.keypoints import Keypoints

    few = v.verify(Keypoints(np.zeros((9, 2), np.float32)), Keypoints(np.zeros((9, 2), np.float32)), np.zeros((3, 2), np.int64), PinholeIntrinsics(), PinholeIntrinsics())
    assert few[0] is None and few[1] is None and few[2].size == 0 and few[3] == 0.0  # no GPU needed for the early-outs
