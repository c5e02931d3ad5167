"""GPU: gtsfm_triangulate_tracks_f64 against its specification, tests/triangulation_reference.py.

Exit codes, inlier masks and the RANSAC statistics must be EQUAL (except on tracks the restatement itself marks non-decisive: an error
within 1e-6 px of the threshold, or a rival hypothesis with another inlier set within 1e-6 px of the winner at equal votes; at most
0.1 % of a scene's tracks). Points and average errors are compared within a MEASURED tolerance: 8 x the largest difference between the
restatement run on each track's measurements in forward and in reversed order -- the same mathematics on another rounding path; the
factor covers the device's Givens / one-sided Jacobi solve in place of LAPACK's SVD. For the Lund door that figure is recorded in the
fixture (tools/make_triangulation_fixture.py); for the synthetic scenes it is measured here, on the scene the test uses."""

import itertools

import numpy as np
import pytest

from tests import triangulation_reference as ref
from tests import triangulation_scenes as scenes
from tests.conftest import REPO

pytestmark = pytest.mark.gpu

OUTPUTS = ("point", "avg_error", "exit_code", "inlier_mask", "stats")


@pytest.fixture(scope="module")
def engine(gpu_device):
    from gtsfm_amd.runtime.triangulation_engine import TriangulationEngine

    return TriangulationEngine(gpu_device)


@pytest.fixture(scope="module")
def door():
    return dict(np.load(REPO / "tests" / "golden" / "triangulation_lund_door.npz"))


@pytest.fixture(scope="module")
def small():
    scene = scenes.small_shapes()
    scene["tolerance"] = scenes.reversal_tolerance(scene)
    scene["expected"] = {}  # restatement outputs by options, computed once
    return scene


def run_device(engine, scene, sub=None, **opts):
    off, image, uv = (scene[k] for k in ("track_off", "image", "uv")) if sub is None else sub
    out = engine.triangulate(off, image, uv, scene["cameras"], mode=ref.MODE_NAMES[opts.get("mode", 0)], reproj_error_threshold=opts.get("threshold", np.inf),
                             min_triangulation_angle_deg=opts.get("min_angle_deg", 0.0), num_hypotheses=opts.get("num_hypotheses", 2749), seed=opts.get("seed", 0))
    return {k: out[k].cpu().numpy() for k in OUTPUTS}


def expected(scene, **opts):
    key = tuple(sorted(opts.items()))
    if key not in scene["expected"]:
        scene["expected"][key] = ref.triangulate_tracks(scene["cameras"], scene["track_off"], scene["image"], scene["uv"], **opts)
    return scene["expected"][key]


def assert_matches(out, exp, off, non_decisive, point_rtol, avg_atol, label):
    t = len(off) - 1
    assert non_decisive.sum() <= 0.001 * t, f"{label}: {non_decisive.sum()} non-decisive tracks of {t}"
    keep = ~non_decisive
    keep_meas = np.repeat(keep, np.diff(off))
    ok = keep & (exp["exit_code"] == ref.SUCCESS)
    rel = np.linalg.norm(out["point"][ok] - exp["point"][ok], axis=1) / np.linalg.norm(exp["point"][ok], axis=1)
    fin = keep & np.isfinite(exp["avg_error"])
    dif = np.abs(out["avg_error"][fin] - exp["avg_error"][fin])
    print(f"{label}: {t} tracks, exit codes {np.bincount(exp['exit_code'], minlength=6).tolist()}, left out {int(non_decisive.sum())}; "
          f"point rel max {rel.max(initial=0.0):.3e} (allowed {point_rtol:.3e}), avg error max {dif.max(initial=0.0):.3e} px (allowed {avg_atol:.3e})")
    np.testing.assert_array_equal(out["exit_code"][keep], exp["exit_code"][keep])
    np.testing.assert_array_equal(out["inlier_mask"][keep_meas], exp["inlier_mask"][keep_meas])
    np.testing.assert_array_equal(out["stats"][keep], exp["stats"][keep])
    np.testing.assert_array_equal(np.isnan(out["point"][keep]), np.isnan(exp["point"][keep]))
    np.testing.assert_array_equal(np.isnan(out["avg_error"][keep]), np.isnan(exp["avg_error"][keep]))
    assert rel.max(initial=0.0) <= point_rtol and dif.max(initial=0.0) <= avg_atol


@pytest.mark.parametrize("name,mode", [("no_ransac", ref.NO_RANSAC), ("ransac_uniform", ref.RANSAC_SAMPLE_UNIFORM)])
def test_door_fixture_one_launch(engine, door, name, mode):
    scene = {k: door[k] for k in ("track_off", "image", "uv", "cameras")}
    out = run_device(engine, scene, mode=mode, threshold=float(door[f"{name}_threshold"]), num_hypotheses=int(door[f"{name}_num_hypotheses"]))
    exp = {k: door[f"{name}_{k}"] for k in OUTPUTS}
    assert_matches(out, exp, door["track_off"], door[f"{name}_non_decisive"], float(door[f"{name}_point_rtol"]), float(door[f"{name}_avg_error_atol"]), f"door {name}")
    if mode == ref.NO_RANSAC:
        assert np.where(out["exit_code"] != ref.SUCCESS)[0].tolist() == [3668, 7439]


SMALL_CASES = [dict(mode=ref.NO_RANSAC), dict(mode=ref.NO_RANSAC, threshold=10.0, min_angle_deg=3.0), dict(mode=ref.RANSAC_SAMPLE_UNIFORM, **scenes.LOOSE),
               dict(mode=ref.RANSAC_SAMPLE_UNIFORM, min_angle_deg=3.0, seed=9, **scenes.LOOSE), dict(mode=ref.RANSAC_SAMPLE_BIASED_BASELINE, **scenes.LOOSE),
               dict(mode=ref.RANSAC_TOPK_BASELINES, **scenes.LOOSE), dict(mode=ref.RANSAC_SAMPLE_UNIFORM, threshold=np.inf, num_hypotheses=100)]


@pytest.mark.parametrize("case", range(len(SMALL_CASES)))
def test_small_shapes_against_live_restatement(engine, small, case):
    opts = SMALL_CASES[case]
    exp = expected(small, **opts)
    out = run_device(engine, small, **opts)
    assert_matches(out, exp, small["track_off"], exp["non_decisive"], *small["tolerance"], f"small shapes {opts}")
    lengths = np.diff(small["track_off"])
    assert len(lengths) % 256 != 0 and len(lengths) % 64 != 0 and len(lengths) > 256 and {0, 1, 2, 3, 14, 15, 75} <= set(lengths.tolist())
    if opts["mode"] != ref.NO_RANSAC:  # the sampler ran, and hypothesis segments straddle wave and workgroup boundaries
        hyp = np.concatenate([[0], np.cumsum(exp["stats"][:, 0])])
        assert (exp["stats"][lengths >= 15, 0] == 100).all() and (exp["stats"][lengths == 14, 0] == 91).all()
        assert any(a // 64 != (b - 1) // 64 for a, b in zip(hyp[:-1], hyp[1:]) if b > a) and any(a // 256 != (b - 1) // 256 for a, b in zip(hyp[:-1], hyp[1:]) if b > a)


def test_small_shapes_reach_every_exit_code(small):
    codes = set()
    for opts in SMALL_CASES[:4]:
        codes |= set(expected(small, **opts)["exit_code"].tolist())
    assert codes == {0, 1, 2, 3, 4, 5}


def _subset(scene, tracks):
    off = scene["track_off"]
    sel = np.concatenate([np.arange(off[j], off[j + 1]) for j in tracks] + [np.zeros(0, np.int64)]).astype(np.int64)
    sub_off = np.concatenate([[0], np.cumsum([off[j + 1] - off[j] for j in tracks])]).astype(np.int64)
    return sub_off, scene["image"][sel], scene["uv"][sel], sel


def test_track_of_75_with_the_default_hypothesis_count(engine, small):
    """2 775 pairs > 2 749 hypotheses: the sampler leaves 26 pairs out; one track alone (T = 1)."""
    j = int(np.argmax(np.diff(small["track_off"])))
    off, image, uv, _ = _subset(small, [j])
    opts = dict(mode=ref.RANSAC_SAMPLE_UNIFORM, threshold=10.0, num_hypotheses=2749, seed=4)
    exp = ref.triangulate_tracks(small["cameras"], off, image, uv, **opts)
    out = run_device(engine, small, sub=(off, image, uv), **opts)
    assert exp["stats"][0, 0] == 2749 and exp["exit_code"][0] == ref.SUCCESS and exp["inlier_mask"].sum() == 73
    assert_matches(out, exp, off, exp["non_decisive"], *small["tolerance"], "75 measurements")


def test_empty_track_list_and_bad_arguments(engine, small):
    import torch

    out = engine.triangulate(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros((0, 2), np.float32), small["cameras"], mode="RANSAC_SAMPLE_UNIFORM")
    assert out["point"].shape == (0, 3) and out["exit_code"].numel() == 0 and out["inlier_mask"].numel() == 0
    off = small["track_off"].copy()
    off[5] = off[4] - 1  # not ascending
    with pytest.raises(RuntimeError, match="ascending"):
        engine.triangulate(off, small["image"], small["uv"], small["cameras"])
    with pytest.raises(RuntimeError, match="mode"):
        engine.triangulate(small["track_off"], small["image"], small["uv"], small["cameras"], mode=7)
    with pytest.raises(RuntimeError, match="threshold"):
        engine.triangulate(small["track_off"], small["image"], small["uv"], small["cameras"], reproj_error_threshold=-1.0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", (ref.NO_RANSAC, ref.RANSAC_SAMPLE_UNIFORM, ref.RANSAC_SAMPLE_BIASED_BASELINE))
def test_determinism(engine, small, mode):
    opts = dict(mode=mode, **scenes.LOOSE)
    first, second = run_device(engine, small, **opts), run_device(engine, small, **opts)
    assert all(first[k].tobytes() == second[k].tobytes() for k in OUTPUTS)
    t = len(small["track_off"]) - 1
    order = np.random.default_rng(3).permutation(t)
    off, image, uv, sel = _subset(small, order)
    perm = run_device(engine, small, sub=(off, image, uv), **opts)
    for k in ("point", "avg_error", "exit_code", "stats"):
        assert perm[k].tobytes() == first[k][order].tobytes(), k
    assert perm["inlier_mask"].tobytes() == first["inlier_mask"][sel].tobytes()
    lengths = np.diff(small["track_off"])
    for j in (int(np.argmax(lengths)), int(np.where(lengths == 15)[0][0]), int(np.where(lengths == 3)[0][0])):
        off, image, uv, sel = _subset(small, [j])
        alone = run_device(engine, small, sub=(off, image, uv), **opts)
        assert all(alone[k].tobytes() == first[k][j : j + 1].tobytes() for k in ("point", "avg_error", "exit_code", "stats"))
        assert alone["inlier_mask"].tobytes() == first["inlier_mask"][sel].tobytes()


# ---- hard geometry against the high-precision arbiter; launch structure at scale ----

from tests.test_triangulation_arbiter_host import FAMILIES, held_to_rule  # noqa: E402


@pytest.mark.parametrize("name", list(FAMILIES))
def test_hard_fixture_against_arbiter(engine, name):
    """tests/golden/triangulation_hard_scenes.npz (tools/make_triangulation_hard_fixture.py): parallax, world offset, scale, rank, depth,
    sampler ties and hostile image indices. Discrete outputs equal the arbiter's; cost(x) - cost(minimiser) <= 1e-5 max(1, cost); point
    and average error within 8 x the port-to-arbiter difference of the family."""
    fam = FAMILIES[name]
    held_to_rule(fam, run_device(engine, fam, **fam["options"]), f"device, {name}")


def _interleave(small, long_track, copies):
    """``copies`` x the long track, a short track of the scene after each."""
    lengths = np.diff(small["track_off"])
    short = [int(j) for j in np.where((lengths >= 2) & (lengths <= 4))[0]]
    order = [j for c in range(copies) for j in (long_track, short[c % len(short)])]
    return _subset(small, order)


def test_grid_stride_loop_runs_twice(engine, small):
    """200 copies of the 75-measurement track at the default 2 749 hypotheses, interleaved with short tracks: 549 800 hypotheses and
    more, above the 2048 x 256 lanes of the hypothesis kernel's grid. Every copy is byte-equal to the track launched alone (the launch
    ``test_track_of_75_with_the_default_hypothesis_count`` pins to the restatement)."""
    j = int(np.argmax(np.diff(small["track_off"])))
    opts = dict(mode=ref.RANSAC_SAMPLE_UNIFORM, threshold=10.0, num_hypotheses=2749, seed=4)
    off1, image1, uv1, _ = _subset(small, [j])
    alone = run_device(engine, small, sub=(off1, image1, uv1), **opts)
    off, image, uv, _ = _interleave(small, j, 200)
    out = run_device(engine, small, sub=(off, image, uv), **opts)
    assert alone["stats"][0, 0] == 2749 and out["stats"][:, 0].sum() > 2048 * 256 and out["stats"][::2, 0].sum() == 549800
    for k in ("point", "avg_error", "exit_code", "stats"):
        assert out[k][::2].tobytes() == alone[k].tobytes() * 200, k
    for c in range(200):
        assert out["inlier_mask"][off[2 * c] : off[2 * c + 1]].tobytes() == alone["inlier_mask"].tobytes(), c


def test_rows_do_not_depend_on_the_batch_size(engine, small):
    """Prefixes of the scene around the 64 tracks of a final workgroup and the 256 of a count workgroup, and the scene twice over."""
    off, image, uv = small["track_off"], small["image"], small["uv"]
    for opts in (dict(mode=ref.NO_RANSAC, threshold=10.0, min_angle_deg=3.0), dict(mode=ref.RANSAC_TOPK_BASELINES, **scenes.LOOSE)):
        full = run_device(engine, small, **opts)
        for t in (1, 63, 64, 65, 255, 256, 257):
            part = run_device(engine, small, sub=(off[: t + 1], image[: off[t]], uv[: off[t]]), **opts)
            for k in ("point", "avg_error", "exit_code", "stats"):
                assert part[k].tobytes() == full[k][:t].tobytes(), (t, k)
            assert part["inlier_mask"].tobytes() == full["inlier_mask"][: off[t]].tobytes(), t
        twice = run_device(engine, small, sub=(np.concatenate([off, off[1:] + off[-1]]), np.tile(image, 2), np.tile(uv, (2, 1))), **opts)
        assert len(twice["exit_code"]) == 602
        for k in OUTPUTS:
            assert twice[k].tobytes() == full[k].tobytes() * 2, k


def test_a_call_does_not_depend_on_what_the_workspace_held(gpu_device, small):
    """The cached workspace, sized by a larger call, is filled with 0xFF before a smaller one: the bytes equal a fresh engine's."""
    from gtsfm_amd.runtime.triangulation_engine import TriangulationEngine

    lengths = np.diff(small["track_off"])
    sub = _subset(small, [int(j) for j in np.where(lengths >= 3)[0][:70]])[:3]
    for opts in (dict(mode=ref.NO_RANSAC, threshold=10.0), dict(mode=ref.RANSAC_SAMPLE_UNIFORM, **scenes.LOOSE), dict(mode=ref.RANSAC_TOPK_BASELINES, **scenes.LOOSE)):
        fresh = run_device(TriangulationEngine(gpu_device), small, sub=sub, **opts)
        used = TriangulationEngine(gpu_device)
        run_device(used, small, **dict(opts, num_hypotheses=2749))
        size = used._ws.numel()
        used._ws.fill_(0xFF)
        again = run_device(used, small, sub=sub, **opts)
        assert used._ws.numel() == size  # the same allocation served the smaller call
        assert all(again[k].tobytes() == fresh[k].tobytes() for k in OUTPUTS), opts


def test_longest_track_is_accepted_and_one_more_is_refused(engine, small):
    table = small["cameras"]
    valid = [i for i in range(scenes.NUM_CAMERAS) if i not in scenes.INVALID]
    x = np.array([0.4, -0.7, 0.2])
    pixel = {i: ref.project(table[i], x)[:2] for i in valid}
    for n in (65535, 65536):
        image = np.array([valid[k % len(valid)] for k in range(n)], np.int32)
        uv = np.array([pixel[i] for i in image], np.float32)
        off = np.array([0, n], np.int64)
        if n == 65535:
            out = run_device(engine, small, sub=(off, image, uv), mode=ref.NO_RANSAC)
            assert out["exit_code"][0] == ref.SUCCESS and out["inlier_mask"].all() and out["avg_error"][0] < 1e-3
            np.testing.assert_allclose(out["point"][0], x, rtol=0, atol=1e-5)  # float32 pixels
        else:
            with pytest.raises(RuntimeError, match="longer than"):
                run_device(engine, small, sub=(off, image, uv), mode=ref.NO_RANSAC)


def _circle_cameras():
    from gtsfm_amd.common.calibration import PinholeCamera, PinholeIntrinsics
    from tests.test_triangulation_host import circle_scene

    table, images, uv = circle_scene()
    cams = {i: PinholeCamera(table[i, 5:14].reshape(3, 3), table[i, 14:17], PinholeIntrinsics(50.0)) for i in range(8)}
    return cams, uv


def test_point3d_initializer_known_answers_and_batch_rows(gpu_device):
    from gtsfm_amd.common.sfm_track import SfmMeasurement, SfmTrack2d
    from gtsfm_amd.data_association.data_assoc import run_triangulation
    from gtsfm_amd.data_association.point3d_initializer import Point3dInitializer, TriangulationExitCode, TriangulationOptions, TriangulationSamplingMode

    cams, uv = _circle_cameras()
    full = [SfmMeasurement(i, uv[i]) for i in range(8)]
    outlier = list(full)
    outlier[5] = SfmMeasurement(5, uv[5] + np.array([20.0, -10.0]))
    tracks = [SfmTrack2d(full), SfmTrack2d(full[:2]), SfmTrack2d(full[:1]), SfmTrack2d(outlier), SfmTrack2d(full + [SfmMeasurement(0, uv[0] + np.array([2.0, -3.0]))])]
    for mode in TriangulationSamplingMode:
        options = TriangulationOptions(mode=mode, reproj_error_threshold=5)
        init = Point3dInitializer(cams, options)
        batch = init.triangulate_batch(tracks)
        codes = [r[2] for r in batch]
        ransac = mode != TriangulationSamplingMode.NO_RANSAC
        assert codes == [TriangulationExitCode.SUCCESS, TriangulationExitCode.SUCCESS, TriangulationExitCode.INLIERS_UNDERCONSTRAINED,
                         TriangulationExitCode.SUCCESS if ransac else TriangulationExitCode.EXCEEDS_REPROJ_THRESH, TriangulationExitCode.SUCCESS]
        for j in (0, 1):
            np.testing.assert_allclose(batch[j][0].point3(), np.zeros(3), atol=1e-5)  # float32 pixels
            assert batch[j][0].numberMeasurements() == len(tracks[j].measurements)
        assert batch[2][0] is None and batch[2][1] is None
        if ransac:
            np.testing.assert_allclose(batch[3][0].point3(), np.zeros(3), atol=1e-5)
            assert [batch[3][0].measurement(k)[0] for k in range(batch[3][0].numberMeasurements())] == [0, 1, 2, 3, 4, 6, 7]
        else:
            assert batch[3][0] is None and batch[3][1] > 0
        np.testing.assert_allclose(batch[4][0].point3(), np.zeros(3), atol=1, rtol=0.1)
        for j, track in enumerate(tracks):  # triangulate == row j of triangulate_batch
            one = init.triangulate(track)
            assert one[2] == batch[j][2] and one[1] == batch[j][1]
            assert (one[0] is None) == (batch[j][0] is None) and (one[0] is None or one[0].point3().tobytes() == batch[j][0].point3().tobytes())
        order = [4, 2, 0, 3, 1]
        sfm, errors, exit_codes = run_triangulation(cams, [tracks[j] for j in order], options)
        assert exit_codes == [codes[j] for j in order] and errors == [batch[j][1] for j in order]
        assert [None if s is None else s.point3().tobytes() for s in sfm] == [None if batch[j][0] is None else batch[j][0].point3().tobytes() for j in order]


def test_verified_scene_triangulates_its_own_tracks(gpu_device, views):  # noqa: F811
    from gtsfm_amd.common.calibration import PinholeCamera, PinholeIntrinsics
    from gtsfm_amd.common.image import Image
    from gtsfm_amd.data_association.point3d_initializer import Point3dInitializer, TriangulationOptions, TriangulationSamplingMode
    from gtsfm_amd.frontend.correspondence_generator.batched_twoway_correspondence_generator import BatchedTwoWayCorrespondenceGenerator
    from gtsfm_amd.frontend.detector_descriptor import SIFTDetectorDescriptor
    from gtsfm_amd.frontend.matcher.twoway_matcher import TwoWayMatcher
    from gtsfm_amd.frontend.verifier.ransac import Ransac

    images = [Image(value_array=v) for v in views]
    intrinsics = [PinholeIntrinsics(400.0 + 5 * i, 80.0, 60.0) for i in range(4)]
    edges = list(itertools.combinations(range(4), 2))
    gen = BatchedTwoWayCorrespondenceGenerator(TwoWayMatcher(ratio_test_threshold=0.8), SIFTDetectorDescriptor(max_keypoints=300), image_batch=4, pair_batch=2)
    scene = gen.generate_verified_scene(None, images, edges, intrinsics, Ransac(True, 1.0))
    cams = {i: PinholeCamera(np.eye(3), [0.3 * i, 0.02 * i, 0.0], intrinsics[i]) for i in range(4)}
    for mode in (TriangulationSamplingMode.NO_RANSAC, TriangulationSamplingMode.RANSAC_SAMPLE_UNIFORM):
        options = TriangulationOptions(mode=mode, reproj_error_threshold=50.0, max_num_hypotheses=100)
        out = scene.triangulate(cams, options)
        tracks = scene.tracks_2d()
        t = len(tracks)
        assert t >= 20 and out["point"].shape == (t, 3) and out["exit_code"].shape == (t,) and len(out["inlier_mask"]) == out["track_off"][-1]
        batch = Point3dInitializer(cams, options).triangulate_batch(tracks)
        print(mode.name, "exit codes", np.bincount(out["exit_code"], minlength=6).tolist())
        for j, (sfm, err, code) in enumerate(batch):
            assert code.value == out["exit_code"][j]
            assert (err is None and np.isnan(out["avg_error"][j])) or err == out["avg_error"][j]
            assert (sfm is None and np.isnan(out["point"][j]).all()) or sfm.point3().tobytes() == out["point"][j].tobytes()
            if sfm is not None:
                a, b = out["track_off"][j], out["track_off"][j + 1]
                assert [sfm.measurement(k)[0] for k in range(sfm.numberMeasurements())] == out["image"][a:b][out["inlier_mask"][a:b] != 0].tolist()
        subset = scene.triangulate(cams, options, edges=[(0, 1), (1, 2)])
        assert len(subset["exit_code"]) == len(scene.tracks_2d(edges=[(0, 1), (1, 2)]))


from tests.test_batched_twoway_gpu import views  # noqa: E402,F401  (the four-view SIFT scene, a module fixture there)
