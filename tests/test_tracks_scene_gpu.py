"""GPU: feature tracks where the verified match lists lie. The four-view SIFT scene of tests/test_batched_twoway_gpu.py (plus its
unrelated view, its fully masked view and its skewed camera) goes through ``generate_verified_scene``; the tracks built on the device
from the verifier's own outputs equal the CPU restatement run on the ``verified`` dict the caller gets, for the whole graph and for an
edge subset, and the edges that were verified on the host (skew, an empty side) come in through ``extra``."""

import itertools

import numpy as np
import pytest

from gtsfm_amd.utils import synthetic
from tests import tracks_reference as TR
from tests.test_batched_twoway_gpu import _assert_same_results, _skewed, views  # noqa: F401  (views: the module's fixture)

pytestmark = pytest.mark.gpu


def _equal(out, ref, rounds):
    c = out["counts"]
    print(c, "restatement:", {k: ref[k] for k in ("tracks", "measurements", "discarded", "components")}, "rounds", rounds)
    assert (c["tracks"], c["measurements"], c["discarded"], c["components"], c["rounds"]) == (ref["tracks"], ref["measurements"], ref["discarded"],
                                                                                             ref["components"], rounds)
    assert all(out[k].dtype == ref[k].dtype and np.array_equal(out[k], ref[k]) for k in ("track_off", "image", "kp"))


def test_verified_scene_builds_the_tracks_of_its_own_verified_dict(gpu_device, views):  # noqa: F811
    from gtsfm_amd.common.calibration import PinholeIntrinsics
    from gtsfm_amd.common.image import Image
    from gtsfm_amd.common.sfm_track import SfmMeasurement, SfmTrack2d
    from gtsfm_amd.frontend.correspondence_generator.batched_twoway_correspondence_generator import BatchedTwoWayCorrespondenceGenerator
    from gtsfm_amd.frontend.correspondence_generator.verified_scene import VerifiedScene
    from gtsfm_amd.frontend.detector_descriptor import SIFTDetectorDescriptor
    from gtsfm_amd.frontend.matcher.twoway_matcher import TwoWayMatcher
    from gtsfm_amd.frontend.verifier.ransac import Ransac

    images = [Image(value_array=v) for v in views] + [Image(value_array=synthetic.synthetic_gray_image(120, 160, seed=77)),
                                                      Image(value_array=views[0].copy(), mask=np.zeros((120, 160), dtype=np.uint8))]
    cams = [PinholeIntrinsics(400.0 + 5 * i, 80.0, 60.0) for i in range(6)]
    cams[3] = _skewed(415.0, 80.0, 60.0)
    edges = list(itertools.combinations(range(4), 2)) + [(0, 4), (0, 5)]
    gen = BatchedTwoWayCorrespondenceGenerator(TwoWayMatcher(ratio_test_threshold=0.8), SIFTDetectorDescriptor(max_keypoints=300), image_batch=4, pair_batch=2)
    scene = gen.generate_verified_scene(None, images, edges, cams, Ransac(True, 1.0))
    assert isinstance(scene, VerifiedScene)
    _assert_same_results(scene.as_tuple(), gen.generate_correspondences_and_verify(None, images, edges, cams, Ransac(True, 1.0)))

    kps, verified = scene.keypoints_list, scene.verified
    sizes = [len(k) for k in kps]
    corr = {e: verified[e][2] for e in edges}
    # the skewed camera's edges and the edge with an empty side were verified per pair on the host: they reach the device through `extra`
    assert set(scene.extra) == {(0, 3), (1, 3), (2, 3), (0, 5)} and scene.extra[(0, 5)].size == 0
    assert sum(len(scene.extra[e]) for e in ((0, 3), (1, 3), (2, 3))) >= 50 and all(np.array_equal(scene.extra[e], corr[e]) for e in scene.extra)

    ref = TR.tracks_reference(corr, sizes)
    out = scene.tracks()
    _equal(out, ref, TR.emulate_rounds(corr, sizes)[1])
    assert ref["tracks"] >= 50 and ref["longest"] >= 3
    uv = np.stack([kps[i].coordinates[k] for i, k in zip(out["image"], out["kp"])])
    assert out["track_uv"].dtype == uv.dtype == np.float32 and out["track_uv"].tobytes() == uv.tobytes()
    without_extra = TR.tracks_reference({e: corr[e] for e in edges if e not in scene.extra}, sizes)
    assert without_extra["measurements"] < ref["measurements"]  # the fallback edges matter to the result

    for subset in ([(0, 1), (1, 2), (1, 3)], [(2, 3)], []):
        sub = {e: corr[e] for e in subset}
        _equal(scene.tracks(edges=subset), TR.tracks_reference(sub, sizes), TR.emulate_rounds(sub, sizes)[1] or 1)
    again = scene.tracks()
    assert all(again[k].tobytes() == out[k].tobytes() for k in ("track_off", "image", "kp", "track_uv"))

    tracks = scene.tracks_2d()
    expected = [SfmTrack2d([SfmMeasurement(int(i), kps[i].coordinates[k]) for i, k in zip(ref["image"][a:b], ref["kp"][a:b])])
                for a, b in zip(ref["track_off"][:-1], ref["track_off"][1:])]
    assert len(tracks) == len(expected) and all(t == e for t, e in zip(tracks, expected))
