"""CPU: the host side of ``BatchedTwoWayCorrespondenceGenerator`` (SIFT / D2-Net + TwoWayMatcher + Ransac kept on the device) -- the two
new entry points' argument checks, the configs, the constructor's refusals, pickling -- and the fixture of the GPU chain test: on four
small overlapping views the contract's distance order differs from the row order and is full of ties, the uint8 cast of SIFT's
descriptors changes no match, and every pair yields a model. None of it needs a GPU."""

import importlib
import itertools
import pickle

import numpy as np
import pytest
import yaml

from tests.conftest import REPO

CONFIGS = REPO / "gtsfm_amd" / "configs"


def _instantiate(node):
    if isinstance(node, dict):
        kwargs = {k: _instantiate(v) for k, v in node.items() if k != "_target_"}
        if "_target_" not in node:
            return kwargs
        module, _, name = node["_target_"].rpartition(".")
        return getattr(importlib.import_module(module), name)(**kwargs)
    return node


def test_library_exports_the_new_entry_points_and_they_reject_bad_arguments(built_library):
    import ctypes

    from gtsfm_amd.runtime import lib as L

    raw = ctypes.CDLL(str(built_library))
    assert hasattr(raw, "gtsfm_twoway_order_matches") and hasattr(raw, "gtsfm_pack_rows_f32_to_u8")
    assert "gtsfm_twoway_order_matches" in L.SIGNATURES and "gtsfm_pack_rows_f32_to_u8" in L.SIGNATURES
    h = L.load()
    p = 0x1000  # never dereferenced: every call below is refused before a launch
    for args, word in (((None, p, p, 1, p, p, None), b"null"), ((p, None, p, 1, p, p, None), b"null"), ((p, p, None, 1, p, p, None), b"null"),
                       ((p, p, p, 1, None, p, None), b"null"), ((p, p, p, 1, p, None, None), b"null"), ((p, p, p, -1, p, p, None), b"-1"),
                       ((p, p, p, 65536, p, p, None), b"65535")):
        assert h.gtsfm_twoway_order_matches(*args) < 0
        assert b"twoway_order_matches" in h.gtsfm_last_error() and word in h.gtsfm_last_error()
    for args, word in (((None, 4, 128, 128, p, 128, p, None), b"null"), ((p, 4, 128, 128, None, 128, p, None), b"null"),
                       ((p, 4, 128, 128, p, 128, None, None), b"null"), ((p, -1, 128, 128, p, 128, p, None), b"sizes"),
                       ((p, 4, 0, 128, p, 128, p, None), b"sizes"), ((p, 4, 128, 127, p, 128, p, None), b"stride"),
                       ((p, 4, 128, 128, p, 127, p, None), b"stride")):
        assert h.gtsfm_pack_rows_f32_to_u8(*args) < 0
        assert b"pack_rows_f32_to_u8" in h.gtsfm_last_error() and word in h.gtsfm_last_error()


@pytest.fixture
def d2_checkpoint(tmp_path):
    import torch

    from tests import d2net_reference as dr

    torch.save({"model": dr.seeded_weights(0)}, str(tmp_path / "d2_tf.pth"))
    return str(tmp_path / "d2_tf.pth")


def test_configs_instantiate_the_generator_and_it_pickles_before_first_use(d2_checkpoint):
    from gtsfm_amd.frontend.correspondence_generator.batched_twoway_correspondence_generator import BatchedTwoWayCorrespondenceGenerator
    from gtsfm_amd.frontend.detector_descriptor import D2NetDetDesc, SIFTDetectorDescriptor
    from gtsfm_amd.frontend.matcher.twoway_matcher import TwoWayMatcher

    for name, cls in (("sift_front_end_amd_batched.yaml", SIFTDetectorDescriptor), ("d2net_twoway_amd_batched.yaml", D2NetDetDesc)):
        node = yaml.safe_load((CONFIGS / name).read_text())["correspondence_generator"]
        assert node["detector_descriptor"]["max_keypoints"] == 5000 and node["matcher"]["ratio_test_threshold"] == 0.8
        if cls is D2NetDetDesc:
            node["detector_descriptor"]["model_path"] = d2_checkpoint  # the checkpoint's default location is outside the repository
        gen = _instantiate(node)
        assert isinstance(gen, BatchedTwoWayCorrespondenceGenerator) and isinstance(gen._detector_descriptor, cls)
        assert isinstance(gen._matcher, TwoWayMatcher) and gen._matcher._ratio_test_threshold == 0.8
        assert gen._matcher._model is None and gen._detector_descriptor._model is None and (gen._image_batch, gen._pair_batch) == (8, 32)
        again = pickle.loads(pickle.dumps(gen))
        assert again._matcher._model is None and again._detector_descriptor._model is None and again._detector_descriptor.max_keypoints == 5000


def test_constructor_refuses_other_detectors_matchers_and_hamming(tmp_path):
    import torch

    from gtsfm_amd.frontend.correspondence_generator.batched_twoway_correspondence_generator import BatchedTwoWayCorrespondenceGenerator
    from gtsfm_amd.frontend.detector_descriptor import SIFTDetectorDescriptor
    from gtsfm_amd.frontend.detector_descriptor.superpoint import SuperPointDetectorDescriptor
    from gtsfm_amd.frontend.matcher.lightglue_matcher import LightGlueMatcher
    from gtsfm_amd.frontend.matcher.twoway_matcher import MatchingDistanceType, TwoWayMatcher
    from gtsfm_amd.utils import synthetic

    torch.save(synthetic.synthetic_superpoint_state_dict(), str(tmp_path / "sp.pth"))
    torch.save(synthetic.synthetic_lightglue_state_dict(num_layers=3), str(tmp_path / "lg.pth"))
    with pytest.raises(TypeError, match="BatchedDetDescCorrespondenceGenerator"):
        BatchedTwoWayCorrespondenceGenerator(TwoWayMatcher(), SuperPointDetectorDescriptor(weights_path=str(tmp_path / "sp.pth")))
    with pytest.raises(TypeError, match="SIFTDetectorDescriptor or D2NetDetDesc"):
        BatchedTwoWayCorrespondenceGenerator(TwoWayMatcher(), object())
    with pytest.raises(TypeError, match="TwoWayMatcher"):
        BatchedTwoWayCorrespondenceGenerator(LightGlueMatcher("superpoint", weights_path=tmp_path / "lg.pth"), SIFTDetectorDescriptor())
    with pytest.raises(TypeError, match="EUCLIDEAN"):
        BatchedTwoWayCorrespondenceGenerator(TwoWayMatcher(MatchingDistanceType.HAMMING), SIFTDetectorDescriptor())
    with pytest.raises(ValueError, match="positive"):
        BatchedTwoWayCorrespondenceGenerator(TwoWayMatcher(), SIFTDetectorDescriptor(), pair_batch=0)
    from gtsfm_amd.frontend.verifier.ransac import Ransac  # noqa: F401  (the verifier type is checked before any device work)

    gen = BatchedTwoWayCorrespondenceGenerator(TwoWayMatcher(ratio_test_threshold=0.8), SIFTDetectorDescriptor(max_keypoints=300))
    with pytest.raises(TypeError, match="Ransac"):
        gen.generate_correspondences_and_verify(None, [], [], [], object())


def test_the_chain_fixture_exercises_ties_inversions_the_uint8_cast_and_the_verifier():
    """The inputs of the GPU chain test, on the CPU restatements: per pair of the 4 views >= 100 matches that are the same for float32
    and uint8 descriptors, >= 20 adjacent equal distances (the tie-break is live), >= 20 row inversions (the distance order is not the
    row order) and a model from the verifier oracle at 1 px."""
    from gtsfm_amd.runtime.twoway_engine import kept_in_distance_order
    from gtsfm_amd.utils import synthetic
    from oracle import verifier_oracle as vo
    from tests import sift_reference as S
    from tests import twoway_reference as T

    views = synthetic.synthetic_overlapping_views(4, 120, 160, seed=9)
    feats = [S.detect_and_describe(v, 300) for v in views]
    for i, j in itertools.combinations(range(4), 2):
        d1, d2 = feats[i][3], feats[j][3]
        assert d1.dtype == np.float32 and np.array_equal(d1, d1.astype(np.uint8).astype(np.float32))
        m = T.twoway_match(d1, d2, T.EUCLIDEAN, 0.8)
        mu = T.twoway_match(d1.astype(np.uint8), d2.astype(np.uint8), T.EUCLIDEAN, 0.8)
        assert m.dtype == mu.dtype and m.shape == mu.shape and np.array_equal(m, mu)
        dist = np.sqrt(((d1[m[:, 0]].astype(np.float64) - d2[m[:, 1]]) ** 2).sum(1)).astype(np.float32)
        ties, inversions = int((np.diff(dist) == 0).sum()), int((np.diff(m[:, 0].astype(np.int64)) < 0).sum())
        intr_i, intr_j = (400.0 + 5 * i, 400.0 + 5 * i, 80.0, 60.0), (400.0 + 5 * j, 400.0 + 5 * j, 80.0, 60.0)
        model = vo.verify(feats[i][0], feats[j][0], m, intr_i, intr_j, 1.0, seed=(i << 32) | j)
        print(f"pair {(i, j)}: {len(m)} matches, {ties} adjacent equal distances, {inversions} row inversions, {len(model['v_corr_idxs'])} verified")
        assert (np.diff(dist) >= 0).all()
        assert len(m) >= 100 and ties >= 20 and inversions >= 20 and model["R"] is not None
        # the engine's host ordering (what the device kernel restates) reproduces the contract's order from the raw per-row output
        matches0 = np.full(len(d1), -1, np.int32)
        dist0 = np.zeros(len(d1), np.float32)
        matches0[m[:, 0]], dist0[m[:, 0]] = m[:, 1].astype(np.int32), dist
        assert np.array_equal(kept_in_distance_order(matches0, dist0), m)
