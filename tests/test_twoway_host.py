"""CPU: the TwoWayMatcher contract -- the restatement in tests/twoway_reference.py against the reference's known answers and the
recorded Lund-door expectations, its properties on seeded data, and the plugin's host side (laziness, pickling, registration,
input validation, config) -- none of which needs a GPU."""

import importlib
import pickle

import numpy as np
import pytest
import yaml

from tests.conftest import GOLDEN, REPO
from tests.twoway_reference import HAMMING, twoway_match

# gtsfm/tests/frontend/matcher/test_twoway_with{,out}ratiotest_matcher.py (known answers, as data)
DESC_1 = np.array([0.4865, 0.3752, 0.3077, 0.9188, 0.7837, 0.1083, 0.6822, 0.3764, 0.2288, 0.8018, 1.1]).reshape(-1, 1).astype(np.float32)
DESC_2 = np.array([0.9995, 0.3376, 0.9005, 0.5382, 0.3162, 0.7974, 0.1785, 0.3491, 0.8658, 0.2912]).reshape(-1, 1).astype(np.float32)
EXPECTED_RATIO_0_8 = [[9, 5], [2, 4], [3, 2], [0, 3]]
EXPECTED_NO_RATIO = [[9, 5], [2, 4], [3, 2], [1, 7], [8, 6], [0, 3]]


def test_restatement_reproduces_the_reference_known_answers():
    for ratio, expected in ((0.8, EXPECTED_RATIO_0_8), (None, EXPECTED_NO_RATIO)):
        got = twoway_match(DESC_1, DESC_2, ratio=ratio)
        assert got.dtype == np.uint32
        np.testing.assert_array_equal(got, np.array(expected))


def test_restatement_reproduces_the_lund_door_fixture():
    f = np.load(GOLDEN / "twoway_lund_door_sift.npz")
    d0, d1 = f["descriptors_0"].astype(np.float32), f["descriptors_1"].astype(np.float32)
    assert d0.shape == d1.shape == (5000, 128)
    # exactness premise: every squared distance fits fp32's integer range
    assert (d0.astype(np.float64) ** 2).sum(1).max() + (d1.astype(np.float64) ** 2).sum(1).max() < 2**24
    np.testing.assert_array_equal(twoway_match(d0, d1, ratio=0.8), f["expected_ratio_0_8"])
    np.testing.assert_array_equal(twoway_match(d0, d1, ratio=None), f["expected_no_ratio"])
    assert f["expected_ratio_0_8"].dtype == np.uint32 and len(f["expected_ratio_0_8"]) > 1000


def _check_properties(m, d1, d2, metric=2):
    from tests.twoway_reference import float32_distances, squared_distances

    assert m.dtype == np.uint32 and m.ndim == 2 and m.shape[1] == 2
    assert len(np.unique(m[:, 0])) == len(m) and len(np.unique(m[:, 1])) == len(m)  # one-to-one
    dist = float32_distances(squared_distances(d1[m[:, 0]], d2[m[:, 1]], metric).diagonal().copy(), metric)
    assert np.all(np.diff(dist) >= 0)  # sorted by distance
    ties = np.flatnonzero(np.diff(dist) == 0)
    assert np.all(m[ties, 0] < m[ties + 1, 0])  # ties in row order


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_properties_on_seeded_integer_data(seed):
    rng = np.random.default_rng(seed)
    d1 = rng.integers(0, 4, size=(120, 8)).astype(np.float32)  # coarse values: many exact ties
    d2 = np.concatenate([d1[:30], rng.integers(0, 4, size=(70, 8)).astype(np.float32)])  # zero-distance duplicates
    for ratio in (None, 0.8, 1.0):
        _check_properties(twoway_match(d1, d2, ratio=ratio), d1, d2)
    # the inclusive 0 <= r * 0 case: a row with two zero-distance partners passes the ratio test
    a = np.array([[0.0, 0.0], [5.0, 5.0]], dtype=np.float32)
    b = np.array([[20.0, 20.0], [0.0, 0.0], [0.0, 0.0]], dtype=np.float32)
    np.testing.assert_array_equal(twoway_match(a, b, ratio=0.8), np.array([[0, 1]]))


def test_restatement_hamming_properties():
    rng = np.random.default_rng(5)
    d1 = rng.integers(0, 256, size=(90, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, size=(80, 32), dtype=np.uint8)
    m = twoway_match(d1, d2, HAMMING, ratio=None)
    _check_properties(m, d1, d2, HAMMING)


def test_restatement_nan_rows_and_empty_conventions():
    rng = np.random.default_rng(3)
    d1 = rng.integers(0, 50, size=(40, 4)).astype(np.float32)
    d2 = rng.integers(0, 50, size=(30, 4)).astype(np.float32)
    nan1, nan2 = [3, 17, 39], [0, 11]
    e1, e2 = d1.copy(), d2.copy()
    e1[nan1, 1] = np.nan
    e2[nan2, 3] = np.nan
    got = twoway_match(e1, e2, ratio=0.9)
    keep1, keep2 = np.setdiff1d(np.arange(40), nan1), np.setdiff1d(np.arange(30), nan2)
    inner = twoway_match(d1[keep1], d2[keep2], ratio=0.9)
    np.testing.assert_array_equal(got, np.stack([keep1[inner[:, 0]], keep2[inner[:, 1]]], 1))
    for empty in (np.array([]), np.zeros((0, 4), np.float32)):
        out = twoway_match(empty, d2)
        assert out.shape == (0,) and out.dtype == np.float64
    with pytest.raises(ValueError):
        twoway_match(d1, d2[:1], ratio=0.8)
    assert twoway_match(d1, d2[:1], ratio=None).shape == (1, 2)


# ---- the plugin's host side -------------------------------------------------------------------------------------------------


def test_plugin_is_lazy_picklable_registered_and_named_like_the_reference():
    from gtsfm_amd.frontend.matcher.matcher_base import MatcherBase
    from gtsfm_amd.frontend.matcher.twoway_matcher import MatchingDistanceType, TwoWayMatcher

    assert [(m.name, m.value) for m in MatchingDistanceType] == [("HAMMING", 1), ("EUCLIDEAN", 2)]
    m = TwoWayMatcher(ratio_test_threshold=0.8)
    assert m._model is None and isinstance(m, MatcherBase) and type(m).__name__ == "TwoWayMatcher"
    assert m._distance_type is MatchingDistanceType.EUCLIDEAN
    m._model = object()  # stands for a device engine: never pickled
    clone = pickle.loads(pickle.dumps(m))
    assert clone._model is None and clone._ratio_test_threshold == 0.8
    try:
        from gtsfm.frontend.matcher.matcher_base import MatcherBase as _  # type: ignore  # noqa: F401
    except Exception:  # noqa: BLE001
        from gtsfm_amd.frontend.registry import GTSFMProcess

        assert type(GTSFMProcess).get_registry()["TwoWayMatcher"] is TwoWayMatcher


def test_plugin_input_validation_needs_no_gpu():
    from gtsfm_amd.frontend.matcher.twoway_matcher import MatchingDistanceType, TwoWayMatcher

    f = np.zeros((4, 8), np.float32)
    u = np.zeros((4, 8), np.uint8)
    euclid, hamming = TwoWayMatcher(), TwoWayMatcher(MatchingDistanceType.HAMMING)
    for matcher, d1, d2 in [(hamming, f, f), (euclid, f.astype(np.float64), f.astype(np.float64)), (euclid, f, u),
                            (euclid, f.astype(np.int32), f.astype(np.int32)), (euclid, f, np.zeros((4, 6), np.float32))]:
        with pytest.raises(TypeError):
            matcher.match(None, None, d1, d2, (1, 1, 1), (1, 1, 1))
    with pytest.raises(ValueError):
        TwoWayMatcher(ratio_test_threshold=0.8).match(None, None, f, f[:1], (1, 1, 1), (1, 1, 1))
    with pytest.raises(NotImplementedError):
        TwoWayMatcher("L1").match(None, None, f, f, (1, 1, 1), (1, 1, 1))
    for d1, d2 in [(np.array([]), f), (f, np.zeros((0, 8), np.float32))]:
        out = euclid.match(None, None, d1, d2, (1, 1, 1), (1, 1, 1))
        assert out.shape == (0,) and out.dtype == np.float64
    all_nan = np.full((3, 8), np.nan, np.float32)
    assert euclid.match(None, None, all_nan, f, (1, 1, 1), (1, 1, 1)).shape == (0,)
    assert euclid._model is None  # nothing above reached the device


def test_kept_in_distance_order():
    from gtsfm_amd.runtime.twoway_engine import kept_in_distance_order

    m0 = np.array([4, -1, 0, 2, -1, 7], np.int32)
    d0 = np.array([0.5, 0.1, 0.25, 0.5, 0.0, 0.125], np.float32)
    np.testing.assert_array_equal(kept_in_distance_order(m0, d0), np.array([[5, 7], [2, 0], [0, 4], [3, 2]], np.uint32))
    assert kept_in_distance_order(np.full(3, -1, np.int32), np.zeros(3, np.float32)).shape == (0,)


def _instantiate(node):
    if isinstance(node, dict):
        kwargs = {k: _instantiate(v) for k, v in node.items() if k != "_target_"}
        if "_target_" not in node:
            return kwargs
        module, _, name = node["_target_"].rpartition(".")
        return getattr(importlib.import_module(module), name)(**kwargs)
    return node


@pytest.fixture
def sp_weights(tmp_path):
    import torch

    from gtsfm_amd.utils import synthetic

    torch.save(synthetic.synthetic_superpoint_state_dict(), str(tmp_path / "sp.pth"))
    return str(tmp_path / "sp.pth")


def test_configs_instantiate_the_matcher(sp_weights):
    from gtsfm_amd.frontend.correspondence_generator.batched_det_desc_correspondence_generator import BatchedDetDescCorrespondenceGenerator
    from gtsfm_amd.frontend.matcher.twoway_matcher import TwoWayMatcher

    sift = yaml.safe_load((REPO / "gtsfm_amd" / "configs" / "sift_twoway_amd.yaml").read_text())
    node = sift["CorrespondenceGenerator"]["matcher"]["matcher_obj"]
    m = _instantiate(node)
    assert isinstance(m, TwoWayMatcher) and m._ratio_test_threshold == 0.8
    # the detector stays the reference's
    assert sift["CorrespondenceGenerator"]["detector_descriptor"]["detector_descriptor_obj"]["_target_"].startswith("gtsfm.frontend.")
    batched = yaml.safe_load((REPO / "gtsfm_amd" / "configs" / "superpoint_twoway_amd_batched.yaml").read_text())
    node = batched["correspondence_generator"]
    node["detector_descriptor"]["weights_path"] = sp_weights  # the checkpoint's default location is outside the repository
    gen = _instantiate(node)
    assert isinstance(gen, BatchedDetDescCorrespondenceGenerator) and isinstance(gen._matcher, TwoWayMatcher)
    assert gen._matcher._model is None
    pickle.dumps(gen)


def test_batched_generator_refuses_device_verification_of_twoway(sp_weights):
    from gtsfm_amd.frontend.correspondence_generator.batched_det_desc_correspondence_generator import BatchedDetDescCorrespondenceGenerator
    from gtsfm_amd.frontend.detector_descriptor.superpoint import SuperPointDetectorDescriptor
    from gtsfm_amd.frontend.matcher.twoway_matcher import TwoWayMatcher
    from gtsfm_amd.frontend.verifier.ransac import Ransac

    gen = BatchedDetDescCorrespondenceGenerator(TwoWayMatcher(), SuperPointDetectorDescriptor(weights_path=sp_weights))
    with pytest.raises(TypeError, match="TwoWayMatcher"):
        gen.generate_correspondences_and_verify(None, [], [], [], Ransac(True, 2.0))


def test_library_builds_with_the_twoway_entry_points(built_library):
    import ctypes

    lib = ctypes.CDLL(str(built_library))
    assert hasattr(lib, "gtsfm_twoway_match") and hasattr(lib, "gtsfm_twoway_workspace_bytes")
    from gtsfm_amd.runtime import lib as L

    h = L.load()
    pairs = np.array([[0, 5000, 5000, 4800]], np.int32)
    assert h.gtsfm_twoway_workspace_bytes(0, 2, 128, 128, 1, pairs.ctypes.data) > 5000 * 4
    assert h.gtsfm_twoway_workspace_bytes(0, 1, 128, 128, 1, pairs.ctypes.data) == 0  # HAMMING on float32: refused
    assert b"HAMMING" in h.gtsfm_last_error()
    bad = np.array([[0, 0, 5, 3]], np.int32)
    assert h.gtsfm_twoway_workspace_bytes(1, 1, 32, 32, 1, bad.ctypes.data) == 0


def test_workspace_plan_for_batches_beyond_32_bit_partial_offsets(built_library):
    """A batch whose per-pair partials add up past 2^31 entries (10 800 pairs of 5000 x 5000: 40 row blocks x 5000 columns each)
    gets a workspace that holds all of them; a batch the ABI cannot launch is refused with a message, never planned."""
    from gtsfm_amd.runtime import lib as L

    h = L.load()
    one = np.array([[0, 5000, 5000, 5000]], np.int32)
    many = np.ascontiguousarray(np.repeat(one, 10800, axis=0))
    per_pair_min = (40 * 5000 + 5000) * 16  # column partials of 40 row blocks + at least one chunk of row partials, 16 bytes each
    ws_one = h.gtsfm_twoway_workspace_bytes(0, 2, 128, 128, 1, one.ctypes.data)
    ws_many = h.gtsfm_twoway_workspace_bytes(0, 2, 128, 128, len(many), many.ctypes.data)
    assert ws_one >= per_pair_min
    assert ws_many >= 10800 * per_pair_min > (1 << 31) * 16
    too_many = np.ascontiguousarray(np.repeat(one, 65536, axis=0))
    assert h.gtsfm_twoway_workspace_bytes(0, 2, 128, 128, len(too_many), too_many.ctypes.data) == 0
    assert b"65535" in h.gtsfm_last_error()
