"""Two-way (mutual nearest neighbour) matcher with an optional ratio test, on the MI355X HIP path.

Drop-in for ``gtsfm/frontend/matcher/twoway_matcher.py:17-147``: same enum (``MatchingDistanceType``), class name, constructor
(``distance_type``, ``ratio_test_threshold``) and ``match`` signature and output -- a (K, 2) ``uint32`` array sorted by the 1->2
distance (ties in i1 order), or ``np.array([])`` when either image has no descriptors or nothing matches. Rows holding a NaN are
dropped before matching and the indices mapped back, as the reference does.

The reference runs ``cv.BFMatcher`` on the CPU twice per pair; here one device call computes the pair's distance product once
(exact fp32 MFMA) and reduces it in both directions (``gtsfm_amd/csrc/twoway_kernels.hip``). OpenCV SIFT / ORB / BRISK descriptors
are integer-valued; with max|a|^2 + max|b|^2 < 2^24 (SIFT-128, ORB, BRISK; uint8 rows of D <= 129) every distance is exact, so the
matches and their order follow the contract bit for bit.

Deviation: dtypes OpenCV rejects (``cv2.error`` in the reference) raise ``TypeError`` here.
"""

from __future__ import annotations

from enum import Enum
from typing import Optional, Tuple

import numpy as np

from gtsfm_amd.common.keypoints import Keypoints
from gtsfm_amd.frontend.matcher.matcher_base import MatcherBase
from gtsfm_amd.runtime import twoway_engine as _tw


class MatchingDistanceType(Enum):
    """Type of distance metric to use for matching descriptors."""

    HAMMING = 1
    EUCLIDEAN = 2


def _metric(distance_type) -> int:
    # by value, so that the reference's own enum (same names and values) is accepted too
    value = getattr(distance_type, "value", None)
    if value not in (_tw.HAMMING, _tw.EUCLIDEAN) or getattr(distance_type, "name", None) not in ("HAMMING", "EUCLIDEAN"):
        raise NotImplementedError("The distance type is not in MatchingDistanceType")
    return int(value)


class TwoWayMatcher(MatcherBase):
    """Two way (mutual nearest neighbor) matcher, with optional ratio test (HIP / gfx950)."""

    def __init__(self, distance_type: MatchingDistanceType = MatchingDistanceType.EUCLIDEAN, ratio_test_threshold: Optional[float] = None):
        super().__init__()
        self._distance_type = distance_type
        self._ratio_test_threshold: Optional[float] = ratio_test_threshold
        self._model = None  # lazy: the device engine is built on first use, in the worker

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_model"] = None
        return state

    def __repr__(self) -> str:
        return f"TwoWayMatcher(distance_type={self._distance_type}, ratio_test_threshold={self._ratio_test_threshold})"

    def _ensure_model_loaded(self):
        if self._model is not None:
            return
        from gtsfm_amd.frontend.registry import MODEL_LOAD_LOCK

        with MODEL_LOAD_LOCK:
            if self._model is None:
                self._model = _tw.TwoWayEngine()

    def match(
        self,
        keypoints_i1: Keypoints,  # unused, as in the reference
        keypoints_i2: Keypoints,
        descriptors_i1: np.ndarray,
        descriptors_i2: np.ndarray,
        im_shape_i1: Tuple[int, int, int],
        im_shape_i2: Tuple[int, int, int],
    ) -> np.ndarray:
        """Match descriptor vectors; returns (K, 2) uint32 indices sorted by distance, or ``np.array([])``."""
        descriptors_i1, descriptors_i2 = np.asarray(descriptors_i1), np.asarray(descriptors_i2)
        if descriptors_i1.size == 0 or descriptors_i2.size == 0:
            return np.array([])
        metric = _metric(self._distance_type)
        _tw.check_inputs(descriptors_i1, descriptors_i2, metric)
        valid_i1 = np.nonzero(~(np.isnan(descriptors_i1).any(axis=1)))[0]
        valid_i2 = np.nonzero(~(np.isnan(descriptors_i2).any(axis=1)))[0]
        _tw.check_ratio_sizes(len(valid_i1), len(valid_i2), self._ratio_test_threshold)
        if len(valid_i1) == 0 or len(valid_i2) == 0:
            return np.array([])
        self._ensure_model_loaded()
        match_indices = self._model.match_pair(descriptors_i1[valid_i1], descriptors_i2[valid_i2], metric, self._ratio_test_threshold)
        if match_indices.size == 0:
            return np.array([])
        match_indices[:, 0] = valid_i1[match_indices[:, 0]]
        match_indices[:, 1] = valid_i2[match_indices[:, 1]]
        return match_indices
