"""Track estimators on the MI355X HIP path.

Drop-ins for ``gtsfm/data_association/dsf_tracks_estimator.py:25-93`` and ``cpp_dsf_tracks_estimator.py:26-88``: same class names, same
``run(matches_dict, keypoints_list) -> List[SfmTrack2d]``. Both run ``gtsfm_tracks_from_matches``: the keypoints (image, k) are the
nodes of a union-find, every match row joins two of them, and a component that holds two keypoints of one image is dropped.

Stated rather than hidden: the reference returns the tracks in the iteration order of gtsam's ``DSFMap`` (a ``std::map`` over
``IndexPair``); here the order is a contract -- tracks by their smallest (image, keypoint) member, the measurements of a track by image
ascending -- which is the order the reference's ``test_track_generation`` asserts. ``SfmTrack2d.__eq__`` ignores the order inside a track.
``uv`` is the caller's own ``coordinates[k]`` row (dtype untouched); only indices travel to the device.
"""

from __future__ import annotations

import logging
import time
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from gtsfm_amd.common.keypoints import Keypoints
from gtsfm_amd.common.sfm_track import SfmMeasurement, SfmTrack2d
from gtsfm_amd.data_association.tracks_estimator_base import TracksEstimatorBase

logger = logging.getLogger("gtsfm_amd")


def pack_matches(matches_dict: Dict[Tuple[int, int], np.ndarray], keypoints_list: List[Optional[Keypoints]]):
    """Host marshalling, checked before upload: (match_idx [M, 2] int32, match_off [P + 1], pair_images [P, 2], node_off [I + 1]).
    Empty arrays (``np.array([])``) contribute nothing; an index outside a keypoint table raises ``IndexError``, as numpy indexing does in
    the reference and as ``Ransac.verify`` does here."""
    sizes = [0 if kps is None else int(np.asarray(kps.coordinates).shape[0]) for kps in keypoints_list]
    node_off = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]).astype(np.int64)
    rows, off, pairs = [], [0], []
    for (i1, i2), k_pairs in matches_dict.items():
        m = np.asarray(k_pairs)
        if m.size == 0:
            continue
        if m.ndim != 2 or m.shape[1] != 2:
            raise ValueError(f"matches of pair ({i1}, {i2}) must be a (K, 2) array, got shape {m.shape}")
        i1, i2 = int(i1), int(i2)
        if not (0 <= i1 < len(sizes) and 0 <= i2 < len(sizes)):
            raise IndexError(f"pair ({i1}, {i2}) refers to an image outside the keypoints list of {len(sizes)}")
        if m.min() < 0 or m[:, 0].max() >= sizes[i1] or m[:, 1].max() >= sizes[i2]:
            raise IndexError(f"matches of pair ({i1}, {i2}) refer to keypoints outside the keypoint tables")
        rows.append(m.astype(np.int32))
        off.append(off[-1] + m.shape[0])
        pairs.append((i1, i2))
    match_idx = np.concatenate(rows) if rows else np.zeros((0, 2), dtype=np.int32)
    return match_idx, np.asarray(off, dtype=np.int64), np.asarray(pairs, dtype=np.int32).reshape(-1, 2), node_off


def tracks_from_csr(track_off: np.ndarray, image: np.ndarray, kp: np.ndarray, keypoints_list: List[Keypoints]) -> List[SfmTrack2d]:
    """CSR arrays -> ``SfmTrack2d`` objects whose ``uv`` are rows of the caller's coordinate arrays."""
    coords = [None if kps is None else kps.coordinates for kps in keypoints_list]
    meas = [SfmMeasurement(int(i), coords[i][k]) for i, k in zip(image.tolist(), kp.tolist())]
    off = track_off.tolist()
    return [SfmTrack2d(meas[a:b]) for a, b in zip(off[:-1], off[1:])]


class _DeviceTracksEstimator(TracksEstimatorBase):
    def __init__(self) -> None:
        self._engine = None  # lazy: the object must pickle before first use (Dask scatter)

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_engine"] = None
        return state

    def _ensure_engine(self):
        if getattr(self, "_engine", None) is None:
            from gtsfm_amd.runtime.tracks_engine import TracksEngine

            self._engine = TracksEngine()
        return self._engine

    def run_arrays(self, matches_dict: Dict[Tuple[int, int], np.ndarray], keypoints_list: List[Keypoints]) -> Dict[str, Any]:
        """The tracks as CSR arrays, without Python objects: ``track_off`` [T + 1] int64, ``image`` / ``kp`` [S] int32 (track t owns
        entries track_off[t] .. track_off[t + 1]) and ``counts`` (tracks, measurements, discarded, components, rounds)."""
        import torch

        match_idx, match_off, pair_images, node_off = pack_matches(matches_dict, keypoints_list)
        engine = self._ensure_engine()
        out = engine.tracks_from_device(torch.from_numpy(match_idx).to(engine.device), match_off, pair_images, node_off, num_nodes=int(node_off[-1]))
        return {"track_off": out["track_off"].cpu().numpy(), "image": out["image"].cpu().numpy(), "kp": out["kp"].cpu().numpy(), "counts": out["counts"]}

    def _run(self, matches_dict, keypoints_list) -> Tuple[List[SfmTrack2d], Dict[str, int]]:
        res = self.run_arrays(matches_dict, keypoints_list)
        return tracks_from_csr(res["track_off"], res["image"], res["kp"], keypoints_list), res["counts"]


class DsfTracksEstimator(_DeviceTracksEstimator):
    """Estimates tracks using a disjoint-set forest on the device (``dsf_tracks_estimator.py:25``)."""

    def run(self, matches_dict: Dict[Tuple[int, int], np.ndarray], keypoints_list: List[Keypoints]) -> List[SfmTrack2d]:
        start_time = time.time()
        if not all(kps.coordinates.ndim == 2 for kps in keypoints_list if kps is not None):
            raise Exception("Dimensions for Keypoint coordinates incorrect. Array needs to be 2D")
        tracks, counts = self._run(matches_dict, keypoints_list)
        erroneous_track_pct = counts["discarded"] / counts["components"] * 100 if counts["components"] > 0 else np.nan
        logger.info("DSF Union-Find: %.2f%% of tracks discarded from multiple obs. in a single image." % erroneous_track_pct)
        logger.info("DsfTracksEstimator took %.2f sec. to estimate %d tracks.", time.time() - start_time, len(tracks))
        return tracks


class CppDsfTracksEstimator(_DeviceTracksEstimator):
    """The same estimator under the name ``multi_view_optimizer.get_2d_tracks`` constructs (``cpp_dsf_tracks_estimator.py:26``)."""

    def run(self, matches_dict: Dict[Tuple[int, int], np.ndarray], keypoints_list: List[Keypoints]) -> List[SfmTrack2d]:
        start_time = time.time()
        bad = [f"i={i}: shape={kps.coordinates.shape}," for i, kps in enumerate(keypoints_list) if kps.coordinates.ndim != 2]
        if bad:
            raise ValueError(f"Dimensions for Keypoint coordinates incorrect. Array needs to be 2D, but found {' '.join(bad)}")
        tracks, _ = self._run(matches_dict, keypoints_list)
        logger.info("CppDsfTracksEstimator took %.2f sec. to estimate %d tracks.", time.time() - start_time, len(tracks))
        return tracks


def get_2d_tracks(correspondences: Dict[Tuple[int, int], np.ndarray], keypoints_list: List[Keypoints]) -> List[SfmTrack2d]:
    """``gtsfm/multi_view_optimizer.py:266-268`` with the device estimator."""
    return CppDsfTracksEstimator().run(correspondences, keypoints_list)
