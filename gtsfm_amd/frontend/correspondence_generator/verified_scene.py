"""What the batched generators' ``generate_verified_scene`` returns: the three host objects of ``generate_correspondences_and_verify``
plus the handles of what stayed in HBM, so that the next stage -- feature tracks, ``gtsfm/multi_view_optimizer.py:185,199`` -- runs where
the verified match lists lie."""

from __future__ import annotations

from typing import Any, Dict, Iterable, List, Optional, Tuple

import numpy as np

from gtsfm_amd.common.keypoints import Keypoints


class VerifiedScene:
    """``keypoints_list``, ``putative`` and ``verified`` are exactly the return values of ``generate_correspondences_and_verify``.
    ``feats`` is the device feature table (``xy`` [num_images, capacity, 2] float32), ``launches`` the verifier launches' device outputs,
    ``extra`` the verified correspondences of the edges that went through the per-pair fallback (host arrays)."""

    def __init__(self, keypoints_list: List[Keypoints], putative: Dict[Tuple[int, int], np.ndarray], verified: Dict[Tuple[int, int], Tuple[Any, Any, np.ndarray, float]],
                 feats: Optional[Dict[str, Any]], launches: List[Dict[str, Any]], extra: Dict[Tuple[int, int], np.ndarray]) -> None:
        self.keypoints_list = keypoints_list
        self.putative = putative
        self.verified = verified
        self.feats = feats
        self.launches = launches
        self.extra = extra
        self._engine = None

    def as_tuple(self):
        return self.keypoints_list, self.putative, self.verified

    def tracks(self, edges: Optional[Iterable[Tuple[int, int]]] = None) -> Dict[str, Any]:
        """The feature tracks of the verified correspondences (of ``edges`` only, when given: ``filter_corr_by_idx`` followed by
        ``get_2d_tracks``) as CSR arrays on the host: ``track_off`` [T + 1] int64, ``image`` / ``kp`` [S] int32, ``track_uv`` [S, 2]
        float32 gathered from the device's ``xy`` table, and ``counts``. A second call uploads only the edge mask."""
        if self.feats is None:
            return {"track_off": np.zeros(1, np.int64), "image": np.zeros(0, np.int32), "kp": np.zeros(0, np.int32), "track_uv": np.zeros((0, 2), np.float32),
                    "counts": {"tracks": 0, "measurements": 0, "discarded": 0, "components": 0, "rounds": 0}}
        if self._engine is None:
            from gtsfm_amd.runtime.tracks_engine import TracksEngine

            self._engine = TracksEngine(self.feats["xy"].device)
        xy = self.feats["xy"]
        out = self._engine.tracks_from_verified(self.launches, int(xy.shape[1]), int(xy.shape[0]), edges=edges, extra=self.extra, kp_xy=xy.reshape(-1, 2))
        return {"track_off": out["track_off"].cpu().numpy(), "image": out["image"].cpu().numpy(), "kp": out["kp"].cpu().numpy(),
                "track_uv": out["uv"].cpu().numpy(), "counts": out["counts"]}

    def triangulate(self, cameras: Dict[int, Any], options, edges: Optional[Iterable[Tuple[int, int]]] = None, seed: int = 0) -> Dict[str, Any]:
        """Tracks -> triangulation (``DataAssociation.run_triangulation``) with the track arrays staying on the device: the CSR arrays
        that the track builder writes are the triangulation's inputs where they lie. Returns host arrays: ``track_off``, ``image``,
        ``kp``, ``point`` [T, 3], ``avg_error`` [T], ``exit_code`` [T], ``inlier_mask`` [S]."""
        from gtsfm_amd.data_association.point3d_initializer import Point3dInitializer

        if self.feats is None:
            return {"track_off": np.zeros(1, np.int64), "image": np.zeros(0, np.int32), "kp": np.zeros(0, np.int32), "point": np.zeros((0, 3)),
                    "avg_error": np.zeros(0), "exit_code": np.zeros(0, np.int32), "inlier_mask": np.zeros(0, np.uint8)}
        if self._engine is None:
            from gtsfm_amd.runtime.tracks_engine import TracksEngine

            self._engine = TracksEngine(self.feats["xy"].device)
        xy = self.feats["xy"]
        trk = self._engine.tracks_from_verified(self.launches, int(xy.shape[1]), int(xy.shape[0]), edges=edges, extra=self.extra, kp_xy=xy.reshape(-1, 2))
        out = Point3dInitializer(cameras, options, seed=seed, device=xy.device).triangulate_arrays(trk["track_off"], trk["image"], trk["uv"])
        res = {k: trk[k].cpu().numpy() for k in ("track_off", "image", "kp")}
        res.update({k: out[k].cpu().numpy() for k in ("point", "avg_error", "exit_code", "inlier_mask")})
        return res

    def tracks_2d(self, edges: Optional[Iterable[Tuple[int, int]]] = None) -> list:
        """The same tracks as ``SfmTrack2d`` objects over ``keypoints_list``'s coordinates."""
        from gtsfm_amd.data_association.dsf_tracks_estimator import tracks_from_csr

        res = self.tracks(edges)
        return tracks_from_csr(res["track_off"], res["image"], res["kp"], self.keypoints_list)
