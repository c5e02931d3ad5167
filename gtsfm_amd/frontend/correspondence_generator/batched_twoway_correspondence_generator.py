"""GPU-resident correspondence generator for the classical front ends: SIFT or D2-Net + ``TwoWayMatcher`` (+ ``Ransac``).

Same contract as ``DetDescCorrespondenceGenerator`` (``gtsfm/frontend/correspondence_generator/det_desc_correspondence_generator.py:19-87``)
and the same extra method as ``BatchedDetDescCorrespondenceGenerator``: the images of a scene are detected in batches per shape, the
keypoints and descriptors stay in HBM (SIFT's as uint8), every edge of the visibility graph is matched from that table, the kept rows
are ordered by distance on the device (``gtsfm_twoway_order_matches``) and one verifier launch reads them where they lie. Per image
and per edge the results equal the per-call plugins' (``detect_and_describe``, ``TwoWayMatcher.match``, ``Ransac.verify`` with the
seed ``i1 << 32 | i2``).

The work runs in the calling process, which must own a GPU; ``client`` is only used to resolve image futures. SuperPoint has its own
resident path in ``BatchedDetDescCorrespondenceGenerator``.
"""

from __future__ import annotations

from typing import Any, Dict, List, Tuple

import numpy as np

from gtsfm_amd.common.keypoints import Keypoints
from gtsfm_amd.frontend.correspondence_generator.correspondence_generator_base import CorrespondenceGeneratorBase
from gtsfm_amd.frontend.correspondence_generator.verified_scene import VerifiedScene
from gtsfm_amd.frontend.detector_descriptor.d2net import D2NetDetDesc, check_size
from gtsfm_amd.frontend.detector_descriptor.sift import SIFTDetectorDescriptor
from gtsfm_amd.frontend.detector_descriptor.superpoint import SuperPointDetectorDescriptor
from gtsfm_amd.frontend.matcher.twoway_matcher import TwoWayMatcher, _metric
from gtsfm_amd.runtime.twoway_engine import EUCLIDEAN

MAX_VERIFY_PAIRS = 65535  # pairs per verifier call (include/gtsfm_amd.h)


class BatchedTwoWayCorrespondenceGenerator(CorrespondenceGeneratorBase):
    """Batched, GPU-resident {SIFT, D2-Net} + TwoWayMatcher correspondence generation and verification."""

    def __init__(self, matcher: TwoWayMatcher, detector_descriptor: Any, image_batch: int = 8, pair_batch: int = 32) -> None:
        if isinstance(detector_descriptor, SuperPointDetectorDescriptor):
            raise TypeError("BatchedTwoWayCorrespondenceGenerator takes SIFT or D2-Net; SuperPoint's resident path is "
                            "BatchedDetDescCorrespondenceGenerator")
        if not isinstance(detector_descriptor, (SIFTDetectorDescriptor, D2NetDetDesc)):
            raise TypeError("BatchedTwoWayCorrespondenceGenerator needs gtsfm_amd's SIFTDetectorDescriptor or D2NetDetDesc")
        if not isinstance(matcher, TwoWayMatcher):
            raise TypeError("BatchedTwoWayCorrespondenceGenerator needs gtsfm_amd's TwoWayMatcher")
        if _metric(matcher._distance_type) != EUCLIDEAN:
            # the per-call plugin refuses these detectors' float32 descriptors under HAMMING too
            raise TypeError("TwoWayMatcher on SIFT / D2-Net descriptors needs MatchingDistanceType.EUCLIDEAN")
        if image_batch < 1 or pair_batch < 1:
            raise ValueError(f"image_batch and pair_batch must be positive (got {image_batch} and {pair_batch})")
        self._detector_descriptor = detector_descriptor
        self._matcher = matcher
        self._image_batch = int(image_batch)
        self._pair_batch = int(pair_batch)

    def __repr__(self) -> str:
        return f"""
        BatchedTwoWayCorrespondenceGenerator:
           {self._detector_descriptor}
           {self._matcher}
        """

    @staticmethod
    def _resolve(client: Any, images: List[Any]) -> List[Any]:
        if client is not None and len(images) > 0 and hasattr(images[0], "key"):  # Dask futures
            return list(client.gather(list(images)))
        return [im.result() if hasattr(im, "result") else im for im in images]

    def generate_correspondences(
        self, client: Any, images: List[Any], visibility_graph: List[Tuple[int, int]]
    ) -> Tuple[List[Keypoints], Dict[Tuple[int, int], np.ndarray]]:
        keypoints_list, putative, _ = self._detect_and_match(client, images, visibility_graph)
        return keypoints_list, putative

    def generate_correspondences_and_verify(
        self, client: Any, images: List[Any], visibility_graph: List[Tuple[int, int]], camera_intrinsics: List[Any], verifier: Any
    ) -> Tuple[List[Keypoints], Dict[Tuple[int, int], np.ndarray], Dict[Tuple[int, int], Tuple[Any, Any, np.ndarray, float]]]:
        """``generate_correspondences`` followed by the verifier stage of ``TwoViewEstimator.run_2view`` for every edge, with keypoints
        and the ordered match lists staying in HBM between the stages. ``verifier``: a ``gtsfm_amd.frontend.verifier.ransac.Ransac``
        (threshold and estimation mode are read from it); ``camera_intrinsics``: one calibration per image. Returns the keypoints, the
        putative correspondences and, per edge, the verifier's return tuple ``(i2Ri1, i2Ui1, v_corr_idxs, inlier_ratio_est_model)``; edge
        (i1, i2) draws its samples from the seed ``i1 << 32 | i2``. Edges with an empty side, with a calibration that has lens distortion
        or skew, or matched on the host (a NaN descriptor row) fall back to the per-pair plugin call."""
        return self.generate_verified_scene(client, images, visibility_graph, camera_intrinsics, verifier).as_tuple()

    def generate_verified_scene(self, client: Any, images: List[Any], visibility_graph: List[Tuple[int, int]], camera_intrinsics: List[Any],
                                verifier: Any) -> VerifiedScene:
        """``generate_correspondences_and_verify`` that also keeps the handles of what stayed in HBM: the returned ``VerifiedScene`` holds
        the same three objects and builds the scene's feature tracks on the device (``.tracks()`` / ``.tracks_2d()``)."""
        from gtsfm_amd.common.calibration import pinhole_parameters
        from gtsfm_amd.frontend.verifier.ransac import Ransac

        if not isinstance(verifier, Ransac):
            raise TypeError("generate_correspondences_and_verify needs gtsfm_amd's Ransac verifier")
        keypoints_list, putative, state = self._detect_and_match(client, images, visibility_graph)
        params = [pinhole_parameters(c) for c in camera_intrinsics]
        use_intrinsics = bool(verifier._use_intrinsics_in_verification)
        matched = state["matched"]
        pairs = matched["pairs"] if matched is not None else []
        launches: List[Dict[str, Any]] = []
        verified_on_device = set()
        if pairs:
            import torch

            # every edge owns its rows of the capacity layout, so an edge that goes to the host stays in the launch with a count of zero
            on_device = np.array([not use_intrinsics or (params[i][4] and params[j][4]) for i, j in pairs], dtype=bool)
            count = matched["match_count"]
            if not on_device.all():
                count = count * torch.from_numpy(on_device.astype(np.int32)).to(count.device)
            engine = verifier._ensure_engine()
            feats, off = state["feats"], matched["match_off"]
            cap = feats["xy"].shape[1]
            table = feats["xy"].reshape(-1, 2)
            intr = np.array([p[:4] for p in params], dtype=np.float64)
            for a in range(0, len(pairs), MAX_VERIFY_PAIRS):
                part = pairs[a : a + MAX_VERIFY_PAIRS]
                b = a + len(part)
                idx = matched["match_idx"][off[a] : off[b]]
                ver = engine.verify_batch(table, [i * cap for i, _ in part], [j * cap for _, j in part], idx, [o - off[a] for o in off[a : b + 1]],
                                          np.concatenate([intr[[i for i, _ in part]], intr[[j for _, j in part]]], axis=1),
                                          float(verifier._estimation_threshold_px), seeds=[(i << 32) | j for i, j in part], match_count=count[a:b].contiguous(),
                                          use_intrinsics=use_intrinsics)
                ver.update(match_idx=idx, match_off=[o - off[a] for o in off[a : b + 1]], match_count=count[a:b], pairs=part)
                launches.append(ver)
            verified_on_device = {p for p, dev in zip(pairs, on_device) if dev}
        # an empty side, a host-matched edge, or a calibration the device path does not model: the per-pair fallback
        return VerifiedScene.from_launches(keypoints_list, putative, state["feats"], launches, verified_on_device, verifier, camera_intrinsics)

    def _detect_table(self, imgs: List[Any]) -> Dict[str, Any]:
        """The scene's device-resident feature table (``SiftEngine.detect_table`` / ``D2NetEngine.detect_table``)."""
        det = self._detector_descriptor
        arrays = [np.asarray(im.value_array) for im in imgs]
        det._ensure_model_loaded()
        if isinstance(det, SIFTDetectorDescriptor):
            from gtsfm_amd.runtime.sift_engine import check_image

            for a in arrays:
                check_image(a)
            return det._model.detect_table(arrays, det.max_keypoints, [im.mask for im in imgs], image_batch=self._image_batch)
        for a in arrays:
            check_size(a.shape)
        return det._model.detect_table(arrays, det.max_keypoints, image_batch=self._image_batch)

    def _detect_and_match(self, client: Any, images: List[Any], visibility_graph: List[Tuple[int, int]]):
        imgs = self._resolve(client, images)
        matcher = self._matcher
        pairs = [(int(i1), int(i2)) for (i1, i2) in visibility_graph]
        if not imgs:
            return [], {p: np.array([]) for p in pairs}, {"feats": None, "matched": None}
        feats = self._detect_table(imgs)
        counts = feats["count"].cpu().numpy().astype(np.int64)
        keypoints_list = keypoints_from_table(feats, counts)
        matcher._ensure_model_loaded()

        # TwoWayMatcher drops rows that hold a NaN and maps the indices back on the host: an image with such a row (float32 tables only)
        # sends all its edges through the plugin's own match()
        descriptors = feats["descriptors"]
        has_nan = np.zeros(len(imgs), dtype=bool)
        if descriptors.is_floating_point():
            import torch

            valid = torch.arange(descriptors.shape[1], device=descriptors.device)[None, :] < feats["count"][:, None]
            has_nan = (torch.isnan(descriptors).any(dim=2) & valid).any(dim=1).cpu().numpy()
        result: Dict[Tuple[int, int], np.ndarray] = {}
        host_rows: Dict[int, np.ndarray] = {}
        for i1, i2 in pairs:
            if has_nan[i1] or has_nan[i2]:
                for i in (i1, i2):
                    if i not in host_rows:
                        host_rows[i] = descriptors[i, : int(counts[i])].cpu().numpy()
                shapes = [tuple(np.asarray(imgs[i].value_array).shape) for i in (i1, i2)]
                result[(i1, i2)] = matcher.match(keypoints_list[i1], keypoints_list[i2], host_rows[i1], host_rows[i2], shapes[0], shapes[1])
        device_pairs = [p for p in pairs if p not in result]
        matched = matcher._model.match_table_device(descriptors, counts, device_pairs, _metric(matcher._distance_type), matcher._ratio_test_threshold,
                                                    pair_batch=self._pair_batch)
        result.update(matcher._model.matches_to_numpy(matched))
        return keypoints_list, {p: result[p] for p in pairs}, {"feats": feats, "matched": matched}


def keypoints_from_table(feats: Dict[str, Any], counts) -> List[Keypoints]:
    """Per image the first ``count`` rows of the table, in the plugin's own order (strongest first); ``scales`` are SIFT's sizes,
    ``None`` for D2-Net."""
    xy, resp = feats["xy"].cpu().numpy(), feats["responses"].cpu().numpy()
    sizes = feats["sizes"].cpu().numpy() if "sizes" in feats else None
    return [Keypoints(coordinates=xy[i, : int(c)].copy(), scales=None if sizes is None else sizes[i, : int(c)].copy(), responses=resp[i, : int(c)].copy())
            for i, c in enumerate(counts)]
