"""What the batched generators' ``generate_verified_scene`` returns: the three host objects of ``generate_correspondences_and_verify``
plus the handles of what stayed in HBM, so that the next stage -- feature tracks, ``gtsfm/multi_view_optimizer.py:185,199`` -- runs where
the verified match lists lie."""

from __future__ import annotations

from functools import cached_property
from typing import Any, Dict, Iterable, List, Optional, Set, Tuple

import numpy as np

from gtsfm_amd.common.keypoints import Keypoints
from gtsfm_amd.frontend.correspondence_generator.scene_edges import SceneEdges
from gtsfm_amd.runtime.engine_base import named
from gtsfm_amd.runtime.tracks_engine import COUNT_FIELDS, TracksEngine
from gtsfm_amd.runtime.two_view_ba_engine import STATS_FIELDS, STATUS_NAMES

FAILURE = (None, None, np.array([], dtype=np.uint64), 0.0)  # VerifierBase._failure_result


def empty_tracks() -> Dict[str, Any]:  # what ``VerifiedScene.tracks`` returns for a scene without rows
    return {"track_off": np.zeros(1, np.int64), "image": np.zeros(0, np.int32), "kp": np.zeros(0, np.int32), "track_uv": np.zeros((0, 2), np.float32),
            "counts": dict.fromkeys(COUNT_FIELDS, 0)}


def empty_triangulation() -> Dict[str, Any]:  # and what ``triangulate`` does
    return {"track_off": np.zeros(1, np.int64), "image": np.zeros(0, np.int32), "kp": np.zeros(0, np.int32), "point": np.zeros((0, 3)), "avg_error": np.zeros(0),
            "exit_code": np.zeros(0, np.int32), "inlier_mask": np.zeros(0, np.uint8)}


def empty_bundle_adjustment() -> Dict[str, Any]:  # and what ``bundle_adjust`` does
    from gtsfm_amd.runtime.global_ba_engine import COST_FIELDS, COUNTER_FIELDS, NO_VALID_ROW

    return {"track_off": np.zeros(1, np.int64), "image": np.zeros(0, np.int32), "kp": np.zeros(0, np.int32), "point": np.zeros((0, 3)), "cameras": np.zeros((0, 17)),
            "track_valid": np.zeros(0, np.uint8), "camera_kept": np.zeros(0, np.uint8), "reproj_error": np.zeros(0), "exit_code": np.zeros(0, np.int32),
            "counters": dict(dict.fromkeys(COUNTER_FIELDS, 0), status=NO_VALID_ROW, anchor=-1), "costs": dict.fromkeys(COST_FIELDS, float("nan")), "status": "NO_VALID_ROW"}


class ViewGraph:
    """What ``VerifiedScene.view_graph`` returns. ``pairs``: the scene's edge rows (the launches' pairs, then the edges of ``extra``);
    ``edges``: the view-graph edges, those every pass kept, in row order; ``pruned_edges``: those of them in the largest connected
    component; ``passes``: per pass its criterion, threshold, counts and the per-row ``num_triplets`` / ``aggregate_error`` / ``keep``;
    ``component``: the component's counts (None without the prune)."""

    def __init__(self, pairs: List[Tuple[int, int]], keep: np.ndarray, pruned: np.ndarray, passes: List[Dict[str, Any]], component: Optional[Dict[str, int]]) -> None:
        self.pairs, self.keep, self.pruned, self.passes, self.component = pairs, keep, pruned, passes, component
        self.edges = [p for p, k in zip(pairs, keep.tolist()) if k]
        self.pruned_edges = [p for p, k in zip(pairs, pruned.tolist()) if k]

    @classmethod
    def empty(cls) -> "ViewGraph":
        """The result for a scene without rows."""
        return cls([], np.zeros(0, np.uint8), np.zeros(0, np.uint8), [], {"nodes": 0, "edges": 0, "components": 0})

    def per_edge(self, index: int = -1) -> Dict[Tuple[int, int], Tuple[int, float, bool]]:
        """(num_triplets, aggregate_error, kept) of pass ``index`` per edge row; a row that did not enter the pass has (0, NaN, False)."""
        res = self.passes[index]
        return {p: (int(n), float(a), bool(k)) for p, n, a, k in zip(self.pairs, res["num_triplets"].tolist(), res["aggregate_error"].tolist(), res["keep"].tolist())}


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
        self.two_view_stats: Dict[Tuple[int, int], Dict[str, Any]] = {}  # filled by two_view()
        self._engines: Dict[type, Any] = {}

    @classmethod
    def from_launches(cls, keypoints_list: List[Keypoints], putative: Dict[Tuple[int, int], np.ndarray], feats: Optional[Dict[str, Any]], launches: List[Dict[str, Any]],
                      on_device: Set[Tuple[int, int]], verifier, camera_intrinsics: List[Any]) -> "VerifiedScene":
        """The scene of the verifier ``launches``: the launches' results as the verifier plugin's tuples for the edges of ``on_device`` (those that
        count as verified on the device), and every other edge of ``putative`` through the per-pair ``Ransac`` (seed ``i1 << 32 | i2``) on the
        host's keypoints; these are the scene's ``extra``."""
        from gtsfm_amd.frontend.verifier.ransac import Ransac, _to_pose_types
        from gtsfm_amd.runtime.pipeline import FrontEndPipeline

        verified, extra = {}, {}
        for pair, res in FrontEndPipeline.verified_to_numpy(launches).items():
            if pair in on_device and res["R"] is None:
                verified[pair] = verifier._failure_result
            elif pair in on_device:
                verified[pair] = (*_to_pose_types(res["R"], res["t"]), res["v_corr_idxs"].astype(putative[pair].dtype), res["inlier_ratio"])
        for pair in putative:
            if pair not in verified:  # an empty side, a host-matched edge, or a calibration the device path does not model
                i1, i2 = pair
                per_pair = Ransac(bool(verifier._use_intrinsics_in_verification), verifier._estimation_threshold_px, seed=(i1 << 32) | i2)
                per_pair._engine = verifier._ensure_engine()  # one lib handle / workspace for every fallback edge
                verified[pair] = per_pair.verify(keypoints_list[i1], keypoints_list[i2], putative[pair], camera_intrinsics[i1], camera_intrinsics[i2])
                extra[pair] = verified[pair][2]
        return cls(keypoints_list, putative, {p: verified[p] for p in putative}, feats, launches, extra)

    def as_tuple(self):
        return self.keypoints_list, self.putative, self.verified

    @cached_property
    def edge_table(self) -> SceneEdges:
        """The scene's edge rows on the device, built on first use (a scene with ``feats``)."""
        return SceneEdges(self.feats, self.launches, self.extra, self.verified)

    def _engine_of(self, cls):
        """The scene's engine of that class, made on first use on the feature table's device."""
        if cls not in self._engines:
            self._engines[cls] = cls(self.feats["xy"].device)
        return self._engines[cls]

    def _tracks_on_device(self, edges: Optional[Iterable[Tuple[int, int]]]) -> Dict[str, Any]:
        """``TracksEngine.tracks_from_verified`` for the scene: device tensors ``track_off``, ``image``, ``kp``, ``uv`` and ``counts``."""
        xy = self.feats["xy"]
        return self._engine_of(TracksEngine).tracks_from_verified(self.launches, int(xy.shape[1]), int(xy.shape[0]), edges=edges, extra=self.extra, kp_xy=xy.reshape(-1, 2))

    def two_view(self, options=None, camera_intrinsics: Optional[List[Any]] = None) -> "VerifiedScene":
        """The rest of ``TwoViewEstimator.run_2view`` for every edge that was verified on the device (``two_view_estimator.py:411-450``):
        two-view bundle adjustment (``gtsfm_two_view_ba_f64``, one call per verifier launch, on the launch's arrays where they lie) and
        the ``InlierSupportProcessor``'s two tests (``inlier_support_processor.py:73-95``: the inlier ratio first, then the inlier
        count of a model that has inliers). Returns a NEW scene; this one is untouched. Its launches carry the refined poses and the
        valid mask in place of the inlier mask (zeroed for edges without support), so ``tracks()`` / ``triangulate()`` on it see what
        the reference's multi-view stage sees, and no correspondence is downloaded for them. ``verified`` holds the post-ISP tuples
        (built from one download per launch) and ``two_view_stats`` the per-edge status, counts and step counts. The reference's hack
        ``post_ba_inlier_ratio = pre_ba_inlier_ratio`` (``:423-426``) is kept. ``options``: ``gtsfm_amd.bundle.two_view_ba.TwoViewOptions``;
        ``camera_intrinsics``: a calibration per image (a non-pinhole one raises ``NotImplementedError``, for an edge of ``extra`` as well)."""
        from gtsfm_amd.bundle.two_view_ba import TwoViewOptions

        opt = options or TwoViewOptions()
        on_device = self.feats is not None and bool(self.launches)
        if opt.bundle_adjust_2view and camera_intrinsics is None and (on_device or self.extra):
            raise ValueError("two_view needs camera_intrinsics for the bundle adjustment")
        verified = dict(self.verified)
        stats_by_edge, launches, poses = {}, [], {}  # per edge its stats; the new launch dicts; per edge its (rotation, direction) on the host
        if on_device:
            ba = opt.optimizer() if opt.bundle_adjust_2view else None
            for ver in self.launches:
                launches.append(self._two_view_launch(ver, opt, ba, camera_intrinsics, stats_by_edge, poses))
            verified.update(self._two_view_verified(launches, poses, stats_by_edge))
        extra = self._two_view_extra(opt, camera_intrinsics, verified, stats_by_edge) if self.extra else {}
        scene = VerifiedScene(self.keypoints_list, self.putative, verified, self.feats, launches if launches else list(self.launches), extra)
        scene.two_view_stats = stats_by_edge
        return scene

    def _two_view_launch(self, ver: Dict[str, Any], opt, ba, camera_intrinsics, stats_by_edge, poses) -> Dict[str, Any]:
        """``two_view`` for one verifier launch, on the device: returns the new launch dict and adds per edge its stats to ``stats_by_edge`` and its
        (rotation, direction) on the host to ``poses``. ``ba``: the options' optimizer, None when the adjustment is off and the verifier's result
        passes through."""
        import torch

        xy = self.feats["xy"]
        cap, col = int(xy.shape[1]), STATS_FIELDS.index
        pairs = [tuple(p) for p in ver["pairs"]]
        pre = ver["stats"][:, 0].cpu().numpy().astype(np.int64)  # the verifier's inlier counts
        if ba is None:
            rot, trans, mask, valid = ver["R"], ver["t"], ver["mask"], pre
            ba_stats = np.zeros((len(pairs), len(STATS_FIELDS)), np.int32)
            ba_stats[:, col("status")], ba_stats[:, col("verified")], ba_stats[:, col("valid")] = STATUS_NAMES.index("SKIPPED"), pre, pre
        else:
            out = ba.run_launch(
                {"kp_xy": xy.reshape(-1, 2), "kp_off1": [i * cap for i, _ in pairs], "kp_off2": [j * cap for _, j in pairs], "match_idx": ver["match_idx"],
                 "match_off": list(ver["match_off"]), "match_count": ver["match_count"], "inlier_mask": ver["mask"],
                 "intrinsics": [ba.pair_intrinsics(camera_intrinsics[i], camera_intrinsics[j]) for i, j in pairs], "rotation": ver["R"], "translation": ver["t"]},
                device=xy.device, min_verified=opt.min_num_inliers_est_model, triangulation_threshold=opt.triangulation_reproj_error_threshold,
                triangulation_min_angle_deg=opt.triangulation_min_angle_deg)
            rot, trans, mask, ba_stats = out["rotation"], out["translation"], out["valid_mask"], out["stats"]
            valid = ba_stats[:, col("valid")].astype(np.int64)
        # InlierSupportProcessor: the ratio is the verifier's (the reference's hack), the count is the post-adjustment one
        ratio = np.array([self.verified[p][3] if p in self.verified and self.verified[p][0] is not None else 0.0 for p in pairs], dtype=np.float64)
        supported = ~(ratio < opt.min_inlier_ratio_est_model) & ~((valid > 0) & (valid < opt.min_num_inliers_est_model))
        lengths = torch.from_numpy(np.diff(np.asarray(list(ver["match_off"]), dtype=np.int64))).to(xy.device)
        rows = torch.repeat_interleave(torch.from_numpy(supported.astype(np.uint8)).to(xy.device), lengths)
        stats = ver["stats"].clone()
        stats[:, 0] = torch.from_numpy(np.where(supported, valid, 0).astype(np.int32)).to(xy.device)
        new = dict(ver)
        new.update(R=rot, t=trans, mask=(mask * rows).contiguous(), stats=stats, two_view=ba_stats)
        rot_host, trans_host = rot.cpu().numpy().reshape(-1, 3, 3), trans.cpu().numpy().reshape(-1, 3)
        for k, p in enumerate(pairs):
            row = named(ba_stats[k], STATS_FIELDS)
            poses[p] = (rot_host[k], trans_host[k])
            stats_by_edge[p] = {"status": STATUS_NAMES[row["status"]], **{f: row[f] for f in ("verified", "triangulated", "valid", "accepted_steps", "solves_tried")},
                                "supported": bool(supported[k])}
        return new

    def _two_view_verified(self, launches: List[Dict[str, Any]], poses, stats_by_edge) -> Dict[Tuple[int, int], Tuple[Any, Any, np.ndarray, float]]:
        """The post-ISP ``verified`` tuples of the edges that ``two_view`` refined on the device, from one download per launch."""
        from gtsfm_amd.frontend.verifier.ransac import _to_pose_types
        from gtsfm_amd.runtime.pipeline import FrontEndPipeline

        verified = {}
        for pair, res in FrontEndPipeline.verified_to_numpy(launches).items():
            if pair not in self.verified or pair in self.extra:
                continue
            old = self.verified[pair]
            rot_np, dir_np = poses[pair]
            corr = res["v_corr_idxs"].astype(np.asarray(old[2]).dtype if np.asarray(old[2]).ndim == 2 else np.int32).reshape(-1, 2)
            posed = bool(np.isfinite(rot_np).all() and np.isfinite(dir_np).all())
            status = stats_by_edge[pair]["status"]
            if status == "NONE_TRIANGULATED" or (status == "INDETERMINATE" and not posed):
                corr = np.zeros(shape=(0, 2), dtype=np.int32)  # bundle_adjust's own early returns (two_view_estimator.py:263, 276)
            if not stats_by_edge[pair]["supported"]:
                verified[pair] = FAILURE
            elif posed:
                verified[pair] = (*_to_pose_types(rot_np, dir_np), corr, old[3])
            else:
                verified[pair] = (None, None, corr, old[3])
        return verified

    def _two_view_extra(self, opt, camera_intrinsics, verified, stats_by_edge) -> Dict[Tuple[int, int], np.ndarray]:
        """``two_view`` for the edges of ``extra`` (verified through the per-pair host fallback), through the per-pair drop-ins:
        ``TwoViewEstimator.bundle_adjust`` on their verified tuple and keypoints (when they have at least ``min_num_inliers_est_model``
        correspondences, ``:412``), then ``InlierSupportProcessor.run_inlier_support``. Their tuples go into ``verified``, their stats into
        ``stats_by_edge``; returns the new scene's ``extra``, their post-ISP correspondences."""
        from gtsfm_amd.data_association.point3d_initializer import TriangulationOptions, TriangulationSamplingMode
        from gtsfm_amd.frontend.inlier_support_processor import InlierSupportProcessor
        from gtsfm_amd.two_view_estimator import TwoViewEstimator, generate_two_view_report

        extra: Dict[Tuple[int, int], np.ndarray] = {}
        isp = InlierSupportProcessor(opt.min_num_inliers_est_model, opt.min_inlier_ratio_est_model)
        estimator = TwoViewEstimator(None, isp, opt.bundle_adjust_2view, 4.0,
                                     TriangulationOptions(mode=TriangulationSamplingMode.NO_RANSAC, reproj_error_threshold=opt.triangulation_reproj_error_threshold,
                                                          min_triangulation_angle=opt.triangulation_min_angle_deg),
                                     bundle_adjust_2view_maxiters=opt.bundle_adjust_2view_maxiters, ba_reproj_error_thresholds=opt.ba_reproj_error_thresholds,
                                     allow_indeterminate_linear_system=opt.allow_indeterminate_linear_system)
        for pair in self.extra:
            i1, i2 = pair
            rot_obj, dir_obj, corr, ratio = self.verified[pair]
            adjust = opt.bundle_adjust_2view and len(corr) >= opt.min_num_inliers_est_model  # two_view_estimator.py:412
            info = {"status": "NO_INITIAL_POSE" if adjust else "SKIPPED", "verified": int(len(corr))}
            row = None
            if adjust:
                rot_obj, dir_obj, corr, row = estimator.bundle_adjust_with_stats(self.keypoints_list[i1], self.keypoints_list[i2], corr, camera_intrinsics[i1],
                                                                                 camera_intrinsics[i2], rot_obj, dir_obj, None)
            report = generate_two_view_report(ratio, np.asarray(corr).reshape(-1, 2) if np.asarray(corr).size else np.zeros((0, 2), np.int32))
            isp_rot, isp_dir, isp_corr, _ = isp.run_inlier_support(rot_obj, dir_obj, corr, report)
            count = int(np.asarray(corr).reshape(-1, 2).shape[0])
            supported = not (ratio < opt.min_inlier_ratio_est_model) and not (0 < count < opt.min_num_inliers_est_model)  # what the processor decided
            verified[pair] = (isp_rot, isp_dir, isp_corr, ratio) if supported else FAILURE
            extra[pair] = isp_corr
            info.update(valid=count, supported=bool(supported), host_fallback=True)
            if row is not None:
                row = named(row, STATS_FIELDS)
                info.update(status=STATUS_NAMES[row["status"]], triangulated=row["triangulated"], accepted_steps=row["accepted_steps"], solves_tried=row["solves_tried"])
            stats_by_edge[pair] = info
        return extra

    def view_graph(self, estimators=None, prune: bool = True) -> "ViewGraph":
        """View-graph estimation for the scene's edges (``gtsfm/multi_view_optimizer.py:130-175``), on the launches' rotations where they
        lie: the configured ``CycleConsistentRotationViewGraphEstimator`` (``estimators``: one estimator, or a list of them that is run as
        given; None: ``MEDIAN_EDGE_ERROR``, ``deep_front_end.yaml``'s), then once more with ``MEDIAN_EDGE_ERROR`` as the reference's
        ``view_graph_estimator_v2``, each pass taking the edges the last one kept; then, with ``prune``, the largest connected component.
        An edge takes part when it has a model (``stats[:, 0] > 0``, computed on the device) or, for the edges of ``extra``, when
        ``verified`` holds a pose for it (those few rotations are uploaded; the rows are the scene's ``SceneEdges``). No correspondence and no pose is downloaded: only the
        per-edge results are. ``scene.tracks(edges=vg.edges)`` and ``scene.triangulate(..., edges=vg.edges)`` take the result."""
        from gtsfm_amd.runtime.view_graph_engine import ViewGraphEngine, criterion_code
        from gtsfm_amd.view_graph_estimator.cycle_consistent_rotation_estimator import CycleConsistentRotationViewGraphEstimator, EdgeErrorAggregationCriterion

        median = EdgeErrorAggregationCriterion.MEDIAN_EDGE_ERROR
        if estimators is None:
            passes = [CycleConsistentRotationViewGraphEstimator(median), CycleConsistentRotationViewGraphEstimator(median)]
        elif isinstance(estimators, (list, tuple)):
            passes = list(estimators)
        else:
            passes = [estimators, CycleConsistentRotationViewGraphEstimator(median)]
        if self.feats is None:
            return ViewGraph.empty()
        engine, table = self._engine_of(ViewGraphEngine), self.edge_table
        on = table.has_model
        results = []
        for est in passes:
            out = engine.cycle_filter(table.pair_images, table.rotation, on, num_images=table.num_images, criterion=criterion_code(est._edge_error_aggregation_criterion),
                                      error_threshold=float(est._error_threshold))
            on = out["keep"]
            results.append({"criterion": est._edge_error_aggregation_criterion.value, "error_threshold": float(est._error_threshold), "counts": out["counts"],
                            "num_triplets": out["num_triplets"].cpu().numpy(), "aggregate_error": out["aggregate_error"].cpu().numpy(), "keep": out["keep"].cpu().numpy()})
        keep = on.cpu().numpy()
        pruned, component = keep, None
        if prune:
            comp = engine.largest_component(table.pair_images, on, num_images=table.num_images)
            pruned, component = comp["pair_keep"].cpu().numpy(), comp["counts"]
        return ViewGraph(list(table.pairs), keep, pruned, results, component)

    def rotation_averaging(self, edges: Optional[Iterable[Tuple[int, int]]] = None, averaging=None):
        """Rotation averaging for the scene's edges (``gtsfm/multi_view_optimizer.py``: ``ShonanRotationAveraging.run_rotation_averaging``
        between the view graph and 1DSfM) on the launches' rotations ``R`` where they lie. ``edges``: normally ``ViewGraph.edges`` (None:
        every edge with a model); ``averaging``: a ``ShonanRotationAveraging`` (None: its defaults). The weight of an edge is the square of
        the count of verified correspondences the launch holds on the device (``stats[:, 0]``: after ``two_view`` the count of the valid
        mask), i.e. sigma = 1 / count as the reference weights by inliers; with ``weight_by_inliers`` off it is
        ``1 / two_view_rotation_sigma^2``. Edges of ``extra`` take part with their uploaded rotations and the length of their host record.
        No correspondence is downloaded: the rotations, the mask and the counters come back. On a status other than CONVERGED with weights
        on, the solve is repeated unweighted and ``averaging`` is left unweighted, as the reference does after gtsam's RuntimeError
        (``ShonanRotationAveraging.solve_with_retry``, the one place that rule lives); nothing else of ``averaging`` is changed.
        Returns a ``RotationAverages``."""
        from gtsfm_amd.averaging.rotation.shonan import RotationAverages, ShonanRotationAveraging
        from gtsfm_amd.runtime.rotation_averaging_engine import COST_FIELDS, COUNTER_FIELDS

        averaging = averaging or ShonanRotationAveraging()
        if self.feats is None:
            return RotationAverages.empty()
        table = self.edge_table
        engine, counts = averaging.engine(table.device), table.count
        on = ((counts > 0) * table.mask(edges)).contiguous()  # uint8; an ``extra`` row with an empty record has a model and no weight

        def solve(weighted):
            sigma = float(averaging._two_view_rotation_sigma)
            weight = (counts * counts).contiguous() if weighted else counts.new_full(counts.shape, 1.0 / (sigma * sigma))
            out = engine.average(table.pair_images, table.rotation, weight, on, num_images=table.num_images, **averaging._solver_options)
            return out["status"][0], (weight, out)

        weight, out = averaging.solve_with_retry(solve)
        wri, valid = out["wRi"][0].cpu().numpy(), out["node_valid"][0].cpu().numpy()
        return RotationAverages([wri[i].reshape(3, 3).copy() if valid[i] else None for i in range(table.num_images)], out["status"][0],
                                named(out["counters"][0], COUNTER_FIELDS), named(out["costs"][0], COST_FIELDS, float), list(table.pairs), weight.cpu().numpy(), on.cpu().numpy())

    def translation_inliers(self, wRi_list: List[Any], camera_intrinsics: List[Any], edges: Optional[Iterable[Tuple[int, int]]] = None, averaging=None):  # noqa: N803
        """1DSfM outlier rejection for the scene's edges (the first half of translation averaging, ``gtsfm/multi_view_optimizer.py:175-199``
        with ``averaging_1dsfm.py:234-315,530-549``) on the launches' unit translations ``t`` and the tracks of ``edges`` (normally
        ``ViewGraph.edges``; None: every edge) where they lie. ``wRi_list``: a rotation (3 x 3 array or anything with ``.matrix()``) or None
        per image, whoever computed them; ``camera_intrinsics``: a pure pinhole calibration per image that has one; ``averaging``: a
        ``TranslationAveraging1DSFM`` (None: its defaults) whose sampling method, track settings and threshold are used. Only ``track_off``
        and ``image`` are downloaded, for the host's sequential track selection; the track mask and the projection directions are
        uploaded; counts, masks and the mean weights come back. The two sampling modes that draw from the measurements take one more
        call, which downloads the world directions. Edges of ``extra`` take part with their uploaded directions. Returns a
        ``TranslationInliers``: ``.edges`` (the inlier pairs: the ``edges=`` argument of ``tracks()`` and ``triangulate()``),
        ``.inlier_cameras``, ``.mean_weights``."""
        return self._translation_inliers_on_device(wRi_list, camera_intrinsics, edges, averaging)[0]

    def translation_averaging(self, wRi_list: List[Any], camera_intrinsics: List[Any], edges: Optional[Iterable[Tuple[int, int]]] = None, averaging=None,  # noqa: N803
                              scale_factor: float = 1.0):
        """Translation averaging for the scene's edges (``gtsfm/multi_view_optimizer.py``: ``TranslationAveraging1DSFM.run_translation_averaging``):
        the outlier rejection of ``translation_inliers``, then the recovery (``gtsfm_translation_recovery_f64``) on the rejection's device
        outputs where they lie -- the world directions, the two inlier masks, the pair rows and the track CSR; no direction is downloaded.
        With ``averaging._reject_outliers`` off every valid row takes part. Positions, mask, counters and costs come back. Returns a
        ``TranslationAverages``: ``.wti_list``, ``.wTi_list``, ``.cameras(intrinsics)`` for ``triangulate``, ``.landmarks``, ``.inliers``."""
        from gtsfm_amd.averaging.translation.averaging_1dsfm import HUBER_LOSS_K, NOISE_MODEL_SIGMA, TranslationAveraging1DSFM, TranslationAverages, recovery_engine
        from gtsfm_amd.runtime.translation_recovery_engine import COST_FIELDS, COUNTER_FIELDS

        averaging = averaging or TranslationAveraging1DSFM(translation_recovery="device")
        inliers, rows = self._translation_inliers_on_device(wRi_list, camera_intrinsics, edges, averaging)
        if rows is None:
            return TranslationAverages.empty(inliers)
        num_images = int(self.feats["xy"].shape[0])
        rotations = [wRi_list[i] if i < len(wRi_list) else None for i in range(num_images)]
        if not averaging._reject_outliers:  # a row that is not valid carries NaN directions: it stays out without a mask
            rows = dict(rows, pair_enable=None, meas_enable=None)
        opts = dict(sigma=NOISE_MODEL_SIGMA, huber_k=HUBER_LOSS_K if averaging._robust_measurement_noise else 0.0)
        opts.update(getattr(averaging, "_recovery_options", {}))
        out = recovery_engine(self.feats["xy"].device).recover(rows["pair_images"], rows["world_pair"], rows["pair_enable"], rows["track_off"], rows["image"], rows["world_meas"],
                                                               rows["meas_enable"], num_images=num_images, scale_factor=scale_factor, **opts)
        x, valid = out["translation"][0].cpu().numpy(), out["node_valid"][0].cpu().numpy()
        wti = [x[i].copy() if valid[i] and rotations[i] is not None else None for i in range(num_images)]
        return TranslationAverages(rotations, wti, x[num_images:].copy(), inliers, out["status"][0], named(out["counters"][0], COUNTER_FIELDS),
                                   named(out["costs"][0], COST_FIELDS, float), rows)

    def _translation_inliers_on_device(self, wRi_list, camera_intrinsics, edges, averaging):  # noqa: N803
        """The body of ``translation_inliers``: (the ``TranslationInliers``, the rows as they lie on the device for the recovery: ``pair_images``,
        ``world_pair``, ``pair_enable`` = the inlier mask, ``track_off``, ``image``, ``world_meas``, ``meas_enable`` = the inlier mask; None
        for an empty scene)."""
        from gtsfm_amd.averaging.translation.averaging_1dsfm import TranslationAveraging1DSFM, TranslationInliers, matrix3, select_tracks_csr
        from gtsfm_amd.common.calibration import pinhole_parameters

        averaging = averaging or TranslationAveraging1DSFM()
        if self.feats is None:
            return TranslationInliers.empty(), None
        import torch

        table = self.edge_table
        device, num_images, pairs = table.device, table.num_images, list(table.pairs)
        averaging._device = averaging._device or device
        engine = averaging.engine()
        edges = None if edges is None else [(int(a), int(b)) for a, b in edges]
        wanted = None if edges is None else set(edges)
        on, pair_direction = table.mask(edges), table.direction
        rotation, rotation_valid, intrinsics = np.zeros((num_images, 9)), np.zeros(num_images, np.uint8), np.ones((num_images, 4))
        for i in range(num_images):
            if i < len(wRi_list) and wRi_list[i] is not None:
                rotation[i], rotation_valid[i] = matrix3(wRi_list[i]).reshape(9), 1
            if i < len(camera_intrinsics) and camera_intrinsics[i] is not None:
                *intrinsics[i], pure = pinhole_parameters(camera_intrinsics[i])
                if not pure:
                    raise NotImplementedError(f"image {i}: {type(camera_intrinsics[i]).__name__} is not a pure pinhole calibration")
        # get_valid_measurements_in_world_frame on the host's record of the edges: i1 enters although wRi1 is not looked at
        live = [p for p in pairs if (wanted is None or p in wanted) and p in self.verified and self.verified[p][1] is not None and rotation_valid[p[1]]]
        valid_cameras = {c for p in live for c in p}
        use_tracks = averaging._use_tracks_for_averaging
        if use_tracks:
            trk = self._tracks_on_device(edges)
            track_off, image, uv = trk["track_off"].contiguous(), trk["image"].contiguous(), trk["uv"].contiguous()
            track_off_host, image_host = track_off.cpu().numpy(), image.cpu().numpy()
            track_enable, meas_enable = select_tracks_csr(track_off_host, image_host, valid_cameras, use_all_tracks=averaging._use_all_tracks_for_averaging)
        else:
            track_off, image = torch.zeros(1, dtype=torch.int64, device=device), torch.empty(0, dtype=torch.int32, device=device)
            uv = torch.empty((0, 2), dtype=torch.float32, device=device)
            track_off_host, image_host, track_enable, meas_enable = np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.uint8)
        if not averaging._use_relative_camera_poses:
            on = torch.zeros_like(on)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
        args = [table.pair_images, pair_direction, on, up(rotation), up(rotation_valid), up(intrinsics), track_off, image, uv, up(track_enable),
                up(meas_enable)]
        capacity = num_images + int(track_enable.sum())
        methods, world = TranslationAveraging1DSFM.ProjectionSamplingMethod, None
        if averaging._projection_sampling_method == methods.SAMPLE_WITH_UNIFORM_DENSITY:
            directions = averaging.sample_projection_directions(np.zeros((0, 3)))
        else:  # the measurements themselves are sampled: one call for the world directions, which are then given
            first = engine.inliers(*args, up(np.array([[1.0, 0.0, 0.0]])), threshold=averaging._outlier_weight_threshold, node_capacity=capacity)
            world = (first["world_pair"], first["world_meas"])
            combined = np.concatenate([world[0].cpu().numpy(), world[1].cpu().numpy()])
            directions = averaging.sample_projection_directions(combined[np.isfinite(combined).all(axis=1)])
        out = engine.inliers(*args, up(np.asarray(directions, np.float64).reshape(-1, 3)), threshold=averaging._outlier_weight_threshold, world=world, node_capacity=capacity)
        tracks = {"track_off": track_off_host, "image": image_host, "track_enable": track_enable, "meas_enable": meas_enable}
        rows = {"pair_images": args[0], "world_pair": out["world_pair"], "pair_enable": out["pair_inlier"], "track_off": track_off, "image": image,
                "world_meas": out["world_meas"], "meas_enable": out["meas_inlier"]}
        return TranslationInliers(pairs, out["pair_weight"].cpu().numpy(), out["pair_inlier"].cpu().numpy(), out["camera_inlier"].cpu().numpy(),
                                  out["meas_weight"].cpu().numpy(), out["meas_inlier"].cpu().numpy(), out["counts"], tracks), rows

    def tracks(self, edges: Optional[Iterable[Tuple[int, int]]] = None) -> Dict[str, Any]:
        """The feature tracks of the verified correspondences (of ``edges`` only, when given: ``filter_corr_by_idx`` followed by
        ``get_2d_tracks``) as CSR arrays on the host: ``track_off`` [T + 1] int64, ``image`` / ``kp`` [S] int32, ``track_uv`` [S, 2]
        float32 gathered from the device's ``xy`` table, and ``counts``. A second call uploads only the edge mask."""
        if self.feats is None:
            return empty_tracks()
        out = self._tracks_on_device(edges)
        return {**{k: out[k].cpu().numpy() for k in ("track_off", "image", "kp")}, "track_uv": out["uv"].cpu().numpy(), "counts": out["counts"]}

    def triangulate(self, cameras: Dict[int, Any], options, edges: Optional[Iterable[Tuple[int, int]]] = None, seed: int = 0) -> Dict[str, Any]:
        """Tracks -> triangulation (``DataAssociation.run_triangulation``) with the track arrays staying on the device: the CSR arrays
        that the track builder writes are the triangulation's inputs where they lie. Returns host arrays: ``track_off``, ``image``,
        ``kp``, ``point`` [T, 3], ``avg_error`` [T], ``exit_code`` [T], ``inlier_mask`` [S]."""
        from gtsfm_amd.data_association.point3d_initializer import Point3dInitializer

        if self.feats is None:
            return empty_triangulation()
        trk = self._tracks_on_device(edges)
        out = Point3dInitializer(cameras, options, seed=seed, device=self.feats["xy"].device).triangulate_arrays(trk["track_off"], trk["image"], trk["uv"])
        return {**{k: trk[k].cpu().numpy() for k in ("track_off", "image", "kp")}, **{k: out[k].cpu().numpy() for k in ("point", "avg_error", "exit_code", "inlier_mask")}}

    def bundle_adjust(self, cameras: Dict[int, Any], triangulation_options, optimizer=None, edges: Optional[Iterable[Tuple[int, int]]] = None, seed: int = 0) -> Dict[str, Any]:
        """Tracks -> triangulation -> global bundle adjustment (``gtsfm/multi_view_optimizer.py:200-221``: ``DataAssociation`` then
        ``bundle_adjustment_module``) on the device arrays where they lie: the track CSR the track builder writes and the points, exit
        codes and inlier mask the triangulation writes are the adjustment's inputs; no track, point or mask is downloaded in between.
        ``optimizer``: a ``BundleAdjustmentOptimizer`` (None: ``unified.yaml``'s). A track takes part when its exit code is SUCCESS, a
        measurement when the triangulation kept it. Returns host arrays: the track CSR (``track_off``, ``image``, ``kp``), ``point``
        [T, 3], ``cameras`` [N, 17], ``track_valid`` [T], ``camera_kept`` [N], ``reproj_error`` [S], ``exit_code`` [T], ``counters`` and
        ``costs`` by name, ``status``."""
        from gtsfm_amd.bundle.bundle_adjustment import BundleAdjustmentOptimizer, RobustBAMode
        from gtsfm_amd.data_association.point3d_initializer import Point3dInitializer
        from gtsfm_amd.runtime.global_ba_engine import COST_FIELDS, COUNTER_FIELDS

        if self.feats is None:
            return empty_bundle_adjustment()
        import torch

        optimizer = optimizer or BundleAdjustmentOptimizer(reproj_error_thresholds=(10, 5, 3), robust_ba_mode=RobustBAMode.HUBER, measurement_noise_sigma=1.0)
        device = self.feats["xy"].device
        trk = self._tracks_on_device(edges)
        initializer = Point3dInitializer(cameras, triangulation_options, seed=seed, device=device)
        tri = initializer.triangulate_arrays(trk["track_off"], trk["image"], trk["uv"])
        from gtsfm_amd.runtime.triangulation_engine import pack_cameras

        table = torch.from_numpy(pack_cameras(cameras, num_images=int(self.feats["xy"].shape[0]))).to(device)
        track_enable = (tri["exit_code"] == 0).to(torch.uint8).contiguous()
        out = optimizer.run_ba_device(table, trk["track_off"].contiguous(), trk["image"].contiguous(), trk["uv"].contiguous(), tri["point"].contiguous(), track_enable,
                                      tri["inlier_mask"].contiguous())
        return {**{k: trk[k].cpu().numpy() for k in ("track_off", "image", "kp")}, "point": out["point"].cpu().numpy(), "cameras": out["cameras"][0].cpu().numpy(),
                "track_valid": out["track_valid"].cpu().numpy(), "camera_kept": out["camera_kept"][0].cpu().numpy(), "reproj_error": out["reproj_error"].cpu().numpy(),
                "exit_code": tri["exit_code"].cpu().numpy(), "counters": named(out["counters"][0], COUNTER_FIELDS), "costs": named(out["costs"][0], COST_FIELDS, float),
                "status": out["status"][0]}

    def tracks_2d(self, edges: Optional[Iterable[Tuple[int, int]]] = None) -> list:
        """The same tracks as ``SfmTrack2d`` objects over ``keypoints_list``'s coordinates."""
        from gtsfm_amd.data_association.dsf_tracks_estimator import tracks_from_csr

        res = self.tracks(edges)
        return tracks_from_csr(res["track_off"], res["image"], res["kp"], self.keypoints_list)
