"""The rotation cycle-consistency view-graph estimator on the MI355X HIP path.

Drop-in for ``gtsfm/view_graph_estimator/cycle_consistent_rotation_estimator.py:34-240``: the same class and enum names, the same
constructor and ``run(...) -> Set[Tuple[int, int]]``. The triplets of the pair graph, their cycle errors and the per-edge aggregate are
computed by ``gtsfm_view_graph_cycle_filter_f64``; only the rotations travel to the device and only the per-edge results come back.

Stated rather than hidden (PARITY UNPINNED, see include/gtsfm_amd.h): gtsam's ``Rot3.between`` / ``compose`` are restated as float64 matrix
products; the plots of ``output_dir`` are not drawn (the argument is accepted and ignored)."""

from __future__ import annotations

import logging
import time
from enum import Enum
from pathlib import Path
from typing import Any, Dict, List, Optional, Set, Tuple

import numpy as np

from gtsfm_amd.view_graph_estimator.view_graph_estimator_base import ViewGraphEstimatorBase

logger = logging.getLogger("gtsfm_amd")

# threshold for cycle consistency inference
ERROR_THRESHOLD = 7.0


class EdgeErrorAggregationCriterion(str, Enum):
    """MIN_EDGE_ERROR: an edge that appears in ANY cycle of low error is accepted. MEDIAN_EDGE_ERROR: at least half of its cycles are."""

    MIN_EDGE_ERROR = "MIN_EDGE_ERROR"
    MEDIAN_EDGE_ERROR = "MEDIAN_EDGE_ERROR"


def rotation_matrix(rot: Any) -> np.ndarray:
    """What ``_to_pose_types`` yields: an object with ``.matrix()`` (gtsam's Rot3) or a 3 x 3 array."""
    m = rot.matrix() if hasattr(rot, "matrix") else rot
    m = np.asarray(m, dtype=np.float64)
    if m.shape != (3, 3):
        raise ValueError(f"a rotation must be 3 x 3, got shape {m.shape}")
    return m


class CycleConsistentRotationViewGraphEstimator(ViewGraphEstimatorBase):
    """Filters two-view edges by the rotation cycle error of the triplets they take part in."""

    def __init__(self, edge_error_aggregation_criterion: EdgeErrorAggregationCriterion, error_threshold: float = ERROR_THRESHOLD) -> None:
        self._edge_error_aggregation_criterion = EdgeErrorAggregationCriterion(edge_error_aggregation_criterion)
        self._error_threshold = error_threshold
        self._engine = None  # lazy: the object must pickle before first use (Dask scatter)

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_engine"] = None
        return state

    def __repr__(self) -> str:
        return f"CycleConsistentRotationViewGraphEstimator({self._edge_error_aggregation_criterion.value}, error_threshold={self._error_threshold})"

    def _ensure_engine(self):
        if getattr(self, "_engine", None) is None:
            from gtsfm_amd.runtime.view_graph_engine import ViewGraphEngine

            self._engine = ViewGraphEngine()
        return self._engine

    def run_arrays(self, i2Ri1_dict: Dict[Tuple[int, int], Any], want_triplets: bool = False) -> Dict[str, Any]:  # noqa: N803
        """The per-edge arrays on the host, in the order of ``edges`` (the dict's keys whose rotation is not None): ``num_triplets`` int32,
        ``aggregate_error`` float64 (NaN without a triplet), ``keep`` uint8, ``counts``; with ``want_triplets`` also ``triplets`` [T, 3] and
        ``cycle_error`` [T]. A key with i1 >= i2 raises ``ValueError``: the reference's ``_get_valid_input_edges`` removes those first."""
        edges = [(int(i1), int(i2)) for (i1, i2), rot in i2Ri1_dict.items() if rot is not None]
        bad = [e for e in edges if e[0] >= e[1] or e[0] < 0]
        if bad:
            raise ValueError(f"incorrectly ordered edge indices {bad[:5]}: the view graph estimator takes edges with 0 <= i1 < i2")
        empty = {"edges": edges, "num_triplets": np.zeros(0, np.int32), "aggregate_error": np.zeros(0), "keep": np.zeros(0, np.uint8),
                 "counts": {"input_edges": 0, "kept_edges": 0, "triplets": 0, "max_triplets_per_edge": 0}}
        if want_triplets:
            empty.update(triplets=np.zeros((0, 3), np.int32), cycle_error=np.zeros(0))
        if not edges:
            return empty
        rotation = np.stack([rotation_matrix(i2Ri1_dict[e]).reshape(9) for e in edges])
        engine = self._ensure_engine()
        pair_images, rot_dev, _ = engine.upload(np.asarray(edges, np.int32), rotation)
        out = engine.cycle_filter(pair_images, rot_dev, None, num_images=max(e[1] for e in edges) + 1, criterion=self._edge_error_aggregation_criterion,
                                  error_threshold=float(self._error_threshold), want_triplets=want_triplets)
        res = {"edges": edges, "counts": out["counts"]}
        res.update({k: v.cpu().numpy() for k, v in out.items() if k != "counts"})
        return res

    def run(self, i2Ri1_dict: Dict[Tuple[int, int], Any], i2Ui1_dict: Dict[Tuple[int, int], Any], calibrations: List[Any],  # noqa: N803
            corr_idxs_i1i2: Dict[Tuple[int, int], np.ndarray], keypoints: List[Any], two_view_reports: Dict[Tuple[int, int], Any],
            output_dir: Optional[Path] = None) -> Set[Tuple[int, int]]:
        """Only ``i2Ri1_dict`` is used, as in the reference (whose other arguments serve its plots)."""
        start_time = time.time()
        logger.info("Input number of edges: %d", len(i2Ri1_dict))
        res = self.run_arrays(i2Ri1_dict)
        logger.info("Number of triplets: %d", res["counts"]["triplets"])
        valid_edges = {edge for edge, kept in zip(res["edges"], res["keep"].tolist()) if kept}
        logger.info("Found %d consistent rel. rotations from %d original edges in %.2f sec.", len(valid_edges), len(res["edges"]), time.time() - start_time)
        return valid_edges
