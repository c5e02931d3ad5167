"""``ViewGraphEstimatorBase``: the reference's class when GTSfM is importable, else a stand-in with the same contract
(``gtsfm/view_graph_estimator/view_graph_estimator_base.py:38-159``): ``run`` is abstract; ``_get_valid_input_edges`` and
``_filter_with_edges`` are the reference's. ``create_computation_graph`` (dask), ``compute_metrics`` and the plots are out of scope."""

from __future__ import annotations

import abc
import logging
from typing import Any, Dict, List, Set, Tuple

import numpy as np

from gtsfm_amd.frontend.registry import GTSFMProcess, UiMetadata

logger = logging.getLogger("gtsfm_amd")

try:  # pragma: no cover
    from gtsfm.view_graph_estimator.view_graph_estimator_base import ViewGraphEstimatorBase  # type: ignore  # noqa: F401
except Exception:  # noqa: BLE001

    class ViewGraphEstimatorBase(GTSFMProcess):  # type: ignore[no-redef]
        """Aggregates two-view estimates into a view graph, filtering them on the way."""

        @staticmethod
        def get_ui_metadata() -> UiMetadata:
            return UiMetadata(
                display_name="View-Graph Estimator",
                input_products=("Optimized Relative Rotation", "Optimized Relative Translation", "Camera Intrinsics", "Inlier Correspondences", "Keypoints"),
                output_products=("View-Graph Relative Rotations", "View-Graph Relative Translations", "View-Graph Correspondences"),
                parent_plate="Sparse Reconstruction",
            )

        @abc.abstractmethod
        def run(self, i2Ri1_dict: Dict[Tuple[int, int], Any], i2Ui1_dict: Dict[Tuple[int, int], Any], calibrations: List[Any],  # noqa: N803
                corr_idxs_i1i2: Dict[Tuple[int, int], np.ndarray], keypoints: List[Any], two_view_reports: Dict[Tuple[int, int], Any]) -> Set[Tuple[int, int]]:
            """The edges of the view graph, a subset of the input pairs. The inputs are valid: i1 < i2 and neither i2Ri1 nor i2Ui1 is None."""

        def _get_valid_input_edges(self, i2Ri1_dict: Dict[Tuple[int, int], Any], i2Ui1_dict: Dict[Tuple[int, int], Any]) -> List[Tuple[int, int]]:  # noqa: N803
            """The input edges with i1 < i2 whose rotation and unit translation are both present (``:93-121``)."""
            valid_edges = []
            for (i1, i2), i2Ri1 in i2Ri1_dict.items():  # noqa: N806
                if i1 >= i2:
                    logger.error("Incorrectly ordered edge indices found in cycle consistency for (%d, %d)", i1, i2)
                    continue
                if i2Ri1 is None:
                    continue  # edge was previously discarded for insufficient support
                if (i1, i2) not in i2Ui1_dict:
                    logger.error("Found edge (%d, %d) in rotations dict but not in unit translations", i1, i2)
                    continue
                if i2Ui1_dict[(i1, i2)] is None:
                    continue
                valid_edges.append((i1, i2))
            return valid_edges

        def _filter_with_edges(self, i2Ri1_dict, i2Ui1_dict, corr_idxs_i1i2, two_view_reports, edges_to_select: Set[Tuple[int, int]]):  # noqa: N803
            """The four dicts restricted to ``edges_to_select`` (``:123-159``)."""
            return (
                {edge: i2Ri1_dict[edge] for edge in edges_to_select},
                {edge: i2Ui1_dict[edge] for edge in edges_to_select},
                {edge: corr_idxs_i1i2[edge] for edge in edges_to_select},
                {edge: two_view_reports[edge] for edge in edges_to_select},
            )
