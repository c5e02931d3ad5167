"""Host side of the device view-graph stage: ``gtsfm_view_graph_cycle_filter_f64`` filters the edges of the pair graph by the rotation
cycle consistency of their triplets (``gtsfm/view_graph_estimator/cycle_consistent_rotation_estimator.py:80-157``) and
``gtsfm_largest_component`` prunes to the largest connected component (``gtsfm/utils/graph.py:24-89``), on the two-view stage's arrays where
they lie. PyTorch provides device memory and streams only."""

from __future__ import annotations

import ctypes as C
from typing import Dict

import numpy as np

from gtsfm_amd.runtime.engine_base import EngineBase, named

MIN_EDGE_ERROR, MEDIAN_EDGE_ERROR = 0, 1
CRITERIA = {"MIN_EDGE_ERROR": MIN_EDGE_ERROR, "MEDIAN_EDGE_ERROR": MEDIAN_EDGE_ERROR}
FILTER_COUNT_FIELDS = ("input_edges", "kept_edges", "triplets", "max_triplets_per_edge")
COMPONENT_COUNT_FIELDS = ("nodes", "edges", "components")
WORKSPACE_ERROR = -3  # GTSFM_ERR_WORKSPACE


def criterion_code(criterion) -> int:
    """0 / 1, the names, or the drop-in's ``EdgeErrorAggregationCriterion`` (a str enum whose value is the name)."""
    if isinstance(criterion, str):  # the enum is a str as well
        name = getattr(criterion, "value", criterion)
        if name not in CRITERIA:
            raise ValueError(f"unknown edge error aggregation criterion {criterion!r}")
        return CRITERIA[name]
    if int(criterion) not in (MIN_EDGE_ERROR, MEDIAN_EDGE_ERROR):
        raise ValueError(f"unknown edge error aggregation criterion {criterion!r}")
    return int(criterion)


class ViewGraphEngine(EngineBase):
    def __init__(self, device=None):
        super().__init__(device)
        self._triplet_capacity = 0

    def _check(self, pair_images, rotation, pair_enable, num_images):
        torch = self._torch
        num_edges = int(pair_images.shape[0]) if pair_images.dim() == 2 else -1
        self._check_tensors((("pair_images", pair_images, torch.int32, 2 * num_edges), ("rotation", rotation, torch.float64, 9 * num_edges),
                             ("pair_enable", pair_enable, torch.uint8, num_edges)), optional=("pair_images", "rotation", "pair_enable"))
        if num_edges < 0 or int(num_images) < 0:
            raise ValueError(f"pair_images must be [E, 2] and num_images >= 0 (got {tuple(pair_images.shape)}, {num_images})")
        return num_edges

    def cycle_filter(self, pair_images, rotation, pair_enable=None, *, num_images: int, criterion=MEDIAN_EDGE_ERROR, error_threshold: float = 7.0,
                     want_triplets: bool = False) -> Dict[str, object]:
        """``pair_images`` [E, 2] int32, ``rotation`` [E, 9] (or [E, 3, 3]) float64 i2Ri1, ``pair_enable`` [E] uint8 (optional): device tensors,
        see include/gtsfm_amd.h. Returns device tensors ``num_triplets`` [E] int32, ``aggregate_error`` [E] float64, ``keep`` [E] uint8, with
        ``want_triplets`` also ``triplets`` [T, 3] int32 and ``cycle_error`` [T]; and ``counts`` as a dict of ints (``FILTER_COUNT_FIELDS``).
        The triplet capacity of the workspace grows to what a scene needed; a call that finds more triplets than it holds is repeated once."""
        torch = self._torch
        num_edges = self._check(pair_images, rotation, pair_enable, num_images)
        code = criterion_code(criterion)
        num = torch.empty(num_edges, dtype=torch.int32, device=self.device)
        agg = torch.empty(num_edges, dtype=torch.float64, device=self.device)
        keep = torch.empty(num_edges, dtype=torch.uint8, device=self.device)
        counts = torch.empty(8, dtype=torch.int32, device=self.device)
        capacity = max(self._triplet_capacity, 8 * num_edges)
        found = C.c_longlong(-1)
        ptr = self._ptr
        for attempt in range(2):
            ws = self._sized_workspace("gtsfm_view_graph_workspace_bytes", num_edges, int(num_images), capacity)
            trip = torch.empty((capacity, 3), dtype=torch.int32, device=self.device) if want_triplets else None
            cyc = torch.empty(capacity, dtype=torch.float64, device=self.device) if want_triplets else None
            rc = self._lib.gtsfm_view_graph_cycle_filter_f64(
                ptr(pair_images), ptr(rotation), ptr(pair_enable), num_edges, int(num_images), code, float(error_threshold), capacity, ws.data_ptr(), ws.numel(), ptr(num),
                ptr(agg), ptr(keep), counts.data_ptr(), ptr(trip), ptr(cyc), C.byref(found), self._stream())
            if rc == WORKSPACE_ERROR and found.value > capacity and attempt == 0:
                capacity = int(found.value)  # the call counted them before it refused
                continue
            break
        self._L.check(rc, "gtsfm_view_graph_cycle_filter_f64")
        self._triplet_capacity = capacity
        c = counts.cpu().numpy()
        out = {"num_triplets": num, "aggregate_error": agg, "keep": keep, "counts": named(c, FILTER_COUNT_FIELDS)}
        if want_triplets:
            out["triplets"], out["cycle_error"] = trip[: int(c[2])], cyc[: int(c[2])]
        return out

    def largest_component(self, pair_images, pair_enable=None, *, num_images: int) -> Dict[str, object]:
        """Device tensors ``node_mask`` [num_images] uint8 and ``pair_keep`` [E] uint8, ``counts`` as a dict (``COMPONENT_COUNT_FIELDS``)."""
        torch = self._torch
        num_edges = self._check(pair_images, None, pair_enable, num_images)
        node_mask = torch.empty(int(num_images), dtype=torch.uint8, device=self.device)
        pair_keep = torch.empty(num_edges, dtype=torch.uint8, device=self.device)
        counts = torch.empty(8, dtype=torch.int32, device=self.device)
        ws = self._sized_workspace("gtsfm_view_graph_workspace_bytes", num_edges, int(num_images), 0)
        ptr = self._ptr
        rc = self._lib.gtsfm_largest_component(ptr(pair_images), ptr(pair_enable), num_edges, int(num_images), ws.data_ptr(), ws.numel(), ptr(node_mask), ptr(pair_keep),
                                               counts.data_ptr(), self._stream())
        self._L.check(rc, "gtsfm_largest_component")
        return {"node_mask": node_mask, "pair_keep": pair_keep, "counts": named(counts.cpu().numpy(), COMPONENT_COUNT_FIELDS)}

    def upload(self, pair_images, rotation=None, pair_enable=None):
        """Host arrays -> the device tensors the two methods take."""
        return self._up(pair_images, np.int32, (-1, 2)), self._up(rotation, np.float64, (-1, 9)), self._up(pair_enable, np.uint8, (-1,))
