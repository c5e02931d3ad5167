"""The edge rows of a ``VerifiedScene`` as the multi-view stages take them: built once per scene, on the device the launches lie on."""

from __future__ import annotations

from functools import cached_property

import numpy as np

from gtsfm_amd.runtime.tracks_engine import edge_selection
from gtsfm_amd.view_graph_estimator.cycle_consistent_rotation_estimator import rotation_matrix


class SceneEdges:
    """One row per edge: the launches' pairs in launch order, then the edges of ``extra`` that have a model, in ``extra``'s order. An ``extra``
    edge has a model when ``verified`` holds both a rotation and a direction for it: every producer of such a tuple in this package
    (``VerifierBase._failure_result``, ``TwoViewEstimator.bundle_adjust*``, ``InlierSupportProcessor``, ``VerifiedScene.two_view``) sets the
    two to None together, so the stages that looked at one of them see the rows they saw. The columns lie on the device of ``feats["xy"]``
    (whichever it is) and each is built on first use: the launches' part is used where it lies, the few ``extra`` rows are uploaded.
    ``pairs``: the rows as tuples; ``pair_images`` [E, 2] int32; ``rotation`` [E, 9] and ``direction`` [E, 3] float64 (i2Ri1, i2Ui1; NaN for a
    launch row without a model); ``count`` [E] float64: the launches' ``stats[:, 0]`` (the verified correspondences on the device), the length
    of the host record of an ``extra`` row; ``has_model`` [E] uint8: ``stats[:, 0] > 0`` of a launch row, 1 for an ``extra`` row."""

    def __init__(self, feats, launches, extra, verified) -> None:
        import torch

        self._torch, self.device, self.num_images = torch, feats["xy"].device, int(feats["xy"].shape[0])
        modelled = [p for p in extra if p in verified and verified[p][0] is not None and verified[p][1] is not None]
        self._launches, self._extra = launches, [verified[p] for p in modelled]
        self.pairs = [(int(p[0]), int(p[1])) for v in launches for p in v["pairs"]] + [(int(p[0]), int(p[1])) for p in modelled]

    def _column(self, launch_rows, extra_row, dtype, width=()):
        torch = self._torch
        parts = [launch_rows(v).reshape(-1, *width).to(dtype) for v in self._launches]
        if self._extra:
            parts.append(torch.from_numpy(np.stack([extra_row(tup) for tup in self._extra])).to(device=self.device, dtype=dtype))
        return torch.cat(parts).contiguous() if parts else torch.empty((0, *width), dtype=dtype, device=self.device)

    @cached_property
    def pair_images(self):
        return self._torch.from_numpy(np.asarray(self.pairs, np.int32).reshape(-1, 2)).to(self.device)

    @cached_property
    def rotation(self):
        return self._column(lambda v: v["R"], lambda tup: rotation_matrix(tup[0]).reshape(9), self._torch.float64, (9,))

    @cached_property
    def direction(self):
        from gtsfm_amd.averaging.translation.averaging_1dsfm import vector3

        return self._column(lambda v: v["t"], lambda tup: vector3(tup[1]), self._torch.float64, (3,))

    @cached_property
    def count(self):
        return self._column(lambda v: v["stats"][:, 0], lambda tup: np.float64(len(tup[2])), self._torch.float64)

    @cached_property
    def has_model(self):
        return self._column(lambda v: v["stats"][:, 0] > 0, lambda tup: np.uint8(1), self._torch.uint8)

    def mask(self, edges=None):
        """``has_model`` restricted to ``edges`` (None: every edge)."""
        if edges is None or not self.pairs:
            return self.has_model
        return (self.has_model * self._torch.from_numpy(edge_selection(self.pairs, edges)).to(self.device)).contiguous()
