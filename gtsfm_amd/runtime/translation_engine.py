"""Host side of the device's 1DSfM outlier rejection: ``gtsfm_translation_inliers_f64`` runs ``TranslationAveraging1DSFM.compute_inliers``
(``gtsfm/averaging/translation/averaging_1dsfm.py:234-315``, with gtsam's MFAS ordering per projection direction) on the pair rows and the
track builder's CSR arrays where they lie. PyTorch provides device memory and streams only."""

from __future__ import annotations

import os
from typing import Dict, Optional

import numpy as np

from gtsfm_amd.runtime.engine_base import EngineBase, named

COUNT_FIELDS = ("pair_edges", "measurement_edges", "nodes", "inlier_pairs", "inlier_measurements", "inlier_cameras")
OUTLIER_WEIGHT_THRESHOLD = 0.125
LDS_NODES = 2048  # TR_LDS_NODES of translation_kernels.hip
LDS_NODES_ENV = "GTSFM_AMD_TRANSLATION_LDS_NODES"


def lds_node_limit(value: Optional[int] = None) -> int:
    """The node count up to which the MFAS state lives in LDS: ``value``, else $GTSFM_AMD_TRANSLATION_LDS_NODES, else 2048 (the most)."""
    if value is None:
        value = int(os.environ.get(LDS_NODES_ENV, LDS_NODES))
    return LDS_NODES if value < 0 or value > LDS_NODES else int(value)


class TranslationInliersEngine(EngineBase):
    def inliers(self, pair_images, pair_direction, pair_enable, rotation, rotation_valid, intrinsics, track_off, image, uv, track_enable, meas_enable, directions, *,
                threshold: float = OUTLIER_WEIGHT_THRESHOLD, world=None, node_capacity: Optional[int] = None, lds_nodes: Optional[int] = None,
                want_position: bool = False) -> Dict[str, object]:
        """Device tensors as in include/gtsfm_amd.h: ``pair_images`` [E, 2] int32, ``pair_direction`` [E, 3] float64 (i2Ui1), ``pair_enable``
        [E] uint8 or None, ``rotation`` [N, 9] float64 wRi, ``rotation_valid`` [N] uint8, ``intrinsics`` [N, 4] float64, ``track_off`` [T + 1]
        int64, ``image`` [S] int32, ``uv`` [S, 2] float32, ``track_enable`` [T] uint8, ``meas_enable`` [S] uint8 or None, ``directions`` [D, 3]
        float64. ``world``: (``world_pair`` [E, 3], ``world_meas`` [S, 3]) float64 given instead of computed (rotation, intrinsics,
        pair_direction and uv may then be None); the tensors are not changed. ``node_capacity``: the most nodes with an edge (default
        N + T). Returns device tensors ``world_pair``, ``world_meas``, ``pair_weight``, ``meas_weight``, ``pair_inlier``, ``meas_inlier``,
        ``camera_inlier``, with ``want_position`` also ``position`` [D, N + T] int32; ``counts`` as a dict of ints and ``tier``."""
        torch = self._torch
        dev = self.device
        e, n = int(pair_images.shape[0]), int(rotation_valid.shape[0])
        t, s, d = int(track_off.shape[0]) - 1, int(image.shape[0]), int(directions.shape[0])
        given = world is not None
        spec = [("pair_images", pair_images, torch.int32, 2 * e), ("pair_enable", pair_enable, torch.uint8, e), ("rotation_valid", rotation_valid, torch.uint8, n),
                ("track_off", track_off, torch.int64, t + 1), ("image", image, torch.int32, s), ("track_enable", track_enable, torch.uint8, t),
                ("meas_enable", meas_enable, torch.uint8, s), ("directions", directions, torch.float64, 3 * d)]
        if given:
            spec += [("world[0]", world[0], torch.float64, 3 * e), ("world[1]", world[1], torch.float64, 3 * s)]
        else:
            spec += [("pair_direction", pair_direction, torch.float64, 3 * e), ("rotation", rotation, torch.float64, 9 * n), ("intrinsics", intrinsics, torch.float64, 4 * n),
                     ("uv", uv, torch.float32, 2 * s)]
        self._check_tensors(spec, optional=("pair_enable", "meas_enable"))
        if t < 0 or (s > 0 and t == 0):
            raise ValueError("track_off must be [T + 1] with T > 0 when there are measurements")
        limit = lds_node_limit(lds_nodes)
        cap = n + t if node_capacity is None else min(int(node_capacity), n + t)
        ws = self._sized_workspace("gtsfm_translation_inliers_workspace_bytes", e, s, n, t, d, cap, limit)
        world_pair = world[0].clone() if given else torch.empty((e, 3), dtype=torch.float64, device=dev)
        world_meas = world[1].clone() if given else torch.empty((s, 3), dtype=torch.float64, device=dev)
        pair_weight, meas_weight = torch.empty(e, dtype=torch.float64, device=dev), torch.empty(s, dtype=torch.float64, device=dev)
        pair_inlier, meas_inlier = torch.empty(e, dtype=torch.uint8, device=dev), torch.empty(s, dtype=torch.uint8, device=dev)
        camera_inlier = torch.empty(n, dtype=torch.uint8, device=dev)
        position = torch.empty((d, n + t), dtype=torch.int32, device=dev) if want_position else None
        counts = torch.empty(8, dtype=torch.int32, device=dev)
        p = self._ptr
        rc = self._lib.gtsfm_translation_inliers_f64(
            p(pair_images), p(pair_direction), p(pair_enable), e, p(rotation), p(rotation_valid), p(intrinsics), n, track_off.data_ptr(), p(image), p(uv), p(track_enable),
            p(meas_enable), t, s, p(directions), d, float(threshold), 1 if given else 0, cap, limit, ws.data_ptr(), ws.numel(), p(world_pair), p(world_meas), p(pair_weight),
            p(meas_weight), p(pair_inlier), p(meas_inlier), p(camera_inlier), p(position), counts.data_ptr(), self._stream())
        self._L.check(rc, "gtsfm_translation_inliers_f64")
        c = counts.cpu().numpy()
        out = {"world_pair": world_pair, "world_meas": world_meas, "pair_weight": pair_weight, "meas_weight": meas_weight, "pair_inlier": pair_inlier,
               "meas_inlier": meas_inlier, "camera_inlier": camera_inlier, "counts": named(c, COUNT_FIELDS), "counts_raw": c,
               "tier": "lds" if int(c[2]) <= limit else "workspace"}
        if want_position:
            out["position"] = position
        return out

    def upload(self, pair_images, pair_direction, pair_enable, rotation, rotation_valid, intrinsics, track_off, image, uv, track_enable, meas_enable, directions):
        """Host arrays -> the twelve device tensors ``inliers`` takes, in its order (None stays None)."""
        up = self._up
        return (up(pair_images, np.int32, (-1, 2)), up(pair_direction, np.float64, (-1, 3)), up(pair_enable, np.uint8, (-1,)), up(rotation, np.float64, (-1, 9)),
                up(rotation_valid, np.uint8, (-1,)), up(intrinsics, np.float64, (-1, 4)), up(track_off, np.int64, (-1,)), up(image, np.int32, (-1,)),
                up(uv, np.float32, (-1, 2)), up(track_enable, np.uint8, (-1,)), up(meas_enable, np.uint8, (-1,)), up(directions, np.float64, (-1, 3)))

    def upload_world(self, world_pair, world_meas):
        """Host world directions [E, 3] and [S, 3] -> the ``world=`` pair of ``inliers``."""
        return self._up(world_pair, np.float64, (-1, 3)), self._up(world_meas, np.float64, (-1, 3))
