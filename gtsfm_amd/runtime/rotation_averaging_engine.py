"""Host side of the device's rotation averaging: ``gtsfm_rotation_averaging_f64`` runs what ``ShonanRotationAveraging`` asks of gtsam
(``gtsfm/averaging/rotation/shonan.py:122-204``: the chordal initialisation and the chordal cost at p = 3) on the pair rows
``(i1, i2, i2Ri1)`` where they lie. PyTorch provides device memory and streams only."""

from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from gtsfm_amd.runtime.engine_base import EngineBase, merge_options

COUNTER_FIELDS = ("status", "outer_iterations", "accepted_steps", "hessian_applications", "chordal_cg_steps", "component_size", "anchor", "valid_rows")
COST_FIELDS = ("initial_cost", "chordal_cost", "final_cost", "gradient_inf_norm")
STATUS_NAMES = ("CONVERGED", "MAX_ITERATIONS", "NO_VALID_ROW", "NON_FINITE")
CONVERGED, MAX_ITERATIONS, NO_VALID_ROW, NON_FINITE = 0, 1, 2, 3
# chosen on the restatement (tests/rotation_averaging_reference.py): see its scenes for the iteration counts they give
DEFAULTS = dict(chordal_tol=1e-10, chordal_max_iterations=2000, delta0=1.0, kappa_cg=0.1, theta=1.0, gradient_tol=1e-9, max_outer=100, max_inner=0)


class RotationAveragingEngine(EngineBase):
    def average(self, pair_images, rotation, weight, pair_enable=None, *, num_images: int, anchor: int = -1, problem_row_off=None, **options) -> Dict[str, object]:
        """Device tensors as in include/gtsfm_amd.h: ``pair_images`` [E, 2] int32 = (i1, i2), ``rotation`` [E, 9] float64 = i2Ri1, ``weight`` [E]
        float64, ``pair_enable`` [E] uint8 or None, ``problem_row_off`` [P + 1] int64 or None (one problem over every row). ``options``: the keys
        of ``DEFAULTS``. Returns device tensors ``wRi`` [P, N, 9] and ``node_valid`` [P, N], and, read back, ``counters`` [P, 8] int32, ``costs``
        [P, 4] float64 and ``status`` (a list of names). The inputs are not changed."""
        torch = self._torch
        dev = self.device
        o = merge_options(DEFAULTS, options)
        e, n = int(pair_images.shape[0]), int(num_images)
        p = 1 if problem_row_off is None else int(problem_row_off.shape[0]) - 1
        if p < 1:
            raise ValueError("problem_row_off must be [P + 1] with P >= 1")
        self._check_tensors((("pair_images", pair_images, torch.int32, 2 * e), ("rotation", rotation, torch.float64, 9 * e), ("weight", weight, torch.float64, e),
                             ("pair_enable", pair_enable, torch.uint8, e), ("problem_row_off", problem_row_off, torch.int64, p + 1)), optional=("pair_enable", "problem_row_off"))
        ws = self._sized_workspace("gtsfm_rotation_averaging_workspace_bytes", e, n, p)
        wri = torch.empty((p, n, 9), dtype=torch.float64, device=dev)
        node_valid = torch.empty((p, n), dtype=torch.uint8, device=dev)
        counters = torch.empty((p, 8), dtype=torch.int32, device=dev)
        costs = torch.empty((p, 4), dtype=torch.float64, device=dev)
        q = self._ptr
        rc = self._lib.gtsfm_rotation_averaging_f64(
            q(pair_images), q(rotation), q(weight), q(pair_enable), e, n, q(problem_row_off), p, int(anchor), float(o["chordal_tol"]), int(o["chordal_max_iterations"]),
            float(o["delta0"]), float(o["kappa_cg"]), float(o["theta"]), float(o["gradient_tol"]), int(o["max_outer"]), int(o["max_inner"]), ws.data_ptr(), ws.numel(),
            q(wri), q(node_valid), counters.data_ptr(), costs.data_ptr(), self._stream())
        self._L.check(rc, "gtsfm_rotation_averaging_f64")
        c = counters.cpu().numpy()
        return {"wRi": wri, "node_valid": node_valid, "counters": c, "costs": costs.cpu().numpy(), "status": [STATUS_NAMES[int(s)] for s in c[:, 0]]}

    def upload(self, pair_images, rotation, weight, pair_enable=None, problem_row_off=None):
        """Host arrays -> the five device tensors ``average`` takes, in its order (None stays None)."""
        up = self._up
        return (up(pair_images, np.int32, (-1, 2)), up(rotation, np.float64, (-1, 9)), up(weight, np.float64, (-1,)), up(pair_enable, np.uint8, (-1,)),
                up(problem_row_off, np.int64, (-1,)))
