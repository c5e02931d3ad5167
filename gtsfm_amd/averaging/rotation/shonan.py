"""``ShonanRotationAveraging`` on the device: a drop-in for ``gtsfm/averaging/rotation/shonan.py``. The host logic is the reference's, quirks
included; what it asks of gtsam (the chordal initialisation and ``ShonanAveraging3.run`` at p = 3) is ``gtsfm_rotation_averaging_f64``.

PARITY UNPINNED towards gtsam, none of which was observed running: its Levenberg-Marquardt path, the soft anchor, the Karcher and gauge
terms, ``Rot3::ClosestTo`` in the last bits and its output gauge (here: the anchor's rotation is the identity). NOT DONE: the optimality
certificate and the rank staircase p > 3 -- the device returns a critical point reached from the chordal start."""

from __future__ import annotations

import logging
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from gtsfm_amd.averaging.rotation.rotation_averaging_base import RotationAveragingBase
from gtsfm_amd.view_graph_estimator.cycle_consistent_rotation_estimator import rotation_matrix

logger = logging.getLogger("gtsfm_amd")

_DEFAULT_TWO_VIEW_ROTATION_SIGMA = 1.0


def prior_rotation(prior: Any) -> np.ndarray:
    """i1Ri2 of a ``PosePrior``: ``prior.value`` is a pose with ``.rotation()``, a 4 x 4 or a 3 x 3 array."""
    value = prior.value
    if hasattr(value, "rotation"):
        return rotation_matrix(value.rotation())
    value = np.asarray(value, dtype=np.float64)
    return rotation_matrix(value[:3, :3] if value.shape == (4, 4) else value)


def prior_sigma(prior: Any) -> float:
    """The isotropic sigma of a prior: the square root of the mean diagonal entry of its covariance."""
    return float(np.sqrt(np.average(np.diag(np.asarray(prior.covariance, dtype=np.float64)), axis=None)))


class RotationAverages:
    """What ``VerifiedScene.rotation_averaging`` returns. ``wRi_list``: a 3 x 3 array or None per image (the argument of
    ``translation_inliers`` and the rotations of the cameras for ``triangulate``); ``status``: CONVERGED, MAX_ITERATIONS, NO_VALID_ROW or
    NON_FINITE; ``counters`` and ``costs``: the device's, as dicts; ``pairs``, ``weight`` and ``enabled``: the rows that were given."""

    def __init__(self, wRi_list, status, counters, costs, pairs, weight, enabled):  # noqa: N803
        self.wRi_list, self.status, self.counters, self.costs = wRi_list, status, counters, costs  # noqa: N815
        self.pairs, self.weight, self.enabled = pairs, weight, enabled

    @classmethod
    def empty(cls) -> "RotationAverages":
        """The result for a scene without rows."""
        from gtsfm_amd.runtime.rotation_averaging_engine import COST_FIELDS, COUNTER_FIELDS

        return cls([], "NO_VALID_ROW", dict.fromkeys(COUNTER_FIELDS, 0), dict.fromkeys(COST_FIELDS, float("nan")), [], np.zeros(0), np.zeros(0, np.uint8))


class ShonanRotationAveraging(RotationAveragingBase):
    """Performs rotation averaging on Shonan's chordal cost at p = 3."""

    def __init__(self, two_view_rotation_sigma: float = _DEFAULT_TWO_VIEW_ROTATION_SIGMA, weight_by_inliers: bool = True, use_chordal_init: bool = True,
                 device=None, **solver_options) -> None:
        """``solver_options``: the keys of ``gtsfm_amd.runtime.rotation_averaging_engine.DEFAULTS``."""
        if not use_chordal_init:
            raise NotImplementedError("use_chordal_init=False (gtsam's random start) is not available on the device")
        self._two_view_rotation_sigma = two_view_rotation_sigma
        self._p_min = 3
        self._p_max = 3
        self._weight_by_inliers = weight_by_inliers
        self._use_chordal_init = use_chordal_init
        self._solver_options = dict(solver_options)
        self._device = device
        self._engine = None  # lazy: the object must pickle before first use (Dask scatter)
        self.last_result = None  # status, counters and costs of the last run_rotation_averaging

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_engine"] = None
        return state

    def __repr__(self) -> str:
        return f"ShonanRotationAveraging(two_view_rotation_sigma={self._two_view_rotation_sigma}, weight_by_inliers={self._weight_by_inliers})"

    def engine(self, device=None):
        """The engine, made on first use on the constructor's ``device``, else on ``device`` (a scene's); the object's settings are not changed."""
        if getattr(self, "_engine", None) is None:
            from gtsfm_amd.runtime.rotation_averaging_engine import RotationAveragingEngine

            self._engine = RotationAveragingEngine(self._device if self._device is not None else device)
        return self._engine

    def solve_with_retry(self, solve):
        """``solve(weighted) -> (status name, result)``, once with ``weight_by_inliers`` as it stands; on a status other than CONVERGED with
        weights on, once more unweighted, and ``_weight_by_inliers`` STAYS False, as the reference leaves it after gtsam's RuntimeError. The one
        place this rule lives: ``run_rotation_averaging`` and ``VerifiedScene.rotation_averaging`` both go through it."""
        status, res = solve(bool(self._weight_by_inliers))
        if status != "CONVERGED" and self._weight_by_inliers is True:
            logger.error("Rotation averaging ended with %s; reattempting without inlier-weighted costs...", status)
            self._weight_by_inliers = False
            status, res = solve(False)
        return res

    def measurement_rows(self, i2Ri1_dict, i1Ti2_priors, v_corr_idxs, weight_by_inliers=None):  # noqa: N803
        """The rows (i1, i2, i2Ri1, kappa) as the reference builds its BinaryMeasurementsRot3: the two-view rotations in the dict's order, then
        the priors as rows (i2, i1, i1Ri2). kappa = 1 / sigma^2 with sigma = 1 / len(v_corr_idxs) per edge when weighting by inliers; an
        edge with zero correspondences keeps the noise model of the entry before it (``two_view_rotation_sigma`` if it is the first)."""
        pairs, rotation, weight = [], [], []
        weighted = self._weight_by_inliers if weight_by_inliers is None else weight_by_inliers
        sigma = float(self._two_view_rotation_sigma)
        for (i1, i2), i2Ri1 in i2Ri1_dict.items():  # noqa: N806
            if i2Ri1 is None:
                continue
            if weighted and len(v_corr_idxs[(i1, i2)]) > 0:
                sigma = 1.0 / len(v_corr_idxs[(i1, i2)])
            pairs.append((int(i1), int(i2)))
            rotation.append(rotation_matrix(i2Ri1).reshape(9))
            weight.append(1.0 / (sigma * sigma))
        for (i1, i2), prior in i1Ti2_priors.items():
            s = prior_sigma(prior)
            pairs.append((int(i2), int(i1)))
            rotation.append(prior_rotation(prior).reshape(9))
            weight.append(1.0 / (s * s))
        return np.asarray(pairs, np.int32).reshape(-1, 2), np.asarray(rotation, np.float64).reshape(-1, 9), np.asarray(weight, np.float64)

    def run_arrays(self, num_images: int, i2Ri1_dict, i1Ti2_priors, v_corr_idxs, weight_by_inliers=None) -> Dict[str, Any]:  # noqa: N803
        """One solve on the device: the rows, and on the host ``wRi`` [N, 9], ``node_valid`` [N], ``status`` (a name), ``counters`` and
        ``costs`` as dicts."""
        from gtsfm_amd.runtime.rotation_averaging_engine import COST_FIELDS, COUNTER_FIELDS

        pairs, rotation, weight = self.measurement_rows(i2Ri1_dict, i1Ti2_priors, v_corr_idxs, weight_by_inliers)
        engine = self.engine()
        dev = engine.upload(pairs, rotation, weight)
        out = engine.average(dev[0], dev[1], dev[2], None, num_images=int(num_images), **self._solver_options)
        return {"pair_images": pairs, "rotation": rotation, "weight": weight, "wRi": out["wRi"][0].cpu().numpy(), "node_valid": out["node_valid"][0].cpu().numpy(),
                "status": out["status"][0], "counters": dict(zip(COUNTER_FIELDS, (int(x) for x in out["counters"][0]))),
                "costs": dict(zip(COST_FIELDS, (float(x) for x in out["costs"][0])))}

    def run_rotation_averaging(self, num_images: int, i2Ri1_dict: Dict[Tuple[int, int], Optional[Any]], i1Ti2_priors: Dict[Tuple[int, int], Any],  # noqa: N803
                               v_corr_idxs: Dict[Tuple[int, int], np.ndarray]) -> List[Optional[np.ndarray]]:
        """Global rotations wRi (3 x 3 arrays) for the images of the anchor's component, None elsewhere. The anchor -- the second image of the
        first measurement, as ``measurements[0].key1()`` -- gets the identity."""
        if len(i2Ri1_dict) == 0:
            logger.warning("Shonan cannot proceed: No cycle-consistent triplets found after filtering.")
            return [None] * num_images
        # the reference's node set: every key, those of None-valued entries too; nothing outside it gets a rotation
        nodes_with_edges = {i for pair in list(i2Ri1_dict.keys()) + list(i1Ti2_priors.keys()) for i in pair}

        def solve(weighted):
            res = self.run_arrays(num_images, i2Ri1_dict, i1Ti2_priors, v_corr_idxs, weight_by_inliers=weighted)
            return res["status"], res

        res = self.solve_with_retry(solve)
        self.last_result = {k: res[k] for k in ("status", "counters", "costs")}
        return [res["wRi"][i].reshape(3, 3).copy() if i in nodes_with_edges and res["node_valid"][i] else None for i in range(num_images)]
