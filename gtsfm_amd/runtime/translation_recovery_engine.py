"""Host side of the device's translation recovery: ``gtsfm_translation_recovery_f64`` runs what ``TranslationAveraging1DSFM`` asks of gtsam's
``TranslationRecovery`` (``gtsfm/averaging/translation/averaging_1dsfm.py:439-495``) on the arrays ``gtsfm_translation_inliers_f64`` takes and
leaves on the device: the pair rows and track measurements with their world directions and the two inlier masks. PyTorch provides device
memory and streams only."""

from __future__ import annotations

from typing import Dict

import numpy as np

from gtsfm_amd.runtime.engine_base import EngineBase, merge_options

COUNTER_FIELDS = ("status", "outer_iterations", "accepted_steps", "hessian_applications", "init_cg_steps", "component_size", "anchor", "valid_rows")
COST_FIELDS = ("init_cost", "final_cost", "gradient_inf_norm", "trust_radius")
STATUS_NAMES = ("CONVERGED", "MAX_ITERATIONS", "NO_VALID_ROW", "NON_FINITE")
CONVERGED, MAX_ITERATIONS, NO_VALID_ROW, NON_FINITE = 0, 1, 2, 3
# sigma and huber_k are the reference's NOISE_MODEL_SIGMA and HUBER_LOSS_K; rel_tol and abs_tol gtsam's documented LM defaults; the rest was
# chosen on the restatement (tests/translation_recovery_reference.py): see its scenes for the iteration counts they give
DEFAULTS = dict(scale_factor=1.0, sigma=0.01, huber_k=1.3, init_tol=1e-10, init_max_iterations=2000, delta0=1e4, kappa_cg=0.1, gradient_tol=1e-9, rel_tol=1e-5,
                abs_tol=1e-5, max_outer=100, max_inner=0)


class TranslationRecoveryEngine(EngineBase):
    def recover(self, pair_images, world_pair, pair_enable, track_off, image, world_meas, meas_enable, *, num_images: int, anchor: int = -1, problem_row_off=None,
                **options) -> Dict[str, object]:
        """Device tensors as in include/gtsfm_amd.h: ``pair_images`` [E, 2] int32 = (i1, i2), ``world_pair`` [E, 3] float64 = w_i2Ui1, ``pair_enable``
        [E] uint8 or None, ``track_off`` [T + 1] int64 or None (no tracks), ``image`` [S] int32, ``world_meas`` [S, 3] float64, ``meas_enable`` [S] uint8
        or None. ``problem_row_off`` [P + 1, 2] = (first pair row, first track) per problem, a HOST array (the widest problem sizes the outputs) or
        None: one problem over everything. ``options``: the keys of ``DEFAULTS``. Returns device tensors ``translation`` [P, M, 3] and ``node_valid``
        [P, M] with M = num_images + the most tracks of a problem (cameras first, then the problem's tracks), and, read back, ``counters`` [P, 8]
        int32, ``costs`` [P, 4] float64 and ``status`` (a list of names). The inputs are not changed."""
        torch = self._torch
        dev = self.device
        o = merge_options(DEFAULTS, options)
        e, n = int(pair_images.shape[0]) if pair_images is not None else 0, int(num_images)
        t = 0 if track_off is None else int(track_off.shape[0]) - 1
        s = 0 if image is None else int(image.shape[0])
        if t < 0:
            raise ValueError("track_off must be [T + 1]")
        off_dev, p, t_max = None, 1, t
        if problem_row_off is not None:
            off = np.ascontiguousarray(np.asarray(problem_row_off.cpu() if isinstance(problem_row_off, torch.Tensor) else problem_row_off, dtype=np.int64).reshape(-1, 2))
            p = len(off) - 1
            if p < 1:
                raise ValueError("problem_row_off must be [P + 1, 2] with P >= 1")
            t_max = int(min(max(int(np.diff(off[:, 1]).max()), 0), t))
            off_dev = torch.from_numpy(off).to(dev)
        spec = (("pair_images", pair_images, torch.int32, 2 * e), ("world_pair", world_pair, torch.float64, 3 * e), ("pair_enable", pair_enable, torch.uint8, e),
                ("track_off", track_off, torch.int64, t + 1), ("image", image, torch.int32, s), ("world_meas", world_meas, torch.float64, 3 * s),
                ("meas_enable", meas_enable, torch.uint8, s))
        self._check_tensors(spec, optional={"pair_enable", "meas_enable", "track_off"} | {row[0] for row in spec if row[3] == 0})  # or nothing to hold
        m = n + t_max
        ws = self._sized_workspace("gtsfm_translation_recovery_workspace_bytes", e, s, n, t, t_max, p)
        translation = torch.empty((p, m, 3), dtype=torch.float64, device=dev)
        node_valid = torch.empty((p, m), dtype=torch.uint8, device=dev)
        counters = torch.empty((p, 8), dtype=torch.int32, device=dev)
        costs = torch.empty((p, 4), dtype=torch.float64, device=dev)
        q = self._ptr
        rc = self._lib.gtsfm_translation_recovery_f64(
            q(pair_images), q(world_pair), q(pair_enable), e, q(track_off) if t > 0 else None, q(image), q(world_meas), q(meas_enable), t, s, n, q(off_dev), p, t_max, int(anchor),
            float(o["scale_factor"]), float(o["sigma"]), float(o["huber_k"]), float(o["init_tol"]), int(o["init_max_iterations"]), float(o["delta0"]), float(o["kappa_cg"]),
            float(o["gradient_tol"]), float(o["rel_tol"]), float(o["abs_tol"]), int(o["max_outer"]), int(o["max_inner"]), ws.data_ptr(), ws.numel(), q(translation),
            q(node_valid), counters.data_ptr(), costs.data_ptr(), self._stream())
        self._L.check(rc, "gtsfm_translation_recovery_f64")
        c = counters.cpu().numpy()
        return {"translation": translation, "node_valid": node_valid, "counters": c, "costs": costs.cpu().numpy(), "status": [STATUS_NAMES[int(k)] for k in c[:, 0]]}

    def upload(self, pair_images, world_pair, pair_enable=None, track_off=None, image=None, world_meas=None, meas_enable=None):
        """Host arrays -> the seven device tensors ``recover`` takes, in its order (None stays None)."""
        up = self._up
        return (up(pair_images, np.int32, (-1, 2)), up(world_pair, np.float64, (-1, 3)), up(pair_enable, np.uint8, (-1,)), up(track_off, np.int64, (-1,)),
                up(image, np.int32, (-1,)), up(world_meas, np.float64, (-1, 3)), up(meas_enable, np.uint8, (-1,)))
