"""Drop-in for ``gtsfm/common/two_view_estimation_report.py``: what is known about the estimate on one edge (i1, i2). The fields, their
order and their defaults are the reference's, so that its consumers (metrics, the inlier support processor, the view graph) read them
unchanged. ``i2Ri1`` / ``i2Ui1`` hold whatever the verifier plugin returns (gtsam's ``Rot3`` / ``Unit3`` where gtsam is installed, numpy
arrays elsewhere)."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Optional

import numpy as np


@dataclass(frozen=False)
class TwoViewEstimationReport:
    v_corr_idxs: np.ndarray  # verified correspondence indices
    num_inliers_est_model: float  # correspondences consistent with the estimated model
    inlier_ratio_est_model: Optional[float] = None  # the former over the putative matches
    num_inliers_gt_model: Optional[float] = None  # correspondences that are correct under the ground truth
    inlier_ratio_gt_model: Optional[float] = None
    v_corr_idxs_inlier_mask_gt: Optional[np.ndarray] = None
    R_error_deg: Optional[float] = None
    U_error_deg: Optional[float] = None
    i2Ri1: Optional[Any] = None
    i2Ui1: Optional[Any] = None
    reproj_error_gt_model: Optional[np.ndarray] = None
    inlier_avg_reproj_error_gt_model: Optional[float] = None
    outlier_avg_reproj_error_gt_model: Optional[float] = None
