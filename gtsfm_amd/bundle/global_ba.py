"""``GlobalBundleAdjustment``, the name ``gtsfm/bundle/global_ba.py`` gives the multi-view optimiser's ``BundleAdjustmentOptimizer``."""

from gtsfm_amd.bundle.bundle_adjustment import BundleAdjustmentOptimizer, RobustBAMode  # noqa: F401


class GlobalBundleAdjustment(BundleAdjustmentOptimizer):
    pass
