"""View-graph estimation on the MI355X HIP path: rotation cycle consistency over the triplets of the pair graph."""

from gtsfm_amd.view_graph_estimator.cycle_consistent_rotation_estimator import (  # noqa: F401
    CycleConsistentRotationViewGraphEstimator,
    EdgeErrorAggregationCriterion,
)
from gtsfm_amd.view_graph_estimator.view_graph_estimator_base import ViewGraphEstimatorBase  # noqa: F401
