"""Data association on the MI355X HIP path: feature tracks from verified matches."""

from gtsfm_amd.data_association.dsf_tracks_estimator import CppDsfTracksEstimator, DsfTracksEstimator, get_2d_tracks  # noqa: F401
from gtsfm_amd.data_association.tracks_estimator_base import TracksEstimatorBase  # noqa: F401
