"""Translation averaging on the MI355X HIP path: 1DSfM outlier rejection (MFAS over sampled projection directions)."""

from gtsfm_amd.averaging.translation.averaging_1dsfm import (  # noqa: F401
    ProjectionSamplingMethod,
    TranslationAveraging1DSFM,
    TranslationInliers,
    get_valid_measurements_in_world_frame,
)
