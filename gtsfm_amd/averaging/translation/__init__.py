"""Translation averaging on the MI355X HIP path: 1DSfM outlier rejection (MFAS over sampled projection directions) and translation recovery."""

from gtsfm_amd.averaging.translation.averaging_1dsfm import (  # noqa: F401
    ProjectionSamplingMethod,
    TranslationAverages,
    TranslationAveraging1DSFM,
    TranslationInliers,
    device_translation_recovery,
    get_valid_measurements_in_world_frame,
)
