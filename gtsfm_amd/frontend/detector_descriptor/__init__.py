from gtsfm_amd.frontend.detector_descriptor.d2net import D2NetDetDesc  # noqa: F401
from gtsfm_amd.frontend.detector_descriptor.sift import SIFTDetectorDescriptor  # noqa: F401
