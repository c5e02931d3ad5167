"""Rotation averaging on the MI355X HIP path: chordal initialisation and a Riemannian trust region on the chordal cost (Shonan at p = 3)."""

from gtsfm_amd.averaging.rotation.rotation_averaging_base import RotationAveragingBase  # noqa: F401
from gtsfm_amd.averaging.rotation.shonan import RotationAverages, ShonanRotationAveraging  # noqa: F401
