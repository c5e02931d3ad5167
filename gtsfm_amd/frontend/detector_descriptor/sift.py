"""SIFT detector-descriptor plugin on the MI355X HIP path.

Drop-in for ``gtsfm/frontend/detector_descriptor/sift.py``: same class name (the front-end cachers key on ``type(obj).__name__``), the
base class's constructor (``max_keypoints=5000``) and the same ``detect_and_describe`` signature; the engine is built lazily, so the object
pickles before any device state exists. The reference wraps ``cv.SIFT_create().detectAndCompute``; here OpenCV's algorithm with its
default parameters runs as hand-written HIP (``gtsfm_amd/csrc/sift_kernels.hip``) and cv2 is not needed.

Deviations ("SIFT"): the returned arrays are ordered by response descending, equal responses by (octave, layer, row,
column, angle) -- OpenCV orders by coordinates and the reference's ``get_top_k`` is an unordered ``argpartition``; the parameters of
``SIFT_create`` are fixed at their defaults (the reference never passes any)."""

from __future__ import annotations

from typing import Tuple

import numpy as np

from gtsfm_amd.common.image import Image
from gtsfm_amd.common.keypoints import Keypoints
from gtsfm_amd.frontend.detector_descriptor.detector_descriptor_base import DetectorDescriptorBase

DESCRIPTOR_DIM = 128


class SIFTDetectorDescriptor(DetectorDescriptorBase):
    """OpenCV's SIFT on gfx950 behind the reference's detector-descriptor plugin interface."""

    _model = None  # SiftEngine, built in the process that first calls detect_and_describe

    def __getstate__(self):
        return {**self.__dict__, "_model": None}

    def _ensure_model_loaded(self) -> None:
        if self._model is not None:
            return
        from gtsfm_amd.frontend.registry import MODEL_LOAD_LOCK

        with MODEL_LOAD_LOCK:
            if self._model is not None:
                return
            from gtsfm_amd.runtime.sift_engine import SiftEngine

            self._model = SiftEngine()

    def detect_and_describe(self, image: Image) -> Tuple[Keypoints, np.ndarray]:
        """Keypoints ((N, 2) float32 coordinates, (N,) scales = OpenCV's ``kp.size``, (N,) responses; N <= max_keypoints, strongest
        first) and (N, 128) float32 descriptors holding the integers 0 .. 255 that cv2 returns."""
        from gtsfm_amd.runtime.sift_engine import check_image

        array = np.asarray(image.value_array)
        check_image(array)
        self._ensure_model_loaded()
        xy, sizes, responses, descriptors = self._model.detect(array, self.max_keypoints, image.mask)
        if len(xy) == 0:
            return Keypoints(coordinates=np.zeros((0, 2), dtype=np.float32), scales=sizes, responses=responses), np.zeros((0, DESCRIPTOR_DIM), dtype=np.float32)
        return Keypoints(coordinates=xy, scales=sizes, responses=responses), descriptors
