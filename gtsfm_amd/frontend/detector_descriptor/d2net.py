"""D2-Net detector-descriptor plugin (single scale) on the MI355X HIP path.

Drop-in for ``gtsfm/frontend/detector_descriptor/d2net.py``: same class name (the front-end cachers key on ``type(obj).__name__``), same
constructor and ``detect_and_describe`` signatures, ``FileNotFoundError`` at construction when the checkpoint is missing, lazy engine so
that the object pickles before any device state exists. The model (``thirdparty/d2net/lib/{model_test,pyramid,utils}.py``) runs as
hand-written HIP (``gtsfm_amd/csrc/d2net_kernels.hip``, ``dense_kernels.hip``).

Deviations: the checkpoint is never downloaded; equal scores are ordered by (channel, row, column) where the
reference's ``np.argsort`` makes no promise; an image beyond the reference's size limits raises ``ValueError`` (the reference calls
``scipy.misc.imresize``, which current SciPy does not have, so it raises there too); multi-scale (``USE_MULTISCALE``, ``False`` in the
reference) is not implemented."""

from __future__ import annotations

from pathlib import Path
from typing import Tuple, Union

import numpy as np

from gtsfm_amd.common.image import Image
from gtsfm_amd.common.keypoints import Keypoints
from gtsfm_amd.frontend.detector_descriptor.detector_descriptor_base import DetectorDescriptorBase

MAX_EDGE_PX = 1600
MAX_SUM_EDGES_PX = 2800
USE_MULTISCALE = False

MODEL_PATH = Path(__file__).resolve().parent.parent.parent.parent / "thirdparty" / "d2net" / "weights" / "d2_tf.pth"


class D2NetDetDesc(DetectorDescriptorBase):
    """D2-Net on gfx950 behind the reference's detector-descriptor plugin interface."""

    def __init__(self, max_keypoints: int = 5000, model_path: Union[Path, str] = MODEL_PATH, use_cuda: bool = True) -> None:
        super().__init__()
        self.max_keypoints = max_keypoints
        self.model_path = Path(model_path)
        self.use_cuda = use_cuda
        if not self.model_path.exists():  # same failure point as the reference: construction
            raise FileNotFoundError(
                f"D2-Net weights not found at {self.model_path}. Fetch them with scripts/download_model_weights.sh or pass model_path=."
            )
        self._model = None  # D2NetEngine, built in the process that first calls detect_and_describe

    def __getstate__(self):
        return {**self.__dict__, "_model": None}

    def _ensure_model_loaded(self) -> None:
        if self._model is not None:
            return
        from gtsfm_amd.frontend.registry import MODEL_LOAD_LOCK, warn_if_cpu_requested

        with MODEL_LOAD_LOCK:
            if self._model is not None:
                return
            warn_if_cpu_requested(bool(self.use_cuda), "D2NetDetDesc")
            from gtsfm_amd.runtime.d2net_engine import D2NetEngine

            self._model = D2NetEngine.from_checkpoint(self.model_path)

    def detect_and_describe(self, image: Image) -> Tuple[Keypoints, np.ndarray]:
        """Keypoints ((N, 2) float32 coordinates, (N,) responses, N <= max_keypoints, strongest first) and (N, 512) float32 unit descriptors."""
        array = np.asarray(image.value_array)
        check_size(array.shape)
        self._ensure_model_loaded()
        xy, responses, descriptors = self._model.detect(array, self.max_keypoints)
        return Keypoints(coordinates=xy, responses=responses), descriptors


def check_size(shape: Tuple[int, ...], max_edge_px: int = MAX_EDGE_PX, max_sum_edges_px: int = MAX_SUM_EDGES_PX) -> None:
    """The reference downsamples an image whose longest edge exceeds 1600 px or whose height + width exceeds 2800 px with
    ``scipy.misc.imresize`` (d2net.py:120-125), a function SciPy removed in 1.3: with a current SciPy the reference raises
    ``AttributeError`` there. This plugin does not restate that resize; it raises ``ValueError`` and says so."""
    if len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] != 3):
        raise ValueError(f"D2NetDetDesc takes (H, W, 3) or (H, W) images (got shape {tuple(shape)})")
    full = tuple(shape) if len(shape) == 3 else (*shape, 3)
    if max(full) > max_edge_px or sum(full[:2]) > max_sum_edges_px:
        raise ValueError(
            f"image of {full[0]} x {full[1]} pixels exceeds D2-Net's limits (longest edge {max_edge_px}, height + width {max_sum_edges_px}); the "
            "reference would downsample it with scipy.misc.imresize, which SciPy no longer has, and this plugin does not restate that resize: "
            "downsample the image first"
        )
