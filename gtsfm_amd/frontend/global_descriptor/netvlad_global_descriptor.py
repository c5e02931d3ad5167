"""NetVLAD global descriptor on the MI355X HIP path: drop-in for ``gtsfm/frontend/global_descriptor/netvlad_global_descriptor.py``
(class name, constructor without required arguments, ``describe_batch`` returning one float32 (4096,) row per image,
``get_preprocessing_transforms``). The model (``thirdparty/hloc/netvlad.py``) runs as hand-written HIP
(``gtsfm_amd/csrc/netvlad_kernels.hip``); the object pickles without device state and builds its engine on first use.

Deviations: the checkpoint is never downloaded (a missing file raises ``FileNotFoundError``); the input range is
checked on the device and reported after the forward, as an ``AssertionError`` like the reference's."""

from __future__ import annotations

from pathlib import Path
from typing import Union

import numpy as np

from gtsfm_amd.frontend.global_descriptor.global_descriptor_base import GlobalDescriptorBase

ROOT_PATH = Path(__file__).resolve().parent.parent.parent.parent
MODEL_WEIGHTS_PATH = ROOT_PATH / "thirdparty" / "hloc" / "weights" / "VGG16-NetVLAD-Pitts30K.mat"


def _to_chw_tensor(x):
    """HWC array -> CHW uint8 tensor (the reference's resize transform: ``torch.from_numpy(np.array(x, copy=True)).permute(2, 0, 1)``)."""
    import torch

    return torch.from_numpy(np.array(x, copy=True)).permute(2, 0, 1)


def _to_unit_float(x):
    """The reference's batch transform: ``x.type(torch.float32) / 255.0``."""
    import torch

    return x.type(torch.float32) / 255.0


class NetVLADGlobalDescriptor(GlobalDescriptorBase):
    """NetVLAD global descriptor (HIP / gfx950)."""

    def __init__(self, weights_path: Union[Path, str] = MODEL_WEIGHTS_PATH) -> None:
        super().__init__()
        self._weights_path = Path(weights_path)
        self._model = None  # lazy: the device engine is built on first use, in the worker

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_model"] = None
        return state

    def __repr__(self) -> str:
        return f"NetVLADGlobalDescriptor(weights_path={str(self._weights_path)!r})"

    def _ensure_model_loaded(self) -> None:
        if self._model is not None:
            return
        from gtsfm_amd.frontend.registry import MODEL_LOAD_LOCK
        from gtsfm_amd.runtime.netvlad_engine import NetVLADEngine

        with MODEL_LOAD_LOCK:
            if self._model is None:
                self._model = NetVLADEngine.from_checkpoint(self._weights_path)

    def get_preprocessing_transforms(self):
        """(HWC uint8 -> CHW tensor, CHW uint8 -> float32 / 255), as plain callables (torchvision's ``Compose`` / ``Lambda`` in the reference)."""
        return _to_chw_tensor, _to_unit_float

    def describe_batch(self, images) -> list:
        """(B, 3, H, W) float tensor in [0, 1] (CPU or device) -> B float32 (4096,) arrays."""
        if images.dim() != 4 or images.shape[1] != 3:
            raise AssertionError(f"NetVLAD takes a (B, 3, H, W) batch (got shape {tuple(images.shape)})")
        self._ensure_model_loaded()
        out = self._model.describe(images).cpu().numpy()
        return [desc for desc in out]
