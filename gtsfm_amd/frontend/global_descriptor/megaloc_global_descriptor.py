"""MegaLoc global descriptor on the MI355X HIP path: drop-in for ``gtsfm/frontend/global_descriptor/megaloc_global_descriptor.py``
(class name, constructor without required arguments, ``describe_batch`` returning one float32 (8448,) row per image,
``get_preprocessing_transforms``). The model (``thirdparty/megaloc/megaloc.py``: DINOv2 ViT-B/14 + SALAD + linear) runs as hand-written
HIP (``gtsfm_amd/csrc/megaloc_kernels.hip``); the object pickles without device state and builds its engine on first use.

Deviations: the checkpoint is never downloaded (a missing file raises ``FileNotFoundError`` where the reference falls
back to random weights); heights / widths that are not multiples of 14 raise ``ValueError`` (the reference resizes inside ``forward``;
its own transforms never trigger that: 322 = 23 * 14); the resize transform is ``torch.nn.functional.interpolate`` (bilinear, antialias),
what torchvision's tensor ``Resize`` dispatches to, unpinned towards torchvision itself."""

from __future__ import annotations

from pathlib import Path
from typing import Union

import numpy as np

from gtsfm_amd.frontend.global_descriptor.global_descriptor_base import GlobalDescriptorBase

ROOT_PATH = Path(__file__).resolve().parent.parent.parent.parent
MODEL_WEIGHTS_PATH = ROOT_PATH / "thirdparty" / "megaloc" / "weights" / "megaloc.torch"
INPUT_SIZE = (322, 322)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _resize_to_input(x):
    """HWC uint8 array -> CHW uint8 tensor at 322 x 322 (the reference's resize transform: ``from_numpy``, ``permute(2, 0, 1)``,
    ``Resize((322, 322), antialias=True)``). On the host, like the reference's loader. For a uint8 tensor torchvision interpolates in
    float32 (bilinear, antialias), rounds and casts back; so does this."""
    import torch

    chw = torch.from_numpy(np.asarray(x)).permute(2, 0, 1)
    if tuple(chw.shape[1:]) == INPUT_SIZE:
        return chw.contiguous()
    out = torch.nn.functional.interpolate(chw[None].to(torch.float32), size=INPUT_SIZE, mode="bilinear", antialias=True, align_corners=False)
    return out.round().clamp(0, 255).to(torch.uint8)[0]


def _normalise(x):
    """The reference's batch transform: ``x.type(torch.float32) / 255.0``, then ``Normalize`` with the ImageNet mean / std (``(x - mean) / std``)."""
    import torch

    x = x.type(torch.float32) / 255.0
    mean = torch.as_tensor(IMAGENET_MEAN, dtype=torch.float32, device=x.device).view(-1, 1, 1)
    std = torch.as_tensor(IMAGENET_STD, dtype=torch.float32, device=x.device).view(-1, 1, 1)
    return (x - mean) / std


class MegaLocGlobalDescriptor(GlobalDescriptorBase):
    """MegaLoc global descriptor (HIP / gfx950)."""

    def __init__(self, weights_path: Union[Path, str] = MODEL_WEIGHTS_PATH) -> None:
        super().__init__()
        self._weights_path = Path(weights_path)
        self._model = None  # lazy: the device engine is built on first use, in the worker

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_model"] = None
        return state

    def __repr__(self) -> str:
        return f"MegaLocGlobalDescriptor(weights_path={str(self._weights_path)!r})"

    def _ensure_model_loaded(self) -> None:
        if self._model is not None:
            return
        from gtsfm_amd.frontend.registry import MODEL_LOAD_LOCK
        from gtsfm_amd.runtime.megaloc_engine import MegaLocEngine

        with MODEL_LOAD_LOCK:
            if self._model is None:
                self._model = MegaLocEngine.from_checkpoint(self._weights_path)

    def get_preprocessing_transforms(self):
        """(HWC uint8 -> CHW uint8 at 322 x 322, batch -> float32 / 255 normalised by the ImageNet statistics), as plain callables."""
        return _resize_to_input, _normalise

    def describe_batch(self, images) -> list:
        """(B, 3, H, W) normalised float tensor (CPU or device; a raw uint8 batch is normalised on the device) -> B float32 (feat_dim,) arrays."""
        if images.dim() != 4 or images.shape[1] != 3:
            raise AssertionError(f"MegaLoc takes a (B, 3, H, W) batch (got shape {tuple(images.shape)})")
        if images.shape[0] == 0:
            return []
        self._ensure_model_loaded()
        out = self._model.describe(images).cpu().numpy()
        return [desc for desc in out]
