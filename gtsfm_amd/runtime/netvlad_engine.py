"""Host side of the NetVLAD global descriptor: the checkpoint parse, the weight packing and ``gtsfm_netvlad_forward``
(``gtsfm_amd/csrc/netvlad_kernels.hip``). PyTorch provides device memory and streams only; every stage of the model runs in the
library, and there is no fallback.

The checkpoint is the file the reference reads, ``VGG16-NetVLAD-Pitts30K.mat`` (netvlad_tf_open's ``net_class2struct.m`` export),
parsed as ``thirdparty/hloc/netvlad.py:125-163`` does. It is never downloaded: a missing file raises ``FileNotFoundError``."""

from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Dict, List, Optional, Union

import numpy as np

from gtsfm_amd.runtime.engine_base import EngineBase

NUM_CONVS = 13
# index of each VGG16 convolution among the backbone's 29 children (conv / ReLU / max-pool), = its index in ``net.layers``
CONV_LAYER_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
NETVLAD_LAYER, WHITEN_LAYER = 30, 33
DESCRIPTOR_DIM, VLAD_DIM = 4096, 32768
EPS = 1e-6  # the reference's input range tolerance (netvlad.py:27,177)


def load_checkpoint(path: Union[str, Path], whiten: bool = True) -> Dict[str, np.ndarray]:
    """The ``.mat`` parse: conv weights S x S x IN x OUT -> OUT x IN x S x S, layer 30's weights[0] (D x K) transposed as the score
    projection, centres = -weights[1], layer 33 (1 x 1 x IN x OUT, squeezed) transposed as the whitening, ``averageImage[0, 0]`` as the
    mean. Returns float32 arrays in torch layouts."""
    import scipy.io

    path = Path(path)
    if not path.exists():
        raise FileNotFoundError(f"NetVLAD checkpoint not found: {path} (gtsfm_amd never downloads weights)")
    mat = scipy.io.loadmat(str(path), struct_as_record=False, squeeze_me=True)
    layers = mat["net"].layers
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))  # noqa: E731
    out: Dict[str, np.ndarray] = {}
    for i, li in enumerate(CONV_LAYER_INDEX):
        out[f"conv{i}.weight"] = f32(np.asarray(layers[li].weights[0]).transpose(3, 2, 0, 1))
        out[f"conv{i}.bias"] = f32(layers[li].weights[1])
    out["score_w"] = f32(np.asarray(layers[NETVLAD_LAYER].weights[0]).T)
    out["centers"] = f32(-np.asarray(layers[NETVLAD_LAYER].weights[1]))
    if whiten:
        out["whiten.weight"] = f32(np.asarray(layers[WHITEN_LAYER].weights[0]).squeeze().T)
        out["whiten.bias"] = f32(np.asarray(layers[WHITEN_LAYER].weights[1]).squeeze())
    out["mean"] = f32(np.asarray(mat["net"].meta.normalization.averageImage[0, 0]))
    return out


def tensor_order(whiten: bool) -> List[str]:
    names = [n for i in range(NUM_CONVS) for n in (f"conv{i}.weight", f"conv{i}.bias")] + ["score_w", "centers", "mean"]
    return names + (["whiten.weight", "whiten.bias"] if whiten else [])


def pack_weights(weights: Dict[str, object], whiten: bool = True) -> np.ndarray:
    """Named weights (numpy arrays or CPU tensors, torch layouts) -> the packed float32 blob of ``gtsfm_netvlad_pack_weights``."""
    from gtsfm_amd.runtime import lib as _lib

    lib = _lib.load()
    names = tensor_order(whiten)
    missing = [n for n in names if n not in weights]
    if missing:
        raise KeyError(f"NetVLAD weights are missing {missing}")
    arrays = []
    for n in names:
        a = weights[n]
        a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        arrays.append(np.ascontiguousarray(a, dtype=np.float32))
    expect = {"score_w": (64, 512), "centers": (512, 64), "mean": (3,), "whiten.weight": (DESCRIPTOR_DIM, VLAD_DIM), "whiten.bias": (DESCRIPTOR_DIM,)}
    for n, a in zip(names, arrays):
        if n in expect and a.shape != expect[n]:
            raise ValueError(f"NetVLAD weight {n} has shape {a.shape}, expected {expect[n]}")
    ptrs = (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
    out = np.empty(lib.gtsfm_netvlad_packed_weight_floats(int(whiten)), dtype=np.float32)
    _lib.check(lib.gtsfm_netvlad_pack_weights(ptrs, int(whiten), out.ctypes.data), "gtsfm_netvlad_pack_weights")
    return out


class NetVLADEngine(EngineBase):
    """Packed weights resident on one device, a cached workspace; one instance per process / GPU."""

    WS_SLACK = "exact"

    def __init__(self, weights: Dict[str, object], device=None, whiten: bool = True):
        super().__init__(device)
        self.whiten = bool(whiten)
        self._weights = self._torch.from_numpy(pack_weights(weights, whiten)).to(self.device)
        self._flag = self._torch.zeros(1, dtype=self._torch.int32, device=self.device)

    @classmethod
    def from_checkpoint(cls, path: Union[str, Path], device=None, whiten: bool = True) -> "NetVLADEngine":
        return cls(load_checkpoint(path, whiten), device, whiten)

    def _workspace(self, b: int, h: int, w: int):
        need = int(self._lib.gtsfm_netvlad_workspace_bytes(b, h, w))
        if need == 0:
            # the reference raises RuntimeError too (torch's max_pool2d: the fourth pool's output would be empty)
            raise RuntimeError(f"NetVLAD needs images of at least 16 x 16 pixels (got a batch of {b} x {h} x {w})")
        return self._grow(need)

    def _prepare(self, images):
        """(B, 3, H, W) float (any float dtype: converted to float32) or (B, H, W, 3) uint8, CPU or device -> (device tensor, layout, B, H, W).
        A device tensor stays on the device."""
        torch = self._torch
        if images.dim() != 4:
            raise AssertionError(f"NetVLAD takes a (B, 3, H, W) batch (got shape {tuple(images.shape)})")
        if images.dtype == torch.uint8:
            if images.shape[3] != 3:
                raise AssertionError(f"a uint8 batch must be (B, H, W, 3) (got {tuple(images.shape)})")
            layout, (b, h, w) = 1, images.shape[:3]
        else:
            if images.shape[1] != 3:
                raise AssertionError(f"NetVLAD takes 3-channel images (got shape {tuple(images.shape)})")
            images = images.to(torch.float32)
            layout, b, h, w = 0, images.shape[0], images.shape[2], images.shape[3]
        images = images.to(self.device, non_blocking=True).contiguous()
        return images, layout, int(b), int(h), int(w)

    def describe(self, images, whiten: Optional[bool] = None):
        """Descriptors of a batch as a device tensor, (B, 4096) with whitening, (B, 32768) without. Raises ``AssertionError`` when a
        float image is outside [-1e-6, 1 + 1e-6] or holds a NaN (the reference's assert); the check reads one flag after the call."""
        torch = self._torch
        whiten = self.whiten if whiten is None else bool(whiten)
        if whiten and not self.whiten:
            raise ValueError("this engine was loaded without the whitening weights")
        images, layout, b, h, w = self._prepare(images)
        out = torch.empty((b, DESCRIPTOR_DIM if whiten else VLAD_DIM), dtype=torch.float32, device=self.device)
        ws = self._workspace(b, h, w)
        self._flag.zero_()
        rc = self._lib.gtsfm_netvlad_forward(self._weights.data_ptr(), images.data_ptr(), layout, b, h, w, int(whiten), out.data_ptr(),
                                             self._flag.data_ptr(), ws.data_ptr(), ws.numel(), self._L.current_stream_handle())
        self._L.check(rc, "gtsfm_netvlad_forward")
        if layout == 0 and int(self._flag.item()) != 0:
            raise AssertionError("NetVLAD input outside [0, 1] (the reference asserts image.min() >= -1e-6 and image.max() <= 1 + 1e-6)")
        return out

    def stage(self, images, stage: int):
        """Stage-wise outputs (device): 0 = relu(conv1_1) [B][H][W][64], 1 = conv5_3 [B][H/16][W/16][512], 2 = pre-whitening [B][32768]."""
        torch = self._torch
        images, layout, b, h, w = self._prepare(images)
        shapes = {0: (b, h, w, 64), 1: (b, h // 2 // 2 // 2 // 2, w // 2 // 2 // 2 // 2, 512), 2: (b, VLAD_DIM)}
        if stage not in shapes:
            raise ValueError(f"stage must be 0, 1 or 2 (got {stage})")
        out = torch.empty(shapes[stage], dtype=torch.float32, device=self.device)
        ws = self._workspace(b, h, w)
        rc = self._lib.gtsfm_netvlad_stage(self._weights.data_ptr(), images.data_ptr(), layout, b, h, w, stage, out.data_ptr(), ws.data_ptr(),
                                           ws.numel(), self._L.current_stream_handle())
        self._L.check(rc, "gtsfm_netvlad_stage")
        return out
