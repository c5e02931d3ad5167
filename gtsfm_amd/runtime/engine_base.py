"""What every single-workspace engine shares: the device, the library handle, one cached workspace that grows when a call needs more,
and the host-or-device upload helper. An engine adds which size function it asks and what it raises when that function refuses."""

from __future__ import annotations

import numpy as np


def require_gpu(device=None):
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("gtsfm_amd requires an AMD GPU visible to PyTorch-ROCm; there is no CPU fallback.")
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


# WS_SLACK -> (bytes to allocate for a workspace of `need` bytes, whether the old buffer is dropped before the new one is allocated)
_SLACK = {
    "exact": (lambda need: need, True),  # the model engines: their workspaces are the largest allocations of a run, so two never coexist
    "pad": (lambda need: need + 256, False),
    "quarter": (lambda need: int(need * 1.25) + 256, False),  # engines whose batches vary from call to call
}


class EngineBase:
    """Lib handle and a cached workspace; one instance per process / GPU."""

    WS_SLACK = "pad"

    def __init__(self, device=None):
        import torch

        from gtsfm_amd.runtime import lib as _lib

        self._torch = torch
        self.device = require_gpu(device)
        self._L = _lib
        self._lib = _lib.load()
        self._ws = None

    def _grow(self, need: int):
        """The workspace, at least ``need`` bytes."""
        if self._ws is None or self._ws.numel() < need:
            size, drop_first = _SLACK[self.WS_SLACK]
            if drop_first:
                self._ws = None
            self._ws = self._torch.empty(size(need), dtype=self._torch.uint8, device=self.device)
        return self._ws

    def _dev(self, a, dtype):
        """``a`` on the device as a contiguous ``dtype`` tensor: a tensor is converted where it lies, anything else goes up through numpy."""
        torch = self._torch
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        np_dtype = {torch.int32: np.int32, torch.int64: np.int64, torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64}[dtype]
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype)).to(self.device)
