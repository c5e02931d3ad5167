"""What every single-workspace engine shares: the device, the library handle, one cached workspace that grows when a call needs more
(sized by the size function an engine names), the check of the tensors a call is given, NULL for an absent or empty tensor, the
current stream's handle and the upload helpers; and, for their results and options, counters by name and options over defaults."""

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


def named(row, fields, cast=int):
    """One row of counters (or costs, with ``cast=float``) as a dict by ``fields``; spare columns past the names are dropped."""
    return {k: cast(row[i]) for i, k in enumerate(fields)}


def merge_options(defaults, options):
    """``options`` over ``defaults``; a key that ``defaults`` does not have is a ``TypeError``, as an unknown keyword is."""
    unknown = set(options) - set(defaults)
    if unknown:
        raise TypeError(f"unknown options {sorted(unknown)}")
    return dict(defaults, **options)


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

    def _sized_workspace(self, size_fn: str, *sizes):
        """The workspace, as large as the library's ``size_fn(*sizes)`` asks; 0 is its refusal of the sizes."""
        need = int(getattr(self._lib, size_fn)(*sizes))
        if need == 0:
            raise ValueError(f"{size_fn} refuses {sizes}")
        return self._grow(need)

    def _check_tensors(self, rows, optional=()):
        """Every ``(name, tensor, dtype, count)`` row is a contiguous device tensor of that dtype and size; a name in ``optional`` may be None."""
        for name, x, dt, count in rows:
            if x is None and name in optional:
                continue
            if not (isinstance(x, self._torch.Tensor) and x.is_cuda and x.dtype == dt and x.is_contiguous() and x.numel() == count):
                raise TypeError(f"{name} must be a contiguous {dt} device tensor of {max(count, 0)} entries")

    @staticmethod
    def _ptr(x):
        """The address of a tensor; NULL for None and for an empty one."""
        return None if x is None or x.numel() == 0 else x.data_ptr()

    def _stream(self) -> int:
        return self._torch.cuda.current_stream(self.device).cuda_stream

    def _up(self, a, np_dtype, shape):
        """A host array on the device as a contiguous ``np_dtype`` tensor of ``shape``; None stays None. What every ``upload()`` is made of."""
        return None if a is None else self._torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np_dtype).reshape(shape))).to(self.device)

    def _dev(self, a, dtype):
        """``a`` on the device as a contiguous ``dtype`` tensor: a tensor is converted where it lies, anything else goes up through numpy."""
        torch = self._torch
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        np_dtype = {torch.int32: np.int32, torch.int64: np.int64, torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64}[dtype]
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np_dtype)).to(self.device)
