"""Host side of similarity retrieval: ``gtsfm_retrieval_topk`` computes S = D D^T in exact fp32 on the device and keeps each row's
best columns j > i (``gtsfm/retriever/similarity_retriever.py:98-245``); the host lists the pairs row-major over (i, rank).
PyTorch provides device memory and streams only."""

from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from gtsfm_amd.runtime.engine_base import EngineBase


def pairs_from_topk(idx: np.ndarray) -> List[Tuple[int, int]]:
    """[N][k] column indices (-1 = empty rank) -> (i, j) pairs, row-major over (i, rank): the order of the reference's
    ``zip(*np.where(valid))``."""
    rows, ranks = np.nonzero(idx >= 0)
    return [(int(i), int(idx[i, r])) for i, r in zip(rows, ranks)]


class RetrievalEngine(EngineBase):
    """Lib handle and a cached workspace; one instance per process / GPU."""

    WS_SLACK = "exact"

    def topk(self, descriptors, k: int, min_score: Optional[float], blocksize: int = 50, with_sim: bool = False):
        """``descriptors``: (N, D) float32, host array or tensor (CPU or device). Returns device tensors idx [N][min(k, N)] int32,
        scores [N][min(k, N)] float32 and, with ``with_sim``, the (N, N) similarity in the reference's block layout (else None)."""
        torch = self._torch
        d = descriptors if isinstance(descriptors, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(descriptors))
        if d.dim() != 2:
            raise ValueError(f"descriptors must be an (N, D) array (got shape {tuple(d.shape)})")
        d = d.to(device=self.device, dtype=torch.float32).contiguous()
        n, dim = int(d.shape[0]), int(d.shape[1])
        kk = max(0, min(int(k), n))
        need = int(self._lib.gtsfm_retrieval_workspace_bytes(n, dim, int(with_sim)))
        if need == 0:
            raise ValueError(f"retrieval needs at least one descriptor of dimension >= 1 (got shape {(n, dim)})")
        ws = self._grow(need)
        idx = torch.empty((n, kk), dtype=torch.int32, device=self.device)
        scores = torch.empty((n, kk), dtype=torch.float32, device=self.device)
        sim = torch.empty((n, n), dtype=torch.float32, device=self.device) if with_sim else None
        threshold = float("-inf") if min_score is None else float(min_score)
        rc = self._lib.gtsfm_retrieval_topk(d.data_ptr(), n, dim, int(k), threshold, int(blocksize), idx.data_ptr(), scores.data_ptr(),
                                            None if sim is None else sim.data_ptr(), ws.data_ptr(), ws.numel(),
                                            self._L.current_stream_handle())
        self._L.check(rc, "gtsfm_retrieval_topk")
        return idx, scores, sim

    def pairs(self, descriptors, k: int, min_score: Optional[float]) -> List[Tuple[int, int]]:
        idx, _, _ = self.topk(descriptors, k, min_score)
        return pairs_from_topk(idx.cpu().numpy())
