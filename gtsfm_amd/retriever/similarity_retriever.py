"""Similarity retriever on the MI355X HIP path: drop-in for ``gtsfm/retriever/similarity_retriever.py`` (class name, constructor,
``get_image_pairs``, ``compute_similarity_matrix``, ``set_num_matched``, ``save_diagnostics``). One device call computes S = D D^T
in exact fp32 and each row's best ``num_matched`` columns j > i with S[i][j] >= min_score (``gtsfm_retrieval_topk``); the pairs are
listed row-major over (image, rank) like the reference's ``pairs_from_score_matrix``.

Deviations: equal scores are ranked by the lower column index (``torch.topk`` makes no promise); descriptors of
another float dtype are converted to float32 (the reference's einsum would run in that dtype); NaN scores are never selected; the
host copy of the similarity matrix behind ``_latest_similarity_matrix`` is made when it is first read."""

from __future__ import annotations

import logging
import os
from pathlib import Path
from typing import List, Optional

import numpy as np

from gtsfm_amd.retriever.retriever_base import RetrieverBase

logger = logging.getLogger(__name__)
MAX_NUM_IMAGES = 10000


def _stack(global_descriptors) -> np.ndarray:
    num_images = len(global_descriptors)
    if num_images > MAX_NUM_IMAGES:
        raise RuntimeError("Cannot construct similarity matrix of this size.")
    return np.ascontiguousarray(np.array(global_descriptors), dtype=np.float32)


class SimilarityRetriever(RetrieverBase):
    def __init__(self, num_matched: int, min_score: float = 0.1, blocksize: int = 50) -> None:
        self._num_matched = num_matched
        self._blocksize = blocksize
        self._min_score = min_score
        self._latest_similarity_matrix = None
        self._engine = None

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_engine"] = None
        state["_latest_sim"] = None
        return state

    def __repr__(self) -> str:
        return f"SimilarityRetriever(num_matched={self._num_matched}, blocksize={self._blocksize}, min_score={self._min_score})"

    # The CPU copy of the latest similarity matrix is made on first read; the device copy is kept until then.
    @property
    def _latest_similarity_matrix(self):
        sim = self.__dict__.get("_latest_sim")
        if sim is not None and sim.device.type != "cpu":
            sim = sim.cpu()
            self.__dict__["_latest_sim"] = sim
        return sim

    @_latest_similarity_matrix.setter
    def _latest_similarity_matrix(self, value) -> None:
        self.__dict__["_latest_sim"] = value

    def set_num_matched(self, n) -> None:
        self._num_matched = n

    def _ensure_engine(self):
        if self._engine is None:
            from gtsfm_amd.frontend.registry import MODEL_LOAD_LOCK
            from gtsfm_amd.runtime.retrieval_engine import RetrievalEngine

            with MODEL_LOAD_LOCK:
                if self._engine is None:
                    self._engine = RetrievalEngine()
        return self._engine

    def compute_similarity_matrix(self, global_descriptors: List[np.ndarray]):
        """(N, N) CPU float32 tensor in the reference's block layout: (i, j) = D_i . D_j iff j // blocksize >= i // blocksize, else 0."""
        import torch

        desc = _stack(global_descriptors)
        if len(desc) == 0:
            return torch.zeros((0, 0))
        _, _, sim = self._ensure_engine().topk(desc, 0, None, self._blocksize, with_sim=True)
        return sim.cpu()

    def get_image_pairs(self, global_descriptors: Optional[List[np.ndarray]], image_fnames: List[str], plots_output_dir: Optional[Path] = None):
        if global_descriptors is None:
            raise ValueError("Global descriptors need to be provided")
        from gtsfm_amd.runtime.retrieval_engine import pairs_from_topk

        desc = _stack(global_descriptors)
        if len(desc) == 0:
            self._latest_similarity_matrix = None
            return []
        idx, _, sim = self._ensure_engine().topk(desc, self._num_matched, self._min_score, self._blocksize, with_sim=True)
        self._latest_similarity_matrix = sim
        pairs = pairs_from_topk(idx.cpu().numpy())
        logger.info("Found %d pairs from the Similarity Retriever.", len(pairs))
        return pairs

    def save_diagnostics(self, image_fnames: List[str], pairs, plots_output_dir: Optional[Path]) -> None:
        """similarity_matrix.txt and similarity_named_pairs.txt as the reference writes them; the heatmap only where matplotlib imports."""
        if plots_output_dir is None:
            return
        sim_cpu = self._latest_similarity_matrix
        if sim_cpu is None:
            logger.warning("No cached similarity matrix available to save.")
            return
        plots_output_dir = Path(plots_output_dir)
        os.makedirs(plots_output_dir, exist_ok=True)
        try:
            import matplotlib.pyplot as plt
        except Exception:  # noqa: BLE001
            plt = None
        if plt is not None:
            plt.imshow(np.triu(sim_cpu.numpy()))
            plt.title("Image Similarity Matrix")
            plt.savefig(str(plots_output_dir / "similarity_matrix.jpg"), dpi=500)
            plt.close("all")
        np.savetxt(fname=str(plots_output_dir / "similarity_matrix.txt"), X=sim_cpu.numpy(), fmt="%.2f", delimiter=",")
        with open(plots_output_dir / "similarity_named_pairs.txt", "w") as fid:
            for i, j in pairs:
                fid.write("%.4f %s %s\n" % (sim_cpu[i, j].item(), image_fnames[i], image_fnames[j]))
        self._latest_similarity_matrix = None
