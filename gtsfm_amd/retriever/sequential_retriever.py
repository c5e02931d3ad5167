"""Sequential retriever (``gtsfm/retriever/sequential_retriever.py``), host only: pairs (i1, i2) with 0 < i2 - i1 <= max_frame_lookahead."""

from __future__ import annotations

import logging

from gtsfm_amd.retriever.retriever_base import RetrieverBase

logger = logging.getLogger(__name__)


class SequentialRetriever(RetrieverBase):
    def __init__(self, max_frame_lookahead: int) -> None:
        self._max_frame_lookahead = max_frame_lookahead

    def __repr__(self) -> str:
        return f"SequentialRetriever(max_frame_lookahead={self._max_frame_lookahead})"

    def set_max_frame_lookahead(self, n) -> None:
        self._max_frame_lookahead = n

    def get_image_pairs(self, global_descriptors, image_fnames, plots_output_dir=None):
        num_images = len(image_fnames)
        pairs = [(i1, i2) for i1 in range(num_images) for i2 in range(i1 + 1, min(i1 + self._max_frame_lookahead + 1, num_images))]
        logger.info("Found %d pairs from the SequentialRetriever", len(pairs))
        return pairs
