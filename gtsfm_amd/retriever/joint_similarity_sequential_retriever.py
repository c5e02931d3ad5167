"""Similarity + sequential retriever (``gtsfm/retriever/joint_similarity_sequential_retriever.py``): the union of the two pair lists,
``list(set(sim_pairs).union(set(seq_pairs)))`` as the reference evaluates it (so the order is the same)."""

from __future__ import annotations

import logging

from gtsfm_amd.retriever.retriever_base import RetrieverBase
from gtsfm_amd.retriever.sequential_retriever import SequentialRetriever
from gtsfm_amd.retriever.similarity_retriever import SimilarityRetriever

logger = logging.getLogger(__name__)


class JointSimilaritySequentialRetriever(RetrieverBase):
    def __init__(self, num_matched: int, min_score: float, max_frame_lookahead: int) -> None:
        self._num_matched = num_matched
        self._similarity_retriever = SimilarityRetriever(num_matched=num_matched, min_score=min_score)
        self._seq_retriever = SequentialRetriever(max_frame_lookahead=max_frame_lookahead)

    def set_max_frame_lookahead(self, n) -> None:
        self._seq_retriever.set_max_frame_lookahead(n)

    def set_num_matched(self, n) -> None:
        self._num_matched = n
        self._similarity_retriever.set_num_matched(n)

    def __repr__(self) -> str:
        return f"JointSimilaritySequentialRetriever({self._similarity_retriever!r}, {self._seq_retriever!r})"

    def get_image_pairs(self, global_descriptors, image_fnames, plots_output_dir=None):
        sim_pairs = self._similarity_retriever.get_image_pairs(global_descriptors=global_descriptors, image_fnames=image_fnames,
                                                               plots_output_dir=plots_output_dir)
        seq_pairs = self._seq_retriever.get_image_pairs(global_descriptors=None, image_fnames=image_fnames, plots_output_dir=plots_output_dir)
        return self._aggregate_pairs(sim_pairs=sim_pairs, seq_pairs=seq_pairs)

    def _aggregate_pairs(self, sim_pairs, seq_pairs):
        pairs = list(set(sim_pairs).union(set(seq_pairs)))
        logger.info("Found %d pairs from the Similarity + Sequential Retriever.", len(pairs))
        return pairs
