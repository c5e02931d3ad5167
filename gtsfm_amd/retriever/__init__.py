"""Image-pair retrievers (``gtsfm/retriever``): short-name exports (``_target_: gtsfm_amd.retriever.Similarity``)."""

from .joint_similarity_sequential_retriever import JointSimilaritySequentialRetriever
from .sequential_retriever import SequentialRetriever
from .similarity_retriever import SimilarityRetriever

JointSimilaritySequential = JointSimilaritySequentialRetriever
Similarity = SimilarityRetriever

__all__ = ["JointSimilaritySequential", "JointSimilaritySequentialRetriever", "SequentialRetriever", "Similarity", "SimilarityRetriever"]
