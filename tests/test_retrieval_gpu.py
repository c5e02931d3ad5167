"""GPU: similarity retrieval (gtsfm_retrieval_topk, SimilarityRetriever) against the CPU restatement of the reference's
pairs_from_score_matrix: clustered unit descriptors whose decisions all lie >= 1e-5 from their boundaries (asserted in float64), the
documented tie rule on exact integer descriptors, k from 0 to N and past 64 (the general path), the block layout of
compute_similarity_matrix and the -inf-free cached matrix."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import netvlad_reference as nr

pytestmark = pytest.mark.gpu


def clustered(n: int, d: int = 4096, seed: int = 0) -> np.ndarray:
    """Unit descriptors in clusters of 4 (within-cluster similarity ~0.35 - 0.99, across ~0): float32 rows."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal(((n + 3) // 4, d))
    noise = rng.standard_normal((n, d)) * rng.uniform(0.1, 1.2, size=(n, 1))
    x = centres[np.arange(n) // 4] + noise
    x = x[rng.permutation(n)]
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def engine():
    from gtsfm_amd.runtime.retrieval_engine import RetrievalEngine

    return RetrievalEngine()


@pytest.mark.parametrize("n", [6, 50, 1000, 5000])
def test_clustered_pairs_equal_restatement(engine, n):
    from gtsfm_amd.runtime.retrieval_engine import pairs_from_topk

    desc = clustered(n, seed=n)
    sim = nr.similarity_matrix(list(desc))
    for k, min_score in [(1, 0.3), (2, 0.5), (10, 0.3), (100, 0.3)]:
        nr.assert_margins(desc.astype(np.float64), k, min_score)
        idx, scores, _ = engine.topk(desc, k, min_score)
        assert idx.shape == (n, min(k, n))
        assert pairs_from_topk(idx.cpu().numpy()) == nr.pairs_from_score_matrix(sim, k, min_score), (n, k, min_score)
        s, i = scores.cpu().numpy(), idx.cpu().numpy()
        assert np.array_equal(np.isfinite(s), i >= 0)
        for row in s:
            assert np.all(np.diff(row[np.isfinite(row)]) <= 0)


def _integer_descriptors(n: int, d: int, seed: int) -> np.ndarray:
    """Small integers / 8: every product and sum is exact in float32, so the device's similarity equals the restatement's bit for bit
    and exact ties are real."""
    return (np.random.default_rng(seed).integers(-3, 4, size=(n, d)) / 8.0).astype(np.float32)


@pytest.mark.parametrize("n,d,k,min_score", [(7, 5, 3, None), (64, 3, 5, 0.0), (300, 6, 300, None), (300, 6, 200, 0.25), (130, 7, 129, None),
                                             (200, 33, 65, None)])
def test_exact_ties_and_general_path(engine, n, d, k, min_score):
    from gtsfm_amd.runtime.retrieval_engine import pairs_from_topk

    desc = _integer_descriptors(n, d, seed=n + d)
    sim = nr.similarity_matrix(list(desc))
    idx, _, _ = engine.topk(desc, k, min_score)
    assert pairs_from_topk(idx.cpu().numpy()) == nr.pairs_from_score_matrix(sim, k, min_score)


def test_tie_rule_lower_column_first(engine):
    """The row [0, .5, .5, .5] with k = 3 gives [1, 2, 3] (torch's CPU topk gives [2, 3, 1] here)."""
    desc = np.array([[1.0, 0.0], [0.5, 0.5], [0.5, -0.5], [0.5, 0.25]], dtype=np.float32)
    idx, scores, _ = engine.topk(desc, 3, None)
    assert idx.cpu().numpy()[0].tolist() == [1, 2, 3]
    assert scores.cpu().numpy()[0].tolist() == [0.5, 0.5, 0.5]
    dup = np.repeat(clustered(8, 64, seed=3), 2, axis=0)  # a dataset holding every image twice
    sim = nr.similarity_matrix(list(dup))
    idx, _, _ = engine.topk(dup, 4, 0.3)
    from gtsfm_amd.runtime.retrieval_engine import pairs_from_topk

    assert pairs_from_topk(idx.cpu().numpy()) == nr.pairs_from_score_matrix(sim, 4, 0.3)


def test_k_range_and_threshold_equality(engine):
    from gtsfm_amd.runtime.retrieval_engine import pairs_from_topk

    desc = _integer_descriptors(40, 4, seed=1)
    sim = nr.similarity_matrix(list(desc))
    for k in (0, 1, 10, 40, 41, 1000):
        idx, _, _ = engine.topk(desc, k, None)
        assert idx.shape == (40, min(k, 40))
        assert pairs_from_topk(idx.cpu().numpy()) == nr.pairs_from_score_matrix(sim, k, None)
    # a score exactly float32(0.7) is kept (torch compares in float32)
    a = np.array([[1.0, 0.0], [np.float32(0.7), 0.0], [0.6, 0.0]], dtype=np.float32)
    idx, _, _ = engine.topk(a, 5, 0.7)
    assert pairs_from_topk(idx.cpu().numpy()) == [(0, 1)] == nr.pairs_from_score_matrix(nr.similarity_matrix(list(a)), 5, 0.7)


def test_retriever_plugin_contract():
    from gtsfm_amd.retriever import JointSimilaritySequential, Similarity

    desc = list(clustered(120, 256, seed=7))
    fnames = [f"{i}.jpg" for i in range(len(desc))]
    r = Similarity(num_matched=5, min_score=0.3)
    pairs = r.get_image_pairs(desc, fnames)
    assert pairs == nr.pairs_from_score_matrix(nr.similarity_matrix(desc), 5, 0.3)
    cached = r._latest_similarity_matrix
    assert cached.device.type == "cpu" and torch.isfinite(cached).all()
    sim = r.compute_similarity_matrix(desc)
    ref = nr.similarity_matrix(desc)
    blk = torch.arange(120) // 50
    filled = blk[None, :] >= blk[:, None]
    assert torch.all(sim[~filled] == 0) and torch.allclose(sim[filled], ref[filled], atol=1e-6)
    r.set_num_matched(2)
    assert r.get_image_pairs(desc, fnames) == nr.pairs_from_score_matrix(nr.similarity_matrix(desc), 2, 0.3)
    assert Similarity(3, None).get_image_pairs(desc[:1], fnames[:1]) == []
    j = JointSimilaritySequential(num_matched=5, min_score=0.3, max_frame_lookahead=2)
    sim_pairs = nr.pairs_from_score_matrix(nr.similarity_matrix(desc), 5, 0.3)
    assert j.get_image_pairs(desc, fnames) == list(set(sim_pairs).union(set(nr.sequential_pairs(len(desc), 2))))
    # float64 descriptors are converted to float32
    assert Similarity(5, 0.3).get_image_pairs([d.astype(np.float64) for d in desc], fnames) == pairs


def test_plugin_several_strips_block_layout():
    """N = 2500 (three 1024-row strips, two of them starting inside a 50-block; blocksize 50): the plugin's pairs equal the
    restatement's and the pairs of the path without the similarity output; compute_similarity_matrix and the cached matrix hold the
    reference's block layout."""
    from gtsfm_amd.retriever import Similarity
    from gtsfm_amd.runtime.retrieval_engine import RetrievalEngine, pairs_from_topk

    n = 2500
    desc = list(clustered(n, 512, seed=25))
    nr.assert_margins(np.array(desc, dtype=np.float64), 10, 0.3)
    ref = nr.similarity_matrix(desc)
    expect = nr.pairs_from_score_matrix(ref, 10, 0.3)
    r = Similarity(num_matched=10, min_score=0.3, blocksize=50)
    pairs = r.get_image_pairs(desc, [f"{i}.jpg" for i in range(n)])
    assert pairs == expect
    idx, _, _ = RetrievalEngine().topk(np.array(desc), 10, 0.3)
    assert pairs_from_topk(idx.cpu().numpy()) == expect
    blk = torch.arange(n) // 50
    filled = blk[None, :] >= blk[:, None]
    for sim in (r._latest_similarity_matrix, r.compute_similarity_matrix(desc)):
        assert sim.shape == (n, n) and torch.isfinite(sim).all()
        assert torch.all(sim[~filled] == 0)
        assert torch.allclose(sim[filled], ref[filled], atol=1e-6)
