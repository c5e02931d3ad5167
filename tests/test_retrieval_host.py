"""CPU: the retriever contract on the restated pairs_from_score_matrix, the plugin's host-side checks (no descriptors, too many
images), the joint retriever's union order and the sequential retriever."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import netvlad_reference as nr


def _scores(rows):
    return torch.tensor(rows, dtype=torch.float32)


def test_k_values_and_order():
    s = torch.from_numpy(np.random.default_rng(0).permutation(36).reshape(6, 6).astype(np.float32) / 36)
    assert nr.pairs_from_score_matrix(s, 0) == []
    one = nr.pairs_from_score_matrix(s, 1)
    assert [i for i, _ in one] == [0, 1, 2, 3, 4]
    full = nr.pairs_from_score_matrix(s, 6)
    assert full == nr.pairs_from_score_matrix(s, 60) and len(full) == 15
    assert [i for i, _ in full] == sorted(i for i, _ in full)  # row-major over (i, rank)
    for i in range(6):
        js = [j for a, j in full if a == i]
        assert [float(s[i, j]) for j in js] == sorted((float(s[i, j]) for j in js), reverse=True)
    assert len(nr.pairs_from_score_matrix(s, 10)) == 15


def test_threshold_compares_in_float32():
    assert not bool(torch.tensor(np.float32(0.7)) < 0.7)  # torch compares against float32(0.7)
    assert np.float64(np.float32(0.7)) < 0.7
    s = _scores([[0, 0.7, 0.6], [0, 0, 0.7], [0, 0, 0]])
    assert nr.pairs_from_score_matrix(s, 5, 0.7) == [(0, 1), (1, 2)]


def test_tie_rule():
    s = _scores([[0, 0.5, 0.5, 0.5], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]])
    assert nr.pairs_from_score_matrix(s, 3) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def test_retriever_host_checks():
    from gtsfm_amd.retriever import Similarity

    r = Similarity(num_matched=10, min_score=0.3)
    with pytest.raises(ValueError):
        r.get_image_pairs(None, ["a.jpg"])
    with pytest.raises(RuntimeError):
        r.get_image_pairs([np.zeros(4, dtype=np.float32)] * 10001, ["x"] * 10001)
    with pytest.raises(RuntimeError):
        nr.similarity_matrix([np.zeros(4, dtype=np.float32)] * 10001)
    assert nr.pairs_from_score_matrix(nr.similarity_matrix([np.ones(4, dtype=np.float32)]), 10, 0.3) == []
    with pytest.raises(AttributeError):
        Similarity(3).set_max_frame_lookahead(2)
    assert r.evaluate(5, [(0, 1)]) is not None


def test_joint_union_order_and_sequential():
    from gtsfm_amd.retriever import JointSimilaritySequential, SequentialRetriever

    assert SequentialRetriever(2).get_image_pairs(None, ["a"] * 5) == nr.sequential_pairs(5, 2) == [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3), (2, 4), (3, 4)]
    j = JointSimilaritySequential(num_matched=2, min_score=0.3, max_frame_lookahead=1)
    sim_pairs, seq_pairs = [(0, 3), (1, 4)], nr.sequential_pairs(5, 1)
    assert j._aggregate_pairs(sim_pairs, seq_pairs) == list(set(sim_pairs).union(set(seq_pairs)))
    j.set_num_matched(4)
    assert j._similarity_retriever._num_matched == 4
