"""Graph utilities on the MI355X HIP path: drop-ins for the functions of ``gtsfm/utils/graph.py:24-149`` that the view-graph stage uses,
with the same names and signatures. The triplets come from ``gtsfm_view_graph_cycle_filter_f64`` (its triplet list, with identity rotations:
only the graph matters) and the largest component from ``gtsfm_largest_component``.

The order of the returned lists is a contract here (triplets lexicographic, nodes ascending), where the reference returns the iteration
order of a Python set."""

from __future__ import annotations

import logging
from collections import defaultdict
from typing import Any, DefaultDict, Dict, List, Optional, Sequence, Set, Tuple

import numpy as np

logger = logging.getLogger("gtsfm_amd")

_ENGINE = None


def _engine():
    global _ENGINE
    if _ENGINE is None:
        from gtsfm_amd.runtime.view_graph_engine import ViewGraphEngine

        _ENGINE = ViewGraphEngine()
    return _ENGINE


def create_adjacency_list(edges: Sequence[Tuple[int, int]]) -> DefaultDict[int, Set[int]]:
    """An image index -> the set of its neighbours (host: the device keeps its own sorted lists)."""
    adj_list: DefaultDict[int, Set[int]] = defaultdict(set)
    for a, b in edges:
        adj_list[a].add(b)
        adj_list[b].add(a)
    return adj_list


def normalise_edges(edges: Sequence[Tuple[int, int]]) -> np.ndarray:
    """[E, 2] int32 with i1 < i2, each pair once, in lexicographic order: the reference's set logic ((b, a) is the edge (a, b), an edge listed
    twice is one edge), done on the host because the device call refuses both."""
    arr = np.asarray([(min(int(a), int(b)), max(int(a), int(b))) for a, b in edges], dtype=np.int64).reshape(-1, 2)
    if len(arr) and (arr[:, 0] == arr[:, 1]).any():
        raise ValueError("an edge joins an image to itself")
    if len(arr) and (arr.min() < 0 or arr.max() >= (1 << 28)):
        raise ValueError("image indices must lie in 0 .. 2^28 - 1")
    return (np.unique(arr, axis=0) if len(arr) else arr).astype(np.int32)


def extract_cyclic_triplets_from_edges(edges: Sequence[Tuple[int, int]]) -> List[Tuple[int, int, int]]:
    """The 3-cycles of the graph, each once with its nodes sorted, in lexicographic order."""
    pairs = normalise_edges(edges)
    if len(pairs) == 0:
        return []
    engine = _engine()
    pair_images, rotation, _ = engine.upload(pairs, np.tile(np.eye(3).reshape(9), (len(pairs), 1)))
    out = engine.cycle_filter(pair_images, rotation, None, num_images=int(pairs.max()) + 1, want_triplets=True)
    return [tuple(t) for t in out["triplets"].cpu().numpy().tolist()]


def get_nodes_in_largest_connected_component(edges: Sequence[Tuple[int, int]]) -> List[int]:
    """The nodes of the largest connected component, ascending; of equally large ones the component of the first such edge listed."""
    if len(edges) == 0:
        return []
    pairs = np.asarray([(int(a), int(b)) for a, b in edges], dtype=np.int32).reshape(-1, 2)
    if pairs.min() < 0:
        raise ValueError("image indices must not be negative")
    engine = _engine()
    pair_images, _, _ = engine.upload(pairs)
    out = engine.largest_component(pair_images, None, num_images=int(pairs.max()) + 1)
    logger.info("Largest of %d connected components: %d nodes.", out["counts"]["components"], out["counts"]["nodes"])
    return [int(v) for v in np.flatnonzero(out["node_mask"].cpu().numpy())]


def prune_to_largest_connected_component(rotations: Dict[Tuple[int, int], Optional[Any]], unit_translations: Dict[Tuple[int, int], Optional[Any]],
                                         relative_pose_priors: Dict[Tuple[int, int], Any]) -> Tuple[Dict[Tuple[int, int], Any], Dict[Tuple[int, int], Any]]:
    """The subsets of the two dicts whose keys have both nodes in the largest connected component of the edges with a rotation followed by
    the edges of ``relative_pose_priors``. A key whose value is None is kept when both its nodes are in that component, as in the reference."""
    input_edges = [k for (k, v) in rotations.items() if v is not None]
    input_edges += relative_pose_priors.keys()
    nodes_in_pruned_graph = set(get_nodes_in_largest_connected_component(input_edges))
    selected_edges = [(i1, i2) for i1, i2 in rotations.keys() if i1 in nodes_in_pruned_graph and i2 in nodes_in_pruned_graph]
    logger.info("Pruned to largest connected component with %d nodes and %d edges.", len(nodes_in_pruned_graph), len(selected_edges))
    return {k: rotations[k] for k in selected_edges}, {k: unit_translations[k] for k in selected_edges}
