"""The specification of the device's view-graph stage (include/gtsfm_amd.h, "View-graph estimation"), restated in numpy and networkx from
that contract: which rows are input edges, the triplets of the pair graph, the cycle error of a triplet, the
per-edge aggregate and the largest connected component. Vectorised over triplets, so the palace graph (4 139 edges, 28 583 triplets) takes
well under a second. ``cycle_error_mp`` evaluates the same definition with 50 digits (mpmath): the distance of the float64 restatement
from it is what the tests' tolerance is measured from.

The reference does this in ``gtsfm/view_graph_estimator/cycle_consistent_rotation_estimator.py:80-157``, ``gtsfm/utils/graph.py:24-149`` and
``gtsfm/utils/geometry_comparisons.py:137-159,226-241``; tests/test_view_graph_host.py holds this file to those functions, loaded live."""

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MIN_EDGE_ERROR, MEDIAN_EDGE_ERROR = 0, 1
CHUNK_BYTES = 1 << 26


def input_edge_mask(pair_images: np.ndarray, rotation: np.ndarray, enable: Optional[np.ndarray] = None) -> np.ndarray:
    """Enabled and nine finite numbers: the device form of ``_get_valid_input_edges``."""
    rot = np.asarray(rotation, np.float64).reshape(-1, 9)
    mask = np.isfinite(rot).all(axis=1)
    if enable is not None:
        mask &= np.asarray(enable).astype(bool)
    return mask


def check_enabled_edges(pair_images: np.ndarray, num_images: int, enable: Optional[np.ndarray] = None, ordered: bool = True) -> Optional[str]:
    """What the device refuses: the reason, or None."""
    pairs = np.asarray(pair_images, np.int64).reshape(-1, 2)
    if enable is not None:
        pairs = pairs[np.asarray(enable).astype(bool)]
    if len(pairs) == 0:
        return None
    if pairs.min() < 0 or pairs.max() >= num_images:
        return "range"
    if ordered and (pairs[:, 0] >= pairs[:, 1]).any():
        return "order"
    if ordered and len(np.unique(pairs, axis=0)) != len(pairs):
        return "duplicate"
    return None


def extract_triplets(edges: np.ndarray) -> np.ndarray:
    """Every (i0, i1, i2), i0 < i1 < i2, whose three pairs are all in ``edges`` [E, 2] (i < j, unique): int64 [T, 3] in lexicographic order.
    Per edge (a, b) the common neighbours are the AND of two rows of a dense adjacency over the compacted node ids."""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    if len(edges) == 0:
        return np.zeros((0, 3), np.int64)
    nodes, compact = np.unique(edges, return_inverse=True)
    compact = compact.reshape(-1, 2)
    order = np.lexsort((compact[:, 1], compact[:, 0]))
    compact = compact[order]
    n = len(nodes)
    adj = np.zeros((n, n), bool)
    adj[compact[:, 0], compact[:, 1]] = True
    adj[compact[:, 1], compact[:, 0]] = True
    out = []
    step = max(1, CHUNK_BYTES // max(n, 1))
    for at in range(0, len(compact), step):
        a, b = compact[at:at + step, 0], compact[at:at + step, 1]
        row, c = np.nonzero(adj[a] & adj[b])
        own = c > b[row]  # the lexicographically first edge of a triplet lists it
        out.append(np.stack([a[row][own], b[row][own], c[own]], axis=1))
    trip = np.concatenate(out) if out else np.zeros((0, 3), np.int64)
    return nodes[trip].astype(np.int64).reshape(-1, 3)


def cycle_errors(i1Ri0: np.ndarray, i2Ri1: np.ndarray, i2Ri0: np.ndarray, return_choice: bool = False):  # noqa: N803
    """The angle in degrees of M = i2Ri0^T . i2Ri1 . i1Ri0 for stacks [T, 3, 3], products in that order: matrix -> quaternion by the largest of
    the diagonal and the trace (the first largest), normalised, then 2 atan2(|q_xyz|, |q_w|). With ``return_choice`` also which of
    (m00, m11, m22, trace) decided, [T] in 0 .. 3."""
    r10, r21, r20 = (np.asarray(x, np.float64).reshape(-1, 3, 3) for x in (i1Ri0, i2Ri1, i2Ri0))
    m = np.matmul(np.matmul(r20.transpose(0, 2, 1), r21), r10)
    t = len(m)
    diag = np.stack([m[:, 0, 0], m[:, 1, 1], m[:, 2, 2]], axis=1)
    trace = diag[:, 0] + diag[:, 1] + diag[:, 2]
    choice = np.argmax(np.concatenate([diag, trace[:, None]], axis=1), axis=1)  # the first largest
    q = np.empty((t, 4))
    rows = np.arange(t)
    for i in range(3):
        sel = rows[choice == i]
        j, k = (i + 1) % 3, (i + 2) % 3
        q[sel, i] = 1 - trace[sel] + 2 * m[sel, i, i]
        q[sel, j] = m[sel, j, i] + m[sel, i, j]
        q[sel, k] = m[sel, k, i] + m[sel, i, k]
        q[sel, 3] = m[sel, k, j] - m[sel, j, k]
    sel = rows[choice == 3]
    q[sel, 0] = m[sel, 2, 1] - m[sel, 1, 2]
    q[sel, 1] = m[sel, 0, 2] - m[sel, 2, 0]
    q[sel, 2] = m[sel, 1, 0] - m[sel, 0, 1]
    q[sel, 3] = 1 + trace[sel]
    q = q / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])[:, None]
    angle = 2 * np.arctan2(np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]), np.abs(q[:, 3]))
    return (np.rad2deg(angle), choice) if return_choice else np.rad2deg(angle)


def cycle_error_mp(i1Ri0: np.ndarray, i2Ri1: np.ndarray, i2Ri0: np.ndarray, digits: int = 50, return_choice: bool = False):  # noqa: N803
    """The same definition for ONE triplet with ``digits`` digits; returned rounded to float64. With ``return_choice`` also which of
    (m00, m11, m22, trace) decided: the first largest."""
    import mpmath as mp

    with mp.workdps(digits):
        r10, r21, r20 = (mp.matrix(np.asarray(x, np.float64).reshape(3, 3).tolist()) for x in (i1Ri0, i2Ri1, i2Ri0))
        m = (r20.T * r21) * r10
        trace = m[0, 0] + m[1, 1] + m[2, 2]
        decision = [m[0, 0], m[1, 1], m[2, 2], trace]
        choice = max(range(4), key=lambda i: (decision[i], -i))
        q = [mp.mpf(0)] * 4
        if choice != 3:
            i, j, k = choice, (choice + 1) % 3, (choice + 2) % 3
            q[i] = 1 - trace + 2 * m[i, i]
            q[j] = m[j, i] + m[i, j]
            q[k] = m[k, i] + m[i, k]
            q[3] = m[k, j] - m[j, k]
        else:
            q = [m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], 1 + trace]
        norm = mp.sqrt(sum(x * x for x in q))
        q = [x / norm for x in q]
        angle = 2 * mp.atan2(mp.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), abs(q[3]))
        return (float(angle * 180 / mp.pi), choice) if return_choice else float(angle * 180 / mp.pi)


def triplet_rotations(triplets: np.ndarray, row_of: Dict[Tuple[int, int], int], rotation: np.ndarray):
    """(i1Ri0, i2Ri1, i2Ri0) stacks and the three edge rows [T, 3] = rows of (i0, i1), (i1, i2), (i0, i2)."""
    rot = np.asarray(rotation, np.float64).reshape(-1, 3, 3)
    rows = np.array([[row_of[(a, b)], row_of[(b, c)], row_of[(a, c)]] for a, b, c in triplets.tolist()], np.int64).reshape(-1, 3)
    return rot[rows[:, 0]], rot[rows[:, 1]], rot[rows[:, 2]], rows


def cycle_filter(pair_images: np.ndarray, rotation: np.ndarray, enable: Optional[np.ndarray] = None, num_images: Optional[int] = None,
                 criterion: int = MEDIAN_EDGE_ERROR, error_threshold: float = 7.0) -> Dict[str, object]:
    """The device call's outputs per edge row (``num_triplets`` int32, ``aggregate_error`` float64, ``keep`` uint8), ``counts`` [8],
    ``triplets`` [T, 3] int32 lexicographic with ``cycle_error`` [T]; also ``input`` (the input-edge mask), ``lists`` (row -> its errors in
    the order of the third node) and ``margin`` [E] = |aggregate - threshold| (inf where there is no aggregate)."""
    pairs = np.asarray(pair_images, np.int64).reshape(-1, 2)
    num_edges = len(pairs)
    if num_images is None:
        num_images = int(pairs.max()) + 1 if num_edges else 0
    reason = check_enabled_edges(pairs, num_images, enable)
    if reason:
        raise ValueError(reason)
    mask = input_edge_mask(pairs, rotation, enable) if num_edges else np.zeros(0, bool)
    rows_in = np.flatnonzero(mask)
    row_of = {(int(a), int(b)): int(r) for r, (a, b) in zip(rows_in, pairs[rows_in])}
    triplets = extract_triplets(pairs[rows_in])
    r10, r21, r20, rows = triplet_rotations(triplets, row_of, np.asarray(rotation, np.float64).reshape(-1, 9) if num_edges else np.zeros((0, 9)))
    err = cycle_errors(r10, r21, r20) if len(triplets) else np.zeros(0)
    # per-edge lists: entry (edge row, third node, error); within an edge the order of the third node
    third = np.stack([triplets[:, 2], triplets[:, 0], triplets[:, 1]], axis=1) if len(triplets) else np.zeros((0, 3), np.int64)
    flat_row, flat_third, flat_err = rows.reshape(-1), third.reshape(-1), np.repeat(err, 3)
    num = np.bincount(flat_row, minlength=num_edges).astype(np.int32) if num_edges else np.zeros(0, np.int32)
    agg = np.full(num_edges, np.nan)
    by_value = np.lexsort((flat_err, flat_row))  # NaN sorts last within an edge
    start = np.concatenate([[0], np.cumsum(num)])[:-1] if num_edges else np.zeros(0, np.int64)
    has = num > 0
    sorted_err = flat_err[by_value]
    if criterion == MEDIAN_EDGE_ERROR:
        lo, hi = start[has] + (num[has] - 1) // 2, start[has] + num[has] // 2
        agg[has] = (sorted_err[lo] + sorted_err[hi]) / 2
    elif criterion == MIN_EDGE_ERROR:
        agg[has] = sorted_err[start[has]]
    else:
        raise ValueError(f"criterion {criterion}")
    any_nan = np.bincount(flat_row, weights=np.isnan(flat_err), minlength=num_edges) > 0 if num_edges else np.zeros(0, bool)
    agg[any_nan] = np.nan
    with np.errstate(invalid="ignore"):
        keep = mask & (~has | (agg < error_threshold))
    in_node_order = flat_err[np.lexsort((flat_third, flat_row))]
    lists = {int(r): in_node_order[start[r]:start[r] + num[r]] for r in np.flatnonzero(has)}
    counts = np.zeros(8, np.int32)
    counts[:4] = [int(mask.sum()), int(keep.sum()), len(triplets), int(num.max()) if num_edges else 0]
    with np.errstate(invalid="ignore"):
        margin = np.where(has & ~any_nan, np.abs(agg - error_threshold), np.inf)
    return {"input": mask, "num_triplets": num, "aggregate_error": agg, "keep": keep.astype(np.uint8), "counts": counts, "triplets": triplets.astype(np.int32),
            "cycle_error": err, "lists": lists, "margin": margin}


def largest_component(pair_images: np.ndarray, enable: Optional[np.ndarray] = None, num_images: Optional[int] = None) -> Dict[str, np.ndarray]:
    """``node_mask`` [num_images], ``pair_keep`` [E] and ``counts`` [8] (nodes, edges, components with an edge), by networkx as
    ``gtsfm/utils/graph.py:24-47`` does it: edges added in row order, the first largest component."""
    import networkx as nx

    pairs = np.asarray(pair_images, np.int64).reshape(-1, 2)
    if num_images is None:
        num_images = int(pairs.max()) + 1 if len(pairs) else 0
    reason = check_enabled_edges(pairs, num_images, enable, ordered=False)
    if reason:
        raise ValueError(reason)
    on = np.ones(len(pairs), bool) if enable is None else np.asarray(enable).astype(bool)
    node_mask, counts = np.zeros(num_images, np.uint8), np.zeros(8, np.int32)
    if on.any():
        graph = nx.Graph()
        graph.add_edges_from([tuple(p) for p in pairs[on].tolist()])
        components = list(nx.connected_components(graph))
        node_mask[list(max(components, key=len))] = 1
        counts[2] = len(components)
    safe = np.where(on[:, None], pairs, 0)  # a disabled row may name anything
    pair_keep = (on & node_mask[safe[:, 0]].astype(bool) & node_mask[safe[:, 1]].astype(bool)).astype(np.uint8) if num_images else np.zeros(len(pairs), np.uint8)
    counts[0], counts[1] = int(node_mask.sum()), int(pair_keep.sum())
    return {"node_mask": node_mask, "pair_keep": pair_keep, "counts": counts}


# ---- the reference's functions, restated on its own types (dicts and lists of tuples) ----

def create_adjacency_list(edges: Sequence[Tuple[int, int]]) -> Dict[int, set]:
    adj: Dict[int, set] = {}
    for a, b in edges:
        adj.setdefault(a, set()).add(b)
        adj.setdefault(b, set()).add(a)
    return adj


def create_components(edges: Sequence[Tuple[int, int]]) -> List[set]:
    """The connected components (node sets) of an edge list, by networkx."""
    import networkx as nx

    graph = nx.Graph()
    graph.add_edges_from([tuple(p) for p in np.asarray(edges, np.int64).reshape(-1, 2).tolist()])
    return list(nx.connected_components(graph))


def normalised_edges(edges: Sequence[Tuple[int, int]]) -> np.ndarray:
    """The reference's set logic: (b, a) is the edge (a, b), and an edge listed twice is one edge."""
    arr = np.asarray([(min(a, b), max(a, b)) for a, b in edges], np.int64).reshape(-1, 2)
    return np.unique(arr, axis=0) if len(arr) else arr


def extract_cyclic_triplets_from_edges(edges: Sequence[Tuple[int, int]]) -> List[Tuple[int, int, int]]:
    return [tuple(t) for t in extract_triplets(normalised_edges(edges)).tolist()]


def get_nodes_in_largest_connected_component(edges: Sequence[Tuple[int, int]]) -> List[int]:
    if len(edges) == 0:
        return []
    pairs = np.asarray(edges, np.int64).reshape(-1, 2)
    return [int(v) for v in np.flatnonzero(largest_component(pairs)["node_mask"])]


def run_estimator(i2Ri1_dict: Dict[Tuple[int, int], np.ndarray], criterion: int = MEDIAN_EDGE_ERROR, error_threshold: float = 7.0) -> set:  # noqa: N803
    """``CycleConsistentRotationViewGraphEstimator.run`` on a dict of 3 x 3 arrays."""
    keys = list(i2Ri1_dict)
    if not keys:
        return set()
    pairs = np.asarray(keys, np.int64).reshape(-1, 2)
    rot = np.stack([np.asarray(i2Ri1_dict[k], np.float64).reshape(9) for k in keys])
    out = cycle_filter(pairs, rot, None, int(pairs.max()) + 1, criterion, error_threshold)
    return {keys[r] for r in np.flatnonzero(out["keep"])}
