"""Scenes for the view-graph tests (host build and GPU): pair graphs with seeded rotations, the smallest at which each mechanism of
gtsfm_amd/csrc/view_graph_kernels.hip can fail. Ground-truth wRi come from a seed; i2Ri1 = wRi2^T wRi1 times a perturbation of about 1
degree on inlier edges and of 20 to 90 degrees on about 10 % of the edges.

Every scene is checked HERE, on the restatement (tests/view_graph_reference.py), for both criteria and every threshold it is run with: no
aggregate lies within ``MARGIN_DEG`` of the threshold, so no edge is ever excluded from the equality of ``keep``; and a scene built with
``mixed=True`` has a kept edge, a dropped edge and an edge without a triplet (the graphs of a handful of edges cannot have all three)."""

import functools
from typing import Dict, List, Optional

import numpy as np

from tests import view_graph_reference as ref
from tests.conftest import REPO

MARGIN_DEG = 1e-6
PALACE = REPO / "tests" / "golden" / "view_graph_palace_edges.npz"
MP_SAMPLE = 48  # triplets per scene evaluated with 50 digits
SCENE_NAMES = ("empty", "one_edge", "triangle", "five_node", "k4", "k5", "k70", "hubs", "gaps", "disabled_nan", "palace")  # of all_scenes(), which is built on first use


def rotvec_to_matrix(v: np.ndarray) -> np.ndarray:
    """Rodrigues, [n, 3] -> [n, 3, 3]."""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    theta = np.linalg.norm(v, axis=1)
    k = v / np.where(theta > 0, theta, 1.0)[:, None]
    kx = np.zeros((len(v), 3, 3))
    kx[:, 0, 1], kx[:, 0, 2], kx[:, 1, 0], kx[:, 1, 2], kx[:, 2, 0], kx[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    s, c = np.sin(theta)[:, None, None], np.cos(theta)[:, None, None]
    return np.eye(3)[None] + s * kx + (1 - c) * np.matmul(kx, kx)


def seeded_rotations(pairs: np.ndarray, seed: int, outliers: float = 0.1) -> np.ndarray:
    """[E, 9] i2Ri1 for ``pairs`` [E, 2] (any ids)."""
    rng = np.random.default_rng(seed)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n = int(pairs.max()) + 1 if len(pairs) else 0
    w_r_i = rotvec_to_matrix(rng.normal(size=(n, 3)) * 1.2)
    axis = rng.normal(size=(len(pairs), 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    angle = np.deg2rad(np.abs(rng.normal(size=len(pairs))) * 1.0 + 0.05)
    bad = rng.random(len(pairs)) < outliers
    angle[bad] = np.deg2rad(rng.uniform(20.0, 90.0, size=int(bad.sum())))
    rel = np.matmul(w_r_i[pairs[:, 1]].transpose(0, 2, 1), w_r_i[pairs[:, 0]])
    return np.matmul(rel, rotvec_to_matrix(axis * angle[:, None])).reshape(-1, 9)


def scene(name: str, pairs, num_images: Optional[int] = None, seed: int = 0, rotation: Optional[np.ndarray] = None, enable: Optional[np.ndarray] = None,
          mixed: bool = False, thresholds=(7.0,), outliers: float = 0.1) -> Dict[str, object]:
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    rot = seeded_rotations(pairs, seed, outliers) if rotation is None else np.asarray(rotation, np.float64).reshape(-1, 9)
    n = (int(pairs.max()) + 1 if len(pairs) else 0) if num_images is None else num_images
    return {"name": name, "pair_images": pairs, "rotation": np.ascontiguousarray(rot), "enable": enable, "num_images": n, "mixed": mixed,
            "thresholds": tuple(thresholds)}


def complete(n: int) -> List:
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def window(n: int, w: int) -> List:
    return [(i, j) for i in range(n) for j in range(i + 1, min(n, i + w + 1))]


def hub_pairs(ring: int = 260, sizes=(63, 64, 65, 255, 256, 257)) -> List:
    """A ring; per size d a hub joined to ring nodes 0 .. d - 1 (a neighbour list of exactly d entries: the wave and workgroup boundaries of the
    list kernels), and a pair of hubs joined to each other and to ring nodes 0 .. d - 1 (an edge with exactly d triplets: the boundaries of
    the aggregate's lane loop, even and odd counts)."""
    edges = [(i, i + 1) for i in range(ring - 1)] + [(0, ring - 1)]
    node = ring
    for d in sizes:
        edges += [(k, node) for k in range(d)]
        node += 1
    for d in sizes:
        edges += [(k, node) for k in range(d)] + [(k, node + 1) for k in range(d)] + [(node, node + 1)]
        node += 2
    return edges


def five_node_reference_case() -> Dict[str, object]:
    """tests/view_graph_estimator/test_cycle_consistent_rotation_estimator.py of the reference: identities, (2, 4) off by 15 degrees about y."""
    pairs = [(0, 1), (1, 2), (0, 2), (2, 3), (3, 4), (2, 4)]
    rot = np.tile(np.eye(3).reshape(9), (6, 1))
    rot[5] = rotvec_to_matrix(np.array([[0.0, np.deg2rad(15.0), 0.0]])).reshape(9)
    return scene("five_node", pairs, rotation=rot)


def half_threshold(sc: Dict[str, object], criterion: int) -> float:
    """A threshold that cuts the scene's aggregates in half: the midpoint of the two middle distinct values."""
    agg = ref.cycle_filter(sc["pair_images"], sc["rotation"], sc["enable"], sc["num_images"], criterion, 7.0)["aggregate_error"]
    values = np.unique(agg[np.isfinite(agg)])
    return float((values[len(values) // 2 - 1] + values[len(values) // 2]) / 2)


@functools.lru_cache(maxsize=None)
def all_scenes() -> List[Dict[str, object]]:
    scenes = [
        scene("empty", np.zeros((0, 2), np.int32), num_images=3),
        scene("one_edge", [(0, 1)]),
        scene("triangle", complete(3), seed=1),
        five_node_reference_case(),
        scene("k4", complete(4), seed=2, outliers=0.3),
        scene("k5", complete(5), seed=3, outliers=0.3),
        scene("k70", complete(70), seed=4),
        scene("hubs", hub_pairs(), seed=5, mixed=True),
    ]
    # image ids with gaps, num_images larger than the largest id, rows shuffled
    rng = np.random.default_rng(6)
    ids = np.sort(rng.choice(500, size=40, replace=False))
    gaps = ids[np.asarray(window(40, 5) + [(0, 39)], np.int64)]
    gaps = np.concatenate([gaps[rng.permutation(len(gaps))], [[600, 640]]])
    scenes.append(scene("gaps", gaps, num_images=777, seed=6, mixed=True))
    # disabled rows (one of them a duplicate of an enabled row, one out of range, one reversed) and NaN rotations in the middle of the rows
    pairs = np.asarray(window(30, 6) + [(0, 29), (40, 41)], np.int32)
    pairs = pairs[np.random.default_rng(7).permutation(len(pairs))]
    rot = seeded_rotations(pairs, 7)
    enable = np.ones(len(pairs), np.uint8)
    enable[[5, 40, 77]] = 0
    pairs[40] = pairs[3]
    pairs[77] = (9, 2)
    pairs[5] = (1, 9999)
    rot[[20, 21, 90]] = np.nan
    rot[55, 4] = np.inf
    scenes.append(scene("disabled_nan", pairs, num_images=50, rotation=rot, enable=enable, mixed=True))
    z = np.load(PALACE)
    scenes.append(scene("palace", z["pair_images"], num_images=int(z["num_images"]), rotation=z["rotation"], mixed=True))
    assert tuple(sc["name"] for sc in scenes) == SCENE_NAMES
    for sc in scenes:
        if sc["name"] in ("k70", "hubs", "palace", "k5"):
            sc["thresholds"] = (7.0, half_threshold(sc, ref.MEDIAN_EDGE_ERROR))
    for sc in scenes:
        check_scene(sc)
    return scenes


def check_scene(sc: Dict[str, object]) -> None:
    """The assertions of this file's docstring, on the restatement."""
    for criterion in (ref.MIN_EDGE_ERROR, ref.MEDIAN_EDGE_ERROR):
        for thr in sc["thresholds"]:
            out = ref.cycle_filter(sc["pair_images"], sc["rotation"], sc["enable"], sc["num_images"], criterion, thr)
            assert out["margin"].size == 0 or out["margin"].min() > MARGIN_DEG, (sc["name"], criterion, thr, float(out["margin"].min()))
            if sc["mixed"]:
                inp = out["input"]
                assert (out["keep"][inp] == 1).any() and (out["keep"][inp] == 0).any() and (out["num_triplets"][inp] == 0).any(), (sc["name"], criterion, thr)


def expected(sc: Dict[str, object], criterion: int, threshold: float) -> Dict[str, object]:
    return _expected(sc["name"], criterion, float(threshold))


@functools.lru_cache(maxsize=None)
def _expected(name: str, criterion: int, threshold: float) -> Dict[str, object]:
    sc = {s["name"]: s for s in all_scenes()}[name]
    out = ref.cycle_filter(sc["pair_images"], sc["rotation"], sc["enable"], sc["num_images"], criterion, threshold)
    out["component"] = ref.largest_component(sc["pair_images"], out["keep"], sc["num_images"])
    return out


@functools.lru_cache(maxsize=None)
def measured_tolerance() -> Dict[str, float]:
    """The distance of the float64 restatement from the 50-digit evaluation of the same definition, on ``MP_SAMPLE`` seeded triplets of every
    scene, and the tolerance the device and the host build are held to: 8 x that distance (the project's rule for triangulation and two-view
    bundle adjustment). ``restatement`` is the largest distance over all scenes, in degrees."""
    worst, per_scene = 0.0, {}
    for sc in all_scenes():
        out = _expected(sc["name"], ref.MEDIAN_EDGE_ERROR, 7.0)
        trip = out["triplets"]
        if len(trip) == 0:
            continue
        pick = np.random.default_rng(11).choice(len(trip), size=min(MP_SAMPLE, len(trip)), replace=False)
        rows_in = np.flatnonzero(out["input"])
        row_of = {(int(a), int(b)): int(r) for r, (a, b) in zip(rows_in, sc["pair_images"][rows_in])}
        r10, r21, r20, _ = ref.triplet_rotations(trip[pick].astype(np.int64), row_of, sc["rotation"])
        exact = np.array([ref.cycle_error_mp(a, b, c) for a, b, c in zip(r10, r21, r20)])
        per_scene[sc["name"]] = float(np.abs(out["cycle_error"][pick] - exact).max())
        worst = max(worst, per_scene[sc["name"]])
    return {"restatement": worst, "tolerance": 8 * worst, **{f"scene:{k}": v for k, v in per_scene.items()}}


def check_outputs(name: str, got: Dict[str, np.ndarray], exp: Dict[str, object], tolerance: float) -> Dict[str, float]:
    """The rule the device and the host build are held to: the discrete outputs (``num_triplets``, ``keep``, the triplet list, ``counts``, and
    with ``node_mask`` / ``pair_keep`` / ``component_counts`` the component of the kept edges) equal the restatement's; the aggregates and
    cycle errors lie within ``tolerance`` degrees of it, NaN where it has NaN. Returns the largest distances."""
    np.testing.assert_array_equal(got["num_triplets"], exp["num_triplets"], err_msg=f"{name}: num_triplets")
    np.testing.assert_array_equal(got["keep"], exp["keep"], err_msg=f"{name}: keep")
    np.testing.assert_array_equal(np.asarray(got["counts"])[:8], exp["counts"], err_msg=f"{name}: counts")
    np.testing.assert_array_equal(np.asarray(got["triplets"]).reshape(-1, 3), exp["triplets"], err_msg=f"{name}: triplets")
    if "node_mask" in got:
        comp = exp["component"]
        np.testing.assert_array_equal(got["node_mask"], comp["node_mask"], err_msg=f"{name}: node_mask")
        np.testing.assert_array_equal(got["pair_keep"], comp["pair_keep"], err_msg=f"{name}: pair_keep")
        np.testing.assert_array_equal(np.asarray(got["component_counts"])[:8], comp["counts"], err_msg=f"{name}: component counts")
    dist = {}
    for key in ("aggregate_error", "cycle_error"):
        a, b = np.asarray(got[key], np.float64), np.asarray(exp[key], np.float64)
        assert a.shape == b.shape, f"{name}: {key} shape {a.shape} vs {b.shape}"
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=f"{name}: {key} NaN pattern")
        ok = ~np.isnan(b)
        dist[key] = float(np.abs(a[ok] - b[ok]).max()) if ok.any() else 0.0
        assert dist[key] <= tolerance, f"{name}: {key} off by {dist[key]:.3e} degrees, tolerance {tolerance:.3e}"
    return dist
