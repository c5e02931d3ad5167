"""Scenes for the view-graph tests (host build and GPU): pair graphs with seeded rotations, the smallest at which each mechanism of
gtsfm_amd/csrc/view_graph_kernels.hip can fail. Ground-truth wRi come from a seed; i2Ri1 = wRi2^T wRi1 times a perturbation of about 1
degree on inlier edges and of 20 to 90 degrees on about 10 % of the edges.

Every scene is checked HERE, on the restatement (tests/view_graph_reference.py), for both criteria and every threshold it is run with: no
aggregate lies within ``MARGIN_DEG`` of the threshold, so no edge is ever excluded from the equality of ``keep``; and a scene built with
``mixed=True`` has a kept edge, a dropped edge and an edge without a triplet (the graphs of a handful of edges cannot have all three). The
one exception to the margin is stated with check_scene. The scenes of ``HARD_SCENES`` (ties, cycles of exactly 0 and 180 degrees, every branch
of the quaternion step, rotations that are not orthonormal) assert what they are named for in check_hard_scene."""

import functools
from typing import Dict, List, Optional

import numpy as np

from tests import view_graph_reference as ref
from tests.conftest import REPO

MARGIN_DEG = 1e-6
PALACE = REPO / "tests" / "golden" / "view_graph_palace_edges.npz"
MP_SAMPLE = 48  # triplets per scene evaluated with 50 digits
FIRST_SCENES = ("empty", "one_edge", "triangle", "five_node", "k4", "k5", "k70", "hubs", "gaps", "disabled_nan", "palace")
FIRST_SCENES_RESTATEMENT = "1.421e-14"  # measured_tolerance()["restatement"] of FIRST_SCENES as printed in profiles/view_graph_gpu_tests.txt: it must not move
# Scenes built to be hard: each is held to 8 x ITS OWN distance from the 50-digit evaluation (every triplet, not a sample) and stays out of
# the maximum over FIRST_SCENES, which it would loosen for everything. A restatement value of exactly 0.0 that the 50-digit evaluation
# confirms is held byte-wise.
HARD_CYCLES_TAIL = 5
TIED_HUBS_TIED_LISTS = 2257  # of 3142 per-edge lists of tied_hubs hold two equal values
HARD_SCENES = ("tied_hubs", "hard_cycles", "hard_cycles_tiny", "hard_cycles_skewed")
SCENE_NAMES = FIRST_SCENES + HARD_SCENES  # of all_scenes(), which is built on first use


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


def tied_hubs() -> Dict[str, object]:
    """The hubs graph (per-edge lists of exactly 63, 64, 65, 255, 256 and 257 entries) with identity rotations, but a fixed 10 degrees about z on
    the hub edges of ring nodes a with a % 5 == 0 and a fixed 3 degrees about x on those with a % 7 == 3: the cycle errors take a handful of
    values, two of them apart in the last bit only (the 3 degrees of every second such node are the product of 0.5 and 2.5 degrees), so most lists hold equal values and the (value, index) rank and the successor search of the
    aggregate work on ties. check_scene asserts the counts."""
    pairs = np.asarray(hub_pairs(), np.int32)
    ring = 260
    rot = np.tile(np.eye(3).reshape(9), (len(pairs), 1))
    a, hub_edge = pairs[:, 0], (pairs[:, 0] < ring) & (pairs[:, 1] >= ring)
    about_x = lambda deg: rotvec_to_matrix(np.array([[np.deg2rad(deg), 0.0, 0.0]]))[0]  # noqa: E731
    rot[hub_edge & (a % 7 == 3)] = about_x(3.0).reshape(9)  # reads as 3.0000000000000004 degrees
    rot[hub_edge & (a % 14 == 10)] = (about_x(0.5) @ about_x(2.5)).reshape(9)  # the same rotation one bit away in two entries: reads as 3.0
    rot[hub_edge & (a % 5 == 0)] = rotvec_to_matrix(np.array([[0.0, 0.0, np.deg2rad(10.0)]])).reshape(9)
    return scene("tied_hubs", pairs, rotation=rot, mixed=True)


def axis_angle(axis, degrees: Optional[float] = None, radians: Optional[float] = None) -> np.ndarray:
    """Rodrigues with 50 digits, rounded to float64 once per entry: the nearest matrix to the stated rotation."""
    import mpmath as mp

    with mp.workdps(50):
        k = mp.matrix([mp.mpf(float(x)) for x in axis])
        k = k / mp.sqrt(sum(x * x for x in k))
        theta = mp.mpf(degrees) * mp.pi / 180 if radians is None else mp.mpf(radians)
        kx = mp.matrix([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        m = mp.eye(3) + mp.sin(theta) * kx + (1 - mp.cos(theta)) * (kx * kx)
        return np.array([[float(m[r, c]) for c in range(3)] for r in range(3)])


@functools.lru_cache(maxsize=None)
def hard_cycle_rotations() -> List:
    """(label, C, the stated angle in degrees) of the cycle rotations the hard_cycles scenes are built from."""
    diag, ones, generic = np.eye(3), (1.0, 1.0, 1.0), (0.36, 0.48, 0.8)
    out = [("identity", np.eye(3), 0.0)]
    out += [(f"{r:g} rad", axis_angle(generic, radians=r), float(np.rad2deg(r))) for r in (1e-12, 1e-9, 1e-6)]
    out += [("30", axis_angle(generic, 30.0), 30.0), ("60", axis_angle(generic, 60.0), 60.0)]  # the trace branch, with 1e-6 rad and 119.9
    out += [("90 about z", np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), 90.0)]  # m22 = trace = 1: the diagonal comes first
    out += [("119.9 about 111", axis_angle(ones, 119.9), 119.9), ("120 about 111", np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), 120.0),
            ("120.1 about 111", axis_angle(ones, 120.1), 120.1), ("150", axis_angle(generic, 150.0), 150.0), ("179", axis_angle(generic, 179.0), 179.0),
            ("180 - 1e-6", axis_angle(generic, 180.0 - 1e-6), 180.0 - 1e-6), ("180 - 1e-10", axis_angle(generic, 180.0 - 1e-10), 180.0 - 1e-10)]
    out += [(f"180 about {'xyz'[i]}", np.diag(np.where(np.arange(3) == i, 1.0, -1.0)), 180.0) for i in range(3)]  # q_w = 0 exactly
    out += [("180 about 111", axis_angle(ones, 180.0), 180.0)]
    for i in range(3):  # m_ii the strict largest of the diagonal and above the trace
        axis = np.where(np.arange(3) == i, 0.9, 0.3) * np.array([1.0, -1.0, 1.0])
        out += [(f"{deg:g} about mostly {'xyz'[i]}", axis_angle(axis, deg), deg) for deg in (135.0, 160.0, 175.0)]
    for _, c, _ in out:
        assert np.abs(c @ c.T - diag).max() < 4e-16
    return out


def hard_cycles(name: str) -> Dict[str, object]:
    """Disjoint triangles (3 k, 3 k + 1, 3 k + 2) whose cycle rotation is a chosen C_k. The ``exact`` group has identities on (i0, i1) and (i1, i2)
    and C_k itself on (i0, i2), so the cycle is C_k^T to the bit; the ``composed`` group has seeded rotations on the first two edges and
    i2Ri1 . i1Ri0 . C_k on the third, so it is C_k^T up to rounding. Each triangle is joined to the next by one edge that closes no triangle (the
    spine), so the edges the filter drops cut the spine and the largest-component step has something to decide; a tail of five edges behind the last
triangle keeps the largest component unique at every threshold (check_hard_scene asserts it), so it does not depend on the order of the rows.

    hard_cycles runs with the thresholds 7.0 and 0.0. keep = aggregate < 0.0 is false for the exact identity, whose aggregate IS 0.0 (strict
    comparison); every other aggregate of the scene lies more than MARGIN_DEG from both thresholds. The cycles that lie within MARGIN_DEG of 0.0
    without being exactly 0.0 -- 1e-12 and 1e-9 rad, and the composed identity -- are the scene hard_cycles_tiny, which runs with 7.0 only, so
    the margin rule holds everywhere. hard_cycles_skewed is hard_cycles with every row multiplied element-wise by 1 + N(0, 1e-6): rotations that
    are not orthonormal, held to the stated definition and not to scipy, which re-orthogonalises."""
    cases = hard_cycle_rotations()
    tiny = {"1e-12 rad", "1e-09 rad"}
    if name == "hard_cycles_tiny":
        group = [(c, "exact") for c in cases if c[0] in tiny | {"identity"}] + [(c, "composed") for c in cases if c[0] in tiny | {"identity", "1e-06 rad"}]
    else:
        group = [(c, "exact") for c in cases if c[0] not in tiny] + [(c, "composed") for c in cases if c[0] not in tiny | {"identity"}]
    rng = np.random.default_rng(8)
    pairs, rot, labels = [], [], []
    for k, ((label, c, angle), kind) in enumerate(group):
        r10, r21 = (np.eye(3), np.eye(3)) if kind == "exact" else rotvec_to_matrix(rng.normal(size=(2, 3)) * 1.2)
        pairs += [(3 * k, 3 * k + 1), (3 * k + 1, 3 * k + 2), (3 * k, 3 * k + 2)]
        rot += [r10, r21, r21 @ r10 @ c]
        labels.append((label, kind, angle))
        if k + 1 < len(group):
            pairs.append((3 * k + 2, 3 * k + 3))
            rot.append(rotvec_to_matrix(rng.normal(size=(1, 3)))[0])
    last = 3 * len(group) - 1
    pairs += [(last + k, last + k + 1) for k in range(HARD_CYCLES_TAIL)]  # a tail: the largest component is unique even when only the spine is kept
    rot += list(rotvec_to_matrix(rng.normal(size=(HARD_CYCLES_TAIL, 3))))
    rot = np.asarray(rot).reshape(-1, 9)
    if name == "hard_cycles_skewed":
        rot = rot * (1.0 + np.random.default_rng(9).normal(scale=1e-6, size=rot.shape))
    sc = scene(name, pairs, rotation=rot, mixed=name != "hard_cycles_tiny", thresholds=(7.0, 0.0) if name == "hard_cycles" else (7.0,))
    sc["labels"] = labels  # triplet k is triangle k
    return sc


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
    scenes += [tied_hubs(), hard_cycles("hard_cycles"), hard_cycles("hard_cycles_tiny"), hard_cycles("hard_cycles_skewed")]
    assert tuple(sc["name"] for sc in scenes) == SCENE_NAMES
    for sc in scenes:
        if sc["name"] in ("k70", "hubs", "palace", "k5"):
            sc["thresholds"] = (7.0, half_threshold(sc, ref.MEDIAN_EDGE_ERROR))
    for sc in scenes:
        check_scene(sc)
    return scenes


def triplet_inputs(sc: Dict[str, object], out: Dict[str, object]):
    """(i1Ri0, i2Ri1, i2Ri0, edge rows [T, 3]) of the triplets of a restatement output."""
    rows_in = np.flatnonzero(out["input"])
    row_of = {(int(a), int(b)): int(r) for r, (a, b) in zip(rows_in, sc["pair_images"][rows_in])}
    return ref.triplet_rotations(out["triplets"].astype(np.int64), row_of, sc["rotation"])


@functools.lru_cache(maxsize=None)
def exact_errors(name: str):
    """(50-digit cycle error, its first-largest choice) of EVERY triplet of a scene of all_scenes(); equal rotation triples are evaluated once."""
    sc = {s["name"]: s for s in all_scenes()}[name]
    out = ref.cycle_filter(sc["pair_images"], sc["rotation"], sc["enable"], sc["num_images"], ref.MEDIAN_EDGE_ERROR, 7.0)
    r10, r21, r20, _ = triplet_inputs(sc, out)
    done: Dict[bytes, tuple] = {}
    for a, b, c in zip(r10, r21, r20):
        key = a.tobytes() + b.tobytes() + c.tobytes()
        if key not in done:
            done[key] = ref.cycle_error_mp(a, b, c, return_choice=True)
    both = [done[a.tobytes() + b.tobytes() + c.tobytes()] for a, b, c in zip(r10, r21, r20)]
    return np.array([e for e, _ in both]), np.array([c for _, c in both], np.int64)


def check_scene(sc: Dict[str, object]) -> None:
    """The assertions of this file's docstring, on the restatement. An aggregate may lie within MARGIN_DEG of a threshold in one case only: it
    EQUALS the threshold, both are exactly representable, and the restatement's value is exact -- the aggregate is an entry of its edge's list and
    the 50-digit evaluation of every such entry gives the same float64 (the exact identity cycle against the threshold 0.0). Then the device owes
    the same bytes and the strict comparison drops the edge. Otherwise the margin rule stays."""
    for criterion in (ref.MIN_EDGE_ERROR, ref.MEDIAN_EDGE_ERROR):
        for thr in sc["thresholds"]:
            out = ref.cycle_filter(sc["pair_images"], sc["rotation"], sc["enable"], sc["num_images"], criterion, thr)
            close = np.flatnonzero(out["margin"] <= MARGIN_DEG)
            if len(close):
                assert sc["name"] in HARD_SCENES, (sc["name"], criterion, thr, float(out["margin"].min()))
                r10, r21, r20, rows = triplet_inputs(sc, out)
                for row in close.tolist():
                    agg = out["aggregate_error"][row]
                    deciding = np.flatnonzero((rows == row).any(axis=1) & (out["cycle_error"] == agg))
                    assert agg == thr and out["keep"][row] == 0 and len(deciding), (sc["name"], criterion, thr, row, float(agg))
                    assert all(ref.cycle_error_mp(r10[t], r21[t], r20[t]) == agg for t in deciding.tolist()), (sc["name"], criterion, thr, row, float(agg))
            if sc["mixed"]:
                inp = out["input"]
                assert (out["keep"][inp] == 1).any() and (out["keep"][inp] == 0).any() and (out["num_triplets"][inp] == 0).any(), (sc["name"], criterion, thr)


def check_hard_scene(sc: Dict[str, object]) -> Dict[str, object]:
    """What the hard scenes are named for, asserted on the restatement; returns the figures ``-s`` prints. Called by measured_tolerance(name)."""
    name = sc["name"]
    out = _expected(name, ref.MEDIAN_EDGE_ERROR, 7.0)
    exact, exact_choice = exact_errors(name)
    distance = float(np.abs(out["cycle_error"] - exact).max())
    figures: Dict[str, object] = {"restatement": distance}
    if name == "tied_hubs":
        lists = out["lists"]
        tied = {row for row, v in lists.items() if len(np.unique(v)) < len(v)}
        middle_tie = {row for row, v in lists.items() if len(v) % 2 == 0 and np.sort(v)[len(v) // 2 - 1] == np.sort(v)[len(v) // 2]}
        values = np.unique(out["cycle_error"])
        figures.update(lists=len(lists), tied_lists=len(tied), distinct_errors=len(values), kept={c: int(_expected(name, c, 7.0)["counts"][1]) for c in (0, 1)})
        assert len(out["triplets"]) == 3822 and len(lists) == 3142 and len(tied) == TIED_HUBS_TIED_LISTS and len(values) == 5, figures
        assert {len(lists[row]) for row in tied} >= {63, 64, 65, 255, 256, 257} and {len(lists[row]) for row in middle_tie} >= {64, 256}
        assert (np.diff(values) < 1e-15).any() and values[0] == 0.0  # two values apart in the last bit, not rounded away; identity cycles give 0.0
        assert figures["kept"][0] > figures["kept"][1] and np.abs(out["aggregate_error"][out["num_triplets"] > 0] - 7.0).min() > 0.25
    else:
        r10, r21, r20, _ = triplet_inputs(sc, out)
        _, choice = ref.cycle_errors(r10, r21, r20, return_choice=True)
        labels = sc["labels"]
        for criterion in (ref.MIN_EDGE_ERROR, ref.MEDIAN_EDGE_ERROR):
            for thr in sc["thresholds"]:
                kept = sc["pair_images"][_expected(name, criterion, thr)["keep"] == 1]
                sizes = sorted(len(c) for c in ref.create_components(kept))
                assert len(sizes) == 1 or sizes[-1] > sizes[-2], (name, criterion, thr, sizes[-3:])
        assert out["triplets"].tolist() == [[3 * k, 3 * k + 1, 3 * k + 2] for k in range(len(labels))]
        figures["choices"] = np.bincount(choice, minlength=4).tolist()
        if name != "hard_cycles_tiny":
            assert min(figures["choices"]) >= 8, figures
        if name != "hard_cycles_skewed":
            for k, (label, kind, angle) in enumerate(labels):
                err = out["cycle_error"][k]
                if kind == "exact":
                    assert (err == 0.0 and exact[k] == 0.0) if label == "identity" else abs(err - angle) <= distance, (label, float(err), angle, distance)
                    assert choice[k] == exact_choice[k], (label, int(choice[k]), int(exact_choice[k]))  # exact entries: no rounding decides the branch
                if kind == "exact" and label == "120 about 111":  # the diagonal and the trace are all 0: the first wins, and the arbiter agrees
                    assert choice[k] == exact_choice[k] == 0
                if kind == "exact" and label == "90 about z":  # m22 == trace == 1: the diagonal comes before the trace
                    assert choice[k] == exact_choice[k] == 2
        if name == "hard_cycles":
            zero = _expected(name, ref.MEDIAN_EDGE_ERROR, 0.0)
            at = zero["aggregate_error"] == 0.0
            assert at.sum() == 3 and not zero["keep"][at].any() and zero["counts"][1] == (zero["num_triplets"][zero["input"]] == 0).sum()
            assert out["cycle_error"].max() == 180.0 and (out["cycle_error"] == 180.0).sum() >= 3 and np.sort(out["cycle_error"])[1] < 1e-4
        if name == "hard_cycles_tiny":
            assert (out["cycle_error"] < MARGIN_DEG).sum() >= 5 and out["cycle_error"].max() < 1e-4 and (out["cycle_error"] > 0).sum() >= 5
        if name == "hard_cycles_skewed":
            from scipy.spatial.transform import Rotation

            m = np.matmul(np.matmul(r20.transpose(0, 2, 1), r21), r10)
            figures["scipy"] = float(np.abs(np.rad2deg(Rotation.from_matrix(m).magnitude()) - out["cycle_error"]).max())
            figures["orthonormality"] = float(np.abs(np.matmul(m, m.transpose(0, 2, 1)) - np.eye(3)).max())
            assert 1e-7 < figures["orthonormality"] < 1e-4
    return figures


def expected(sc: Dict[str, object], criterion: int, threshold: float) -> Dict[str, object]:
    return _expected(sc["name"], criterion, float(threshold))


@functools.lru_cache(maxsize=None)
def _expected(name: str, criterion: int, threshold: float) -> Dict[str, object]:
    sc = {s["name"]: s for s in all_scenes()}[name]
    out = ref.cycle_filter(sc["pair_images"], sc["rotation"], sc["enable"], sc["num_images"], criterion, threshold)
    out["component"] = ref.largest_component(sc["pair_images"], out["keep"], sc["num_images"])
    return out


@functools.lru_cache(maxsize=None)
def measured_tolerance(name: Optional[str] = None) -> Dict[str, object]:
    """For a scene of HARD_SCENES: the distance of the restatement from the 50-digit evaluation on every triplet of THAT scene, 8 x it as its
    tolerance (0 where the distance is 0: bytes), the scene's own assertions and figures. For every other scene and without a name: the distance of the float64 restatement from the 50-digit evaluation of the same definition, on ``MP_SAMPLE`` seeded triplets of every
    scene, and the tolerance the device and the host build are held to: 8 x that distance (the project's rule for triangulation and two-view
    bundle adjustment). ``restatement`` is the largest distance over all scenes, in degrees."""
    if name is not None and name in HARD_SCENES:
        figures = check_hard_scene({s["name"]: s for s in all_scenes()}[name])
        return {**figures, "tolerance": 8 * figures["restatement"], "exact_zero": True}
    worst, per_scene = 0.0, {}
    for sc in all_scenes():
        if sc["name"] in HARD_SCENES:
            continue
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
    assert f"{worst:.3e}" == FIRST_SCENES_RESTATEMENT, f"the measured distance of the first scenes moved: {worst:.3e}, recorded {FIRST_SCENES_RESTATEMENT}"
    return {"restatement": worst, "tolerance": 8 * worst, "exact_zero": False, **{f"scene:{k}": v for k, v in per_scene.items()}}


def check_outputs(name: str, got: Dict[str, np.ndarray], exp: Dict[str, object], tolerance: float, exact_zero: bool = False) -> Dict[str, float]:
    """The rule the device and the host build are held to: the discrete outputs (``num_triplets``, ``keep``, the triplet list, ``counts``, and
    with ``node_mask`` / ``pair_keep`` / ``component_counts`` the component of the kept edges) equal the restatement's; the aggregates and
    cycle errors lie within ``tolerance`` degrees of it, NaN where it has NaN; with ``exact_zero`` a restatement value of exactly 0.0 is owed
    byte-wise (the hard scenes assert that the 50-digit evaluation gives 0 there). Returns the largest distances."""
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
        if exact_zero:
            zero = b == 0.0
            assert a[zero].tobytes() == b[zero].tobytes(), f"{name}: {key} is not 0.0 at {int((a[zero] != 0).sum())} of {int(zero.sum())} entries that are exactly 0"
    return dist
