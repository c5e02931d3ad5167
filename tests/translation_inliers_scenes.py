"""The scenes the 1DSfM kernels (gtsfm_amd/csrc/translation_kernels.hip) are tested on, at the smallest shapes that reach each code path.
Every scene is checked HERE, on the restatement (tests/translation_inliers_reference.py), for what it is named for, and no scene may have a
mean weight within 1e-9 of its threshold. ``expected(scene)`` caches the restatement's outputs: they are computed once and never changed."""

from functools import lru_cache
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import translation_inliers_reference as ref
from tests.conftest import REPO

GOLDEN = REPO / "tests" / "golden" / "translation_inliers_five_cameras.npz"
THRESHOLD_MARGIN = 1e-9


def random_rotations(rng, n: int) -> np.ndarray:
    q = rng.normal(size=(n, 4))
    q /= np.sqrt((q * q).sum(1))[:, None]
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)


def random_units(rng, n: int) -> np.ndarray:
    return ref.unit(rng.normal(size=(n, 3)))


def scene(name: str, pairs: Sequence[Tuple[int, int]], pair_direction, num_images: int, directions, *, rotation=None, rotation_valid=None, pair_enable=None,
          tracks: Sequence[Sequence[int]] = (), uv=None, track_enable=None, meas_enable=None, intrinsics=None, world=None, threshold: float = ref.OUTLIER_WEIGHT_THRESHOLD,
          lds_node_limit: int = -1) -> Dict[str, object]:
    e = len(pairs)
    track_off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    image = np.asarray([c for t in tracks for c in t], np.int32)
    return {"name": name, "num_images": num_images, "pair_images": np.asarray(pairs, np.int32).reshape(-1, 2), "pair_direction": np.asarray(pair_direction, np.float64).reshape(e, 3),
            "pair_enable": None if pair_enable is None else np.asarray(pair_enable, np.uint8),
            "rotation": np.tile(np.eye(3).reshape(9), (num_images, 1)) if rotation is None else np.asarray(rotation, np.float64).reshape(num_images, 9),
            "rotation_valid": np.ones(num_images, np.uint8) if rotation_valid is None else np.asarray(rotation_valid, np.uint8),
            "intrinsics": np.tile([100.0, 100.0, 50.0, 40.0], (num_images, 1)) if intrinsics is None else np.asarray(intrinsics, np.float64).reshape(num_images, 4),
            "track_off": track_off, "image": image, "uv": np.zeros((len(image), 2), np.float32) if uv is None else np.asarray(uv, np.float32).reshape(len(image), 2),
            "track_enable": np.ones(len(tracks), np.uint8) if track_enable is None else np.asarray(track_enable, np.uint8),
            "meas_enable": None if meas_enable is None else np.asarray(meas_enable, np.uint8), "directions": np.asarray(directions, np.float64).reshape(-1, 3),
            "world": world, "threshold": threshold, "lds_node_limit": lds_node_limit}


def restate(sc, **kw) -> Dict[str, np.ndarray]:
    return ref.translation_inliers(sc["pair_images"], sc["pair_direction"], sc["pair_enable"], sc["rotation"], sc["rotation_valid"], sc["intrinsics"], sc["track_off"],
                                   sc["image"], sc["uv"], sc["track_enable"], sc["meas_enable"], sc["directions"], sc["threshold"], world=sc["world"], **kw)


# ---- geometry ----

def true_geometry(rng, n: int, landmarks: int, per_landmark: int = 3):
    """Camera centres and rotations, landmarks in front of their cameras, intrinsics; each landmark seen by ``per_landmark`` cameras."""
    centre = rng.uniform(-5, 5, size=(n, 3))
    rot = random_rotations(rng, n)
    point = rng.uniform(-5, 5, size=(landmarks, 3))
    tracks = [sorted(rng.choice(n, per_landmark, replace=False).tolist()) for _ in range(landmarks)]
    return centre, rot, point, tracks


def pair_directions(centre, rot, pairs) -> np.ndarray:
    """i2Ui1 in the frame of i2: wRi2^T (c1 - c2), normalised."""
    out = []
    for i1, i2 in pairs:
        r = rot[i2].reshape(3, 3)
        v = r.T @ (centre[i1] - centre[i2])
        out.append(v / np.linalg.norm(v))
    return np.asarray(out).reshape(-1, 3)


def window(n: int, w: int) -> List[Tuple[int, int]]:
    return [(i, j) for i in range(n) for j in range(i + 1, min(n, i + w + 1))]


def five_cameras() -> Dict[str, object]:
    """The reference's Test1dsfmAllOutliers (tests/averaging/translation/test_averaging_1dsfm.py:239-303): inputs copied as numbers in
    tests/golden/translation_inliers_five_cameras.npz; np.random.seed(0) and 2000 np.random.normal directions."""
    z = np.load(GOLDEN)
    np.random.seed(0)
    directions = ref.sample_uniform_directions(ref.MAX_PROJECTION_DIRECTIONS)
    return scene("five_cameras", [tuple(p) for p in z["pair_images"].tolist()], z["i2Ui1"], 5, directions, rotation=z["wRi"])


def chain_or_ring(n: int, ring: bool, seed: int) -> Dict[str, object]:
    rng = np.random.default_rng(seed)
    pairs = [(i, i + 1) for i in range(n - 1)] + ([(0, n - 1)] if ring else [])
    return scene(f"{'ring' if ring else 'chain'}_{n}", pairs, random_units(rng, len(pairs)), n, random_units(rng, 2), rotation=random_rotations(rng, n))


def hub(degree: int = 300) -> Dict[str, object]:
    rng = np.random.default_rng(5)
    n = degree + 1
    pairs = [(0, j) for j in range(1, n)] + [(j, j + 1) for j in range(1, n - 1, 7)]
    return scene("hub_300", pairs, random_units(rng, len(pairs)), n, random_units(rng, 2), rotation=random_rotations(rng, n))


def lost_camera() -> Dict[str, object]:
    """Eight cameras in true geometry; every pair direction of camera 7 is reversed, its landmarks' directions are true: all its pair edges
    are rejected, so its measurements are dropped by the camera rule although their own edges are inliers."""
    rng = np.random.default_rng(17)
    n = 8
    centre, rot, _, _ = true_geometry(rng, n, 0)
    pairs = window(n, n)
    t = pair_directions(centre, rot, pairs)
    for k, (_, i2) in enumerate(pairs):
        if i2 == n - 1:
            t[k] = -t[k]
    tracks = [[0, 2, 7], [1, 3, 7], [2, 4, 7], [0, 1, 7], [0, 3, 4], [1, 2, 4], [3, 4, 7], [0, 4, 7]]
    k = np.tile([100.0, 100.0, 50.0, 40.0], (n, 1))
    uv = []
    for cams in tracks:
        point = rng.uniform(-3, 3, size=3)
        for c in cams:
            ray = rot[c].reshape(3, 3).T @ (point - centre[c])
            uv.append((k[c, 0] * ray[0] / ray[2] + k[c, 2], k[c, 1] * ray[1] / ray[2] + k[c, 3]))
    return scene("lost_camera", pairs, t, n, random_units(rng, 65), rotation=rot, tracks=tracks, uv=uv, intrinsics=k)


def axis_aligned() -> Dict[str, object]:
    """World directions given: +-e_x, +-e_y, e_z on 12 cameras and 3 landmarks, projected on e_x and e_y: weights in {0, +-1}, zero-weight
    edges, directed triangles of weight 1 (tied scores) and many tied roots."""
    ex, ey, ez = np.eye(3)
    pairs, m = [], []
    for a in (0, 3, 6):  # a -> a+1 -> a+2 -> a on e_x: (i1, i2) runs i2 -> i1 for w >= 0
        pairs += [(a, a + 1), (a + 1, a + 2), (a, a + 2)]
        m += [-ex, -ex, ex]
    pairs += [(9, 10), (10, 11), (9, 11), (2, 3), (5, 6), (8, 9), (0, 11)]
    m += [-ey, -ey, ey, ez, ez, -ez, ez]
    tracks = [[0, 4, 8], [1, 5, 9], [2, 6, 10, 11]]
    wm = [ex, -ex, ey, ez, -ey, ex, ey, ey, -ex, ez]
    return scene("axis_aligned", pairs, np.zeros((len(pairs), 3)), 12, [ex, ey], tracks=tracks, world=(np.asarray(m), np.asarray(wm)))


def cyclic_conflicts() -> Dict[str, object]:
    """Ten disjoint directed triangles with random weights near e_x, projected on e_x first: every triangle costs one score step."""
    rng = np.random.default_rng(17)
    pairs, m = [], []
    for a in range(0, 30, 3):
        pairs += [(a, a + 1), (a + 1, a + 2), (a, a + 2)]
        m += [-1.0, -1.0, 1.0]
    t = ref.unit(np.asarray(m)[:, None] * np.array([1.0, 0.0, 0.0]) + rng.normal(scale=0.2, size=(len(pairs), 3)))
    return scene("cyclic_conflicts", pairs, t, 30, np.concatenate([[[1.0, 0.0, 0.0]], random_units(rng, 6)]))


def gaps_and_invalid() -> Dict[str, object]:
    """Node ids with gaps (images 3, 7, 8 and track 1 have no edge), a disabled row, a NaN row, an invalid wRi[i2] (row dropped) and an
    invalid wRi[i1] (row kept: the reference's quirk), a disabled track and a disabled measurement."""
    rng = np.random.default_rng(23)
    n = 12
    pairs = [(0, 1), (0, 2), (1, 2), (2, 4), (4, 5), (5, 6), (4, 6), (6, 9), (9, 10), (10, 11), (9, 11), (1, 5), (0, 6)]
    t = random_units(rng, len(pairs))
    enable = np.ones(len(pairs), np.uint8)
    enable[3] = 0
    t[5] = np.nan
    valid = np.ones(n, np.uint8)
    valid[[10, 0, 3]] = 0  # (9, 10) is dropped; (0, 1), (0, 2), (0, 6) stay
    tracks = [[1, 2, 4], [5, 6, 9], [4, 6, 11], [1, 9, 11]]
    uv = rng.uniform(0, 100, size=(12, 2))
    meas_enable = np.ones(12, np.uint8)
    meas_enable[7] = 0
    return scene("gaps_and_invalid", pairs, t, n, random_units(rng, 7), rotation=random_rotations(rng, n), rotation_valid=valid, pair_enable=enable, tracks=tracks, uv=uv,
                 track_enable=[1, 0, 1, 1], meas_enable=meas_enable)


def tiers(limit: int) -> Dict[str, object]:
    rng = np.random.default_rng(29)
    n = 300
    pairs = window(n, 2) + [(0, n - 1)]
    sc = scene(f"tier_{'lds' if limit else 'workspace'}", pairs, random_units(rng, len(pairs)), n, random_units(rng, 3), rotation=random_rotations(rng, n),
               lds_node_limit=limit)
    return sc


def direction_counts(d: int) -> Dict[str, object]:
    rng = np.random.default_rng(31)
    n = 9
    centre, rot, point, tracks = true_geometry(rng, n, 4)
    pairs = window(n, 3)
    t = ref.unit(pair_directions(centre, rot, pairs) + rng.normal(scale=0.3, size=(len(pairs), 3)))
    return scene(f"directions_{d}", pairs, t, n, random_units(rng, d), rotation=rot, tracks=tracks, uv=rng.uniform(0, 100, size=(12, 2)))


def triangles_400(tied: bool) -> Dict[str, object]:
    """World directions given: 400 disjoint directed triangles a -> a + 1 -> a + 2 -> a on e_x (nodes 0 .. 1199: a lane of the MFAS kernel owns up
    to five), projected on e_x and e_y. Every triangle costs one score step on e_x and none on e_y (all weights 0: every node is a root).
    ``tied``: all weights exactly 1, so every score step is a tie among all nodes of the unbroken triangles and the smallest id must win across
    the four waves and the nodes of a lane. Otherwise the weights are U(0.2, 1): the scores are distinct and the winner is anywhere in the id range."""
    rng = np.random.default_rng(41)
    ex, ey, _ = np.eye(3)
    pairs, m = [], []
    for a in range(0, 1200, 3):  # (i1, i2) runs i2 -> i1 for w >= 0
        pairs += [(a, a + 1), (a + 1, a + 2), (a, a + 2)]
        m += [-ex, -ex, ex]
    m = np.asarray(m) * (1.0 if tied else rng.uniform(0.2, 1.0, size=(len(pairs), 1)))
    return scene(f"triangles_400_{'tied' if tied else 'random'}", pairs, np.zeros((len(pairs), 3)), 1200, [ex, ey], world=(m, np.zeros((0, 3))))


WINDOW_1100_SEED = 3  # its walk takes roots with 0 < |inW| < 1e-8, left over from subtraction: expected() asserts it


def window_1100_3() -> Dict[str, object]:
    """True geometry with direction noise on a window graph: lanes own four or five nodes, root steps and score steps alternate by the hundred."""
    rng = np.random.default_rng(WINDOW_1100_SEED)
    n = 1100
    centre, rot, _, _ = true_geometry(rng, n, 0)
    pairs = window(n, 3)
    t = ref.unit(pair_directions(centre, rot, pairs) + rng.normal(scale=0.5, size=(len(pairs), 3)))
    return scene("window_1100_3", pairs, t, n, random_units(rng, 2), rotation=rot)


def window_tier_boundary(n: int) -> Dict[str, object]:
    """TR_LDS_NODES = 2048 nodes and one more, with the default lds_node_limit: the largest dynamic-LDS launch and the first graph that goes to
    the workspace by itself."""
    rng = np.random.default_rng(n)
    centre, rot, _, _ = true_geometry(rng, n, 0)
    pairs = window(n, 2)
    t = ref.unit(pair_directions(centre, rot, pairs) + rng.normal(scale=0.5, size=(len(pairs), 3)))
    return scene(f"window_{n}_2", pairs, t, n, random_units(rng, 2), rotation=rot)


MANY_DIRECTIONS = 770  # more than the 768 workgroups of the MFAS kernel: workgroups 0 and 1 walk a second direction


def many_directions(name: str) -> Dict[str, object]:
    """An existing graph with 770 seeded directions: directions_770_workspace is the 13-node directions_* graph on the workspace tier, tier_770 the
    300-node tiers() graph on the LDS tier."""
    sc = dict(direction_counts(7) if name == "directions_770_workspace" else tiers(2048))
    sc["name"], sc["directions"] = name, random_units(np.random.default_rng(43), MANY_DIRECTIONS)
    sc["lds_node_limit"] = 0 if name == "directions_770_workspace" else -1
    return sc


ROOT_EPSILON_TWINS = (5e-9, 2e-8, 1e-8)  # the weight of the edge into the lower camera of twin k (cameras 2 k, 2 k + 1)


def root_epsilon() -> Dict[str, object]:
    """World directions given, projected on e_x: three components of two cameras, the edge pointing into the lower-numbered one with weight 5e-9,
    2e-8 and exactly 1e-8. inW < 1e-8 is strict: only the first lower camera is a root despite its incoming edge and goes before its twin."""
    pairs = [(2 * k, 2 * k + 1) for k in range(len(ROOT_EPSILON_TWINS))]
    m = np.asarray([[x, 0.6, 0.8] for x in ROOT_EPSILON_TWINS])
    return scene("root_epsilon", pairs, np.zeros((len(pairs), 3)), 2 * len(pairs), [[1.0, 0.0, 0.0]], world=(m, np.zeros((0, 3))))


NEW_SCENE_NAMES = ["triangles_400_tied", "triangles_400_random", "window_1100_3", "window_2048_2", "window_2049_2", "directions_770_workspace", "tier_770", "root_epsilon"]
SCENE_NAMES = (["empty", "one_edge", "five_cameras"] + [f"{kind}_{n}" for n in (63, 64, 65, 255, 256, 257, 513) for kind in ("chain", "ring")] +
               ["hub_300", "lost_camera", "axis_aligned", "cyclic_conflicts", "gaps_and_invalid", "directions_1", "directions_7", "directions_65", "tier_lds", "tier_workspace"] +
               NEW_SCENE_NAMES)
BRUTE_FORCE = ("triangles_400_tied", "triangles_400_random", "window_1100_3", "directions_770_workspace", "tier_770", "root_epsilon")  # one direction each


@lru_cache(maxsize=None)
def get(name: str) -> Dict[str, object]:
    if name == "empty":
        return scene("empty", [], np.zeros((0, 3)), 4, random_units(np.random.default_rng(1), 3))
    if name == "one_edge":
        return scene("one_edge", [(1, 3)], [[0.6, 0.0, 0.8]], 4, random_units(np.random.default_rng(2), 3))
    if name == "five_cameras":
        return five_cameras()
    if name.startswith(("chain_", "ring_")):
        kind, n = name.split("_")
        return chain_or_ring(int(n), kind == "ring", seed=int(n))
    if name in ("directions_770_workspace", "tier_770"):
        return many_directions(name)
    if name.startswith("directions_"):
        return direction_counts(int(name.split("_")[1]))
    if name.startswith("triangles_400_"):
        return triangles_400(name.endswith("_tied"))
    if name in ("window_2048_2", "window_2049_2"):
        return window_tier_boundary(int(name.split("_")[1]))
    if name in ("window_1100_3", "root_epsilon"):
        return {"window_1100_3": window_1100_3, "root_epsilon": root_epsilon}[name]()
    return {"hub_300": hub, "lost_camera": lost_camera, "axis_aligned": axis_aligned, "cyclic_conflicts": cyclic_conflicts, "gaps_and_invalid": gaps_and_invalid,
            "tier_lds": lambda: tiers(2048), "tier_workspace": lambda: tiers(128)}[name]()


@lru_cache(maxsize=None)
def expected(name: str) -> Dict[str, np.ndarray]:
    """The restatement's outputs for the scene, and the scene's own assertions."""
    sc = get(name)
    out = restate(sc, want_branches=True)
    for key in ("pair_weight", "meas_weight"):
        w = out[key][np.isfinite(out[key])]
        assert (np.abs(w - sc["threshold"]) > THRESHOLD_MARGIN).all(), f"{name}: a mean weight within {THRESHOLD_MARGIN} of the threshold"
    c = dict(zip(ref.COUNT_FIELDS, out["counts"].tolist()))
    steps = out["score_steps"]
    if name == "empty":
        assert c["nodes"] == 0 and (out["position"] == -1).all()
    elif name == "one_edge":
        assert c["nodes"] == 2 and c["inlier_pairs"] == 1 and out["pair_weight"][0] == 0.0
    elif name == "five_cameras":
        rejected = [tuple(p) for p, k in zip(sc["pair_images"].tolist(), out["pair_inlier"]) if not k]
        assert rejected == [(0, 4), (1, 4), (2, 4), (3, 4)] and out["camera_inlier"].tolist() == [1, 1, 1, 1, 0]
    elif name.startswith(("chain_", "ring_")):
        n = int(name.split("_")[1])
        assert c["nodes"] == n and c["pair_edges"] == (n if name.startswith("ring_") else n - 1)
    elif name == "hub_300":
        assert np.bincount(sc["pair_images"].reshape(-1)).max() >= 300
    elif name == "lost_camera":
        dropped = (out["meas_weight"] < sc["threshold"]) & (out["meas_inlier"] == 0)
        assert out["camera_inlier"].tolist() == [1, 1, 1, 1, 1, 1, 1, 0] and dropped.sum() >= 3 and (sc["image"][dropped] == 7).all() and c["inlier_measurements"] > 0
    elif name == "axis_aligned":
        g = out["graph"]
        w = np.stack([ref.project(g["m"], d) for d in sc["directions"]])
        assert set(np.unique(w).tolist()) <= {-1.0, 0.0, 1.0} and (w == 0).sum() > 10 and steps[0] >= 3 and steps[1] >= 1
    elif name == "cyclic_conflicts":
        assert 3 * steps.max() >= c["nodes"] == 30
    elif name == "gaps_and_invalid":
        on = np.isfinite(out["pair_weight"])
        assert on.tolist() == [1, 1, 1, 0, 1, 0, 1, 1, 0, 1, 1, 1, 1] and c["measurement_edges"] == 8 and c["nodes"] == 12 - 3 + 3
        assert (out["position"][:, [3, 7, 8, 12 + 1]] == -1).all()
    elif name in ("directions_770_workspace", "tier_770"):
        # more directions than the MFAS kernel has workgroups, on either tier; the second walk is not a repeat of the first
        assert len(sc["directions"]) == MANY_DIRECTIONS > 768 and c["nodes"] == (13 if name == "directions_770_workspace" else 300) and steps.max() > 0
        assert (sc["lds_node_limit"] == 0) == (name == "directions_770_workspace") and c["inlier_pairs"] > 0
        assert (out["position"][768] != out["position"][0]).any() and (out["position"][769] != out["position"][1]).any()
    elif name.startswith("directions_"):
        assert len(sc["directions"]) == int(name.split("_")[1]) and c["nodes"] == 13 and c["inlier_pairs"] > 0 and steps.max() > 0
    elif name.startswith("tier_"):
        assert c["nodes"] == 300 and (sc["lds_node_limit"] < 300) == (name == "tier_workspace")
    elif name.startswith("triangles_400_"):
        chosen = out["score_choices"][0]
        assert c["nodes"] == 1200 and steps.tolist() == [400, 0] and sc["lds_node_limit"] == -1
        if name == "triangles_400_tied":
            # every score step is a tie among all nodes of the unbroken triangles: the smallest id wins, so triangle k is walked at steps 3 k ..
            assert out["tied_score_steps"].tolist() == [400, 0] and c["inlier_pairs"] == 800
            assert (out["position"][0][0:1200:3] == np.arange(0, 1200, 3)).all() and chosen.tolist() == list(range(0, 1200, 3))
        else:
            # distinct scores: the winners are anywhere in the id range, in every wave and at every depth of a lane's node list
            assert out["tied_score_steps"].tolist() == [0, 0] and (np.diff(chosen) < 0).sum() > 100 and (np.diff(chosen) > 0).sum() > 100
            assert set((chosen % 256 // 64).tolist()) == {0, 1, 2, 3} and set((chosen // 256).tolist()) == {0, 1, 2, 3, 4}
            assert 800 < c["inlier_pairs"] < 1200
    elif name == "window_1100_3":
        leftovers = np.concatenate(out["epsilon_root_in_w"])
        assert c["nodes"] == 1100 and c["pair_edges"] == 3294 and steps.min() > 200 and (c["nodes"] - steps).min() > 200
        assert ((leftovers != 0) & (np.abs(leftovers) < ref.ROOT_EPSILON)).any(), "no root with 0 < |inW| < 1e-8 left over from subtraction: choose another seed"
        assert all(len(set((ch // 256).tolist())) >= 4 for ch in out["score_choices"])  # score steps won at the fourth and fifth node of a lane
    elif name in ("window_2048_2", "window_2049_2"):
        assert c["nodes"] == int(name.split("_")[1]) and sc["lds_node_limit"] == -1 and steps.min() > 100
        assert all((ch >= 2048 - 256).any() for ch in out["score_choices"])  # a score step won by a lane's last node
    elif name == "root_epsilon":
        p = out["position"][0]
        assert ROOT_EPSILON_TWINS[0] < ref.ROOT_EPSILON == ROOT_EPSILON_TWINS[2] < ROOT_EPSILON_TWINS[1]
        assert p[0] < p[1] and p[2] > p[3] and p[4] > p[5], p  # the root despite its edge goes first; 2e-8 and exactly 1e-8 (strict <) wait for their twins
        assert out["epsilon_roots"][0] >= 1 and out["epsilon_root_in_w"][0].tolist() == [5e-9] and steps[0] == 0
        assert out["pair_weight"].tolist() == [5e-9, 0.0, 0.0]
    if name in BRUTE_FORCE:
        g = out["graph"]
        brute = ref.mfas_positions_brute_force(g["key1"], g["key2"], g["m"], sc["directions"][0], len(out["position"][0]))
        assert brute.tobytes() == out["position"][0].tobytes(), f"{name}: the restatement's positions differ from the brute-force ordering on direction 0"
    return out


def all_names() -> List[str]:
    return list(SCENE_NAMES)


OUTPUT_KEYS = ("world_pair", "world_meas", "pair_weight", "meas_weight", "pair_inlier", "meas_inlier", "camera_inlier", "position", "counts")


def assert_bytes_equal(label: str, got: Dict[str, np.ndarray], exp: Dict[str, np.ndarray], keys: Sequence[str] = OUTPUT_KEYS) -> None:
    for key in keys:
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(exp[key])
        assert a.dtype == b.dtype and a.shape == b.shape, f"{label}: {key} is {a.dtype}{a.shape}, expected {b.dtype}{b.shape}"
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero(a.reshape(-1).view(np.uint8 if a.dtype.itemsize == 1 else f"u{a.dtype.itemsize}") != b.reshape(-1).view(np.uint8 if b.dtype.itemsize == 1 else f"u{b.dtype.itemsize}"))
            raise AssertionError(f"{label}: {key} differs at {len(bad)} of {a.size} entries, first at {bad[:5].tolist()}: {a.reshape(-1)[bad[:5]]} against {b.reshape(-1)[bad[:5]]}")
