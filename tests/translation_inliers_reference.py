"""The specification of the device's 1DSfM outlier rejection (``gtsfm_translation_inliers_f64``, gtsfm_amd/csrc/translation_kernels.hip): a numpy
restatement of ``TranslationAveraging1DSFM.compute_inliers`` and what feeds it (``gtsfm/averaging/translation/averaging_1dsfm.py:234-437,684-707``)
and of gtsam's greedy minimum-feedback-arc-set ordering (``gtsam/sfm/MFAS.cpp``), in float64 with every sum written out in a stated order.
Elementwise numpy ``+ - * /`` and ``sqrt`` are IEEE operations, so each line below is one rounding per element; nothing here goes through
``np.linalg.norm``, ``np.dot`` or BLAS.

PARITY UNPINNED towards gtsam: MFAS iterates an ``unordered_map`` when it looks for a root or the best score, so its choice among several
roots or tied scores follows the hash order; here the smallest node id wins. ``Unit3``'s normalisation may differ in the last bits.

Node ids: camera i -> i, landmark (track) j -> num_images + j. A pair row (i1, i2, i2Ui1) is the measurement (key1, key2) = (i2, i1), a track
measurement is (key1, key2) = (camera, num_images + track); edges are taken in ascending (key1, key2) order."""

from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np

MAX_PROJECTION_DIRECTIONS = 2000
OUTLIER_WEIGHT_THRESHOLD = 0.125
MIN_TRACK_MEASUREMENTS_FOR_AVERAGING = 3
TRACKS_MEASUREMENTS_PER_CAMERA = 12
ROOT_EPSILON = 1e-8
COUNT_FIELDS = ("pair_edges", "measurement_edges", "nodes", "inlier_pairs", "inlier_measurements", "inlier_cameras")


def unit(v: np.ndarray) -> np.ndarray:
    """v / sqrt((x x + y y) + z z), rows of [..., 3]."""
    v = np.asarray(v, np.float64)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    with np.errstate(all="ignore"):
        n = np.sqrt((x * x + y * y) + z * z)
        return np.stack([x / n, y / n, z / n], axis=-1)


def rotate(r9: np.ndarray, v: np.ndarray) -> np.ndarray:
    """Row-major [..., 9] times [..., 3], each row summed as (r0 x + r1 y) + r2 z."""
    r9, v = np.asarray(r9, np.float64), np.asarray(v, np.float64)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    with np.errstate(all="ignore"):
        return np.stack([(r9[..., 3 * k] * x + r9[..., 3 * k + 1] * y) + r9[..., 3 * k + 2] * z for k in range(3)], axis=-1)


def project(m: np.ndarray, d: np.ndarray) -> np.ndarray:
    """w = (mx dx + my dy) + mz dz per row of m."""
    return (m[..., 0] * d[0] + m[..., 1] * d[1]) + m[..., 2] * d[2]


def finite_rows(a: np.ndarray) -> np.ndarray:
    return np.isfinite(a).all(axis=-1)


def world_pair_directions(pair_images, pair_direction, pair_enable, rotation, rotation_valid) -> Tuple[np.ndarray, np.ndarray]:
    """get_valid_measurements_in_world_frame: (world directions [E, 3] with NaN rows where not valid, valid [E]). A row is valid when it is
    enabled, wRi[i2] is valid (wRi[i1] is not looked at: the reference's quirk) and its world direction is three finite numbers (the array
    form of ``i2Ui1 is not None``)."""
    pairs = np.asarray(pair_images, np.int64).reshape(-1, 2)
    e = len(pairs)
    out = np.full((e, 3), np.nan)
    on = np.ones(e, bool) if pair_enable is None else np.asarray(pair_enable).astype(bool)
    rot, rv = np.asarray(rotation, np.float64).reshape(-1, 9), np.asarray(rotation_valid).astype(bool)
    if e == 0:
        return out, np.zeros(0, bool)
    n = len(rv)
    bad = on & ((pairs[:, 0] < 0) | (pairs[:, 0] >= pairs[:, 1]) | (pairs[:, 1] >= n))
    if bad.any():
        raise ValueError(f"an enabled pair row has i1 >= i2 or names an image outside 0 .. {n - 1}")
    i2 = np.where(on, pairs[:, 1], 0)
    valid = on & rv[i2]
    w = unit(rotate(rot[i2], np.asarray(pair_direction, np.float64).reshape(-1, 3)))
    valid &= finite_rows(w)
    out[valid] = w[valid]
    return out, valid


def track_of_measurement(track_off: np.ndarray) -> np.ndarray:
    track_off = np.asarray(track_off, np.int64)
    return np.repeat(np.arange(len(track_off) - 1, dtype=np.int64), np.diff(track_off))


def world_landmark_directions(track_off, image, uv, track_enable, meas_enable, rotation, rotation_valid, intrinsics) -> Tuple[np.ndarray, np.ndarray]:
    """_get_landmark_directions for pinhole cameras (intrinsics [N, 4] = fx, fy, cx, cy; uv float32): unit(wRi unit(((u - cx) / fx,
    (v - cy) / fy, 1))). An enabled measurement of a camera without a valid rotation raises, as the reference asserts."""
    image = np.asarray(image, np.int64)
    s = len(image)
    out = np.full((s, 3), np.nan)
    if s == 0:
        return out, np.zeros(0, bool)
    trk = track_of_measurement(track_off)
    on = np.asarray(track_enable).astype(bool)[trk] & (np.ones(s, bool) if meas_enable is None else np.asarray(meas_enable).astype(bool))
    rot, rv, k = np.asarray(rotation, np.float64).reshape(-1, 9), np.asarray(rotation_valid).astype(bool), np.asarray(intrinsics, np.float64).reshape(-1, 4)
    if (on & ((image < 0) | (image >= len(rv)))).any():
        raise ValueError("an enabled measurement names a camera out of range")
    cam = np.where(on, image, 0)
    if (on & ~rv[cam]).any():
        raise ValueError("Camera must have valid rotation to use tracks for averaging.")
    uv64 = np.asarray(uv, np.float32).reshape(-1, 2).astype(np.float64)
    with np.errstate(all="ignore"):
        x, y = (uv64[:, 0] - k[cam, 2]) / k[cam, 0], (uv64[:, 1] - k[cam, 3]) / k[cam, 1]
    w = unit(rotate(rot[cam], unit(np.stack([x, y, np.ones(s)], axis=-1))))
    valid = on & finite_rows(w)
    out[valid] = w[valid]
    return out, valid


def select_tracks(track_off, image, valid_cameras: Set[int], measurements_per_camera: int = TRACKS_MEASUREMENTS_PER_CAMERA,
                  use_all_tracks: bool = False) -> Tuple[np.ndarray, np.ndarray, List[int]]:
    """_select_tracks_for_averaging on the track builder's CSR arrays: (track_enable [T] uint8, meas_enable [S] uint8, the selected track
    ids in the order of selection). Measurements of cameras outside ``valid_cameras`` are dropped, then tracks left with fewer than 3; then
    ``np.argmax(improvement)`` (the first maximum) with the reference's counters exactly as written."""
    track_off, image = np.asarray(track_off, np.int64), np.asarray(image, np.int64)
    t = len(track_off) - 1
    meas_ok = np.isin(image, np.fromiter(valid_cameras, np.int64, len(valid_cameras)))
    filtered = [j for j in range(t) if int(meas_ok[track_off[j]:track_off[j + 1]].sum()) >= MIN_TRACK_MEASUREMENTS_FOR_AVERAGING]
    cams = {j: [int(c) for c, ok in zip(image[track_off[j]:track_off[j + 1]], meas_ok[track_off[j]:track_off[j + 1]]) if ok] for j in filtered}
    if use_all_tracks:
        chosen = list(filtered)
    else:
        chosen = []
        remaining = {c: measurements_per_camera for c in valid_cameras}
        improvement = [len(cams[j]) for j in filtered]
        lookup: Dict[int, List[int]] = {c: [] for c in valid_cameras}
        for k, j in enumerate(filtered):
            for c in cams[j]:
                lookup[c].append(k)
        for _ in range(len(filtered)):
            best = int(np.argmax(improvement))
            if improvement[best] <= 0:
                break
            chosen.append(filtered[best])
            improvement[best] = 0
            for c in cams[filtered[best]]:
                if remaining[c] == 0:
                    continue
                remaining[c] -= 1
                if remaining[c] == 0:
                    for k in lookup[c]:
                        improvement[k] = improvement[k] - 1 if improvement[k] > 0 else 0
    track_enable = np.zeros(t, np.uint8)
    track_enable[chosen] = 1
    return track_enable, meas_ok.astype(np.uint8), chosen


def build_edges(pair_images, w_pair, pair_valid, track_off, image, w_meas, meas_valid, num_images: int) -> Dict[str, np.ndarray]:
    """The edge table in ascending (key1, key2) order over the valid rows: ``row`` is the unified row (pair row e, or E + s for measurement
    s), ``key1`` / ``key2`` the node ids, ``m`` the world directions. A duplicate key is refused."""
    pairs = np.asarray(pair_images, np.int64).reshape(-1, 2)
    e = len(pairs)
    trk = track_of_measurement(track_off)
    pr, mr = np.flatnonzero(pair_valid), np.flatnonzero(meas_valid)
    key1 = np.concatenate([pairs[pr, 1], np.asarray(image, np.int64)[mr]])
    key2 = np.concatenate([pairs[pr, 0], num_images + trk[mr]])
    row = np.concatenate([pr, e + mr])
    m = np.concatenate([np.asarray(w_pair, np.float64).reshape(-1, 3)[pr], np.asarray(w_meas, np.float64).reshape(-1, 3)[mr]])
    order = np.lexsort((key2, key1))
    key1, key2, row, m = key1[order], key2[order], row[order], m[order]
    if len(key1) > 1 and ((np.diff(key1) == 0) & (np.diff(key2) == 0)).any():
        raise ValueError("a measurement is listed twice")
    return {"key1": key1, "key2": key2, "row": row, "m": m}


def mfas_positions(key1: np.ndarray, key2: np.ndarray, m: np.ndarray, d: np.ndarray, num_nodes: int, return_branches: bool = False):
    """gtsam's MFAS::computeOrdering for one unit projection direction over edges in ascending (key1, key2) order: position [num_nodes] int32,
    -1 for nodes without an edge. With ``return_branches`` also a dict of what the steps did: ``score_steps`` (steps that took the score branch),
    ``tied_score_steps`` (score steps whose largest score two or more live nodes held), ``epsilon_roots`` (root steps whose root had inW != 0,
    what subtraction left or an incoming weight below ROOT_EPSILON), ``score_choices`` (the nodes the score steps chose, in order) and
    ``epsilon_root_in_w`` (the inW of the epsilon roots)."""
    w = project(m, d)
    a = np.abs(w)
    forward = ~(w < 0)  # includes +-0, as gtsam's weight >= 0
    src, dst = np.where(forward, key1, key2), np.where(forward, key2, key1)
    in_w, out_w = np.zeros(num_nodes), np.zeros(num_nodes)
    np.add.at(in_w, dst, a)  # unbuffered, in edge order
    np.add.at(out_w, src, a)
    adj: List[List[Tuple[int, int]]] = [[] for _ in range(num_nodes)]
    for e in range(len(w)):
        adj[key1[e]].append((int(key2[e]), e))
        adj[key2[e]].append((int(key1[e]), e))
    alive = np.zeros(num_nodes, bool)
    alive[key1], alive[key2] = True, True
    position = np.full(num_nodes, -1, np.int32)
    tied_score_steps, score_choices, epsilon_root_in_w = 0, [], []
    for step in range(int(alive.sum())):
        roots = alive & (in_w < ROOT_EPSILON)
        if roots.any():
            choice = int(np.argmax(roots))
            if in_w[choice] != 0:
                epsilon_root_in_w.append(float(in_w[choice]))
        else:
            score = np.where(alive, (out_w + 1.0) / (in_w + 1.0), -np.inf)
            choice = int(np.argmax(score))
            score_choices.append(choice)
            tied_score_steps += int((score == score[choice]).sum() > 1)
        position[choice] = step
        alive[choice] = False
        for nbr, e in adj[choice]:
            if alive[nbr]:
                if src[e] == nbr:
                    out_w[nbr] = out_w[nbr] - a[e]
                else:
                    in_w[nbr] = in_w[nbr] - a[e]
    branches = {"score_steps": len(score_choices), "tied_score_steps": tied_score_steps, "epsilon_roots": len(epsilon_root_in_w),
                "score_choices": np.asarray(score_choices, np.int64), "epsilon_root_in_w": np.asarray(epsilon_root_in_w, np.float64)}
    return (position, branches) if return_branches else position


def mfas_positions_brute_force(key1, key2, m, d, num_nodes: int) -> np.ndarray:
    """The same ordering with dict-of-dicts, every node's sums recomputed at every step from the surviving edges in the same order."""
    w = project(m, d)
    edges = {(int(k1), int(k2)): float(x) for k1, k2, x in zip(key1, key2, w)}
    nodes = sorted({k for pair in edges for k in pair})
    position = np.full(num_nodes, -1, np.int32)
    for step in range(len(nodes)):
        in_w, out_w = {n: 0.0 for n in nodes}, {n: 0.0 for n in nodes}
        for (k1, k2), x in edges.items():
            s, t = (k1, k2) if not x < 0 else (k2, k1)
            in_w[t] += abs(x)
            out_w[s] += abs(x)
        choice = next((n for n in nodes if in_w[n] < ROOT_EPSILON), None)
        if choice is None:
            best = max((out_w[n] + 1.0) / (in_w[n] + 1.0) for n in nodes)
            choice = next(n for n in nodes if (out_w[n] + 1.0) / (in_w[n] + 1.0) == best)
        position[choice] = step
        nodes.remove(choice)
        edges = {k: x for k, x in edges.items() if choice not in k}
    return position


def outlier_weights(key1, key2, m, d, position) -> np.ndarray:
    """MFAS::computeOutlierWeights: |w| where the edge points backwards in the ordering, else 0."""
    w = project(m, d)
    forward = ~(w < 0)
    src, dst = np.where(forward, key1, key2), np.where(forward, key2, key1)
    return np.where(position[src] > position[dst], np.abs(w), 0.0)


def translation_inliers(pair_images, pair_direction, pair_enable, rotation, rotation_valid, intrinsics, track_off, image, uv, track_enable, meas_enable,
                        directions, threshold: float = OUTLIER_WEIGHT_THRESHOLD, world: Optional[Tuple[np.ndarray, np.ndarray]] = None,
                        want_branches: bool = False) -> Dict[str, np.ndarray]:
    """What ``gtsfm_translation_inliers_f64`` computes, array for array. ``world``: (w_pair [E, 3], w_meas [S, 3]) given instead of computed
    (a row is valid when it is enabled and finite)."""
    pairs = np.asarray(pair_images, np.int64).reshape(-1, 2)
    rv = np.asarray(rotation_valid).astype(bool)
    n, e = len(rv), len(pairs)
    track_off, image = np.asarray(track_off, np.int64), np.asarray(image, np.int64)
    t, s = len(track_off) - 1, len(image)
    directions = np.asarray(directions, np.float64).reshape(-1, 3)
    d_count = len(directions)
    if world is None:
        w_pair, pair_valid = world_pair_directions(pairs, pair_direction, pair_enable, rotation, rv)
        w_meas, meas_valid = world_landmark_directions(track_off, image, uv, track_enable, meas_enable, rotation, rv, intrinsics)
    else:
        on_p = np.ones(e, bool) if pair_enable is None else np.asarray(pair_enable).astype(bool)
        on_m = (np.asarray(track_enable).astype(bool)[track_of_measurement(track_off)] if s else np.zeros(0, bool)) & (np.ones(s, bool) if meas_enable is None else np.asarray(meas_enable).astype(bool))
        if (on_p & ((pairs[:, 0] < 0) | (pairs[:, 0] >= pairs[:, 1]) | (pairs[:, 1] >= n))).any() or (on_m & ((image < 0) | (image >= n))).any():
            raise ValueError("an enabled row names an image out of range or has i1 >= i2")
        w_pair, w_meas = np.array(world[0], np.float64).reshape(-1, 3), np.array(world[1], np.float64).reshape(-1, 3)
        pair_valid, meas_valid = on_p & finite_rows(w_pair), on_m & finite_rows(w_meas)
        w_pair[~pair_valid], w_meas[~meas_valid] = np.nan, np.nan
    g = build_edges(pairs, w_pair, pair_valid, track_off, image, w_meas, meas_valid, n)
    if len(g["row"]) and d_count <= 0:
        raise ValueError("no projection direction")
    nodes = n + t
    position = np.full((d_count, nodes), -1, np.int32)
    total = np.zeros(len(g["row"]))
    branches = []
    for k, d in enumerate(directions):
        position[k], taken = mfas_positions(g["key1"], g["key2"], g["m"], d, nodes, return_branches=True)
        branches.append(taken)
        total = total + outlier_weights(g["key1"], g["key2"], g["m"], d, position[k])
    mean = np.full(e + s, np.nan)
    if len(g["row"]):
        mean[g["row"]] = total / d_count
    with np.errstate(invalid="ignore"):
        inlier = mean < threshold
    pair_inlier, edge_inlier = inlier[:e], inlier[e:]
    camera_inlier = np.zeros(n, bool)
    camera_inlier[pairs[pair_inlier].reshape(-1)] = True
    meas_inlier = edge_inlier & camera_inlier[np.where(edge_inlier, image, 0)] if s else np.zeros(0, bool)
    num_nodes = len(np.unique(np.concatenate([g["key1"], g["key2"]]))) if len(g["row"]) else 0
    counts = np.array([pair_valid.sum(), meas_valid.sum(), num_nodes, pair_inlier.sum(), meas_inlier.sum(), camera_inlier.sum(), 0, 0], np.int32)
    if len(g["row"]) == 0:
        position[:] = -1
    out = {"world_pair": w_pair, "world_meas": w_meas, "pair_weight": mean[:e], "meas_weight": mean[e:], "pair_inlier": pair_inlier.astype(np.uint8),
           "meas_inlier": meas_inlier.astype(np.uint8), "camera_inlier": camera_inlier.astype(np.uint8), "position": position, "counts": counts, "graph": g}
    if want_branches:
        for key in ("score_steps", "tied_score_steps", "epsilon_roots"):
            out[key] = np.asarray([b[key] for b in branches], np.int64)
        out["score_choices"], out["epsilon_root_in_w"] = [b["score_choices"] for b in branches], [b["epsilon_root_in_w"] for b in branches]
    return out


def sample_uniform_directions(num_samples: int = MAX_PROJECTION_DIRECTIONS) -> np.ndarray:
    """sampling_utils.sample_random_directions: np.random.normal(size=(n, 3)) from the global generator, normalised."""
    return unit(np.random.normal(size=(num_samples, 3)))


def longdouble_world_pair(pair_direction, rotation_rows) -> np.ndarray:
    """unit(R v) in np.longdouble, for measuring the restatement's own rounding."""
    v, r = np.asarray(pair_direction, np.longdouble).reshape(-1, 3), np.asarray(rotation_rows, np.longdouble).reshape(-1, 9)
    w = np.stack([r[:, 3 * k] * v[:, 0] + r[:, 3 * k + 1] * v[:, 1] + r[:, 3 * k + 2] * v[:, 2] for k in range(3)], axis=-1)
    return w / np.sqrt((w * w).sum(axis=-1))[:, None]
