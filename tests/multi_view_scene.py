"""One planted scene for the chain verifier -> two-view -> view graph -> 1DSfM -> tracks -> triangulation, and that chain restated on the CPU.

The scene: ``NUM_IMAGES`` pinhole cameras with different, anisotropic intrinsics, known ``wRi`` and centres spread in x, y and z, looking at a
slab of ``NUM_POINTS`` world points. Every image has a float32 keypoint table of ``CAP`` rows: the points' projections (0.4 px noise) at
shuffled slots, the rest distractors. The edges are a window of ``WINDOW`` over the camera order, so every edge lies in triplets. Per edge about
``PER_EDGE`` putative matches in i1 order, 20 % of them re-pointed at random keypoints (never at a ghost keypoint: what the tests assert about
ghosts must not be a matter of chance).

Two window edges are planted wrong, both geometrically consistent, so the verifier accepts them:
``WRONG_ROTATION`` = (i, j): image j also holds "ghost" keypoints, the points as camera j rolled by ``ROLL_DEG`` about its axis sees them, and the
edge matches image i's true keypoints to those ghosts; ``WRONG_TRANSLATION``: the same with camera j moved to another centre, its orientation kept.

Two further edges lie beyond the window, one in each launch, for the routes on which an edge leaves the chain: ``LOSES_SUPPORT`` has so few
matches that the adjustment's filter leaves fewer than the inlier support asks for (``two_view`` zeroes its mask and ``stats[:, 0]`` while its pose
stays in the launch), ``NO_MODEL`` has fewer matches than the verifier needs (NaN pose, all counts zero). Neither may reach a later stage.

The edges of ``FALLBACK`` are present in ``putative`` and absent from the device match table: the generator verifies them per pair on the host.
The device match table is in the generators' capacity layout: every edge owns ``CAP`` rows, the first ``match_count`` of them are matches, the
rest hold indices >= 2^20 on both sides (as tests/tracks_reference.scene_capacity_layout fills them). ``LAUNCH_PAIRS`` pairs per verifier launch
make two launches of the device edges.

The restated chain: every stage is a call of a restatement the suite already has, and takes its upstream input as an argument -- the host test
feeds it the previous restatement's output, the GPU test what the device produced upstream.

The ground-truth bounds (``MEASURED_*``) were measured on the restated chain on the CPU (tests/test_multi_view_chain_host.py prints them and
asserts that they have not moved); the device is held to twice each, since it may stop one step to either side. profiles/multi_view_chain.txt
records them."""

from __future__ import annotations

import functools
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from oracle import verifier_oracle as vo
from tests import tracks_reference as TR
from tests import translation_inliers_reference as ti_ref
from tests import triangulation_reference as tri
from tests import two_view_ba_reference as ba_ref
from tests import view_graph_reference as vg_ref

Edge = Tuple[int, int]

SEED = 7
NUM_IMAGES, CAP, NUM_POINTS, WINDOW, PER_EDGE = 10, 512, 260, 3, 110
NOISE_PX, REPOINTED = 0.4, 0.2
WRONG_ROTATION, WRONG_TRANSLATION = (3, 6), (5, 8)
ROLL_DEG = 20.0
FALLBACK = ((1, 2), (6, 9))
LOSES_SUPPORT, NO_MODEL = (0, 4), (5, 9)  # beyond the window: LOSES_SUPPORT_MATCHES matches of which NEAR_MISSES are near misses, and NO_MODEL_MATCHES matches (the verifier needs 6)
LOSES_SUPPORT_MATCHES, NO_MODEL_MATCHES = 20, 5
NEAR_MISSES, NEAR_MISS_PX = 8, 1.7  # of LOSES_SUPPORT's matches: the second keypoint lies this far from the projection, inside the verifier's threshold
LAUNCH_PAIRS = 12  # 24 device edges: two verifier launches
VERIFY_THRESHOLD_PX = 2.0
MIN_INLIERS, MIN_RATIO = 15, 0.1  # TwoViewOptions' defaults, the InlierSupportProcessor's two thresholds
VIEW_GRAPH_THRESHOLD_DEG = 7.0  # CycleConsistentRotationViewGraphEstimator's default
NUM_DIRECTIONS = 64
TRIANGULATION_THRESHOLD_PX = 3.0

# Measured on the restated chain (CPU) for SEED; the bounds the device results are held to are twice these.
MEASURED_ROTATION_DEG = 0.237  # the largest rotation error of a good edge after the verifier and after the adjustment
MEASURED_DIRECTION_DEG = 1.68  # the same for the translation direction
MEASURED_POINT_DISTANCE = 0.571  # the largest distance of a triangulated surviving track from its planted point, world units
MEASURED_POINT_MEDIAN = 0.0082  # the median of those distances: the largest one is a single two-view track of little parallax
PLANTED_ROTATION_MIN_DEG = 15.0  # the wrong-rotation edge lies at ROLL_DEG: far outside
PLANTED_DIRECTION_MIN_DEG = 60.0
ROTATION_BOUND_DEG, DIRECTION_BOUND_DEG = 2 * MEASURED_ROTATION_DEG, 2 * MEASURED_DIRECTION_DEG
POINT_BOUND, POINT_MEDIAN_BOUND = 2 * MEASURED_POINT_DISTANCE, 2 * MEASURED_POINT_MEDIAN


def support(ratio: float, valid: int) -> bool:
    """inlier_support_processor.py:73-95 as tests/test_two_view_scene_gpu.support states it, with this scene's thresholds."""
    return not (ratio < MIN_RATIO) and not (valid > 0 and valid < MIN_INLIERS)


def _rot_z(deg: float) -> np.ndarray:
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _project(k: np.ndarray, w_r_c: np.ndarray, centre: np.ndarray, x: np.ndarray) -> np.ndarray:
    cam = (x - centre) @ w_r_c  # rows of wRc^T (X - c)
    assert (cam[:, 2] > 1.0).all(), "a point behind or too close to a camera"
    return np.stack([k[0] * cam[:, 0] / cam[:, 2] + k[2], k[1] * cam[:, 1] / cam[:, 2] + k[3]], axis=1)


def window_edges() -> List[Edge]:
    return [(i, j) for i in range(NUM_IMAGES) for j in range(i + 1, min(NUM_IMAGES, i + WINDOW + 1))]


@functools.lru_cache(maxsize=None)
def planted_scene(seed: int = SEED) -> Dict[str, object]:
    rng = np.random.default_rng(seed)
    points = np.stack([rng.uniform(-3.5, 3.5, NUM_POINTS), rng.uniform(-2.5, 2.5, NUM_POINTS), rng.uniform(7.0, 9.5, NUM_POINTS)], axis=1)
    idx = np.arange(NUM_IMAGES)
    centre = np.stack([-4.05 + 0.9 * idx, 1.8 * np.sin(1.3 * idx), 1.5 * np.cos(0.9 * idx)], axis=1) + rng.normal(0.0, 0.05, (NUM_IMAGES, 3))
    intrinsics = np.stack([700.0 + 15.0 * idx, (700.0 + 15.0 * idx) * (1.04 + 0.01 * (idx % 4)), 320.0 + 3.0 * idx, 240.0 - 2.0 * idx], axis=1)
    w_r_i = np.zeros((NUM_IMAGES, 3, 3))
    for i in range(NUM_IMAGES):
        z = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), 8.2]) - centre[i]
        z /= np.linalg.norm(z)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        w_r_i[i] = np.stack([x, np.cross(z, x), z], axis=1) @ _rot_z(rng.uniform(-6.0, 6.0))
    window = window_edges()
    edges = sorted(window + [LOSES_SUPPORT, NO_MODEL])
    extra_rng = np.random.default_rng([seed, 1])  # the two edges beyond the window draw from a generator of their own
    assert WRONG_ROTATION in edges and WRONG_TRANSLATION in edges and all(e in edges for e in FALLBACK)
    xy = np.stack([rng.uniform(0.0, 640.0, (NUM_IMAGES, CAP)), rng.uniform(0.0, 480.0, (NUM_IMAGES, CAP))], axis=2)
    slot_all = np.stack([rng.permutation(CAP) for _ in range(NUM_IMAGES)])
    slot = slot_all[:, :NUM_POINTS]
    for i in range(NUM_IMAGES):
        xy[i, slot[i]] = _project(intrinsics[i], w_r_i[i], centre[i], points) + rng.normal(0.0, NOISE_PX, (NUM_POINTS, 2))
    size = {LOSES_SUPPORT: LOSES_SUPPORT_MATCHES, NO_MODEL: NO_MODEL_MATCHES}
    chosen = {e: np.sort(rng.choice(NUM_POINTS, PER_EDGE, replace=False)) for e in window}
    chosen.update({e: np.sort(extra_rng.choice(NUM_POINTS, n, replace=False)) for e, n in size.items()})
    # the ghosts: PER_EDGE further slots of image j, the planted edge's points as the displaced camera sees them
    ghost_slot: Dict[Edge, np.ndarray] = {}
    ghost_pose = {}
    (_, jr), (it, jt) = WRONG_ROTATION, WRONG_TRANSLATION
    assert jr != jt
    ghost_pose[WRONG_ROTATION] = (w_r_i[jr] @ _rot_z(ROLL_DEG), centre[jr])
    ghost_pose[WRONG_TRANSLATION] = (w_r_i[jt], centre[it] + np.array([-2.0, 1.2, -0.3]))
    ghosts = set()
    for e, (rot, c) in ghost_pose.items():
        j = e[1]
        ghost_slot[e] = slot_all[j, NUM_POINTS:NUM_POINTS + PER_EDGE]
        xy[j, ghost_slot[e]] = _project(intrinsics[j], rot, c, points[chosen[e]]) + rng.normal(0.0, NOISE_PX, (PER_EDGE, 2))
        ghosts |= {(j, int(s)) for s in ghost_slot[e]}
    # LOSES_SUPPORT matches image i's true keypoints to keypoints of its own in image j: the projections, NEAR_MISSES of them displaced
    j = LOSES_SUPPORT[1]
    assert j not in (jr, jt)
    near_slot = slot_all[j, NUM_POINTS:NUM_POINTS + LOSES_SUPPORT_MATCHES]
    angle = extra_rng.uniform(0.0, 2.0 * np.pi, LOSES_SUPPORT_MATCHES)
    push = np.where(np.arange(LOSES_SUPPORT_MATCHES) < NEAR_MISSES, NEAR_MISS_PX, 0.0)[:, None] * np.stack([np.cos(angle), np.sin(angle)], axis=1)
    xy[j, near_slot] = _project(intrinsics[j], w_r_i[j], centre[j], points[chosen[LOSES_SUPPORT]]) + extra_rng.normal(0.0, NOISE_PX, (LOSES_SUPPORT_MATCHES, 2)) + push
    xy = xy.astype(np.float32)
    putative: Dict[Edge, np.ndarray] = {}
    for e in window + list(size):
        i, j = e
        second = ghost_slot[e] if e in ghost_slot else (near_slot if e == LOSES_SUPPORT else slot[j, chosen[e]])
        rows = np.stack([slot[i, chosen[e]], second], axis=1)
        moved = np.flatnonzero(rng.random(len(rows)) < REPOINTED) if e not in size else np.zeros(0, np.int64)  # the few matches of the two are all true
        allowed = np.array([s for s in range(CAP) if (j, s) not in ghosts])
        rows[moved, 1] = rng.choice(allowed, len(moved))
        putative[e] = rows[np.argsort(rows[:, 0], kind="stable")].astype(np.uint32)
    device_edges = [e for e in edges if e not in FALLBACK]
    # the device match table in capacity layout: CAP rows per edge (the generators give an edge as many rows as image i1 has keypoints)
    match_idx = rng.integers(1 << 20, 1 << 30, size=(len(device_edges) * CAP, 2)).astype(np.int32)
    match_idx[::2] *= -1
    for p, e in enumerate(device_edges):
        match_idx[p * CAP:p * CAP + len(putative[e])] = putative[e].astype(np.int32)
    point_of = {(i, int(slot[i, p])): p for i in range(NUM_IMAGES) for p in range(NUM_POINTS)}
    return {"points": points, "centre": centre, "wRi": w_r_i, "intrinsics": intrinsics, "xy": xy, "slot": slot, "edges": edges, "device_edges": device_edges,
            "fallback": list(FALLBACK), "putative": putative, "ghosts": ghosts, "point_of": point_of, "match_idx": match_idx,
            "match_off": (np.arange(len(device_edges) + 1, dtype=np.int64) * CAP).tolist(),
            "match_count": np.array([len(putative[e]) for e in device_edges], np.int32), "ghost_pose": ghost_pose,
            "rows": device_edges + list(FALLBACK)}  # the scene's edge rows: the launches' pairs, then the edges of ``extra``


def true_relative_pose(scene: Dict[str, object], edge: Edge) -> Tuple[np.ndarray, np.ndarray]:
    """(i2Ri1, unit i2Ui1) of the TRUE cameras of an edge."""
    i, j = edge
    rot, c = scene["wRi"], scene["centre"]
    t = rot[j].T @ (c[i] - c[j])
    return rot[j].T @ rot[i], t / np.linalg.norm(t)


def pose_errors(scene: Dict[str, object], edge: Edge, rotation: np.ndarray, direction: np.ndarray) -> Tuple[float, float]:
    """(rotation error, translation direction error) in degrees of an estimate against the true relative pose."""
    r_true, t_true = true_relative_pose(scene, edge)
    d = np.asarray(rotation, np.float64).reshape(3, 3).T @ r_true
    angle = np.degrees(np.arccos(np.clip((np.trace(d) - 1.0) / 2.0, -1.0, 1.0)))
    u = np.asarray(direction, np.float64).reshape(3)
    return float(angle), float(np.degrees(np.arccos(np.clip(u @ t_true / np.linalg.norm(u), -1.0, 1.0))))


def good_edges(scene: Dict[str, object]) -> List[Edge]:
    """The window edges that are not planted wrong."""
    return [e for e in window_edges() if e not in (WRONG_ROTATION, WRONG_TRANSLATION)]


# ---- the chain, stage by stage ----


def verifier_stage(scene: Dict[str, object], edges: Optional[Iterable[Edge]] = None) -> Dict[Edge, Dict[str, object]]:
    """oracle/verifier_oracle.verify per edge with the generators' seed ``i << 32 | j``."""
    xy, intr = scene["xy"], scene["intrinsics"]
    return {(i, j): vo.verify(xy[i], xy[j], scene["putative"][(i, j)], tuple(intr[i]), tuple(intr[j]), VERIFY_THRESHOLD_PX, seed=(i << 32) | j)
            for i, j in (scene["edges"] if edges is None else edges)}


def verified_tuples(oracle: Dict[Edge, Dict[str, object]]) -> Dict[Edge, Tuple[Optional[np.ndarray], Optional[np.ndarray], np.ndarray, float]]:
    """The verifier's return tuples (R, t, v_corr_idxs [K, 2], inlier ratio) of the oracle's results."""
    return {e: (r["R"], r["t"], np.asarray(r["v_corr_idxs"], np.int64).reshape(-1, 2), float(r["inlier_ratio"])) for e, r in oracle.items()}


def two_view_pair(scene: Dict[str, object], edge: Edge, verified) -> Dict[str, np.ndarray]:
    """What the two-view bundle adjustment of an edge reads, as tests/two_view_ba_scenes.py lays a pair out: the verified correspondences'
    pixels in the order of the verified rows, the two cameras' intrinsics and the verifier's pose (NaN without one)."""
    i, j = edge
    rot, direction, corr, _ = verified
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    return {"k1": scene["intrinsics"][i], "k2": scene["intrinsics"][j], "uv1": scene["xy"][i, corr[:, 0]], "uv2": scene["xy"][j, corr[:, 1]],
            "R": np.full((3, 3), np.nan) if rot is None else np.asarray(rot, np.float64).reshape(3, 3),
            "t": np.full(3, np.nan) if direction is None else np.asarray(direction, np.float64).reshape(3)}


def after_two_view(verified, ba: Dict[str, object]) -> Dict[str, object]:
    """The rest of ``TwoViewEstimator.run_2view`` on one edge's adjustment result ``ba`` (of tests/two_view_ba_reference.two_view_ba): the two
    inlier-support tests on the verifier's ratio (the reference's hack) and the count after the adjustment; the post-ISP correspondences, pose
    and ``stats[:, 0]``."""
    corr = np.asarray(verified[2], np.int64).reshape(-1, 2)
    valid = np.asarray(ba["valid"], bool)
    ok = support(verified[3] if verified[0] is not None else 0.0, int(valid.sum()))
    posed = bool(np.isfinite(ba["rotation"]).all() and np.isfinite(ba["translation"]).all())
    return {"supported": ok, "valid": valid, "rows": valid & ok, "stats0": int(valid.sum()) if ok else 0, "corr": corr[valid] if ok else corr[:0],
            "R": ba["rotation"] if ok and posed else None, "t": ba["translation"] if ok and posed else None, "ratio": verified[3] if ok else 0.0}


def two_view_stage(scene: Dict[str, object], verified: Dict[Edge, tuple]) -> Dict[Edge, Dict[str, object]]:
    """tests/two_view_ba_reference.two_view_ba (from its own triangulation) and the inlier support, per edge."""
    out = {}
    for e, v in verified.items():
        pair = two_view_pair(scene, e, v)
        ba = ba_ref.two_view_ba(pair["k1"], pair["k2"], pair["uv1"], pair["uv2"], pair["R"], pair["t"], min_verified=MIN_INLIERS)
        out[e] = dict(after_two_view(v, ba), ba=ba)
    return out


def edge_row_arrays(rows: Sequence[Edge], value: Dict[Edge, Optional[np.ndarray]], width: int) -> Tuple[np.ndarray, np.ndarray]:
    """(array [E, width] with NaN rows where an edge has no value, enable [E] uint8) in the scene's row order."""
    arr = np.full((len(rows), width), np.nan)
    for k, e in enumerate(rows):
        if value.get(e) is not None:
            arr[k] = np.asarray(value[e], np.float64).reshape(width)
    return arr, np.isfinite(arr).all(axis=1).astype(np.uint8)


def view_graph_stage(rows: Sequence[Edge], rotation: np.ndarray, enable: np.ndarray) -> Dict[str, object]:
    """tests/view_graph_reference.cycle_filter twice (MEDIAN_EDGE_ERROR, the second pass on what the first kept), then ``largest_component``."""
    pairs = np.asarray(rows, np.int64).reshape(-1, 2)
    passes, on = [], np.asarray(enable, np.uint8)
    for _ in range(2):
        out = vg_ref.cycle_filter(pairs, rotation, on, NUM_IMAGES, vg_ref.MEDIAN_EDGE_ERROR, VIEW_GRAPH_THRESHOLD_DEG)
        out["component"] = vg_ref.largest_component(pairs, out["keep"], NUM_IMAGES)
        passes.append(out)
        on = out["keep"]
    keep = passes[-1]["keep"].astype(bool)
    return {"passes": passes, "keep": keep, "edges": [e for e, k in zip(rows, keep) if k],
            "pruned_edges": [e for e, k in zip(rows, passes[-1]["component"]["pair_keep"]) if k]}


def translation_stage(scene: Dict[str, object], rows: Sequence[Edge], direction: np.ndarray, enable: np.ndarray, corr: Dict[Edge, np.ndarray],
                      edges_in: Iterable[Edge], threshold: float) -> Dict[str, object]:
    """tests/translation_inliers_reference on the arrays ``VerifiedScene.translation_inliers`` assembles: the rows' unit translations, the
    true ``wRi``, the tracks of ``edges_in`` (tests/tracks_reference.py on ``corr``), ``select_tracks`` and ``NUM_DIRECTIONS`` uniform
    directions from numpy's global generator seeded with 0, as ``TranslationAveraging1DSFM`` seeds it."""
    wanted = set(edges_in)
    on = np.array([bool(k) and e in wanted for e, k in zip(rows, enable)], np.uint8)
    live = {e: np.asarray(corr[e], np.int64).reshape(-1, 2) for e in rows if e in wanted and e in corr}
    trk = TR.tracks_reference(live, [CAP] * NUM_IMAGES)
    uv = scene["xy"][trk["image"], trk["kp"]]
    cameras = {c for e, k in zip(rows, on) if k for c in e}
    track_enable, meas_enable, _ = ti_ref.select_tracks(trk["track_off"], trk["image"], cameras)
    np.random.seed(0)
    directions = ti_ref.sample_uniform_directions()[:NUM_DIRECTIONS]
    out = ti_ref.translation_inliers(np.asarray(rows), direction, on, scene["wRi"].reshape(-1, 9), np.ones(NUM_IMAGES, np.uint8), scene["intrinsics"], trk["track_off"],
                                     trk["image"], uv, track_enable, meas_enable, directions, threshold=threshold)
    out.update(enable=on, tracks=trk, track_enable=track_enable, meas_enable=meas_enable, edges=[e for e, k in zip(rows, out["pair_inlier"]) if k])
    return out


def halfway_threshold(pair_weight: np.ndarray) -> Tuple[float, int, float, float]:
    """(threshold, row of the largest mean weight, that weight, the next largest): the threshold lies halfway between the two."""
    w = np.where(np.isfinite(pair_weight), pair_weight, -np.inf)
    order = np.argsort(w)
    return float((w[order[-1]] + w[order[-2]]) / 2), int(order[-1]), float(w[order[-1]]), float(w[order[-2]])


def tracks_stage(corr: Dict[Edge, np.ndarray], edges: Iterable[Edge]) -> Dict[str, object]:
    """tests/tracks_reference.py on the correspondences of ``edges``, and the device scheme's number of rounds."""
    live = {e: np.asarray(corr[e], np.int64).reshape(-1, 2) for e in edges if e in corr}
    out = TR.tracks_reference(live, [CAP] * NUM_IMAGES)
    out["rounds"] = TR.emulate_rounds(live, [CAP] * NUM_IMAGES)[1]
    return out


def camera_table(scene: Dict[str, object]) -> np.ndarray:
    return np.stack([tri.pack_camera(*scene["intrinsics"][i], scene["wRi"][i], scene["centre"][i]) for i in range(NUM_IMAGES)])


def triangulation_options() -> Dict[str, object]:
    return dict(mode=tri.NO_RANSAC, threshold=TRIANGULATION_THRESHOLD_PX)


def triangulation_stage(scene: Dict[str, object], track_off: np.ndarray, image: np.ndarray, kp: np.ndarray) -> Dict[str, np.ndarray]:
    """tests/triangulation_reference.triangulate_tracks with the true cameras on the keypoints' float32 pixels."""
    out = tri.triangulate_tracks(camera_table(scene), track_off, image, scene["xy"][image, kp], **triangulation_options())
    out["uv"] = scene["xy"][image, kp]
    return out


# ---- the ground-truth properties ----


def ghost_measurements(scene: Dict[str, object], image: np.ndarray, kp: np.ndarray) -> int:
    return sum((int(i), int(k)) in scene["ghosts"] for i, k in zip(image, kp))


def track_points(scene: Dict[str, object], track_off: np.ndarray, image: np.ndarray, kp: np.ndarray) -> np.ndarray:
    """Per track the planted point all its keypoints are projections of, -1 where they are not those of one point."""
    out = np.full(len(track_off) - 1, -1, np.int64)
    for t, (a, b) in enumerate(zip(track_off[:-1], track_off[1:])):
        members = {scene["point_of"].get((int(i), int(k)), -1) for i, k in zip(image[a:b], kp[a:b])}
        if len(members) == 1:
            out[t] = members.pop()
    return out


def point_distances(scene: Dict[str, object], track_off: np.ndarray, image: np.ndarray, kp: np.ndarray, point: np.ndarray, exit_code: np.ndarray) -> Dict[str, object]:
    """Of the tracks triangulated with SUCCESS: how many are one planted point's, and their distances from it."""
    which = track_points(scene, track_off, image, kp)
    ok = np.asarray(exit_code) == tri.SUCCESS
    pure = ok & (which >= 0)
    dist = np.linalg.norm(np.asarray(point)[pure] - scene["points"][which[pure]], axis=1)
    return {"success": int(ok.sum()), "pure": int(pure.sum()), "distance": dist, "points": len(set(which[pure].tolist()))}


@functools.lru_cache(maxsize=None)
def restated_chain(seed: int = SEED) -> Dict[str, object]:
    """The whole chain on the CPU, each stage fed the previous restatement's output. Computed once per process."""
    scene = planted_scene(seed)
    rows = scene["rows"]
    oracle = verifier_stage(scene)
    verified = verified_tuples(oracle)
    two_view = two_view_stage(scene, verified)
    rotation, enable = edge_row_arrays(rows, {e: r["R"] for e, r in two_view.items()}, 9)
    direction, _ = edge_row_arrays(rows, {e: r["t"] for e, r in two_view.items()}, 3)
    enable = np.array([two_view[e]["stats0"] > 0 for e in rows], np.uint8)
    view_graph = view_graph_stage(rows, rotation, enable)
    corr = {e: r["corr"] for e, r in two_view.items()}
    probe = translation_stage(scene, rows, direction, enable, corr, view_graph["edges"], ti_ref.OUTLIER_WEIGHT_THRESHOLD)
    threshold, top, first, second = halfway_threshold(probe["pair_weight"])
    translation = translation_stage(scene, rows, direction, enable, corr, view_graph["edges"], threshold)
    tracks = tracks_stage(corr, translation["edges"])
    tracks_all = tracks_stage(corr, rows)
    triangulation = triangulation_stage(scene, tracks["track_off"], tracks["image"], tracks["kp"])
    return {"scene": scene, "oracle": oracle, "verified": verified, "two_view": two_view, "rotation": rotation, "direction": direction, "enable": enable,
            "view_graph": view_graph, "corr": corr, "default_threshold_run": probe, "threshold": threshold, "top_row": top, "top_weights": (first, second),
            "translation": translation, "tracks": tracks, "tracks_all": tracks_all, "triangulation": triangulation}
