"""Times the device's 1DSfM outlier rejection (``TranslationInliersEngine.inliers``: world directions, adjacency, MFAS over 2000 projection
directions, the per-edge aggregate) by HIP events against the numpy restatement (tests/translation_inliers_reference.py) on the same arrays,
at three shapes with 12 landmark measurements per camera: 46 views matched exhaustively, the palace pair graph
(tests/golden/view_graph_palace_edges.npz) and 1000 views with a window of 50.

    python tools/bench_translation_inliers.py [--reps 10] [--directions 2000] [--restated 2] [--out profiles/translation_inliers_bench.txt]

The event interval covers a whole call: every launch, the call's one stream wait (the refusal flags and the node count) and the engine's copy
of the counts. The restatement is a Python loop of N steps per direction on one core, so it is timed on the first ``--restated`` directions
only and scaled to all of them (stated in the output); the device's ``position`` rows of exactly those directions are compared with it byte
for byte. gtsam's own MFAS cannot be timed here (gtsam cannot be imported); the reference scatters it over 16 Dask tasks."""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from tests import translation_inliers_reference as ref  # noqa: E402
from tests import translation_inliers_scenes as scenes  # noqa: E402

PALACE = REPO / "tests" / "golden" / "view_graph_palace_edges.npz"


def small_rotations(rng, n: int, degrees: float = 10.0) -> np.ndarray:
    """Rotations within ``degrees`` of the identity: every landmark placed in front stays in front of every camera."""
    axis = scenes.random_units(rng, n)
    angle = np.deg2rad(rng.uniform(-degrees, degrees, size=n))
    k = np.zeros((n, 3, 3))
    k[:, 0, 1], k[:, 0, 2], k[:, 1, 0], k[:, 1, 2], k[:, 2, 0], k[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    r = np.eye(3)[None] + np.sin(angle)[:, None, None] * k + (1 - np.cos(angle))[:, None, None] * (k @ k)
    return r.reshape(n, 9)


def synthetic(name: str, pairs, n: int, seed: int, directions: int, per_camera: int = 12, outliers: float = 0.1):
    """True geometry with 2 % direction noise; ``outliers`` of the pair rows get a random direction. 4 n landmarks seen by 3 cameras each
    (a camera and two of its neighbours in the pair graph): 12 measurements per camera on average."""
    rng = np.random.default_rng(seed)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    centre = np.column_stack([rng.uniform(-20, 20, size=(n, 2)), rng.uniform(-2, 2, size=n)])
    rot = small_rotations(rng, n)
    nbrs = [[] for _ in range(n)]
    for a, b in pairs.tolist():
        nbrs[a].append(b), nbrs[b].append(a)
    tracks, points = [], []
    for j in range(per_camera * n // 3):
        c = j % n
        if len(nbrs[c]) < 2:
            continue
        tracks.append(sorted([c, *rng.choice(nbrs[c], 2, replace=False).tolist()]))
        points.append(centre[c] + np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(30, 50)]))
    k = np.tile([800.0, 800.0, 512.0, 384.0], (n, 1))
    uv = []
    for cams, p in zip(tracks, points):
        for c in cams:
            ray = rot[c].reshape(3, 3).T @ (p - centre[c])
            uv.append((k[c, 0] * ray[0] / ray[2] + k[c, 2], k[c, 1] * ray[1] / ray[2] + k[c, 3]))
    t = np.einsum("eji,ej->ei", rot[pairs[:, 1]].reshape(-1, 3, 3), centre[pairs[:, 0]] - centre[pairs[:, 1]])
    t = ref.unit(ref.unit(t) + rng.normal(scale=0.02, size=t.shape))
    bad = rng.random(len(pairs)) < outliers
    t[bad] = scenes.random_units(rng, int(bad.sum()))
    np.random.seed(0)
    return scenes.scene(name, [tuple(p) for p in pairs.tolist()], t, n, ref.sample_uniform_directions(directions), rotation=rot, tracks=tracks, uv=uv, intrinsics=k), bad


def shapes(directions: int):
    out = [("46 views, exhaustive", *synthetic("k46", scenes.window(46, 46), 46, 46, directions))]
    if PALACE.exists():
        z = np.load(PALACE)
        out.append(("palace graph", *synthetic("palace", z["pair_images"], int(z["num_images"]), 7, directions)))
    out.append(("1000 views, window 50", *synthetic("w50", scenes.window(1000, 50), 1000, 50, directions)))
    return out


def events_ms(torch, fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return np.array(times)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--directions", type=int, default=ref.MAX_PROJECTION_DIRECTIONS)
    ap.add_argument("--restated", type=int, default=2, help="directions the restatement is timed and compared on (0: none)")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()

    import torch

    from gtsfm_amd.runtime.translation_engine import TranslationInliersEngine

    engine = TranslationInliersEngine()
    lines = [f"1DSfM outlier rejection bench: {args.directions} projection directions, threshold {ref.OUTLIER_WEIGHT_THRESHOLD}, device {torch.cuda.get_device_name(engine.device)}; "
             f"median of {args.reps} calls after 2 warm-up calls, HIP events around the whole call (its stream wait and the counts readback included)"]
    for label, sc, bad in shapes(args.directions):
        dev = engine.upload(sc["pair_images"], sc["pair_direction"], None, sc["rotation"], sc["rotation_valid"], sc["intrinsics"], sc["track_off"], sc["image"], sc["uv"],
                            sc["track_enable"], None, sc["directions"])
        for _ in range(2):
            out = engine.inliers(*dev)
        t_dev = events_ms(torch, lambda: engine.inliers(*dev), args.reps)
        c = out["counts"]
        inlier = out["pair_inlier"].cpu().numpy().astype(bool)
        med = float(np.median(t_dev))
        steps = c["nodes"] * args.directions
        lines += [f"{label}: {len(sc['pair_images'])} pair rows ({int(bad.sum())} with a random direction), {len(sc['image'])} track measurements of {len(sc['track_off']) - 1} "
                  f"landmarks, {c['nodes']} nodes (state in {out['tier']}); {c['inlier_pairs']} inlier pairs ({int((~inlier & bad).sum())} of the random ones rejected, "
                  f"{int((~inlier & ~bad).sum())} others), {c['inlier_measurements']} inlier measurements, {c['inlier_cameras']} inlier cameras",
                  f"  device median {med:.3f} ms (min {t_dev.min():.3f}, max {t_dev.max():.3f}): {steps} greedy steps, {med * 1e6 / max(steps, 1):.1f} ns per step over all workgroups"]
        if args.restated > 0:
            k = min(args.restated, args.directions)
            w_pair, pv = ref.world_pair_directions(sc["pair_images"], sc["pair_direction"], None, sc["rotation"], sc["rotation_valid"])
            w_meas, mv = ref.world_landmark_directions(sc["track_off"], sc["image"], sc["uv"], sc["track_enable"], None, sc["rotation"], sc["rotation_valid"], sc["intrinsics"])
            g = ref.build_edges(sc["pair_images"], w_pair, pv, sc["track_off"], sc["image"], w_meas, mv, sc["num_images"])
            nodes = sc["num_images"] + len(sc["track_off"]) - 1
            t0 = time.perf_counter()
            positions = [ref.mfas_positions(g["key1"], g["key2"], g["m"], d, nodes) for d in sc["directions"][:k]]
            for d, p in zip(sc["directions"][:k], positions):
                ref.outlier_weights(g["key1"], g["key2"], g["m"], d, p)
            cpu = (time.perf_counter() - t0) / k
            sub = engine.upload(sc["pair_images"], sc["pair_direction"], None, sc["rotation"], sc["rotation_valid"], sc["intrinsics"], sc["track_off"], sc["image"], sc["uv"],
                                sc["track_enable"], None, sc["directions"][:k])
            got = engine.inliers(*sub, want_position=True)["position"].cpu().numpy()
            same = got.tobytes() == np.stack(positions).tobytes()
            lines.append(f"  restatement (numpy, one core): {cpu * 1e3:.1f} ms per direction measured on {k} directions -> {cpu * args.directions:.1f} s for {args.directions} "
                         f"(scaled, not run) -> {cpu * args.directions * 1e3 / med:.0f} x; the device's orderings of those {k} directions are "
                         f"{'byte-equal to' if same else 'DIFFERENT from'} the restatement's")
    lines.append("gtsam's MFAS itself cannot be timed here (gtsam cannot be imported); the reference spreads these directions over 16 Dask tasks.")
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
