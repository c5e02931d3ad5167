"""Time the device track builder (gtsfm_tracks_from_matches) at the headline scene's shape: 46 views x 5000 keypoints x 1000 pairs.

The scene is synthetic: latent 3-D points, each seen by a view with probability 0.2 at a keypoint slot of its own; a pair keeps every
shared point with probability 0.8 and adds 10 wrong rows; the match lists lie on the device in the verifier's capacity layout (5000 rows
per pair, a count, an inlier mask that drops 10 % of the rows), as `FrontEndPipeline.verify` leaves them. Timed: the device time of
`TracksEngine.tracks_from_verified` by HIP events after warm-up (the call reads one 4-byte flag per round, so host latency is inside).
Reported next to it: the rounds, the bytes the kernels have to move at least (every round reads the 9 bytes of each row it owns plus two
labels per active row and rewrites two labels per node; the assembly passes over the ~50 bytes of node state once) against the HBM rate,
and the CPU restatement (tests/tracks_reference.py, a Python union-find) on the same rows. There is no pass / fail rate.

Usage: python tools/bench_tracks.py [--iters 10] [--views 46] [--keypoints 5000] [--pairs 1000] [--out profiles/tracks_bench.txt]
"""

from __future__ import annotations

import argparse
import itertools
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

HBM_BYTES_PER_S = 8.0e12


def build_scene(views: int, cap: int, num_pairs: int, seed: int = 0):
    rng = np.random.default_rng(seed)
    points = 4 * cap
    slot = np.full((views, points), -1, dtype=np.int64)
    for i in range(views):
        seen = np.flatnonzero(rng.random(points) < 0.2)[:cap]
        slot[i, seen] = rng.permutation(cap)[: len(seen)]
    all_pairs = list(itertools.combinations(range(views), 2))
    pairs = [all_pairs[p] for p in sorted(rng.permutation(len(all_pairs))[:num_pairs])]
    idx = np.zeros((len(pairs) * cap, 2), dtype=np.int32)
    count = np.zeros(len(pairs), dtype=np.int32)
    mask = (rng.random(len(pairs) * cap) >= 0.1).astype(np.uint8)
    surviving = {}
    for p, (i1, i2) in enumerate(pairs):
        both = np.flatnonzero((slot[i1] >= 0) & (slot[i2] >= 0))
        both = both[rng.random(len(both)) < 0.8]
        rows = np.concatenate([np.stack([slot[i1, both], slot[i2, both]], 1), rng.integers(0, cap, size=(10, 2))])[:cap]
        rows = rows[rng.permutation(len(rows))]
        idx[p * cap : p * cap + len(rows)] = rows
        count[p] = len(rows)
        surviving[(i1, i2)] = rows[mask[p * cap : p * cap + len(rows)].astype(bool)]
    return pairs, idx, count, mask, surviving


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=46)
    ap.add_argument("--keypoints", type=int, default=5000)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from gtsfm_amd.csrc import build

    build.build(verbose=False)
    from gtsfm_amd.runtime.tracks_engine import TracksEngine
    from tests import tracks_reference as TR

    views, cap = args.views, args.keypoints
    pairs, idx, count, mask, surviving = build_scene(views, cap, args.pairs)
    engine = TracksEngine()
    dev = engine.device
    stats = torch.ones((len(pairs), 8), dtype=torch.int32, device=dev)
    launch = {"match_idx": torch.from_numpy(idx).to(dev), "match_off": (np.arange(len(pairs) + 1, dtype=np.int64) * cap).tolist(),
              "match_count": torch.from_numpy(count).to(dev), "mask": torch.from_numpy(mask).to(dev), "stats": stats, "pairs": pairs}
    xy = torch.rand((views * cap, 2), dtype=torch.float32, device=dev)
    for _ in range(args.warmup):
        out = engine.tracks_from_verified([launch], cap, views, kp_xy=xy)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    start.record()
    for _ in range(args.iters):
        out = engine.tracks_from_verified([launch], cap, views, kp_xy=xy)
    stop.record()
    stop.synchronize()
    wall_ms = (time.perf_counter() - t0) / args.iters * 1e3
    ms = start.elapsed_time(stop) / args.iters
    c = out["counts"]
    rows_owned, active, nodes = len(pairs) * cap, int(sum(len(m) for m in surviving.values())), views * cap
    least_bytes = c["rounds"] * (9 * rows_owned + 8 * active + 8 * nodes) + 50 * nodes + 20 * c["measurements"]

    t0 = time.perf_counter()
    ref = TR.tracks_reference(surviving)
    cpu_s = time.perf_counter() - t0
    same = all(np.array_equal(out[k].cpu().numpy(), ref[k]) for k in ("track_off", "image", "kp"))
    row = {"views": views, "keypoints": cap, "pairs": len(pairs), "rows_owned": rows_owned, "active_rows": active, "device_ms": round(ms, 3),
           "wall_ms": round(wall_ms, 3), **c, "least_bytes": least_bytes, "fraction_of_hbm_rate": round(least_bytes / (ms * 1e-3) / HBM_BYTES_PER_S, 4),
           "cpu_restatement_s": round(cpu_s, 2), "equals_cpu_restatement": bool(same)}
    print(json.dumps(row), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
