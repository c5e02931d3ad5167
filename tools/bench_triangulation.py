"""Times the device triangulation by HIP events at the tracks stage's headline shape (46 views, ~11 789 tracks), for NO_RANSAC and
for the shipped RANSAC_SAMPLE_UNIFORM setting (threshold 10 px, at most 100 hypotheses), next to the CPU restatement on a sample of
the same tracks, and relates the bytes moved to the HBM rate.

    python tools/bench_triangulation.py [--tracks 11789] [--views 46] [--reps 20] [--out profiles/triangulation_bench.txt]
"""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from tests import triangulation_reference as ref  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak
TRACKS_STAGE_MS = 0.57    # device time of the tracks stage at this shape (profiles/, parent commit)


def make_scene(views: int, tracks: int, seed: int = 0):
    rng = np.random.default_rng(seed)
    table = np.zeros((views, 17))
    for i in range(views):
        th = 2.0 * np.pi * i / views
        eye = np.array([10.0 * np.cos(th), 10.0 * np.sin(th), 0.0]) + rng.normal(0.0, 0.2, 3)
        table[i] = ref.lookat_camera(eye, rng.normal(0.0, 0.2, 3), [0.0, 0.0, 1.0], 1000.0, 648.0, 432.0)
    # the Lund door's track lengths: 2 .. 12, mean about 5.3
    lengths = np.clip(2 + rng.geometric(1.0 / 4.3, tracks) - 1, 2, 12)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    image = np.empty(off[-1], np.int32)
    uv = np.empty((off[-1], 2), np.float32)
    for j, n in enumerate(lengths):
        x = rng.uniform(-2.0, 2.0, 3)
        start = int(rng.integers(views))
        cams = np.sort((start + np.arange(n)) % views)  # neighbouring views see the same point
        for k, i in enumerate(cams):
            u, v, _ = ref.project(table[i], x)
            noise = rng.normal(0.0, 0.5, 2) + (rng.uniform(-60, 60, 2) if rng.random() < 0.05 else 0.0)
            image[off[j] + k], uv[off[j] + k] = i, (u + noise[0], v + noise[1])
    return table, off, image, uv


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=11789)
    ap.add_argument("--views", type=int, default=46)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-sample", type=int, default=300, help="tracks the restatement is timed on (every k-th track)")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()

    import torch

    from gtsfm_amd.runtime.triangulation_engine import TriangulationEngine

    table, off, image, uv = make_scene(args.views, args.tracks)
    t, s = len(off) - 1, len(image)
    engine = TriangulationEngine()
    dev = engine.device
    d_off, d_img, d_uv, d_cam = (torch.from_numpy(a).to(dev) for a in (off, image, uv, table))
    lines = [f"triangulation bench: {args.views} views, {t} tracks, {s} measurements (lengths 2 - 12, mean {s / t:.2f}), device {torch.cuda.get_device_name(dev)}"]
    step = max(1, t // args.cpu_sample)
    sample = list(range(0, t, step))
    for label, opts in (("NO_RANSAC, no threshold", dict(mode=ref.NO_RANSAC)),
                        ("RANSAC_SAMPLE_UNIFORM, threshold 10 px, max 100 hypotheses", dict(mode=ref.RANSAC_SAMPLE_UNIFORM, threshold=10.0, num_hypotheses=100))):
        kw = dict(mode=ref.MODE_NAMES[opts["mode"]], reproj_error_threshold=opts.get("threshold", np.inf), num_hypotheses=opts.get("num_hypotheses", 0))
        for _ in range(3):
            out = engine.triangulate(d_off, d_img, d_uv, d_cam, **kw)
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = engine.triangulate(d_off, d_img, d_uv, d_cam, **kw)
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        times = np.array(times)
        hyps = int(out["stats"][:, 0].sum().item())
        codes = np.bincount(out["exit_code"].cpu().numpy(), minlength=6).tolist()
        t0 = time.perf_counter()
        for j in sample:
            ref.triangulate_track(table, image[off[j]:off[j + 1]], uv[off[j]:off[j + 1]].astype(np.float64), **opts)
        cpu = (time.perf_counter() - t0) * t / len(sample)
        # every hypothesis lane reads its track's measurements and cameras (from L2 after the first touch) and writes 16 bytes; the final pass
        # reads them again a dozen times; compulsory HBM traffic is the arrays once
        compulsory = s * (4 + 8 + 1) + t * (8 + 24 + 8 + 4 + 16) + hyps * 16 * 2 + table.nbytes
        lines += [f"{label}:",
                  f"  device (events, the call's final 8-byte readback included): median {np.median(times):.3f} ms, min {times.min():.3f} ms over {args.reps} calls; "
                  f"{hyps} hypotheses; exit codes {codes}",
                  f"  restatement (numpy, one core, {len(sample)} of the same tracks, scaled to all): {cpu:.1f} s -> {cpu * 1e3 / np.median(times):.0f} x",
                  f"  tracks stage before it: {TRACKS_STAGE_MS} ms -> triangulation costs {np.median(times) / TRACKS_STAGE_MS:.1f} x that",
                  f"  compulsory traffic {compulsory / 1e6:.2f} MB = {compulsory / HBM_BYTES_PER_S * 1e6:.2f} us at {HBM_BYTES_PER_S / 1e12:.0f} TB/s, "
                  f"{100 * compulsory / HBM_BYTES_PER_S / (np.median(times) * 1e-3):.2f} % of the measured time: not bandwidth-bound. One lane per hypothesis / per "
                  f"track runs a serial chain of float64 divisions and square roots over its measurements (latency- and occupancy-bound: {t} track lanes are "
                  f"{t / (256 * 4 * 64):.2f} of one wave per SIMD on 256 CUs), and a wave waits for its longest track."]
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
