"""Time MegaLoc (gtsfm_megaloc_forward through MegaLocGlobalDescriptor) at 322 x 322, the plugin's input size.

Legs (one JSON line each on stdout; device-event timing after warm-up, seeded synthetic weights at the published model's size: depth 12, 8448):
  describe   MegaLocGlobalDescriptor.describe_batch, batch 16 (unified_megaloc.yaml) and 64: CPU float batch in, list of (8448,) arrays out (upload
             and download included), and MegaLocEngine.describe on a device-resident batch; images/s; the executed FLOP per image (breakdown
             printed) over the device time as a fraction of the fp32 matrix peak the project measured (156.3 TFLOP/s)
  stages     per-stage device time from the stage-wise entry point's prefixes (patch embedding | block 0 | blocks 1 .. 11 + final LayerNorm | SALAD |
             output projection), batch 16 and 64
  cpu        the torch restatement (tests/megaloc_reference.py) per image on the CPU: the CPU baseline
For the kernels' own time run `--legs kernels` under `rocprofv3 --kernel-trace --stats` (batch 16: one warm-up + three forwards), and
`tools/bench_megaloc.py --summarise <kernel_stats.csv>` turns rocprofv3's table into per-kernel rates.

Usage: python tools/bench_megaloc.py [--legs describe,stages,cpu] [--iters 5] [--height 322 --width 322]
"""

from __future__ import annotations

import argparse
import csv
import json
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from tests import megaloc_reference as mr  # noqa: E402

PEAK_FP32_MATRIX = 156.3e12  # measured (profiles/r01_mfma_peak_microbench.txt)
HBM_PEAK = 8.0e12            # bytes / s, the MI355X data sheet
SIZE, DEPTH, FEAT = 322, 12, 8448


def flop_breakdown(height: int = SIZE, width: int = SIZE, depth: int = DEPTH, feat: int = FEAT) -> dict:
    """Executed FLOP per image (2 per multiply-add), by launch kind. The SALAD products run over all 1 + n rows (the cls row rides along)."""
    n = (height // 14) * (width // 14)
    t = n + 1
    return {
        "patch_embed": 2.0 * n * 588 * 768,
        "qkv": depth * 2.0 * t * 768 * 2304,
        "attention": depth * 2.0 * 2 * t * t * 768,
        "proj": depth * 2.0 * t * 768 * 768,
        "fc1": depth * 2.0 * t * 768 * 3072,
        "fc2": depth * 2.0 * t * 3072 * 768,
        "salad_mlps": 2.0 * t * (768 * 1024 + 512 * 256 + 512 * 64) + 2.0 * (768 * 512 + 512 * 256),
        "salad_aggregation": 2.0 * n * 256 * 64,
        "linear": 2.0 * 16640 * feat,
    }


def _events_ms(fn, iters: int) -> float:
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def summarise(path: str) -> None:
    """rocprofv3's kernel_stats.csv -> total ms, calls, ms per call, kernel (sorted by total time)."""
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    for r in rows:
        ns, calls = float(r["TotalDurationNs"]), int(r["Calls"])
        print(f"{ns / 1e6:10.3f} ms {100 * ns / total:5.1f} % {calls:6d} calls {ns / calls / 1e6:9.4f} ms/call  {r['Name'][:110]}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="describe,stages,cpu")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--summarise")
    ap.add_argument("--height", type=int, default=SIZE, help="image height (a multiple of 14; e.g. 308 x 322 gives 507 tokens = four full query tiles of 128 less five)")
    ap.add_argument("--width", type=int, default=SIZE)
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    legs = args.legs.split(",")
    flops = flop_breakdown(args.height, args.width)
    flop = sum(flops.values())
    print(json.dumps({"leg": "flop_per_image", "height": args.height, "width": args.width, "total": flop, **flops}), flush=True)
    weights = mr.seeded_weights(0, DEPTH, FEAT)
    if "cpu" in legs:
        x = mr.normalise(mr.seeded_images(3, 4, args.height, args.width))
        mr.forward(weights, x[:1])
        t0 = time.perf_counter()
        mr.forward(weights, x)
        dt = (time.perf_counter() - t0) / len(x)
        print(json.dumps({"leg": "cpu", "ms_per_image": dt * 1e3, "images_per_s": 1 / dt, "threads": torch.get_num_threads()}), flush=True)
    if not ({"describe", "stages", "kernels"} & set(legs)):
        return
    from gtsfm_amd.frontend.global_descriptor.megaloc_global_descriptor import MegaLocGlobalDescriptor
    from gtsfm_amd.runtime.megaloc_engine import MegaLocEngine

    plugin = MegaLocGlobalDescriptor()
    engine = plugin._model = MegaLocEngine(weights)
    for b in ([16] if "kernels" in legs else [16, 64]):
        images = mr.normalise(mr.seeded_images(b, b, args.height, args.width))
        dev = images.cuda()
        plugin.describe_batch(images)  # warm-up: workspace, position table, code objects
        torch.cuda.synchronize()
        if "kernels" in legs:
            for _ in range(3):
                engine.describe(dev)
            torch.cuda.synchronize()
            continue
        if "describe" in legs:
            for _ in range(2):
                engine.describe(dev)
            ms_dev = _events_ms(lambda: engine.describe(dev), args.iters)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                plugin.describe_batch(images)
            ms_call = (time.perf_counter() - t0) / args.iters * 1e3
            print(json.dumps({"leg": "describe", "batch": b, "ms_device": ms_dev, "images_per_s_device": b / ms_dev * 1e3, "ms_describe_batch": ms_call,
                              "images_per_s_describe_batch": b / ms_call * 1e3, "tflops_device": flop * b / ms_dev / 1e9,
                              "fraction_of_fp32_matrix_peak": flop * b / (ms_dev * 1e-3) / PEAK_FP32_MATRIX}), flush=True)
        if "stages" in legs:
            prefix = []
            for k in range(4):
                engine.stage(dev, k)
                prefix.append(_events_ms(lambda: engine.stage(dev, k), args.iters))
            prefix.append(_events_ms(lambda: engine.describe(dev), args.iters))
            names = ("patch_embed", "block0", "blocks1..+final_norm", "salad", "linear")
            parts = {nm: prefix[i] - (prefix[i - 1] if i else 0.0) for i, nm in enumerate(names)}
            weight_bytes = 16640 * FEAT * 4
            print(json.dumps({"leg": "stages", "batch": b, "ms": parts, "share": {k: v / prefix[-1] for k, v in parts.items()},
                              "linear_fraction_of_hbm_peak": weight_bytes / (parts["linear"] * 1e-3) / HBM_PEAK}), flush=True)


if __name__ == "__main__":
    main()
