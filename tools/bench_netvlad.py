"""Time NetVLAD (gtsfm_netvlad_forward through NetVLADGlobalDescriptor) and similarity retrieval (gtsfm_retrieval_topk).

Legs (one JSON line each on stdout; device-event timing after warm-up, seeded synthetic weights and images):
  describe   NetVLADGlobalDescriptor.describe_batch at 760 x 1013 (the loaders' max_resolution), batch 4 (ImagePairsGenerator's default) and
             32: CPU float batch in, list of (4096,) arrays out (upload and download included); images/s and the backbone's
             algorithmic FLOP rate as a fraction of the 157.3 TFLOP/s fp32 matrix peak (whole call: an upper bound on time)
  retrieval  RetrievalEngine.topk at N = 1000 and 10000 unit descriptors of 4096, k = 10, min_score 0.3 (device-resident input), with and
             without the similarity output (blocksize 50); the FLOP of the row strips actually launched over the whole call's time
  cpu        the torch restatement (tests/netvlad_reference.py) per image on the CPU at 760 x 1013: the CPU baseline
For the kernels' own time run `--legs kernels` under `rocprofv3 --kernel-trace --stats` (a batch of 4, three forwards).

Usage: python tools/bench_netvlad.py [--legs describe,retrieval,cpu] [--iters 5]
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from tests import netvlad_reference as nr  # noqa: E402

PEAK_FP32_MATRIX = 157.3e12
H, W = 760, 1013


def backbone_flop(h: int, w: int) -> float:
    """2 * H_l * W_l * 9 * Cin * Cout summed over conv1_1 .. conv5_3 (floor pooling)."""
    total = 0.0
    for i, (cin, cout) in enumerate(nr.VGG16_CONVS):
        total += 2.0 * h * w * 9 * cin * cout
        if i in nr.POOL_AFTER:
            h, w = h // 2, w // 2
    return total


def launched_product_flop(n: int, d: int, blocksize: int = 1) -> float:
    """FLOP of the row strips gtsfm_retrieval_topk launches: strip r covers rows [1024 r, 1024 r + 1024) against the columns from the
    start of the block (of ``blocksize`` columns; 1 without the similarity output) holding its first row, rounded down to a multiple of 4."""
    total = 0.0
    for r0 in range(0, n, 1024):
        col0 = ((r0 // blocksize) * blocksize) & ~3
        total += 2.0 * min(1024, n - r0) * (n - col0) * d
    return total


def _events_ms(fn, iters: int) -> float:
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="describe,retrieval,cpu")
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    legs = args.legs.split(",")
    weights = nr.seeded_weights(0)
    flop = backbone_flop(H, W)
    if "describe" in legs or "kernels" in legs:
        from gtsfm_amd.frontend.global_descriptor.netvlad_global_descriptor import NetVLADGlobalDescriptor
        from gtsfm_amd.runtime.netvlad_engine import NetVLADEngine

        plugin = NetVLADGlobalDescriptor()
        plugin._model = NetVLADEngine(weights)
        for b in ([4] if "kernels" in legs else [4, 32]):
            images = nr.seeded_images(b, b, H, W)
            plugin.describe_batch(images)
            if "kernels" in legs:
                for _ in range(3):
                    plugin.describe_batch(images)
                torch.cuda.synchronize()
                continue
            ms = _events_ms(lambda: plugin.describe_batch(images), args.iters)
            print(json.dumps({"leg": "describe", "height": H, "width": W, "batch": b, "ms_per_batch": round(ms, 3),
                              "images_per_s": round(1000.0 * b / ms, 2), "backbone_gflop_per_image": round(flop / 1e9, 1),
                              "backbone_frac_of_fp32_peak_whole_call": round(flop * b / (ms * 1e-3) / PEAK_FP32_MATRIX, 3)}), flush=True)
    if "retrieval" in legs:
        from gtsfm_amd.runtime.retrieval_engine import RetrievalEngine

        eng = RetrievalEngine()
        for n in (1000, 10000):
            x = torch.randn((n, 4096), generator=torch.Generator().manual_seed(n))
            d = torch.nn.functional.normalize(x, dim=1).cuda()
            eng.topk(d, 10, 0.3, with_sim=True)
            ms_sim = _events_ms(lambda: eng.topk(d, 10, 0.3, with_sim=True), args.iters)
            ms = _events_ms(lambda: eng.topk(d, 10, 0.3), args.iters)
            flop, flop_sim = launched_product_flop(n, 4096), launched_product_flop(n, 4096, 50)
            print(json.dumps({"leg": "retrieval", "n": n, "d": 4096, "k": 10, "min_score": 0.3, "ms": round(ms, 3), "ms_with_sim_out": round(ms_sim, 3),
                              "product_gflop_launched": round(flop / 1e9, 1), "product_gflop_launched_with_sim_out": round(flop_sim / 1e9, 1),
                              "launched_flop_frac_of_fp32_peak_whole_call": round(flop / (ms * 1e-3) / PEAK_FP32_MATRIX, 3)}), flush=True)
    if "cpu" in legs:
        images = nr.seeded_images(1, 1, H, W)
        with torch.no_grad():
            t0 = time.perf_counter()
            nr.forward(weights, images)
            s = time.perf_counter() - t0
        print(json.dumps({"leg": "cpu_baseline", "what": "torch restatement of the reference's NetVLAD on the CPU", "threads": torch.get_num_threads(),
                          "height": H, "width": W, "s_per_image": round(s, 3)}), flush=True)


if __name__ == "__main__":
    main()
