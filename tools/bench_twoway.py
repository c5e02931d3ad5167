"""Time the two-way matcher (gtsfm_twoway_match) at 5000 x 5000 keypoints per image.

Legs (device-event timing after warm-up; one JSON line per leg on stdout):
  plugin      TwoWayMatcher.match per call (host arrays in, sorted (K, 2) out: upload, launch, download and sort included), SIFT-like
              uint8 D = 128, ratio 0.8
  batched     TwoWayEngine.match_raw on a device-resident table, 32 pairs per launch: D = 128 uint8 (SIFT-like) and D = 256 float32
              (SuperPoint-like, unit norm), ratio 0.8; reports the whole call and the pairs/s
FLOP count 2 * N1 * N2 * D per pair; fraction of the 157.3 TFLOP/s fp32 matrix peak. For the fused kernel's own time run this under
`rocprofv3 --kernel-trace --stats` (tw_tile_kernel).

Usage: python tools/bench_twoway.py [--iters 10] [--n 5000] [--pairs 32] [--out profiles/twoway_bench.json]
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

PEAK_FP32_MATRIX = 157.3e12


def _events_ms(fn, iters: int) -> float:
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def _sift_like(rng, n, d):
    return np.clip(rng.gamma(1.0, 20.0, size=(n, d)), 0, 200).astype(np.uint8)


def bench_plugin(n: int, iters: int, warmup: int):
    from gtsfm_amd.frontend.matcher.twoway_matcher import TwoWayMatcher

    rng = np.random.default_rng(0)
    a, b = _sift_like(rng, n, 128), _sift_like(rng, n, 128)
    b[: n // 2] = np.clip(a[: n // 2].astype(np.int32) + rng.integers(-3, 4, size=(n // 2, 128)), 0, 255).astype(np.uint8)
    m = TwoWayMatcher(ratio_test_threshold=0.8)
    for _ in range(warmup):
        out = m.match(None, None, a, b, (480, 640, 3), (480, 640, 3))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ms = _events_ms(lambda: m.match(None, None, a, b, (480, 640, 3), (480, 640, 3)), iters)
    wall = (time.perf_counter() - t0) / iters * 1e3
    flop = 2.0 * n * n * 128
    return {"leg": "plugin", "n": n, "d": 128, "dtype": "uint8", "ms_per_pair": round(ms, 4), "wall_ms_per_pair": round(wall, 4),
            "pairs_per_s": round(1e3 / wall, 2), "tflops": round(flop / ms * 1e-9, 2), "matches": int(len(out))}


def bench_batched(n: int, d: int, dtype: str, npairs: int, iters: int, warmup: int):
    from gtsfm_amd.runtime.twoway_engine import EUCLIDEAN, TwoWayEngine

    rng = np.random.default_rng(d)
    n_img = npairs + 1
    if dtype == "uint8":
        host = _sift_like(rng, n_img * n, d)
    else:
        host = rng.standard_normal((n_img * n, d)).astype(np.float32)
        host /= np.linalg.norm(host, axis=1, keepdims=True)
    eng = TwoWayEngine()
    table = torch.from_numpy(host).to(eng.device)
    pairs = [(i * n, n, (i + 1) * n, n) for i in range(npairs)]
    for _ in range(warmup):
        m0, _ = eng.match_raw(table, d, pairs, EUCLIDEAN, 0.8)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ms = _events_ms(lambda: eng.match_raw(table, d, pairs, EUCLIDEAN, 0.8), iters)
    wall = (time.perf_counter() - t0) / iters * 1e3
    flop = 2.0 * n * n * d * npairs
    return {"leg": "batched", "n": n, "d": d, "dtype": dtype, "pairs": npairs, "ms_per_launch": round(ms, 4), "wall_ms_per_launch": round(wall, 4),
            "ms_per_pair": round(ms / npairs, 4), "pairs_per_s": round(npairs * 1e3 / wall, 1), "tflops": round(flop / ms * 1e-9, 2),
            "fraction_of_fp32_matrix_peak": round(flop / (ms * 1e-3) / PEAK_FP32_MATRIX, 3),
            "kept_rows_first_pair": int((m0[:n] >= 0).sum().item())}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from gtsfm_amd.csrc import build

    build.build(verbose=False)
    rows = [bench_plugin(args.n, args.iters, args.warmup)]
    rows.append(bench_batched(args.n, 128, "uint8", args.pairs, args.iters, args.warmup))
    rows.append(bench_batched(args.n, 256, "float32", args.pairs, args.iters, args.warmup))
    rows.append(bench_batched(args.n, 128, "uint8", 1, args.iters, args.warmup))
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
