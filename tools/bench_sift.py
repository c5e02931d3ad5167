"""Time the SIFT detector-descriptor (gtsfm_sift_detect_and_describe through SiftEngine).

Images: the two Lund-door photographs of tests/golden (1936 x 1296 gray uint8, the size the reference's SIFT configs run at) and the
760 x 1013 top-left crop of the first (the loaders' max_resolution). Legs (one JSON line each on stdout; device-event timing after warm-up):
  detect   SiftEngine.detect_batch, max_keypoints 5000, at full size with batch 1 and 8 and at 760 x 1013 with batch 1: numpy arrays in,
           numpy keypoints / descriptors out (upload, the count read-back and the download included); images/s
  stages   device time up to each stage of gtsfm_sift_stage for one image (0 pyramid, 1 candidates, 2 keypoints, 3 oriented and sorted)
           and of the whole call; the differences are the stages' own times. For the pyramid: the bytes its kernels have to move
           (every blur pass reads and writes its image once, the DoG reads six images and writes five per octave, plus the stage's
           device-to-device copy of the result) and that traffic over the stage's time as a share of the 8 TB/s HBM rate
For the kernels' own time run `--legs kernels` under `rocprofv3 --kernel-trace --stats` in a run of its own, the program after `--`
(full size, batch 1, four calls; no counters).

Usage: python tools/bench_sift.py [--legs detect,stages] [--iters 5]
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import sift_agreement  # noqa: E402
import sift_reference as S  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
GOLDEN = REPO / "tests" / "golden"


def pyramid_bytes(h: int, w: int) -> float:
    total = h * w + 4.0 * 4 * h * w  # the upsampling reads uint8 and writes the doubled float image
    for o, (oh, ow) in enumerate(S.octave_shapes(h, w)):
        p = 4.0 * oh * ow
        blurs = 6 if o == 0 else 5
        total += blurs * 2 * 2 * p  # row pass and column pass, each one read and one write
        if o:
            total += 2 * p  # the base: one strided read of a quarter of the previous octave's image 3, one write
        total += 11 * p  # DoG: six images read, five written
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
    ap.add_argument("--legs", default="detect,stages")
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    legs = args.legs.split(",")
    from gtsfm_amd.runtime.sift_engine import SiftEngine

    engine = SiftEngine()
    full = [sift_agreement.load_lund_door(GOLDEN, i)[0] for i in (0, 1)]
    mid = np.ascontiguousarray(full[0][:1013, :760])
    eight = [np.ascontiguousarray(a) for im in full for a in (im, im[::-1], im[:, ::-1], im[::-1, ::-1])]
    if "kernels" in legs:
        for _ in range(4):
            engine.detect_batch(full[:1], 5000)
        torch.cuda.synchronize()
    if "detect" in legs:
        for name, images in (("full", full[:1]), ("full", eight), ("mid", [mid])):
            out = engine.detect_batch(images, 5000)
            ms = _events_ms(lambda: engine.detect_batch(images, 5000), args.iters)
            print(json.dumps({"leg": "detect", "image": name, "height": images[0].shape[0], "width": images[0].shape[1], "batch": len(images),
                              "max_keypoints": 5000, "keypoints": [len(o[0]) for o in out], "ms_per_batch": round(ms, 3),
                              "images_per_s": round(1000.0 * len(images) / ms, 2)}), flush=True)
    if "stages" in legs:
        for name, image in (("full", full[0]), ("mid", mid)):
            h, w = image.shape
            upto = {}
            for s in (0, 1, 2, 3):
                engine.stage(image, s)
                upto[f"ms_up_to_stage_{s}"] = round(_events_ms(lambda s=s: engine.stage(image, s, sync=False), args.iters), 3)
            engine.detect(image, 5000)
            upto["ms_whole_call"] = round(_events_ms(lambda: engine.detect(image, 5000), args.iters), 3)
            moved = pyramid_bytes(h, w) + 2 * 4.0 * int(engine._lib.gtsfm_sift_pyramid_floats(h, w))
            print(json.dumps({"leg": "stages", "image": name, "height": h, "width": w, "octaves": S.num_octaves(h, w), **upto,
                              "pyramid_stage_mbytes": round(moved / 1e6, 1),
                              "pyramid_stage_share_of_hbm_rate": round(moved / (upto["ms_up_to_stage_0"] * 1e-3) / HBM_BYTES_PER_S, 3),
                              "what": "each figure includes the upload and that stage's output allocation / copy; differences are the stages' own times"}),
                  flush=True)


if __name__ == "__main__":
    main()
