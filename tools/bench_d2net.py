"""Time the D2-Net detector-descriptor (gtsfm_d2net_forward through D2NetEngine) and its dilated convolution.

Legs (one JSON line each on stdout; device-event timing after warm-up, seeded synthetic weights and images):
  detect   D2NetEngine.detect_batch at 760 x 1013 (the loaders' max_resolution), batch 1 and 8, max_keypoints 5000: uint8 HWC arrays in,
           numpy keypoints / scores / descriptors out (upload, the count read-back and the download included); images/s and the ten
           convolutions' algorithmic FLOP rate as a fraction of the 157.3 TFLOP/s fp32 matrix peak (whole call: an upper bound on time)
  stages   device time up to each stage of gtsfm_d2net_stage at batch 1 (0 relu(conv1_1), 1 relu(conv3_3), 2 dense map, 3 sorted
           candidates) and of the whole forward; the differences are the stages' own times (each includes one device-to-device copy)
  conv     the dilated kernel (gtsfm_conv3x3_dil2_f32) next to the undilated one (gtsfm_conv3x3_f32) on the same 512 -> 512 problem at
           189 x 252 (the dense map of a 760 x 1013 image), in the same process: ms and fraction of the fp32 matrix peak
  cpu      the torch restatement (tests/d2net_reference.py) per image on the CPU at 760 x 1013: the CPU baseline
For the kernels' own time run `--legs kernels` under `rocprofv3 --kernel-trace --stats` (batch 1, three forwards; no counters).

Usage: python tools/bench_d2net.py [--legs detect,stages,conv,cpu] [--iters 5]
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

from tests import d2net_reference as dr  # noqa: E402

PEAK_FP32_MATRIX = 157.3e12
H, W = 760, 1013


def conv_flop(h: int, w: int) -> dict:
    """2 * H_l * W_l * 9 * Cin * Cout per convolution (floor pooling, the stride-1 average pool in front of the dilated layers)."""
    out = {"plain": 0.0, "dilated": 0.0}
    for i, (cin, cout) in enumerate(dr.CONVS):
        if i == dr.FIRST_DILATED:
            h, w = h - 1, w - 1
        out["dilated" if i >= dr.FIRST_DILATED else "plain"] += 2.0 * h * w * 9 * cin * cout
        if i in dr.POOL_AFTER:
            h, w = h // 2, w // 2
    return out


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
    ap.add_argument("--legs", default="detect,stages,conv,cpu")
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    legs = args.legs.split(",")
    weights = dr.seeded_weights(0)
    flop = conv_flop(H, W)
    total = flop["plain"] + flop["dilated"]
    engine = None
    if {"detect", "stages", "kernels"} & set(legs):
        from gtsfm_amd.runtime.d2net_engine import D2NetEngine

        engine = D2NetEngine(weights)
    if "kernels" in legs:
        images = [dr.seeded_image(1, H, W)]
        for _ in range(4):
            engine.detect_batch(images, 5000)
        torch.cuda.synchronize()
    if "detect" in legs:
        for b in (1, 8):
            images = [dr.seeded_image(100 + i, H, W) for i in range(b)]
            out = engine.detect_batch(images, 5000)
            ms = _events_ms(lambda: engine.detect_batch(images, 5000), args.iters)
            print(json.dumps({"leg": "detect", "height": H, "width": W, "batch": b, "max_keypoints": 5000, "keypoints": [len(o[0]) for o in out],
                              "ms_per_batch": round(ms, 3), "images_per_s": round(1000.0 * b / ms, 2), "conv_gflop_per_image": round(total / 1e9, 1),
                              "dilated_share_of_flop": round(flop["dilated"] / total, 3),
                              "conv_frac_of_fp32_peak_whole_call": round(total * b / (ms * 1e-3) / PEAK_FP32_MATRIX, 3)}), flush=True)
    if "stages" in legs:
        images = [dr.seeded_image(100, H, W)]
        upto = {}
        for s in (0, 1, 2, 3):
            engine.stage(images, s)
            upto[f"ms_up_to_stage_{s}"] = round(_events_ms(lambda s=s: engine.stage(images, s), args.iters), 3)
        engine.detect_batch(images, 5000)
        upto["ms_whole_forward"] = round(_events_ms(lambda: engine.detect_batch(images, 5000), args.iters), 3)
        print(json.dumps({"leg": "stages", "height": H, "width": W, "batch": 1, **upto,
                          "what": "each figure includes the upload and that stage's output allocation / copy; differences are the stages' own times"}), flush=True)
    if "conv" in legs:
        from gtsfm_amd.runtime import lib as L

        lib = L.load()
        h2, w2, c = H // 4 - 1, W // 4 - 1, 512
        gen = torch.Generator().manual_seed(0)
        x = torch.randn((1, h2, w2, c), generator=gen).cuda()
        wt = (torch.randn((c, c, 3, 3), generator=gen) * float(np.sqrt(2.0 / (9 * c)))).numpy()
        packed = np.empty(lib.gtsfm_packed_conv3x3_floats(c, c), dtype=np.float32)
        L.check(lib.gtsfm_pack_conv3x3(wt.ctypes.data, c, c, packed.ctypes.data), "gtsfm_pack_conv3x3")
        wp, bias, y = torch.from_numpy(packed).cuda(), torch.zeros(c, device="cuda"), torch.empty((1, h2, w2, c), device="cuda")
        st = L.current_stream_handle()
        plain = lambda: L.check(lib.gtsfm_conv3x3_f32(x.data_ptr(), c, 0, y.data_ptr(), c, 0, wp.data_ptr(), bias.data_ptr(), 1, h2, w2, c, c, 1, 0, st), "c")  # noqa: E731
        dil = lambda: L.check(lib.gtsfm_conv3x3_dil2_f32(x.data_ptr(), c, 0, y.data_ptr(), c, 0, wp.data_ptr(), bias.data_ptr(), 1, h2, w2, c, c, 1, st), "d")  # noqa: E731
        fl = 2.0 * h2 * w2 * 9 * c * c
        row = {"leg": "conv", "problem": f"512 -> 512 at {h2} x {w2}, batch 1", "gflop": round(fl / 1e9, 1)}
        for rep in (1, 2):
            for name, fn in (("dilation_1", plain), ("dilation_2", dil)):
                for _ in range(3):
                    fn()
                ms = _events_ms(fn, 20)
                row[f"{name}_ms_run{rep}"] = round(ms, 4)
                row[f"{name}_frac_of_fp32_peak_run{rep}"] = round(fl / (ms * 1e-3) / PEAK_FP32_MATRIX, 3)
        print(json.dumps(row), flush=True)
    if "cpu" in legs:
        image = dr.seeded_image(100, H, W)
        t0 = time.perf_counter()
        out = dr.forward(weights, image, max_keypoints=5000)
        s = time.perf_counter() - t0
        print(json.dumps({"leg": "cpu_baseline", "what": "torch restatement of the reference's D2-Net on the CPU", "threads": torch.get_num_threads(),
                          "height": H, "width": W, "keypoints": len(out["keypoints"]), "s_per_image": round(s, 3)}), flush=True)


if __name__ == "__main__":
    main()
