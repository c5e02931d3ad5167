"""Time a classical scene (SIFT or D2-Net + TwoWayMatcher + Ransac) through the device-resident generator and through the per-call plugins.

Scene: 16 overlapping views of 760 x 1013 (``synthetic_overlapping_views``), their 120 exhaustive pairs, 5000 keypoints per image at the most,
ratio 0.8, verification at 1 px. One JSON line per leg on stdout (and in ``--out``):
  resident          BatchedTwoWayCorrespondenceGenerator.generate_correspondences (detect_table -> match_table_device -> numpy results)
  resident_verify   ... generate_correspondences_and_verify (the verifier reads the ordered match lists where they lie)
  per_call          the baseline: one detect_and_describe per image, one TwoWayMatcher.match and one Ransac.verify per pair, host arrays between
                    them; the time of the three stages is reported separately (``per_call`` without verification = detect + match)
  order_kernel      gtsfm_twoway_order_matches next to gtsfm_twoway_match on 32 pairs of 5000 x 5000 (uint8 D = 128 and float32 D = 512),
                    device events, per pair
Scene legs are host-clock times around work that ends in a device synchronise (they include the host's share, which is the point); every leg
runs ``--warmup`` times before ``--iters`` timed repeats, and the minimum and the median are reported. D2-Net runs seeded weights
(``tests/d2net_reference.seeded_weights``): the arithmetic does not depend on the values.

Usage: python tools/bench_classical_scene.py [--detectors sift,d2net] [--views 16] [--iters 3] [--warmup 1] [--out profiles/classical_scene_bench.txt]
"""

from __future__ import annotations

import argparse
import itertools
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

H, W = 760, 1013


def _timed(fn, warmup: int, iters: int):
    for _ in range(max(warmup, 1)):
        out = fn()
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, round(min(times), 2), round(statistics.median(times), 2)


def _events_ms(fn, iters: int) -> float:
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def bench_scene(name: str, views: int, height: int, width: int, max_keypoints: int, warmup: int, iters: int, workdir: Path):
    from gtsfm_amd.common.calibration import PinholeIntrinsics
    from gtsfm_amd.common.image import Image
    from gtsfm_amd.frontend.correspondence_generator.batched_twoway_correspondence_generator import BatchedTwoWayCorrespondenceGenerator
    from gtsfm_amd.frontend.detector_descriptor import D2NetDetDesc, SIFTDetectorDescriptor
    from gtsfm_amd.frontend.matcher.twoway_matcher import TwoWayMatcher
    from gtsfm_amd.frontend.verifier.ransac import Ransac
    from gtsfm_amd.utils import synthetic

    if name == "sift":
        det = SIFTDetectorDescriptor(max_keypoints=max_keypoints)
    else:
        from tests import d2net_reference as dr

        torch.save({"model": dr.seeded_weights(0)}, str(workdir / "d2_tf.pth"))
        det = D2NetDetDesc(max_keypoints=max_keypoints, model_path=workdir / "d2_tf.pth")
    images = [Image(value_array=v) for v in synthetic.synthetic_overlapping_views(views, height, width, seed=9)]
    edges = list(itertools.combinations(range(views), 2))
    cams = [PinholeIntrinsics(900.0 + 5 * i, width / 2.0, height / 2.0) for i in range(views)]
    matcher, verifier = TwoWayMatcher(ratio_test_threshold=0.8), Ransac(True, 1.0)
    gen = BatchedTwoWayCorrespondenceGenerator(matcher, det)
    base = {"detector": name, "views": views, "pairs": len(edges), "height": height, "width": width, "max_keypoints": max_keypoints}
    rows = []

    (kps, putative), lo, med = _timed(lambda: gen.generate_correspondences(None, images, edges), warmup, iters)
    rows.append({**base, "leg": "resident", "ms_min": lo, "ms_median": med, "keypoints": int(sum(len(k) for k in kps)),
                 "putative": int(sum(len(m) for m in putative.values()))})
    (_, _, verified), lo, med = _timed(lambda: gen.generate_correspondences_and_verify(None, images, edges, cams, verifier), warmup, iters)
    rows.append({**base, "leg": "resident_verify", "ms_min": lo, "ms_median": med, "models": int(sum(v[0] is not None for v in verified.values())),
                 "verified": int(sum(len(v[2]) for v in verified.values()))})

    shapes = [im.value_array.shape for im in images]
    feats, d_lo, d_med = _timed(lambda: [det.detect_and_describe(im) for im in images], warmup, iters)
    match_all = lambda: {(i, j): matcher.match(feats[i][0], feats[j][0], feats[i][1], feats[j][1], shapes[i], shapes[j]) for i, j in edges}  # noqa: E731
    per_pair, m_lo, m_med = _timed(match_all, warmup, iters)
    verify_all = lambda: {(i, j): Ransac(True, 1.0, seed=(i << 32) | j).verify(feats[i][0], feats[j][0], per_pair[(i, j)], cams[i], cams[j])  # noqa: E731
                          for i, j in edges}
    per_ver, v_lo, v_med = _timed(verify_all, warmup, iters)
    same = all(np.array_equal(per_pair[e], putative[e]) for e in edges) and all(np.array_equal(per_ver[e][2], verified[e][2]) for e in edges)
    rows.append({**base, "leg": "per_call", "detect_ms_min": d_lo, "match_ms_min": m_lo, "verify_ms_min": v_lo, "ms_min": round(d_lo + m_lo, 2),
                 "ms_median": round(d_med + m_med, 2), "with_verify_ms_min": round(d_lo + m_lo + v_lo, 2),
                 "with_verify_ms_median": round(d_med + m_med + v_med, 2), "results_equal_the_resident_path": bool(same)})
    return rows


def bench_order(n: int, dim: int, dtype: str, npairs: int, warmup: int, iters: int):
    from gtsfm_amd.runtime.twoway_engine import EUCLIDEAN, TwoWayEngine

    rng = np.random.default_rng(dim)
    n_img = npairs + 1
    if dtype == "uint8":
        host = np.clip(rng.gamma(1.0, 20.0, size=(n_img * n, dim)), 0, 200).astype(np.uint8)
        host[n:] = np.where(rng.random((npairs * n, 1)) < 0.5, host[:-n], host[n:])  # half of each image's rows reappear in the next: matches and ties
    else:
        host = rng.standard_normal((n_img * n, dim)).astype(np.float32)
        host /= np.linalg.norm(host, axis=1, keepdims=True)
        host[n:] = np.where(rng.random((npairs * n, 1)) < 0.5, host[:-n], host[n:])
    eng = TwoWayEngine()
    table = torch.from_numpy(host).to(eng.device)
    pairs = [(i * n, n, (i + 1) * n, n) for i in range(npairs)]
    blk = torch.arange(npairs + 1, dtype=torch.int64, device=eng.device) * n
    idx = torch.empty((npairs * n, 2), dtype=torch.int32, device=eng.device)
    count = torch.zeros(npairs, dtype=torch.int32, device=eng.device)
    for _ in range(max(warmup, 1)):
        m0, d0 = eng.match_raw(table, dim, pairs, EUCLIDEAN, 0.8)
        eng.order_matches(m0, d0, blk, npairs, idx, count)
    match_ms = _events_ms(lambda: eng.match_raw(table, dim, pairs, EUCLIDEAN, 0.8), iters)
    order_ms = _events_ms(lambda: eng.order_matches(m0, d0, blk, npairs, idx, count), iters * 5)
    one_ms = _events_ms(lambda: eng.order_matches(m0, d0, blk, 1, idx, count), iters * 5)
    return {"leg": "order_kernel", "n": n, "d": dim, "dtype": dtype, "pairs": npairs, "kept_rows_per_pair": round(float(count.sum().item()) / npairs, 1),
            "match_ms_per_pair": round(match_ms / npairs, 4), "order_ms_per_pair": round(order_ms / npairs, 4),
            "order_share_of_match": round(order_ms / match_ms, 4), "order_ms_single_pair_launch": round(one_ms, 4)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--detectors", type=str, default="sift,d2net")
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--max-keypoints", type=int, default=5000)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from gtsfm_amd.csrc import build

    build.build(verbose=False)
    if not torch.cuda.is_available():
        raise SystemExit("bench_classical_scene.py measures on a GPU; none is visible")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    emit(bench_order(args.max_keypoints, 128, "uint8", 32, args.warmup, args.iters))
    emit(bench_order(args.max_keypoints, 512, "float32", 32, args.warmup, args.iters))
    with tempfile.TemporaryDirectory() as tmp:
        for name in [d for d in args.detectors.split(",") if d]:
            if name not in ("sift", "d2net"):
                raise SystemExit(f"unknown detector {name!r}")
            for row in bench_scene(name, args.views, args.height, args.width, args.max_keypoints, args.warmup, args.iters, Path(tmp)):
                emit(row)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
