"""Times the device two-view bundle adjustment by HIP events at the tracks bench's shape (1000 pairs, about 583 verified correspondences
each, in the verifier's capacity layout), reports the step-count distribution and the time per accepted step, and runs the numpy
restatement on a sample of the same pairs as the CPU baseline (the stage has no earlier device version to time against).

    python tools/bench_two_view_ba.py [--pairs 1000] [--matches 583] [--reps 10] [--cpu-sample 4] [--out profiles/two_view_ba_bench.txt]

The event interval covers the whole call: init, prepare, the triangulation call (which waits for the stream once), the adjustment and the
call's own final 16-byte readback."""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from tests import two_view_ba_reference as ref  # noqa: E402
from tests import two_view_ba_scenes as scenes  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--matches", type=int, default=583)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-sample", type=int, default=4, help="pairs the restatement is timed on")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()

    import torch

    from gtsfm_amd.runtime.two_view_ba_engine import TwoViewBAEngine, TwoViewBAOptions

    rng = np.random.default_rng(0)
    counts = np.clip(rng.normal(args.matches, 0.15 * args.matches, args.pairs).astype(int), 20, None)
    pairs = [scenes.make_pair(1000 + i, int(n)) for i, n in enumerate(counts)]
    layout = scenes.capacity_layout(pairs)
    engine = TwoViewBAEngine()
    dev = engine.device
    launch = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v) for k, v in layout.items() if k != "rows"}
    opt = TwoViewBAOptions()
    for _ in range(2):
        out = engine.run(launch, opt)
    times = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = engine.run(launch, opt)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times = np.array(times)
    stats = out["stats"]
    steps, solves = stats[:, 4], stats[:, 5]
    sample = np.linspace(0, args.pairs - 1, args.cpu_sample).astype(int)
    t0 = time.perf_counter()
    same = 0
    for p in sample:
        pair = pairs[p]
        exp = ref.two_view_ba(pair["k1"], pair["k2"], pair["uv1"], pair["uv2"], pair["R"], pair["t"])
        same += int(exp["stats"][4] == steps[p] and exp["stats"][0] == stats[p, 0])
    cpu = (time.perf_counter() - t0) * args.pairs / len(sample)
    med = float(np.median(times))
    lines = [f"two-view bundle adjustment bench: {args.pairs} pairs, {int(counts.sum())} verified correspondences (mean {counts.mean():.0f}) in "
             f"{len(layout['match_idx'])} match rows (capacity layout), device {torch.cuda.get_device_name(dev)}",
             f"  device (events, whole call): median {med:.3f} ms, min {times.min():.3f} ms, max {times.max():.3f} ms over {args.reps} calls after 2 warm-up calls",
             f"  status counts {np.bincount(stats[:, 0], minlength=5).tolist()} (OK, SKIPPED, NO_INITIAL_POSE, NONE_TRIANGULATED, INDETERMINATE); "
             f"valid {int(stats[:, 3].sum())} of {int(stats[:, 1].sum())} verified",
             f"  accepted steps per pair: min {steps.min()}, median {int(np.median(steps))}, mean {steps.mean():.1f}, 95 % {int(np.percentile(steps, 95))}, max {steps.max()}; "
             f"linear solves tried: mean {solves.mean():.1f}, max {solves.max()}",
             f"  {med * 1e3 / max(1, int(steps.sum())):.3f} us per accepted step of one pair (whole call over all steps); the call lasts as long as its slowest "
             f"workgroups: {med * 1e3 / max(1, int(steps.max())):.1f} us per step of the longest pair",
             f"  restatement (numpy, one core, {len(sample)} of the same pairs, scaled to all; {same} of them with the device's status and step count): "
             f"{cpu:.0f} s -> {cpu * 1e3 / med:.0f} x"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
