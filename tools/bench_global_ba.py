"""Times the device's global bundle adjustment (``GlobalBAEngine.adjust``: validity pass, lists, component, Levenberg-Marquardt with the
matrix-free Schur complement, the filter; one workgroup per problem) by HIP events against the numpy restatement
(tests/global_ba_reference.py) on the same arrays, at three shapes: a synthetic scene with the view and track counts of the tracks stage's headline shape (46 views, 11 789 tracks of 2 .. 12
neighbouring views with the Lund door's length distribution, which gives 59 424 measurements here against that shape's 59 173), the cameras of the palace pair graph (tests/golden/view_graph_palace_edges.npz) and 1000 views with tracks inside a
window of 50, the last two with 12 measurements per camera (tracks of 4 views); 0.5 px of noise, a start perturbed by 0.01 rad and 0.05 units.

    python tools/bench_global_ba.py [--reps 10] [--restated 1] [--out profiles/global_ba_bench.txt]

The event interval covers a whole call: every launch, the call's one stream wait (the refusal flags) and the engine's copy of the counters.
One workgroup runs one problem from start to end: spreading one problem over several workgroups is out of scope here, as for the two
averaging kernels, so a call's time grows with measurements x CG iterations on ONE compute unit. gtsam's optimiser cannot be timed here
(gtsam cannot be imported)."""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from tests import global_ba_reference as ref  # noqa: E402
from tests import global_ba_scenes as scenes  # noqa: E402

PALACE = REPO / "tests" / "golden" / "view_graph_palace_edges.npz"


def line_of_cameras(n: int, seed: int):
    """Cameras 0.2 units apart along x, looking down z at a slab ten units away."""
    rng = np.random.default_rng(seed)
    centre = np.stack([0.2 * np.arange(n), rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)], 1)
    rot = np.stack([scenes.look_at(centre[i], centre[i] + [rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 10.0], rng.uniform(-5.0, 5.0)) for i in range(n)])
    intr = np.stack([np.full(n, 1000.0), np.full(n, 1010.0), np.full(n, 648.0), np.full(n, 432.0)], 1)
    return intr, rot, centre


def make(name: str, n: int, views, seed: int):
    intr, rot, centre = line_of_cameras(n, seed)
    rng = np.random.default_rng(seed + 1)
    points = np.stack([centre[[int(np.mean(v)) for v in views], 0] + rng.uniform(-2.0, 2.0, len(views)), rng.uniform(-2.0, 2.0, len(views)), rng.uniform(8.5, 11.5, len(views))], 1)
    return scenes.scene(name, intr, rot, centre, points, views, seed, noise=0.5)


def shapes():
    rng = np.random.default_rng(46)
    lengths = np.clip(2 + rng.geometric(1.0 / 4.3, 11789) - 1, 2, 12)  # the Lund door's track lengths, as tools/bench_triangulation.py
    starts = rng.integers(0, 46, len(lengths))
    out = [("46 views and 11 789 tracks, synthetic (the tracks stage's headline counts)", make("k46", 46, [np.sort((s + np.arange(k)) % 46).tolist() for s, k in zip(starts, lengths)], 46))]

    def windowed(n, window, seed):
        r = np.random.default_rng(seed)
        return [np.sort(s + r.choice(min(window, n), 4, replace=False)).tolist() for s in r.integers(0, max(n - window, 1), 3 * n)]

    if PALACE.exists():
        n = int(np.load(PALACE)["num_images"])
        out.append(("palace graph's cameras", make("palace", n, windowed(n, 20, 7), 7)))
    out.append(("1000 views, window 50", make("w50", 1000, windowed(1000, 50, 50), 50)))
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


def report(lines, out, shown=[0]):  # noqa: B006 - the count of lines already printed
    """Prints the new lines and rewrites ``out``: a long run shows what it has so far."""
    print("\n".join(lines[shown[0]:]), flush=True)
    shown[0] = len(lines)
    if out:
        Path(out).write_text("\n".join(lines) + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--restated", type=int, default=1, help="1: time the numpy restatement too and compare its bytes with the device's")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()

    import torch

    from gtsfm_amd.runtime.global_ba_engine import COUNTER_FIELDS, GlobalBAEngine

    engine = GlobalBAEngine()
    lines = [f"global bundle adjustment bench: defaults {ref.DEFAULTS}, device {torch.cuda.get_device_name(engine.device)}; median of {args.reps} calls after 1 warm-up call, "
             "HIP events around the whole call (its stream wait and the counters readback included); one workgroup per problem"]
    for label, sc in shapes():
        dev = engine.upload(*scenes.arrays_of(sc))
        run = lambda: engine.adjust(*dev)  # noqa: E731
        out = run()
        t = events_ms(torch, run, args.reps)
        c = dict(zip(COUNTER_FIELDS, (int(x) for x in out["counters"][0])))
        med = float(np.median(t))
        lines += [f"{label}: {len(sc['cameras'])} cameras, {len(sc['point'])} tracks, {len(sc['image'])} measurements; {out['status'][0]}, {c['accepted_steps']} accepted steps, "
                  f"{c['solves_tried']} linear solves, {c['cg_iterations']} CG iterations; cost {out['costs'][0][0]:.6g} -> {out['costs'][0][1]:.6g}, |g|_inf {out['costs'][0][2]:.3e}, "
                  f"{int(out['track_valid'].sum())} tracks kept",
                  f"  device median {med:.3f} ms (min {t.min():.3f}, max {t.max():.3f}); {med * 1e3 / max(c['cg_iterations'] + 4 * c['solves_tried'], 1):.1f} us per pass pair "
                  "(a CG iteration, or one of the about four passes around a solve)"]
        if args.restated:
            t0 = time.perf_counter()
            want = scenes.solve(sc)
            cpu = time.perf_counter() - t0
            same = (out["point"].cpu().numpy().tobytes() == want["point"].tobytes() and out["cameras"][0].cpu().numpy().tobytes() == want["cameras"].tobytes()
                    and out["counters"][0].tolist() == [want["counters"][k] for k in ref.COUNTER_FIELDS])
            lines.append(f"  restatement (numpy, one core): {cpu * 1e3:.0f} ms -> {cpu * 1e3 / med:.1f} x the device's call; the device's cameras, points and counters are "
                         f"{'byte-equal to' if same else 'DIFFERENT from'} the restatement's")
        report(lines, args.out)
    lines.append("gtsam's Levenberg-Marquardt itself cannot be timed here (gtsam cannot be imported).")
    report(lines, args.out)


if __name__ == "__main__":
    main()
