"""Times the device's rotation averaging (``RotationAveragingEngine.average``: validity pass, adjacency, component, chordal initialisation and
the Riemannian trust region, one workgroup per problem) by HIP events against the numpy restatement (tests/rotation_averaging_reference.py) on
the same arrays, at three shapes: 46 views matched exhaustively, the palace pair graph (tests/golden/view_graph_palace_edges.npz) and 1000
views with a window of 50 (48 725 edges). 2 degrees of noise per axis, 2 % of the edges a random rotation, weights U[15, 600)^2.

    python tools/bench_rotation_averaging.py [--reps 5] [--restated 1] [--batch 64] [--out profiles/rotation_averaging_bench.txt]

The event interval covers a whole call: every launch, the call's one stream wait (the refusal flags) and the engine's copy of the counters.
A second timing with ``max_outer=0`` stops after the chordal initialisation; the difference divided by the Hessian applications is the time
of one truncated-CG step (a pass over the lists, two or three trees, their barriers). ``--batch`` solves that many copies of the first shape
in one call: one workgroup each, so the call fills that many CUs. gtsam's Shonan cannot be timed here (gtsam cannot be imported)."""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from tests import rotation_averaging_reference as ref  # noqa: E402
from tests import rotation_averaging_scenes as scenes  # noqa: E402


def window(n: int, w: int):
    return [(i, j) for i in range(n) for j in range(i + 1, min(i + w + 1, n))]


def shapes():
    def make(name, n, pairs, seed):
        rng = np.random.default_rng(seed)
        bad = np.flatnonzero(rng.random(len(pairs)) < 0.02).tolist()
        return scenes.planted(name, n, pairs, seed, outliers=bad), len(bad)

    out = [("46 views, exhaustive", *make("k46", 46, window(46, 46), 46))]
    if scenes.PALACE.exists():
        z = np.load(scenes.PALACE)
        out.append(("palace graph", *make("palace", int(z["num_images"]), [tuple(p) for p in z["pair_images"].tolist()], 7)))
    out.append(("1000 views, window 50", *make("w50", 1000, window(1000, 50), 50)))
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--restated", type=int, default=1, help="1: time the numpy restatement too and compare its bytes with the device's")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()

    import torch

    from gtsfm_amd.runtime.rotation_averaging_engine import COUNTER_FIELDS, RotationAveragingEngine

    engine = RotationAveragingEngine()
    lines = [f"rotation averaging bench: defaults {ref.DEFAULTS}, device {torch.cuda.get_device_name(engine.device)}; median of {args.reps} calls after 1 warm-up call, "
             "HIP events around the whole call (its stream wait and the counters readback included)"]
    first = None
    for label, sc, bad in shapes():
        dev = engine.upload(sc["pair_images"], sc["rotation"], sc["weight"])
        first = first or (sc, dev)
        run = lambda **kw: engine.average(*dev[:3], None, num_images=sc["num_images"], **kw)  # noqa: E731
        out = run()
        t_all, t_init = events_ms(torch, run, args.reps), events_ms(torch, lambda: run(max_outer=0), args.reps)
        c = dict(zip(COUNTER_FIELDS, (int(x) for x in out["counters"][0])))
        med, med_init = float(np.median(t_all)), float(np.median(t_init))
        lines += [f"{label}: {len(sc['pair_images'])} rows ({bad} random rotations), {sc['num_images']} images; {out['status'][0]}, {c['outer_iterations']} outer iterations, "
                  f"{c['accepted_steps']} accepted, {c['hessian_applications']} Hessian applications, {c['chordal_cg_steps']} chordal CG steps; cost {out['costs'][0][1]:.6g} -> "
                  f"{out['costs'][0][2]:.6g}, |g|_inf {out['costs'][0][3]:.3e}",
                  f"  device median {med:.3f} ms (min {t_all.min():.3f}, max {t_all.max():.3f}); up to the chordal initialisation {med_init:.3f} ms "
                  f"({med_init * 1e3 / max(c['chordal_cg_steps'], 1):.1f} us per chordal CG step, adjacency and component included); trust region "
                  f"{(med - med_init) * 1e3 / max(c['hessian_applications'], 1):.1f} us per Hessian application"]
        if args.restated:
            t0 = time.perf_counter()
            want = scenes.solve(sc)
            cpu = time.perf_counter() - t0
            same = out["wRi"][0].cpu().numpy().tobytes() == want["wRi"].tobytes() and out["counters"][0].tolist() == [want["counters"][k] for k in ref.COUNTER_FIELDS]
            lines.append(f"  restatement (numpy, one core): {cpu * 1e3:.0f} ms -> {cpu * 1e3 / med:.1f} x the device's call; the device's rotations and counters are "
                         f"{'byte-equal to' if same else 'DIFFERENT from'} the restatement's")
    if args.batch > 1 and first is not None:
        sc, _ = first
        e = len(sc["pair_images"])
        dev = engine.upload(np.tile(sc["pair_images"], (args.batch, 1)), np.tile(sc["rotation"], (args.batch, 1)), np.tile(sc["weight"], args.batch), None,
                            np.arange(args.batch + 1) * e)
        run = lambda: engine.average(*dev[:3], None, num_images=sc["num_images"], problem_row_off=dev[4])  # noqa: E731
        run()
        t = events_ms(torch, run, args.reps)
        lines.append(f"batch: {args.batch} copies of the first shape in one call, one workgroup each: median {float(np.median(t)):.3f} ms "
                     f"({float(np.median(t)) / args.batch:.4f} ms per problem)")
    lines.append("gtsam's ShonanAveraging3 itself cannot be timed here (gtsam cannot be imported).")
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
