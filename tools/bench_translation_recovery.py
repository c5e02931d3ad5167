"""Times the device's translation recovery (``TranslationRecoveryEngine.recover``: validity pass, adjacency, component, the linear
initialisation and the Gauss-Newton trust region, one workgroup per problem) by HIP events against the numpy restatement
(tests/translation_recovery_reference.py) on the same arrays, at three shapes: 46 views matched exhaustively, the palace pair graph
(tests/golden/view_graph_palace_edges.npz) and 1000 views with a window of 50 (48 725 pair rows), each with 12 landmark measurements per
camera (landmarks seen by 4 cameras), 0.01 rad of noise and 2 % of the rows a random direction.

    python tools/bench_translation_recovery.py [--reps 5] [--restated 1] [--batch 64] [--out profiles/translation_recovery_bench.txt]

The event interval covers a whole call: every launch, the call's one stream wait (the refusal flags) and the engine's copy of the counters.
A second timing with ``max_outer=0`` stops after the initialisation; the difference divided by the Hessian applications is the time of one
truncated-CG step (a pass over the lists, two trees, their barriers). ``--batch`` solves that many copies of the first shape in one call:
one workgroup each, so the call fills that many CUs. gtsam's TranslationRecovery cannot be timed here (gtsam cannot be imported)."""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from tests import translation_recovery_reference as ref  # noqa: E402
from tests import translation_recovery_scenes as scenes  # noqa: E402

PALACE = REPO / "tests" / "golden" / "view_graph_palace_edges.npz"
MEASUREMENTS_PER_CAMERA, VIEWS_PER_LANDMARK = 12, 4


def window(n: int, w: int):
    return [(i, j) for i in range(n) for j in range(i + 1, min(i + w + 1, n))]


def shapes():
    def make(name, n, pairs, seed):
        pairs = sorted({(min(a, b), max(a, b)) for a, b in pairs if a != b})
        n_land = n * MEASUREMENTS_PER_CAMERA // VIEWS_PER_LANDMARK
        wrong = int(0.02 * (len(pairs) + n_land * VIEWS_PER_LANDMARK))
        return scenes.planted(name, n, n_land, seed, per_land=VIEWS_PER_LANDMARK, pairs=pairs, noise=0.01, wrong=wrong), wrong

    out = [("46 views, exhaustive", *make("k46", 46, window(46, 46), 46))]
    if PALACE.exists():
        z = np.load(PALACE)
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

    from gtsfm_amd.runtime.translation_recovery_engine import COUNTER_FIELDS, TranslationRecoveryEngine

    engine = TranslationRecoveryEngine()
    lines = [f"translation recovery bench: defaults {ref.DEFAULTS}, device {torch.cuda.get_device_name(engine.device)}; median of {args.reps} calls after 1 warm-up call, "
             "HIP events around the whole call (its stream wait and the counters readback included)"]
    first = None
    for label, sc, wrong in shapes():
        dev = engine.upload(*scenes.arrays_of(sc))
        first = first or sc
        run = lambda **kw: engine.recover(*dev, num_images=sc["num_images"], **kw)  # noqa: E731
        out = run()
        t_all, t_init = events_ms(torch, run, args.reps), events_ms(torch, lambda: run(max_outer=0), args.reps)
        c = dict(zip(COUNTER_FIELDS, (int(x) for x in out["counters"][0])))
        med, med_init = float(np.median(t_all)), float(np.median(t_init))
        lines += [f"{label}: {len(sc['pair_images'])} pair rows + {len(sc['image'])} measurements ({wrong} random directions), {sc['num_images']} cameras + "
                  f"{len(sc['track_off']) - 1} landmarks; {out['status'][0]}, {c['outer_iterations']} outer iterations, {c['accepted_steps']} accepted, "
                  f"{c['hessian_applications']} Hessian applications, {c['init_cg_steps']} init CG steps; cost {out['costs'][0][0]:.6g} -> {out['costs'][0][1]:.6g}, "
                  f"|g|_inf {out['costs'][0][2]:.3e}",
                  f"  device median {med:.3f} ms (min {t_all.min():.3f}, max {t_all.max():.3f}); up to the initialisation {med_init:.3f} ms "
                  f"({med_init * 1e3 / max(c['init_cg_steps'], 1):.1f} us per init CG step, adjacency, component and the first cost pass included); trust region "
                  f"{(med - med_init) * 1e3 / max(c['hessian_applications'], 1):.1f} us per Hessian application"]
        if args.restated:
            t0 = time.perf_counter()
            want = scenes.solve(sc)
            cpu = time.perf_counter() - t0
            same = out["translation"][0].cpu().numpy().tobytes() == want["translation"].tobytes() and out["counters"][0].tolist() == [want["counters"][k] for k in ref.COUNTER_FIELDS]
            lines.append(f"  restatement (numpy, one core): {cpu * 1e3:.0f} ms -> {cpu * 1e3 / med:.1f} x the device's call; the device's positions and counters are "
                         f"{'byte-equal to' if same else 'DIFFERENT from'} the restatement's")
    if args.batch > 1 and first is not None:
        sc = first
        arrays, off, n, _ = scenes.batch_of([sc] * args.batch)
        dev = engine.upload(*arrays)
        run = lambda: engine.recover(*dev, num_images=n, problem_row_off=off)  # noqa: E731
        run()
        t = events_ms(torch, run, args.reps)
        lines.append(f"batch: {args.batch} copies of the first shape in one call, one workgroup each: median {float(np.median(t)):.3f} ms "
                     f"({float(np.median(t)) / args.batch:.4f} ms per problem)")
    lines.append("gtsam's TranslationRecovery itself cannot be timed here (gtsam cannot be imported).")
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
