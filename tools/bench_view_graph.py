"""Times the device view-graph stage (``ViewGraphEngine.cycle_filter`` with MEDIAN_EDGE_ERROR, then ``largest_component`` on what it kept) by
HIP events against the numpy restatement (tests/view_graph_reference.py) on the same arrays, at three shapes: 46 views matched exhaustively,
the palace pair graph (tests/golden/view_graph_palace_edges.npz) and 1000 views with a window of 50.

    python tools/bench_view_graph.py [--reps 10] [--out profiles/view_graph_bench.txt]

The event interval covers a whole call: every launch, the call's two readbacks (the input flags, the triplet count) and the engine's copy
of the counts; for the component, the flag read after each labelling round. The restatement is vectorised numpy on one core; the reference's
own Python loop (set intersections, three Rot3 per cycle, scipy per cycle) is slower than it. The least bytes are what any implementation
has to move: the pairs and rotations in, the three per-edge outputs back."""

from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from tests import view_graph_reference as ref  # noqa: E402
from tests import view_graph_scenes as scenes  # noqa: E402

HBM_BYTES_PER_S = 6.3e12  # what a streaming copy reaches on an MI355X (8 TB/s on paper)


def shapes():
    out = [("46 views, exhaustive", scenes.scene("k46", scenes.complete(46), seed=46))]
    if scenes.PALACE.exists():
        z = np.load(scenes.PALACE)
        out.append(("palace graph", scenes.scene("palace", z["pair_images"], num_images=int(z["num_images"]), rotation=z["rotation"])))
    out.append(("1000 views, window 50", scenes.scene("w50", scenes.window(1000, 50), seed=50)))
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()

    import networkx  # noqa: F401  (the restatement's component search: its import is not part of the timing)
    import torch

    from gtsfm_amd.runtime.view_graph_engine import ViewGraphEngine

    engine = ViewGraphEngine()
    lines = [f"view-graph bench: cycle filter (MEDIAN_EDGE_ERROR, 7 degrees) and largest component, device {torch.cuda.get_device_name(engine.device)}; "
             f"median of {args.reps} calls after 2 warm-up calls, HIP events around the whole call (readbacks included)"]
    for label, sc in shapes():
        pimg, rot, _ = engine.upload(sc["pair_images"], sc["rotation"])
        n, e = sc["num_images"], len(sc["pair_images"])
        for _ in range(2):
            out = engine.cycle_filter(pimg, rot, None, num_images=n)
            comp = engine.largest_component(pimg, out["keep"], num_images=n)
        keep = out["keep"]
        t_filter = events_ms(torch, lambda: engine.cycle_filter(pimg, rot, None, num_images=n), args.reps)
        t_comp = events_ms(torch, lambda: engine.largest_component(pimg, keep, num_images=n), args.reps)
        t0 = time.perf_counter()
        exp = ref.cycle_filter(sc["pair_images"], sc["rotation"], None, n, ref.MEDIAN_EDGE_ERROR, 7.0)
        cpu_filter = time.perf_counter() - t0
        t0 = time.perf_counter()
        exp_comp = ref.largest_component(sc["pair_images"], exp["keep"], n)
        cpu_comp = time.perf_counter() - t0
        same = (np.array_equal(out["keep"].cpu().numpy(), exp["keep"]) and np.array_equal(out["num_triplets"].cpu().numpy(), exp["num_triplets"])
                and np.array_equal(comp["pair_keep"].cpu().numpy(), exp_comp["pair_keep"]))
        least = e * (8 + 72 + 4 + 8 + 1)
        med_f, med_c = float(np.median(t_filter)), float(np.median(t_comp))
        lines += [f"{label}: {e} edges, {n} views, {out['counts']['triplets']} triplets (at most {out['counts']['max_triplets_per_edge']} per edge), "
                  f"{out['counts']['kept_edges']} edges kept, component of {comp['counts']['nodes']} views / {comp['counts']['edges']} edges; discrete outputs "
                  f"{'equal' if same else 'DIFFER from'} the restatement's",
                  f"  cycle filter: device median {med_f:.3f} ms (min {t_filter.min():.3f}, max {t_filter.max():.3f}); restatement {cpu_filter * 1e3:.1f} ms -> {cpu_filter * 1e3 / med_f:.0f} x",
                  f"  largest component: device median {med_c:.3f} ms (min {t_comp.min():.3f}, max {t_comp.max():.3f}); restatement (networkx) {cpu_comp * 1e3:.1f} ms -> {cpu_comp * 1e3 / med_c:.0f} x",
                  f"  least bytes of the filter: {least} ({least / HBM_BYTES_PER_S * 1e6:.3f} us at {HBM_BYTES_PER_S / 1e12:.1f} TB/s); the call takes "
                  f"{med_f * 1e3 / (least / HBM_BYTES_PER_S * 1e6):.0f} x that (eleven launches and two stream waits)"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
