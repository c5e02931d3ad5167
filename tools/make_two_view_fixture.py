"""Records the 60-digit arbiter's minimum (tests/two_view_ba_arbiter.py) for the small pairs of tests/two_view_ba_scenes.py into
tests/golden/two_view_ba_arbiter.json, and into profiles/two_view_ba_arbiter.txt how far gtsam's stopping rule, as the restatement
applies it, leaves the robust cost above that minimum.

    python tools/make_two_view_fixture.py
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
from mpmath import mp

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from tests import two_view_ba_arbiter as arb  # noqa: E402
from tests import two_view_ba_reference as ref  # noqa: E402
from tests import two_view_ba_scenes as scenes  # noqa: E402

PAIRS = {"n15": (102, 15), "n16": (103, 16)}  # batch_pairs()' seeds: the pairs of at most 16 points


def record_door_pair() -> None:
    """The Lund door pair of the GPU scene (cameras 0 and 1 of tests/golden/triangulation_lund_door.npz, their two-image tracks, the pose
    perturbed): the restatement's discrete outputs and the tolerance the device is held to on it -- 8 x the larger of its reversed-order
    and longdouble sensitivities (rotation, direction, points relative, cost / max(cost, 1)) -> tests/golden/two_view_ba_door_pair.json."""
    from tests.test_two_view_ba_gpu import FACTOR, differences

    door = dict(np.load(REPO / "tests" / "golden" / "triangulation_lund_door.npz"))
    pair = scenes.door_pair(door, 0, 1)
    args = (pair["k1"], pair["k2"], pair["uv1"], pair["uv2"], pair["R"], pair["t"])
    exp = ref.two_view_ba(*args)
    n = int(exp["triangulated"].sum())
    back = ref.two_view_ba(*args, order=np.concatenate([[0], np.arange(n - 1, 0, -1)]))
    wide = ref.two_view_ba(*args, dtype=np.longdouble)
    tol = FACTOR * np.maximum(differences(exp, back), differences(exp, wide))
    rec = {"cameras": [0, 1], "verified": len(pair["uv1"]), "stats": [int(v) for v in exp["stats"][:6]], "non_decisive": bool(exp["non_decisive"]),
           "cost": [float(v) for v in exp["cost"]], "rotation": exp["rotation"].tolist(), "translation": exp["translation"].tolist(),
           "valid": int(exp["valid"].sum()), "factor": FACTOR, "tolerance": {"rotation": float(tol[0]), "direction": float(tol[1]), "points_rel": float(tol[2]),
                                                                             "cost_over_max_cost_1": float(tol[3])}}
    (REPO / "tests" / "golden" / "two_view_ba_door_pair.json").write_text(json.dumps(rec, indent=1) + "\n")
    print("door pair:", rec["stats"], rec["tolerance"], flush=True)


def main() -> None:
    record, lines = {}, ["two-view bundle adjustment: the 60-digit arbiter's minimum of the stated cost against the restatement (UNPINNED towards gtsam).",
                         "pair: points; arbiter minimum, its largest gradient entry, Gauss-Newton iterations; restatement cost at the 1e-5 stopping rule (steps) and its",
                         "relative excess over the minimum; restatement continued with both tolerances at 0 in float64 (steps) and its relative excess"]
    for name, (seed, n) in PAIRS.items():
        pair = scenes.make_pair(seed, n)
        args = (pair["k1"], pair["k2"], pair["uv1"], pair["uv2"], pair["R"], pair["t"])
        stop = ref.two_view_ba(*args)
        full = ref.two_view_ba(*args, abs_tol=0.0, rel_tol=0.0, max_iterations=2000)
        start = ref.two_view_ba(*args, max_iterations=0)
        problem = arb.Problem(*args, start["points"][start["triangulated"]])
        out = problem.minimise()
        minimum = float(out["cost"])
        record[name] = {"seed": seed, "points": n, "minimum": mp.nstr(out["cost"], 40), "gradient_max": float(out["gradient_max"]), "iterations": out["iterations"],
                        "rotation": out["rotation"], "translation": out["translation"]}
        lines.append(f"  {name}: {n}; {mp.nstr(out['cost'], 20)}, {float(out['gradient_max']):.1e}, {out['iterations']}; {stop['cost'][1]:.15g} ({stop['stats'][4]}), "
                     f"{(stop['cost'][1] - minimum) / minimum:.3e}; {full['cost'][1]:.15g} ({full['stats'][4]}), {(full['cost'][1] - minimum) / minimum:.3e}")
        print(lines[-1], flush=True)
    record_door_pair()
    (REPO / "tests" / "golden" / "two_view_ba_arbiter.json").write_text(json.dumps(record, indent=1) + "\n")
    (REPO / "profiles" / "two_view_ba_arbiter.txt").write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
