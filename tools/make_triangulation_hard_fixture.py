"""Writes tests/golden/triangulation_hard_scenes.npz (data only) and the CPU part of profiles/triangulation_hard_scenes.txt.

    python tools/make_triangulation_hard_fixture.py

Candidates: ``tests.triangulation_scenes.hard_scenes()``. Per candidate track the high-precision arbiter
(tests/triangulation_arbiter.py) and the float64 port of the device's design (``solver="jacobi"``, 8 steps) are run.

Exclusion rule: a candidate is kept only if the arbiter has an answer for it (every solve has a finite minimiser), it is decisive,
and the port agrees with the arbiter on it: discrete outputs equal and cost(x) - cost(minimiser) <= 1e-5 max(1, cost(minimiser)).
A rung of which more than 10 % of the candidates fail the port lies outside the design's domain: it is dropped WHOLE and named with
its measured gap. Nothing is thinned until it passes.

Per family the fixture holds the kept scene, the arbiter's outputs and the tolerance for whatever is compared with them: 8 x the
largest port-to-arbiter difference over the family (relative point distance, average error in px), both test-side and computed on the
CPU; the factor, kept from the reversal recipe, covers contraction and the device's sqrt / division. Floor: 8 x 2^-52 (relative; for
the average error times the family's largest one): the arbiter's answer is itself rounded to float64.
"""

from __future__ import annotations

import json
import multiprocessing
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from tests import triangulation_arbiter as arbiter  # noqa: E402
from tests import triangulation_reference as ref  # noqa: E402
from tests import triangulation_scenes as scenes  # noqa: E402

FACTOR = 8.0
RUNG_FAILURE_SHARE = 0.10
EPS = 2.0**-52
_STATE = {}
DEVICE_MARKER = "\nDevice (MI355X), tests/test_triangulation_gpu.py::test_hard_fixture_against_arbiter:\n"


def _arbiter_row(args):
    name, j = args
    s = _STATE[name]
    a, b = int(s["track_off"][j]), int(s["track_off"][j + 1])
    return arbiter.triangulate_track(s["cameras"], s["image"][a:b], s["uv"][a:b], **s["options"])


def run_arbiter(name: str, scene, pool):
    rows = pool.map(_arbiter_row, [(name, j) for j in range(len(scene["rung"]))], chunksize=1)
    off = scene["track_off"]
    out = {"point": np.array([r["point"] for r in rows]).reshape(-1, 3), "avg_error": np.array([r["avg_error"] for r in rows]),
           "exit_code": np.array([r["exit_code"] for r in rows], np.int32), "inlier_mask": np.zeros(int(off[-1]), np.uint8),
           "stats": np.array([r["stats"] for r in rows], np.int32).reshape(-1, 4), "cost_min": np.array([r["cost_min"] for r in rows]),
           "non_decisive": [r["non_decisive"] for r in rows], "no_minimiser": np.array([r["no_minimiser"] for r in rows], bool)}
    for j, r in enumerate(rows):
        out["inlier_mask"][off[j] : off[j + 1]] = r["inlier_mask"]
    return out


def subset(scene, arb, keep):
    off = scene["track_off"]
    sel = np.concatenate([np.arange(off[j], off[j + 1]) for j in keep] + [np.zeros(0, np.int64)]).astype(np.int64)
    sub = {"cameras": scene["cameras"], "track_off": np.concatenate([[0], np.cumsum([off[j + 1] - off[j] for j in keep])]).astype(np.int64),
           "image": scene["image"][sel], "uv": scene["uv"][sel], "rung": np.array([scene["rung"][j] for j in keep], dtype=str)}
    out = {k: arb[k][keep] for k in ("point", "avg_error", "exit_code", "stats", "cost_min")}
    out["inlier_mask"] = arb["inlier_mask"][sel]
    return sub, out


def main() -> None:
    families = scenes.hard_scenes()
    _STATE.update(families)
    data, excluded, dropped, lines = {}, [], [], []
    names = []
    with multiprocessing.Pool() as pool:
        for name, scene in families.items():
            opts = scene["options"]
            arb = run_arbiter(name, scene, pool)
            port = ref.triangulate_tracks(scene["cameras"], scene["track_off"], scene["image"], scene["uv"], solver="jacobi", **opts)
            numpy_ = ref.triangulate_tracks(scene["cameras"], scene["track_off"], scene["image"], scene["uv"], **opts)
            res, res_np = arbiter.accept(scene, arb, port), arbiter.accept(scene, arb, numpy_)
            rungs = list(dict.fromkeys(scene["rung"]))
            keep = []
            for rung in rungs:
                idx = [j for j, r in enumerate(scene["rung"]) if r == rung]
                judged = [j for j in idx if not arb["no_minimiser"][j] and not arb["non_decisive"][j]]
                failed = [j for j in judged if res["failures"][j]]
                gaps = [res["gap"][j] for j in judged if np.isfinite(res["gap"][j])]
                np_failed = [j for j in judged if res_np["failures"][j]]
                np_rel = np.nanmax([res_np["point_rel"][j] for j in judged] + [np.nan]) if judged else np.nan
                line = (f"  {rung}: {len(idx)} candidates, {len(judged)} decisive with an arbiter answer, port fails {len(failed)}, worst port cost gap "
                        f"{max(gaps, default=float('nan')):.2e}; numpy-solver restatement fails {len(np_failed)}, its worst point rel {np_rel:.2e}")
                for j in idx:
                    if arb["no_minimiser"][j]:
                        excluded.append({"family": name, "rung": rung, "candidate": j, "reason": "no finite minimiser"})
                    elif arb["non_decisive"][j]:
                        excluded.append({"family": name, "rung": rung, "candidate": j, "reason": "non-decisive: " + arb["non_decisive"][j]})
                if len(failed) > RUNG_FAILURE_SHARE * len(idx):
                    why = sorted({f for j in failed for f in res["failures"][j]})[:3]
                    dropped.append({"family": name, "rung": rung, "candidates": len(idx), "port_failures": len(failed),
                                    "worst_cost_gap": max(gaps, default=float("nan")), "examples": why})
                    line += "  -> DROPPED WHOLE: outside the design's domain (" + "; ".join(why) + ")"
                else:
                    for j in failed:
                        excluded.append({"family": name, "rung": rung, "candidate": j, "reason": "port: " + "; ".join(res["failures"][j])})
                    keep += [j for j in judged if not res["failures"][j]]
                lines.append(line)
            keep = sorted(keep)
            sub, out = subset(scene, arb, keep)
            rel = np.nanmax(np.concatenate([res["point_rel"][keep], [0.0]]))
            dif = np.nanmax(np.concatenate([res["avg_dif"][keep], [0.0]]))
            avg_scale = np.nanmax(np.concatenate([np.abs(out["avg_error"]), [1.0]]))
            rtol, atol = FACTOR * max(rel, EPS), FACTOR * max(dif, EPS * avg_scale)
            pins = ""
            if name.startswith("ties_"):
                original = ref.select_pairs
                ref.select_pairs = scenes.select_pairs_reversed_ties
                try:
                    flipped = ref.triangulate_tracks(sub["cameras"], sub["track_off"], sub["image"], sub["uv"], solver="jacobi", **opts)
                finally:
                    ref.select_pairs = original
                kept_port = ref.triangulate_tracks(sub["cameras"], sub["track_off"], sub["image"], sub["uv"], solver="jacobi", **opts)
                differ = [j for j in range(len(keep)) if not np.array_equal(flipped["stats"][j], kept_port["stats"][j])
                          or not np.array_equal(flipped["inlier_mask"][sub["track_off"][j] : sub["track_off"][j + 1]],
                                                kept_port["inlier_mask"][sub["track_off"][j] : sub["track_off"][j + 1]])]
                pins = f"; reversed tie rule changes stats or mask on {len(differ)} of {len(keep)} kept tracks"
                data[f"{name}/tie_rule_observable"] = np.array(differ, np.int64)
            lines.insert(len(lines) - len(rungs), f"{name}: options {opts}, kept {len(keep)} of {len(scene['rung'])}; port-to-arbiter point rel max {rel:.3e}, avg error max "
                         f"{dif:.3e} px -> tolerance {rtol:.3e} / {atol:.3e} px; exit codes {np.bincount(out['exit_code'], minlength=6).tolist()}{pins}")
            names.append(name)
            for k, v in {**sub, **out}.items():
                data[f"{name}/{k}"] = v
            data[f"{name}/options"] = np.array(json.dumps(opts))
            data[f"{name}/point_rtol"], data[f"{name}/avg_error_atol"] = np.float64(rtol), np.float64(atol)
            data[f"{name}/port_point_rel"], data[f"{name}/port_avg_error"] = np.float64(rel), np.float64(dif)
            print("\n".join(lines[-len(rungs) - 1 :]), flush=True)
    data["families"] = np.array(names, dtype=str)
    data["excluded"] = np.array(json.dumps(excluded))
    data["dropped_rungs"] = np.array(json.dumps(dropped))
    data["non_decisive_share"] = np.float64(0.0)  # non-decisive candidates are excluded, none is kept
    dst = REPO / "tests" / "golden" / "triangulation_hard_scenes.npz"
    np.savez_compressed(dst, **data)
    text = ["Hard-geometry triangulation scenes: the float64 port of the device's design (Givens / Jacobi DLT, 8 steps) and the numpy-solver",
            "restatement against the high-precision arbiter, on the CPU (tools/make_triangulation_hard_fixture.py).", ""] + lines + ["", "Dropped rungs:"]
    text += [f"  {d['family']} / {d['rung']}: {d['port_failures']} of {d['candidates']} fail the port, worst cost gap {d['worst_cost_gap']:.2e} ({'; '.join(d['examples'])})"
             for d in dropped] or ["  none"]
    text += ["", f"Excluded candidates: {len(excluded)}"] + [f"  {e['family']} / {e['rung']} #{e['candidate']}: {e['reason']}" for e in excluded]
    profile = REPO / "profiles" / "triangulation_hard_scenes.txt"
    device = profile.read_text().partition(DEVICE_MARKER)[2] if profile.exists() else ""  # figures from a GPU run, pasted in by hand: kept
    profile.write_text("\n".join(text) + "\n" + (DEVICE_MARKER + device if device else ""))
    print(dst, dst.stat().st_size, "bytes; dropped", len(dropped), "rungs, excluded", len(excluded), "candidates")


if __name__ == "__main__":
    main()
