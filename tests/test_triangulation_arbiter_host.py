"""CPU: the high-precision arbiter (tests/triangulation_arbiter.py) against the hard-scene fixture it recorded, and the float64
restatement -- the device kernels' specification -- against the arbiter: with numpy's SVD on the scenes the suite already uses (the
first independent check of the specification), and with the port of the device's Givens / Jacobi solve on the whole fixture under the
acceptance rule every implementation is held to (``arbiter.accept``: discrete outputs equal; cost gap to the minimiser at most
1e-5 max(1, cost); point and average error within the family's recorded bound, 8 x the port-to-arbiter difference)."""

import json
import math

import numpy as np
import pytest

from tests import triangulation_arbiter as arbiter
from tests import triangulation_reference as ref
from tests import triangulation_scenes as scenes
from tests.conftest import REPO

HARD = REPO / "tests" / "golden" / "triangulation_hard_scenes.npz"
DOOR = REPO / "tests" / "golden" / "triangulation_lund_door.npz"
OUTPUTS = ("point", "avg_error", "exit_code", "inlier_mask", "stats")


def load_hard():
    data = dict(np.load(HARD))
    fams = {}
    for name in data["families"].tolist():
        fam = {k.split("/", 1)[1]: v for k, v in data.items() if k.startswith(name + "/")}
        fam["options"] = json.loads(str(fam["options"]))
        fams[name] = fam
    return data, fams


DATA, FAMILIES = load_hard()


def held_to_rule(fam, out, label, tracks=None):
    """The acceptance rule; prints the worst figures before it asserts."""
    res = arbiter.accept(fam, fam, out, tracks)
    rel, dif = np.nanmax(np.append(res["point_rel"], 0.0)), np.nanmax(np.append(res["avg_dif"], 0.0))
    slack = np.nanmax(np.append(res["gap"] / res["allowed"], -np.inf))
    print(f"{label}: {len(fam['rung'])} tracks, exit codes {np.bincount(fam['exit_code'], minlength=6).tolist()}; point rel max {rel:.3e} (allowed "
          f"{float(fam['point_rtol']):.3e}), avg error max {dif:.3e} px (allowed {float(fam['avg_error_atol']):.3e}), worst cost gap / allowance {slack:.3e}")
    failed = {f"{j} ({fam['rung'][j]})": f for j, f in enumerate(res["failures"]) if f}
    assert not failed, f"{label}: {failed}"
    assert rel <= float(fam["point_rtol"]) and dif <= float(fam["avg_error_atol"]), label
    return res


def test_fixture_is_decisive_small_and_names_what_it_leaves_out():
    assert HARD.stat().st_size < 1 << 20 and float(DATA["non_decisive_share"]) == 0.0
    dropped, excluded = json.loads(str(DATA["dropped_rungs"])), json.loads(str(DATA["excluded"]))
    kept_rungs = {r for fam in FAMILIES.values() for r in fam["rung"].tolist()}
    assert all(d["rung"] not in kept_rungs and d["port_failures"] > 0.10 * d["candidates"] for d in dropped)
    assert all(e["reason"] for e in excluded)
    profile = (REPO / "profiles" / "triangulation_hard_scenes.txt").read_text()
    assert all(d["rung"] in profile for d in dropped)
    # every ladder the families are meant to climb is present after the exclusions
    for want in ("parallax 1e-1 clean", "parallax 1e-4 noisy", "offset utm parallax 1e-1", "scale 1e-3 f 50", "scale 1e4 f 5000", "rank facing 1e-8",
                 "rank rotation 1e-10", "rank final 1e-6", "rank final 1e-12", "depth 1e-06 front", "depth 1e-06 behind", "depth infinity disparity 1e-30",
                 "hostile image -2147483648 at 0", "hostile image 2147483647 at 1", "hostile image num_images at 3", "hostile image -1 at 0"):
        assert want in kept_rungs, want
    assert {len(f["tie_rule_observable"]) > 0 for n, f in FAMILIES.items() if n in ("ties_topk10", "ties_topk1")} == {True}


@pytest.mark.parametrize("name", list(FAMILIES))
def test_fixture_slice_recomputes(name):
    fam = FAMILIES[name]
    tracks = list(range(0, len(fam["rung"]), 5))
    live = arbiter.triangulate_tracks(fam["cameras"], fam["track_off"], fam["image"], fam["uv"], tracks=tracks, **fam["options"])
    for j in tracks:
        a, b = fam["track_off"][j : j + 2]
        assert live["non_decisive"][j] == "" and not live["no_minimiser"][j]
        for k in ("point", "avg_error", "exit_code", "stats", "cost_min"):
            np.testing.assert_array_equal(live[k][j], fam[k][j], err_msg=f"{name} track {j} {k}")
        np.testing.assert_array_equal(live["inlier_mask"][a:b], fam["inlier_mask"][a:b])


@pytest.mark.parametrize("name", list(FAMILIES))
def test_port_against_arbiter_on_the_whole_fixture(name):
    fam = FAMILIES[name]
    port = ref.triangulate_tracks(fam["cameras"], fam["track_off"], fam["image"], fam["uv"], solver="jacobi", **fam["options"])
    res = held_to_rule(fam, port, f"port, {name}")
    # the recorded bound is 8 x what is measured here (or the float64 floor)
    rel, dif = np.nanmax(np.append(res["point_rel"], 0.0)), np.nanmax(np.append(res["avg_dif"], 0.0))
    assert rel == float(fam["port_point_rel"]) and dif == float(fam["port_avg_error"])
    scale = np.nanmax(np.append(np.abs(fam["avg_error"]), 1.0))
    assert float(fam["point_rtol"]) == 8.0 * max(rel, 2.0**-52) and float(fam["avg_error_atol"]) == 8.0 * max(dif, 2.0**-52 * scale)


@pytest.mark.parametrize("name", [n for n in FAMILIES if n.startswith("offset") or n.startswith("rank")])
def test_numpy_solver_miss_on_badly_scaled_families_is_printed(name):
    """No assertion: LAPACK's absolute accuracy is the restatement's limit here, not a property of the device."""
    fam = FAMILIES[name]
    out = ref.triangulate_tracks(fam["cameras"], fam["track_off"], fam["image"], fam["uv"], **fam["options"])
    res = arbiter.accept(fam, fam, out)
    print(f"numpy solver, {name}: {sum(1 for f in res['failures'] if f)} of {len(fam['rung'])} tracks outside the rule; point rel max "
          f"{np.nanmax(np.append(res['point_rel'], 0.0)):.3e}, worst cost gap {np.nanmax(np.append(res['gap'], -np.inf)):.3e}")


@pytest.mark.parametrize("name", [n for n in FAMILIES if n.startswith("ties_")])
def test_sampler_tie_rule_is_pinned_where_it_can_be(name, monkeypatch):
    """Reversing every tie rule in a copy of ``select_pairs`` changes stats or the mask on the recorded tracks (a tie among pairs that
    are all skipped -- zero baseline, a missing camera -- cannot show in any output)."""
    fam = FAMILIES[name]
    run = lambda: ref.triangulate_tracks(fam["cameras"], fam["track_off"], fam["image"], fam["uv"], solver="jacobi", **fam["options"])  # noqa: E731
    kept = run()
    monkeypatch.setattr(ref, "select_pairs", scenes.select_pairs_reversed_ties)
    flipped = run()
    off = fam["track_off"]
    differ = [j for j in range(len(off) - 1) if not np.array_equal(kept["stats"][j], flipped["stats"][j])
              or not np.array_equal(kept["inlier_mask"][off[j] : off[j + 1]], flipped["inlier_mask"][off[j] : off[j + 1]])]
    assert differ == fam["tie_rule_observable"].tolist()
    for j in differ:  # and the recorded answer is the one of the rule as it stands
        np.testing.assert_array_equal(kept["stats"][j], fam["stats"][j])


def _restatement_against_arbiter(scene, tracks, opts, point_rtol, avg_atol, label):
    off = scene["track_off"]
    arb = arbiter.triangulate_tracks(scene["cameras"], off, scene["image"], scene["uv"], tracks=tracks, **opts)
    worst_rel = worst_dif = 0.0
    skipped = 0
    for j in tracks:
        a, b = int(off[j]), int(off[j + 1])
        detail: dict = {}
        x, avg, code, inl, stats = ref.triangulate_track(scene["cameras"], scene["image"][a:b], scene["uv"][a:b].astype(np.float64), detail=detail, **opts)
        if arb["non_decisive"][j] or arb["no_minimiser"][j] or ref.non_decisive(detail, opts.get("threshold", math.inf)):
            skipped += 1
            continue
        assert code == arb["exit_code"][j] and np.array_equal(inl, arb["inlier_mask"][a:b] != 0) and np.array_equal(stats, arb["stats"][j]), f"{label} track {j}"
        assert np.array_equal(np.isnan(x), np.isnan(arb["point"][j])) and math.isnan(avg) == math.isnan(arb["avg_error"][j])
        if code == ref.SUCCESS:
            worst_rel = max(worst_rel, float(np.linalg.norm(x - arb["point"][j]) / np.linalg.norm(arb["point"][j])))
        if math.isfinite(avg):
            worst_dif = max(worst_dif, abs(avg - arb["avg_error"][j]))
    print(f"{label}: {len(tracks)} tracks, {skipped} non-decisive or without a finite minimiser; restatement to arbiter point rel max {worst_rel:.3e} "
          f"(allowed {point_rtol:.3e}), avg error max {worst_dif:.3e} px (allowed {avg_atol:.3e})")
    assert skipped <= 0.05 * len(tracks) + 1
    assert worst_rel <= point_rtol and worst_dif <= avg_atol


@pytest.fixture(scope="module")
def small():
    scene = scenes.small_shapes()
    scene["tolerance"] = scenes.reversal_tolerance(scene)
    return scene


def test_restatement_against_arbiter_small_shapes_no_ransac(small):
    for opts in (dict(mode=ref.NO_RANSAC), dict(mode=ref.NO_RANSAC, threshold=10.0, min_angle_deg=3.0)):
        _restatement_against_arbiter(small, list(range(len(small["track_off"]) - 1)), opts, *small["tolerance"], f"small shapes {opts}")


def test_restatement_against_arbiter_small_shapes_ransac(small):
    """Every track that is not plain filler (a length outside 2 .. 4, a measurement without a camera, an exit code other than SUCCESS),
    every fourth filler track, and one track of 14 measurements (91 hypotheses). Which pairs a longer track draws is
    ``ref.select_pairs``, shared with the arbiter, so the 15- and 75-measurement tracks add solves, not cases."""
    off, lengths = small["track_off"], np.diff(small["track_off"])
    opts = dict(mode=ref.RANSAC_SAMPLE_UNIFORM, **scenes.LOOSE)
    table = small["cameras"]
    plain = [j for j in range(len(lengths)) if 2 <= lengths[j] <= 4 and all(0 <= i < len(table) and table[i, 0] != 0.0 for i in small["image"][off[j] : off[j + 1]])
             and ref.triangulate_track(table, small["image"][off[j] : off[j + 1]], small["uv"][off[j] : off[j + 1]].astype(np.float64), **opts)[2] == ref.SUCCESS]
    tracks = sorted(set(np.where(lengths <= 6)[0].tolist()) - set(plain[1::4] + plain[2::4] + plain[3::4])) + [int(np.where(lengths == 14)[0][0])]
    _restatement_against_arbiter(small, tracks, opts, *small["tolerance"], "small shapes RANSAC")


@pytest.mark.parametrize("name,mode", [("no_ransac", ref.NO_RANSAC), ("ransac_uniform", ref.RANSAC_SAMPLE_UNIFORM)])
def test_restatement_against_arbiter_door(name, mode):
    door = dict(np.load(DOOR))
    tracks = list(range(0, 8824, 97)) + [3668, 7439]
    assert len(tracks) == 93
    scene = {k: door[k] for k in ("cameras", "track_off", "image", "uv")}
    opts = dict(mode=mode, threshold=float(door[f"{name}_threshold"]), num_hypotheses=int(door[f"{name}_num_hypotheses"]))
    _restatement_against_arbiter(scene, tracks, opts, float(door[f"{name}_point_rtol"]), float(door[f"{name}_avg_error_atol"]), f"door {name}")


def test_jacobi_port_keeps_small_singular_values_where_lapack_does_not():
    """The 8-camera circle at world offset (5e5, 4e6, 100): for the facing pair (0, 4) the exact sigma_3 is far below rank_tol; LAPACK
    reports it above. For the neighbours (0, 1) the port's DLT point is orders of magnitude nearer the exact one."""
    from tests.test_triangulation_host import circle_scene

    table, _, uv = circle_scene()
    table = table.copy()
    shift = np.array([5e5, 4e6, 100.0])
    table[:, 14:17] += shift
    uv = uv.astype(np.float32).astype(np.float64)
    hp = lambda pair: arbiter.dlt([arbiter.Cam(table[i]) for i in pair], [arbiter._mp_uv(uv[i]) for i in pair])  # noqa: E731
    sigma, x = hp((0, 4))
    assert float(sigma[2]) < 1e-12 and x is None
    assert ref.dlt_jacobi([table[0], table[4]], [uv[0], uv[4]]) is None
    assert ref.dlt([table[0], table[4]], [uv[0], uv[4]]) is not None  # the restatement's limit, stated in its docstring
    _, exact = hp((0, 1))
    exact = np.array([float(c) for c in exact])
    miss_port = np.linalg.norm(ref.dlt_jacobi([table[0], table[1]], [uv[0], uv[1]]) - exact)
    miss_numpy = np.linalg.norm(ref.dlt([table[0], table[1]], [uv[0], uv[1]]) - exact)
    print(f"pair (0, 1): DLT point off by {miss_port:.2e} (port), {miss_numpy:.2e} (numpy)")
    assert miss_port < 1e-8 and miss_port < 1e-3 * miss_numpy
