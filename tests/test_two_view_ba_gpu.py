"""GPU: gtsfm_two_view_ba_f64 against its specification, tests/two_view_ba_reference.py, on the pairs of tests/two_view_ba_scenes.py.

Status, valid mask, accepted steps and linear solves tried must be EQUAL on every pair the restatement itself calls decisive (at most 1 pair
in 16 may be non-decisive; such a pair's final cost must still be <= the restatement's x (1 + 2e-5): two applications of the 1e-5 stopping
rule, either neighbouring stopping point is acceptable). Rotation, direction, points and costs are compared within a MEASURED tolerance: per
scene, 8 x the larger of two measures of the restatement's own float64 sensitivity -- (a) the same run with points 1 .. n-1 in reversed
order (the first carries the prior and stays first), (b) the same run in np.longdouble. The factor is the project's standing one; it covers
the device's reduction tree and solve order. Cost differences are taken relative to max(cost, 1): a cost is a sum of squared pixel residuals, and a
noise-free pair's cost of 1e-9 px^2 must not set a relative bound for the whole scene.

The points that enter the adjustment are the device triangulation's (byte-equal to gtsfm_triangulate_tracks_f64 on the same two-measurement
tracks, checked here; that call is pinned to its own specification by tests/test_triangulation_gpu.py), and the restatement starts from them."""

import numpy as np
import pytest

from tests import two_view_ba_reference as ref
from tests import two_view_ba_scenes as scenes
from tests.conftest import REPO

pytestmark = pytest.mark.gpu

DEVICE_OUTPUTS = ("rotation", "translation", "valid_mask", "point", "cost")
FACTOR = 8.0


@pytest.fixture(scope="module")
def engine(gpu_device):
    from gtsfm_amd.runtime.two_view_ba_engine import TwoViewBAEngine

    return TwoViewBAEngine(gpu_device)


def scene_pairs():
    door = dict(np.load(REPO / "tests" / "golden" / "triangulation_lund_door.npz"))
    pairs = scenes.batch_pairs() + list(scenes.special_pairs().values()) + [scenes.door_pair(door, 0, 1), scenes.make_pair(201, 33, fy_ratio=1.1), scenes.make_pair(202, 64)]
    names = [f"n{n}" for n in scenes.BATCH_COUNTS] + list(scenes.special_pairs()) + ["door_0_1", "anisotropic", "one_wave"]
    return names, pairs


def run_device(engine, layout, **options):
    from gtsfm_amd.runtime.two_view_ba_engine import TwoViewBAOptions

    out = engine.run(layout, TwoViewBAOptions(**options))
    res = {k: out[k].cpu().numpy() for k in DEVICE_OUTPUTS}
    res["stats"] = out["stats"]
    return res


def differences(a, b):
    """(rotation, direction, points relative, final cost relative) between two restatement runs of one pair; None where they took different paths."""
    if a["status"] != b["status"] or a["stats"][4] != b["stats"][4] or a["stats"][5] != b["stats"][5]:
        return None
    if a["status"] not in (ref.OK, ref.INDETERMINATE) or not np.isfinite(a["cost"]).all():
        return np.zeros(4)
    ok = a["triangulated"]
    pts = np.linalg.norm(a["points"][ok] - b["points"][ok], axis=1) / np.linalg.norm(a["points"][ok], axis=1)
    rot = np.abs(a["rotation"] - b["rotation"]).max() if np.isfinite(a["rotation"]).all() else 0.0
    direction = np.abs(a["translation"] - b["translation"]).max() if np.isfinite(a["translation"]).all() else 0.0
    return np.array([rot, direction, pts.max(initial=0.0), abs(a["cost"][1] - b["cost"][1]) / max(a["cost"][1], 1.0)])


def expected_and_tolerance(names, pairs, layout, entering, options=None):
    """The restatement from the entering points (once per pair), and the measured tolerance of the scene. ``options``: what the device call got."""
    expected, tol = [], np.zeros(4)
    lines = []
    options = options or {}
    for name, pair, rows in zip(names, pairs, layout["rows"]):
        args = (pair["k1"], pair["k2"], pair["uv1"], pair["uv2"], pair["R"], pair["t"])
        exp = ref.two_view_ba(*args, initial_points=entering[rows], **options)
        n_tri = int(exp["triangulated"].sum())
        if exp["status"] in (ref.OK, ref.INDETERMINATE) and n_tri > 1:
            order = np.concatenate([[0], np.arange(n_tri - 1, 0, -1)])
            back = ref.two_view_ba(*args, initial_points=entering[rows], order=order, **options)
            # a cost that overflows float64 is finite in longdouble: another RANGE, not another rounding path, and no measure of sensitivity
            wide = ref.two_view_ba(*args, initial_points=entering[rows], dtype=np.longdouble, **options) if np.isfinite(exp["cost"][0]) else exp
            da, db = differences(exp, back), differences(exp, wide)
            if da is None or db is None:
                assert exp["non_decisive"], f"{name}: the restatement takes another path reversed / in longdouble, yet calls the pair decisive"
            elif not exp["non_decisive"]:
                tol = np.maximum(tol, np.maximum(da, db))
            lines.append(f"{name}: {len(pair['uv1'])} verified, {ref.STATUS_NAMES[exp['status']]}, steps {exp['stats'][4]} / solves {exp['stats'][5]}, "
                         f"non-decisive {exp['non_decisive']}; reversed {None if da is None else ['%.2e' % v for v in da]}, "
                         f"longdouble {None if db is None else ['%.2e' % v for v in db]}")
        else:
            lines.append(f"{name}: {len(pair['uv1'])} verified, {ref.STATUS_NAMES[exp['status']]}")
        expected.append(exp)
    print("\n".join(lines))
    print("restatement sensitivity (rotation, direction, points rel, cost / max(cost, 1)):", ["%.3e" % v for v in tol], "-> tolerance x", FACTOR)
    return expected, FACTOR * tol


@pytest.fixture(scope="module")
def batch(engine):
    """The scene, the device's entering points, the restatement from them, and the measured tolerance."""
    names, pairs = scene_pairs()
    layout = scenes.capacity_layout(pairs)
    entering = run_device(engine, layout, max_iterations=0)["point"]
    expected, tolerance = expected_and_tolerance(names, pairs, layout, entering)
    return {"names": names, "pairs": pairs, "layout": layout, "entering": entering, "expected": expected, "tolerance": tolerance}


def compare_pair(name, out, p, rows, exp, tolerance):
    """The rule of the module's docstring for one pair of a device result. Returns whether the pair was left out of the equality checks."""
    stats = out["stats"][p]
    dev_cost = out["cost"][p]
    print(f"{name}: device {ref.STATUS_NAMES[stats[0]]} stats {stats[:6].tolist()} cost {dev_cost.tolist()}; restatement stats {exp['stats'][:6].tolist()} "
          f"cost {exp['cost'].tolist()} non-decisive {exp['non_decisive']}")
    if exp["non_decisive"]:
        if np.isfinite(exp["cost"][1]):
            assert dev_cost[1] <= exp["cost"][1] * (1.0 + 2e-5), f"{name}: non-decisive, device cost {dev_cost[1]!r} above the restatement's {exp['cost'][1]!r} x (1 + 2e-5)"
        return True
    np.testing.assert_array_equal(stats[:6], exp["stats"][:6], err_msg=name)
    np.testing.assert_array_equal(out["valid_mask"][rows].astype(bool), exp["valid"], err_msg=name)
    rot, direction, pts = out["rotation"][p], out["translation"][p], out["point"][rows]
    np.testing.assert_array_equal(np.isnan(rot), np.isnan(exp["rotation"]), err_msg=name)
    np.testing.assert_array_equal(np.isnan(direction), np.isnan(exp["translation"]), err_msg=name)
    np.testing.assert_array_equal(np.isnan(pts), np.isnan(exp["points"]), err_msg=name)
    np.testing.assert_array_equal(np.isnan(dev_cost), np.isnan(exp["cost"]), err_msg=name)
    if exp["status"] in (ref.SKIPPED, ref.NONE_TRIANGULATED):  # the verifier's pose passes through
        np.testing.assert_array_equal(rot, exp["rotation"], err_msg=name)
        np.testing.assert_array_equal(direction, exp["translation"], err_msg=name)
        return False
    if not np.isfinite(exp["cost"]).all():
        return False
    ok = exp["triangulated"]
    d_pts = (np.linalg.norm(pts[ok] - exp["points"][ok], axis=1) / np.linalg.norm(exp["points"][ok], axis=1)).max(initial=0.0)
    d_cost = np.abs(dev_cost - exp["cost"]) / np.maximum(exp["cost"], 1.0)
    d_rot = np.abs(rot - exp["rotation"]).max() if np.isfinite(exp["rotation"]).all() else 0.0
    d_dir = np.abs(direction - exp["translation"]).max() if np.isfinite(exp["translation"]).all() else 0.0
    print(f"    rotation {d_rot:.3e} (allowed {tolerance[0]:.3e}), direction {d_dir:.3e} ({tolerance[1]:.3e}), points rel {d_pts:.3e} ({tolerance[2]:.3e}), "
          f"cost rel {d_cost.max():.3e} ({tolerance[3]:.3e})")
    assert d_rot <= tolerance[0] and d_dir <= tolerance[1] and d_pts <= tolerance[2] and d_cost.max() <= tolerance[3], name
    return False


def test_batch_against_the_restatement(engine, batch):
    out = run_device(engine, batch["layout"])
    assert len(batch["pairs"]) == 16
    assert sum(e["non_decisive"] for e in batch["expected"]) <= len(batch["pairs"]) // 16, "the scene's seeds leave too many non-decisive pairs"
    statuses = {e["status"] for e in batch["expected"]}
    assert {ref.OK, ref.SKIPPED, ref.NO_INITIAL_POSE, ref.NONE_TRIANGULATED} <= statuses
    failures = []
    for p, (name, rows, exp) in enumerate(zip(batch["names"], batch["layout"]["rows"], batch["expected"])):
        try:
            compare_pair(name, out, p, rows, exp, batch["tolerance"])
        except AssertionError as e:
            failures.append(f"{name}: {e}")
    assert not failures, "\n".join(failures)
    # rows that are no verified correspondence: never valid, never a point
    other = np.ones(len(batch["layout"]["inlier_mask"]), bool)
    other[np.concatenate(batch["layout"]["rows"])] = False
    assert not out["valid_mask"][other].any() and np.isnan(out["point"][other]).all()


def test_entering_points_are_the_triangulation_calls(engine, batch, gpu_device):
    """max_iterations = 0 returns the points as they enter: byte-equal to gtsfm_triangulate_tracks_f64 on the same two-measurement tracks."""
    from gtsfm_amd.runtime.triangulation_engine import TriangulationEngine
    from tests import triangulation_reference as tri

    uv, image, cams = [], [], []
    for p, pair in enumerate(batch["pairs"]):
        r, t = pair["R"], pair["t"]
        ok = np.isfinite(r).all() and np.isfinite(t).all()
        centre = [-(float(r[0, i]) * float(t[0]) + float(r[1, i]) * float(t[1]) + float(r[2, i]) * float(t[2])) for i in range(3)]  # the kernel's order of operations
        c0, c1 = tri.pack_camera(*pair["k1"], np.eye(3), np.zeros(3)), tri.pack_camera(*pair["k2"], r.T, centre)
        if not ok:
            c0, c1 = np.zeros(17), np.zeros(17)
        cams += [c0, c1]
        n = len(pair["uv1"])
        uv.append(np.stack([pair["uv1"], pair["uv2"]], axis=1).reshape(2 * n, 2))
        image.append(np.tile([2 * p, 2 * p + 1], n))
    uv, image = np.concatenate(uv).astype(np.float32), np.concatenate(image).astype(np.int32)
    out = TriangulationEngine(gpu_device).triangulate(np.arange(len(image) // 2 + 1, dtype=np.int64) * 2, image, uv, np.asarray(cams), mode="NO_RANSAC")
    point = out["point"].cpu().numpy()
    rows = np.concatenate(batch["layout"]["rows"])
    skipped = np.concatenate([np.full(len(pair["uv1"]), len(pair["uv1"]) < 15) for pair in batch["pairs"]])
    assert np.isfinite(point[~skipped]).any()
    assert batch["entering"][rows][~skipped].tobytes() == point[~skipped].tobytes()
    assert np.isnan(batch["entering"][rows][skipped]).all()  # SKIPPED pairs report no points


def test_run_to_run_and_position_in_the_batch(engine, batch):
    """A pair's output bytes depend on its data (its rows' places in its slice included: they decide which lane owns a point) and the options
    only: not on the run, the batch, its position in it, or the capacity behind its matches."""
    first = run_device(engine, batch["layout"])
    again = run_device(engine, batch["layout"])
    for k in (*DEVICE_OUTPUTS, "stats"):
        assert first[k].tobytes() == again[k].tobytes(), k
    names, pairs = batch["names"], batch["pairs"]
    for p in (names.index("n257"), names.index("n600"), names.index("door_0_1"), names.index("behind")):
        rows = batch["layout"]["rows"][p]
        alone_layout = scenes.capacity_layout([pairs[p]], slack=3)
        alone = run_device(engine, alone_layout)
        moved_layout = scenes.capacity_layout([pairs[0], pairs[4], pairs[p], pairs[2]], slack=11)
        moved = run_device(engine, moved_layout)
        for res, lay, q in ((alone, alone_layout, 0), (moved, moved_layout, 2)):
            for k in ("rotation", "translation", "cost", "stats"):
                assert res[k][q].tobytes() == first[k][p].tobytes(), (names[p], k)
            for k in ("point", "valid_mask"):
                assert res[k][lay["rows"][q]].tobytes() == first[k][rows].tobytes(), (names[p], k)


def test_options_reach_the_kernel(engine, batch):
    """allow_indeterminate, another threshold, no robust loss and a step limit against the restatement on three pairs."""
    names = batch["names"]
    picks = [names.index("n16"), names.index("rotation"), names.index("one_wave")]
    pairs = [batch["pairs"][p] for p in picks]
    layout = scenes.capacity_layout(pairs)
    opts = dict(allow_indeterminate=True, reproj_error_threshold=1.0, huber_k=np.inf, max_iterations=3, min_verified=10)
    out = run_device(engine, layout, **opts)
    for q, p in enumerate(picks):
        exp = ref.two_view_ba(*(pairs[q][k] for k in ("k1", "k2", "uv1", "uv2", "R", "t")), initial_points=batch["entering"][batch["layout"]["rows"][p]], **opts)
        assert exp["stats"][4] <= 3
        compare_pair(names[p] + " (options)", out, q, layout["rows"][q], exp, batch["tolerance"])


def test_door_pair_against_its_fixture(engine, batch):
    """The Lund door pair's expectation and tolerance as tools/make_two_view_fixture.py recorded them (the restatement from its OWN triangulation
    there, from the device's entering points in the scene above): the device's discrete outputs equal the recorded ones, its pose and final cost lie
    within the recorded tolerance of the recorded values. The INITIAL cost (21 387 px^2 at the perturbed pose) is printed only: it is a function of the
    entering points, which differ between the two triangulations by that stage's own tolerance (tests/test_triangulation_gpu.py), not by this one's; from
    equal entering points both costs are held to the tolerance in test_batch_against_the_restatement."""
    import json

    rec = json.loads((REPO / "tests" / "golden" / "two_view_ba_door_pair.json").read_text())
    p = batch["names"].index("door_0_1")
    out = run_device(engine, scenes.capacity_layout([batch["pairs"][p]]))
    tol = rec["tolerance"]
    assert not rec["non_decisive"] and len(batch["pairs"][p]["uv1"]) == rec["verified"]
    d_rot = np.abs(out["rotation"][0] - np.array(rec["rotation"])).max()
    d_dir = np.abs(out["translation"][0] - np.array(rec["translation"])).max()
    d_first, d_cost = np.abs(out["cost"][0] - np.array(rec["cost"])) / np.maximum(np.array(rec["cost"]), 1.0)
    print(f"door pair: stats {out['stats'][0][:6].tolist()} (recorded {rec['stats']}); rotation {d_rot:.3e} (allowed {tol['rotation']:.3e}), direction {d_dir:.3e} "
          f"({tol['direction']:.3e}), final cost {d_cost:.3e} ({tol['cost_over_max_cost_1']:.3e}); initial cost {d_first:.3e} (not held to it)")
    assert out["stats"][0][:6].tolist() == rec["stats"] and int(out["valid_mask"].sum()) == rec["valid"]
    assert d_rot <= tol["rotation"] and d_dir <= tol["direction"] and d_cost <= tol["cost_over_max_cost_1"]


# ---- the catalogue of hard pairs (tests/two_view_ba_scenes.py: hard_pairs): one test per family, the tolerance measured per family.
# The helpers take ``run(layout, **options)``, so the host build (tests/test_two_view_ba_hostbuild.py) goes through the same rule.


def run_family(run, family, entries, cache=None):
    """Every entry of one family under the rule of the module's docstring. Entries that share their options share a launch. Returns one record per
    entry: ``entry``, ``out`` (the launch's outputs), ``p`` (its place in them), ``rows``, ``exp`` (the restatement from the device's
    entering points). ``cache``: a dictionary that keeps the restatement runs for a second caller whose entering points are the same bytes."""
    groups = {}
    for e in entries:
        groups.setdefault(tuple(sorted(e["options"].items())), []).append(e)
    records, tolerance = [], np.zeros(4)
    print(f"==== family {family}")
    for key, group in groups.items():
        options = dict(key)
        names, pairs = [e["name"] for e in group], [e["pair"] for e in group]
        layout = scenes.capacity_layout(pairs)
        entering = run(layout, **{**options, "max_iterations": 0})["point"]
        out = run(layout, **options)
        kept = None if cache is None else cache.get((family, key))
        if kept is None or kept[0] != entering.tobytes():
            kept = (entering.tobytes(), *expected_and_tolerance(names, pairs, layout, entering, options))
            if cache is not None:
                cache[(family, key)] = kept
        tolerance = np.maximum(tolerance, kept[2])
        records += [{"entry": e, "out": out, "p": p, "rows": layout["rows"][p], "exp": kept[1][p], "layout": layout} for p, e in enumerate(group)]
    print(f"family {family}: tolerance (rotation, direction, points rel, cost / max(cost, 1)) {['%.3e' % v for v in tolerance]}")
    failures = []
    for r in records:
        name = f"{family}/{r['entry']['name']}"
        try:
            if family in scenes.DECISIVE_FAMILIES:
                assert not r["exp"]["non_decisive"], f"{name}: the restatement calls the pair non-decisive from the device's entering points; replace its seed"
                assert not compare_pair(name, r["out"], r["p"], r["rows"], r["exp"], tolerance)
            else:
                compare_pair(name, r["out"], r["p"], r["rows"], r["exp"], tolerance)
                check_any_rounding_path(name, r, run)
        except AssertionError as e:
            failures.append(f"{name}: {e}")
        other = np.ones(len(r["layout"]["inlier_mask"]), bool)
        other[np.concatenate(r["layout"]["rows"])] = False
        assert not r["out"]["valid_mask"][other].any() and np.isnan(r["out"]["point"][other]).all(), name
    assert not failures, "\n".join(failures)
    return records


def check_any_rounding_path(name, r, run):
    """What holds for a pair whatever the rounding path (an honestly non-decisive pair is held to this and to the cost rule of compare_pair)."""
    out, p, rows, options = r["out"], r["p"], r["rows"], r["entry"]["options"]
    stats, cost = out["stats"][p], out["cost"][p]
    assert stats[0] in (ref.OK, ref.INDETERMINATE), name
    assert 0 <= stats[4] <= stats[5] and stats[4] <= options.get("max_iterations", ref.DEFAULTS["max_iterations"]), name
    assert cost[1] <= cost[0], name
    valid = out["valid_mask"][rows].astype(bool)
    assert stats[3] == valid.sum() == out["valid_mask"][r["layout"]["match_off"][p]:r["layout"]["match_off"][p + 1]].sum(), name
    assert not (valid & ~np.isfinite(out["point"][rows]).all(axis=1)).any(), f"{name}: a valid row that was not triangulated"
    assert stats[1] == len(rows) and stats[2] == np.isfinite(out["point"][rows]).all(axis=1).sum(), name
    rot, direction = out["rotation"][p], out["translation"][p]
    if np.isfinite(rot).any() or np.isfinite(direction).any():
        assert np.abs(rot @ rot.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(rot) - 1.0) <= 1e-12 and abs(np.linalg.norm(direction) - 1.0) <= 1e-12, name
    else:
        assert np.isnan(rot).all() and np.isnan(direction).all() and stats[0] == ref.INDETERMINATE and not options.get("allow_indeterminate", False), name
    again = run(r["layout"], **options)
    for k in (*DEVICE_OUTPUTS, "stats"):
        assert again[k].tobytes() == out[k].tobytes(), (name, k)


def check_non_finite_family(records):
    """The one decisive handle on the stop at the lambda bound, the rejection of a failed solve and both INDETERMINATE output forms."""
    for r in records:
        e, out, p, exp = r["entry"], r["out"], r["p"], r["exp"]
        pair, stats = e["pair"], out["stats"][p]
        assert stats[:6].tolist() == [ref.INDETERMINATE, 20, 20, int(exp["valid"].sum()), 0, 11] and exp["stop"] == "lambda_bound", e["name"]
        assert np.isinf(out["cost"][p]).all() and (out["cost"][p] > 0).all(), e["name"]
        if e["options"].get("allow_indeterminate"):
            # the input pose passes through: camera 0 is the identity, so the rotation is the input's bytes; the direction is R (R^T t), normalised
            np.testing.assert_array_equal(out["rotation"][p], pair["R"], err_msg=e["name"])
            np.testing.assert_allclose(out["translation"][p], pair["t"], rtol=0, atol=4e-15, err_msg=e["name"])
            np.testing.assert_allclose(out["translation"][p], exp["translation"], rtol=0, atol=4e-15, err_msg=e["name"])
            assert np.isfinite(out["point"][r["rows"]]).all(), e["name"]
        else:
            assert np.isnan(out["rotation"][p]).all() and np.isnan(out["translation"][p]).all() and not out["valid_mask"][r["rows"]].any(), e["name"]


def check_dud_rows(run, pair, verified_decides=False, **options):
    """A verified row that cannot be triangulated -- no keypoint index, or a NaN pixel -- changes no output byte of its pair against the same layout
    with the row's mask at 0, except the verified count. ``verified_decides``: the dud row is the one that lifts the pair to ``min_verified``, so the
    row left out is run with the minimum one lower."""
    base, no_index, nan_pixel, row = scenes.dud_row_layouts(pair)
    least = options.pop("min_verified", ref.DEFAULTS["min_verified"])
    plain = run(base, min_verified=least - 1 if verified_decides else least, **options)
    assert plain["stats"][0][0] == ref.OK and plain["stats"][0][4] > 0
    assert not verified_decides or plain["stats"][0][1] == least - 1
    for name, layout in (("match_idx -1", no_index), ("NaN pixel", nan_pixel)):
        out = run(layout, min_verified=least, **options)
        print(f"dud row {row} ({name}): stats {out['stats'][0][:6].tolist()} against {plain['stats'][0][:6].tolist()} without it")
        for k in DEVICE_OUTPUTS:
            assert out[k].tobytes() == plain[k].tobytes(), (name, k)
        want = plain["stats"][0].copy()
        want[1] += 1
        np.testing.assert_array_equal(out["stats"][0], want, err_msg=name)
        assert out["valid_mask"][row] == 0 and np.isnan(out["point"][row]).all(), name


@pytest.fixture(scope="module")
def hard():
    return scenes.hard_pairs()


@pytest.mark.parametrize("family", scenes.HARD_FAMILIES)
def test_hard_family_against_the_restatement(engine, hard, family):
    records = run_family(lambda layout, **o: run_device(engine, layout, **o), family, hard[family])
    if family == "non_finite":
        check_non_finite_family(records)


def test_dud_rows_change_nothing_but_the_verified_count(engine, hard):
    run = lambda layout, **o: run_device(engine, layout, **o)  # noqa: E731
    check_dud_rows(run, hard["rejections"][0]["pair"])
    check_dud_rows(run, scenes.make_pair(102, 14), verified_decides=True)


def test_hard_pairs_run_to_run_and_position(engine, hard):
    """The alone / moved / re-run check on the pair whose prior sits in a second stride, the 300-point pair with rejections and a pair cut by the
    step limit."""
    picks = (hard["late_first"][0], next(e for e in hard["rejections"] if e["name"] == "far_n300"), hard["step_limit"][1])
    others = scenes.batch_pairs()
    for e in picks:
        pair, options = e["pair"], e["options"]
        alone_layout = scenes.capacity_layout([pair], slack=3)
        alone, again = run_device(engine, alone_layout, **options), run_device(engine, alone_layout, **options)
        moved_layout = scenes.capacity_layout([others[4], others[2], pair, others[3]], slack=11)
        moved = run_device(engine, moved_layout, **options)
        assert alone["stats"][0][0] == ref.OK and alone["stats"][0][4] > 0
        for res, lay, q in ((again, alone_layout, 0), (moved, moved_layout, 2)):
            for k in ("rotation", "translation", "cost", "stats"):
                assert res[k][q].tobytes() == alone[k][0].tobytes(), (e["name"], k)
            for k in ("point", "valid_mask"):
                assert res[k][lay["rows"][q]].tobytes() == alone[k][alone_layout["rows"][0]].tobytes(), (e["name"], k)


def test_many_workgroups(engine, hard):
    """One launch of 1024 pairs, the catalogue's small pairs repeated in a shuffled order: every copy's outputs are the bytes of that pair run alone."""
    small = [e["pair"] for entries in hard.values() for e in entries if len(e["pair"]["uv1"]) <= 64]
    assert len(small) >= 16
    alone = []
    for pair in small:
        layout = scenes.capacity_layout([pair])
        alone.append((run_device(engine, layout), layout["rows"][0]))
    order = np.random.default_rng(1024).permutation(np.arange(1024) % len(small))
    layout = scenes.capacity_layout([small[i] for i in order])
    out = run_device(engine, layout)
    statuses = set()
    for p, i in enumerate(order):
        one, rows = alone[i]
        statuses.add(int(one["stats"][0][0]))
        for k in ("rotation", "translation", "cost", "stats"):
            assert out[k][p].tobytes() == one[k][0].tobytes(), (p, i, k)
        for k in ("point", "valid_mask"):
            assert out[k][layout["rows"][p]].tobytes() == one[k][rows].tobytes(), (p, i, k)
    assert ref.OK in statuses
    other = np.ones(len(layout["inlier_mask"]), bool)
    other[np.concatenate(layout["rows"])] = False
    assert other.any() and not out["valid_mask"][other].any() and np.isnan(out["point"][other]).all()
