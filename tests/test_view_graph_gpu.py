"""GPU: ``gtsfm_view_graph_cycle_filter_f64`` and ``gtsfm_largest_component`` (gtsfm_amd/csrc/view_graph_kernels.hip) through
``ViewGraphEngine`` on every scene of tests/view_graph_scenes.py, both criteria and every threshold of the scene: ``num_triplets``, ``keep``,
the triplet list, ``counts`` and the component of the kept edges equal the restatement's (tests/view_graph_reference.py; no edge is excluded:
the scenes assert that no aggregate lies within 1e-6 degrees of a threshold), the aggregates and cycle errors lie within 8 x the distance of
the float64 restatement from a 50-digit evaluation, measured on the scenes themselves (the hard scenes each on their own triplets, and byte-wise
where the value is exactly 0). The aggregate is numpy's min / median of the device's own errors byte for byte, ties included; thresholds of
+inf and NaN keep what the strict comparison says. A permutation of the rows permutes the per-edge
outputs byte for byte and leaves the triplet list alone; two runs give the same bytes; ties between components go to the first edge listed;
every refusal returns an error and leaves the outputs untouched. ``-s`` prints the lines of profiles/view_graph_gpu_tests.txt."""

import ctypes

import numpy as np
import pytest

from tests import view_graph_reference as ref
from tests import view_graph_scenes as scenes

pytestmark = pytest.mark.gpu

SCENE_NAMES = scenes.SCENE_NAMES
PER_EDGE = ("num_triplets", "aggregate_error", "keep")


@pytest.fixture(scope="module")
def engine(gpu_device):
    from gtsfm_amd.runtime.view_graph_engine import ViewGraphEngine

    return ViewGraphEngine(gpu_device)


def run_scene(engine, sc, criterion, threshold, order=None):
    """Host arrays of one call of each entry point; ``order``: a permutation of the rows."""
    pairs, rot, enable = sc["pair_images"], sc["rotation"], sc["enable"]
    if order is not None:
        pairs, rot, enable = pairs[order], rot[order], None if enable is None else enable[order]
    pimg, rdev, en = engine.upload(pairs, rot, enable)
    out = engine.cycle_filter(pimg, rdev, en, num_images=sc["num_images"], criterion=criterion, error_threshold=threshold, want_triplets=True)
    comp = engine.largest_component(pimg, out["keep"], num_images=sc["num_images"])
    got = {k: out[k].cpu().numpy() for k in (*PER_EDGE, "triplets", "cycle_error")}
    got["counts"] = np.array([out["counts"][k] for k in ("input_edges", "kept_edges", "triplets", "max_triplets_per_edge")] + [0] * 4, np.int32)
    got["node_mask"], got["pair_keep"] = comp["node_mask"].cpu().numpy(), comp["pair_keep"].cpu().numpy()
    got["component_counts"] = np.array([comp["counts"][k] for k in ("nodes", "edges", "components")] + [0] * 5, np.int32)
    return got


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_scene_against_the_restatement(engine, name):
    sc = {s["name"]: s for s in scenes.all_scenes()}[name]
    tol = scenes.measured_tolerance(name)  # a hard scene is held to its own measured distance, every other scene to that of the first scenes
    for criterion in (ref.MIN_EDGE_ERROR, ref.MEDIAN_EDGE_ERROR):
        for thr in sc["thresholds"]:
            got = run_scene(engine, sc, criterion, thr)
            dist = scenes.check_outputs(f"{name}/{criterion}/{thr}", got, scenes.expected(sc, criterion, thr), tol["tolerance"], exact_zero=tol["exact_zero"])
            print(f"{name} criterion {criterion} threshold {thr:.6g}: {len(sc['pair_images'])} edges, {len(got['triplets'])} triplets, aggregate within {dist['aggregate_error']:.3e}, "
                  f"cycle error within {dist['cycle_error']:.3e} degrees (restatement from 50 digits {tol['restatement']:.3e}, tolerance {tol['tolerance']:.3e})")
    if name in scenes.HARD_SCENES:
        print(f"{name}: " + ", ".join(f"{k} {v}" for k, v in tol.items() if k not in ("restatement", "tolerance", "exact_zero")))


def boundary_scene(edges):
    """Exactly ``edges`` enabled edges: window(130, 2) has 257, in lexicographic order, so its first rows are a window graph too."""
    sc = scenes.scene(f"window_{edges}", scenes.window(130, 2)[:edges], seed=8)
    assert len(sc["pair_images"]) == edges and sc["enable"] is None
    scenes.check_scene(sc)
    return sc


@pytest.mark.parametrize("edges", [255, 256, 257])
def test_edge_counts_around_one_workgroup(engine, edges):
    """255, 256 and 257 edges: one lane short of a full workgroup of the per-edge stages, exactly one, and one lane into the second (510, 512
    and 514 slots for the per-slot stages, 64 and 65 workgroups of four waves for the aggregate). Both criteria, then the largest component
    of the kept edges, held to the restatement by the rule of every other scene."""
    sc = boundary_scene(edges)
    tol = scenes.measured_tolerance()
    for criterion in (ref.MIN_EDGE_ERROR, ref.MEDIAN_EDGE_ERROR):
        exp = ref.cycle_filter(sc["pair_images"], sc["rotation"], None, sc["num_images"], criterion, 7.0)
        exp["component"] = ref.largest_component(sc["pair_images"], exp["keep"], sc["num_images"])
        assert 0 < exp["keep"].sum() < edges and len(exp["triplets"]) > 100  # the filter and the component have something to decide
        got = run_scene(engine, sc, criterion, 7.0)
        assert len(got["keep"]) == edges
        scenes.check_outputs(f"{sc['name']}/{criterion}", got, exp, tol["tolerance"], exact_zero=tol["exact_zero"])


@pytest.mark.parametrize("name", [n for n in SCENE_NAMES if n not in ("empty", "one_edge")])
def test_row_permutation_and_rerun_are_byte_equal(engine, name):
    sc = {s["name"]: s for s in scenes.all_scenes()}[name]
    thr = sc["thresholds"][-1]
    base = run_scene(engine, sc, ref.MEDIAN_EDGE_ERROR, thr)
    again = run_scene(engine, sc, ref.MEDIAN_EDGE_ERROR, thr)
    for k, v in base.items():
        assert v.tobytes() == again[k].tobytes(), f"{name}: {k} differs between two runs"
    order = np.random.default_rng(3).permutation(len(sc["pair_images"]))
    moved = run_scene(engine, sc, ref.MEDIAN_EDGE_ERROR, thr, order=order)
    for k in (*PER_EDGE, "pair_keep"):
        assert moved[k].tobytes() == base[k][order].tobytes(), f"{name}: {k} is not the permuted array"
    for k in ("triplets", "cycle_error", "counts", "node_mask", "component_counts"):
        assert moved[k].tobytes() == base[k].tobytes(), f"{name}: {k} changed under a permutation of the rows"


def test_error_bytes_are_shared_by_the_three_edges(engine):
    """With MIN and MEDIAN alike, an edge with one triplet reports that triplet's error: the same bytes as the triplet list holds."""
    sc = {s["name"]: s for s in scenes.all_scenes()}["gaps"]
    got = run_scene(engine, sc, ref.MIN_EDGE_ERROR, 7.0)
    exp = scenes.expected(sc, ref.MIN_EDGE_ERROR, 7.0)
    rows_in = np.flatnonzero(exp["input"])
    row_of = {tuple(p): r for r, p in zip(rows_in, sc["pair_images"][rows_in].tolist())}
    lowest = {}
    for (a, b, c), err in zip(got["triplets"].tolist(), got["cycle_error"]):
        for edge in ((a, b), (b, c), (a, c)):
            lowest[row_of[edge]] = min(lowest.get(row_of[edge], np.inf), err)
    assert len(lowest) > 100
    for row, err in lowest.items():
        assert got["aggregate_error"][row].tobytes() == np.float64(err).tobytes()


@pytest.mark.parametrize("name", [n for n in SCENE_NAMES if n not in ("empty", "one_edge")])
def test_aggregate_is_numpys_selection_of_the_devices_own_errors(engine, name):
    """Byte for byte, on every scene and both criteria: the aggregate of an edge is np.min / np.median of the errors the device itself reports
    for the triplets of that edge, and num_triplets is their number. No tolerance and no atan2 enters: ties, equal middle elements and values
    apart in the last bit are selected or averaged exactly as numpy does."""
    sc = {s["name"]: s for s in scenes.all_scenes()}[name]
    rows_in = np.flatnonzero(scenes.expected(sc, ref.MIN_EDGE_ERROR, 7.0)["input"])
    row_of = {tuple(p): r for r, p in zip(rows_in, sc["pair_images"][rows_in].tolist())}
    for criterion, select in ((ref.MIN_EDGE_ERROR, np.min), (ref.MEDIAN_EDGE_ERROR, np.median)):
        got = run_scene(engine, sc, criterion, 7.0)
        trip, err = got["triplets"].reshape(-1, 3), got["cycle_error"]
        rows = np.array([[row_of[(a, b)], row_of[(b, c)], row_of[(a, c)]] for a, b, c in trip.tolist()], np.int64).reshape(-1, 3)
        order = np.argsort(rows.reshape(-1), kind="stable")
        flat_row, flat_err = rows.reshape(-1)[order], np.repeat(err, 3)[order]
        start = np.flatnonzero(np.concatenate([[True], np.diff(flat_row) != 0]))
        expect_num, expect_agg = np.zeros(len(sc["pair_images"]), np.int32), np.full(len(sc["pair_images"]), np.nan)
        for lo, hi in zip(start, np.concatenate([start[1:], [len(flat_row)]])):
            expect_num[flat_row[lo]], expect_agg[flat_row[lo]] = hi - lo, select(flat_err[lo:hi])
        assert len(start) > 0 and not np.isnan(err).any()
        np.testing.assert_array_equal(got["num_triplets"], expect_num, err_msg=f"{name}/{criterion}: num_triplets")
        bad = np.flatnonzero(got["aggregate_error"].view(np.uint64) != expect_agg.view(np.uint64))
        bad = bad[~(np.isnan(got["aggregate_error"][bad]) & np.isnan(expect_agg[bad]))]
        assert len(bad) == 0, (f"{name}/{criterion}: the aggregate is not numpy's selection of the device's errors at {len(bad)} edges, first rows {bad[:5].tolist()}: "
                               f"{got['aggregate_error'][bad[:5]]} against {expect_agg[bad[:5]]}")


def test_infinite_and_nan_thresholds(engine):
    """keep = aggregate < threshold with +inf keeps every input edge (all aggregates of k5 are finite), with NaN only the input edges without a
    triplet: k5 has none, a triangle with a tail has one."""
    k5 = {s["name"]: s for s in scenes.all_scenes()}["k5"]
    tail = scenes.scene("triangle_and_tail", scenes.complete(3) + [(2, 3)], seed=1)
    for sc, edges, with_triplet in ((k5, 10, 10), (tail, 4, 3)):
        for criterion in (ref.MIN_EDGE_ERROR, ref.MEDIAN_EDGE_ERROR):
            for thr in (float("inf"), float("nan")):
                got = run_scene(engine, sc, criterion, thr)
                exp = ref.cycle_filter(sc["pair_images"], sc["rotation"], sc["enable"], sc["num_images"], criterion, thr)
                exp["component"] = ref.largest_component(sc["pair_images"], exp["keep"], sc["num_images"])
                scenes.check_outputs(f"{sc['name']}/{criterion}/{thr}", got, exp, scenes.measured_tolerance()["tolerance"])
                finite = np.isfinite(got["aggregate_error"])
                # +inf: every finite aggregate is below it, and an input edge without a triplet is kept anyway; NaN: nothing is below it
                assert finite.sum() == with_triplet and got["keep"].tolist() == (exp["input"] & (exp["input"] if thr > 0 else ~finite)).astype(np.uint8).tolist()
                assert int(got["counts"][1]) == (edges if thr > 0 else edges - with_triplet)


def test_component_tie_goes_to_the_first_edge_listed(engine):
    first = [(0, 1), (1, 2), (7, 8), (8, 9), (4, 5)]
    for pairs in (first, [first[2], first[3], first[0], first[1], first[4]], [(9, 8), first[0], (2, 1), first[2], first[4]]):
        pimg, _, _ = engine.upload(np.asarray(pairs, np.int32))
        got = engine.largest_component(pimg, None, num_images=12)
        exp = ref.largest_component(np.asarray(pairs), None, 12)
        np.testing.assert_array_equal(got["node_mask"].cpu().numpy(), exp["node_mask"])
        np.testing.assert_array_equal(got["pair_keep"].cpu().numpy(), exp["pair_keep"])
        assert [got["counts"][k] for k in ("nodes", "edges", "components")] == exp["counts"][:3].tolist() == [3, 2, 3]
        assert exp["node_mask"][pairs[0][0]] == 1
    # a disabled first row does not decide, and a self loop is legal
    pimg, _, en = engine.upload(np.asarray(first + [(11, 11)], np.int32), None, np.array([0, 1, 1, 1, 1, 1], np.uint8))
    got = engine.largest_component(pimg, en, num_images=12)
    assert np.flatnonzero(got["node_mask"].cpu().numpy()).tolist() == [7, 8, 9] and got["counts"]["components"] == 4


REFUSALS = {
    "reversed": ([(0, 1), (2, 1), (0, 2)], None, 3, "i1 >= i2"),
    "equal": ([(0, 1), (1, 1)], None, 3, "i1 >= i2"),
    "duplicate": ([(0, 1), (1, 2), (0, 2), (1, 2)], None, 3, "listed twice"),
    "out_of_range": ([(0, 1), (1, 3)], None, 3, "outside 0 .. 2"),
    "negative": ([(-1, 1), (1, 2)], None, 3, "outside 0 .. 2"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_leave_the_outputs_untouched(engine, case):
    """Argument checks: the call returns an error through gtsfm_last_error and has written nothing."""
    import torch

    pairs, enable, n, message = REFUSALS[case]
    lib, dev = engine._lib, engine.device
    pimg, rot, _ = engine.upload(np.asarray(pairs, np.int32), np.tile(np.eye(3).reshape(9), (len(pairs), 1)))
    e = len(pairs)
    outs = [torch.full((e,), 0x55555555, dtype=torch.int32, device=dev), torch.full((e,), 123.0, dtype=torch.float64, device=dev),
            torch.full((e,), 0x55, dtype=torch.uint8, device=dev), torch.full((8,), 0x55555555, dtype=torch.int32, device=dev),
            torch.full((16, 3), 0x55555555, dtype=torch.int32, device=dev), torch.full((16,), 123.0, dtype=torch.float64, device=dev)]
    before = [t.clone() for t in outs]
    ws = torch.empty(int(lib.gtsfm_view_graph_workspace_bytes(e, n, 16)) + 256, dtype=torch.uint8, device=dev)
    found = ctypes.c_longlong(7)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.gtsfm_view_graph_cycle_filter_f64(pimg.data_ptr(), rot.data_ptr(), None, e, n, 1, 7.0, 16, ws.data_ptr(), ws.numel(), *[t.data_ptr() for t in outs], ctypes.byref(found), stream)
    assert rc == -1 and message in lib.gtsfm_last_error().decode() and found.value == -1
    torch.cuda.synchronize()
    for t, b in zip(outs, before):
        assert torch.equal(t, b)
    # the same rows disabled are nobody's business
    en = torch.tensor([0 if (a >= b or a < 0 or b >= n or i == len(pairs) - 1) else 1 for i, (a, b) in enumerate(pairs)], dtype=torch.uint8, device=dev)
    rc = lib.gtsfm_view_graph_cycle_filter_f64(pimg.data_ptr(), rot.data_ptr(), en.data_ptr(), e, n, 1, 7.0, 16, ws.data_ptr(), ws.numel(), *[t.data_ptr() for t in outs], ctypes.byref(found),
                                               stream)
    assert rc == 0 and found.value >= 0 and outs[2].cpu().numpy().tolist() == en.cpu().numpy().tolist()
    if case in ("out_of_range", "negative"):
        mask, keep, counts = (torch.full((k,), 0x55, dtype=torch.uint8, device=dev) for k in (n, e, 32))
        rc = lib.gtsfm_largest_component(pimg.data_ptr(), None, e, n, ws.data_ptr(), ws.numel(), mask.data_ptr(), keep.data_ptr(), counts.data_ptr(), stream)
        assert rc == -1 and "outside 0 .. 2" in lib.gtsfm_last_error().decode()
        torch.cuda.synchronize()
        assert bool((mask == 0x55).all()) and bool((keep == 0x55).all()) and bool((counts == 0x55).all())


def test_workspace_too_small_and_triplet_capacity(engine):
    import torch

    sc = {s["name"]: s for s in scenes.all_scenes()}["k5"]
    lib, dev = engine._lib, engine.device
    pimg, rot, _ = engine.upload(sc["pair_images"], sc["rotation"])
    e, n = 10, 5
    assert lib.gtsfm_view_graph_workspace_bytes(-1, 5, 0) == 0 and lib.gtsfm_view_graph_workspace_bytes(1 << 28, 5, 0) == 0
    assert lib.gtsfm_view_graph_workspace_bytes(10, 1 << 28, 0) == 0 and lib.gtsfm_view_graph_workspace_bytes(10, 5, (1 << 31) // 3) == 0
    need = int(lib.gtsfm_view_graph_workspace_bytes(e, n, 10))
    assert need > 0
    outs = [torch.full((e,), 0x55555555, dtype=torch.int32, device=dev), torch.full((e,), 123.0, dtype=torch.float64, device=dev),
            torch.full((e,), 0x55, dtype=torch.uint8, device=dev), torch.full((8,), 0x55555555, dtype=torch.int32, device=dev)]
    before = [t.clone() for t in outs]
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    found = ctypes.c_longlong(7)
    stream = torch.cuda.current_stream(dev).cuda_stream
    args = lambda cap, size: (pimg.data_ptr(), rot.data_ptr(), None, e, n, 1, 7.0, cap, ws.data_ptr(), size, *[t.data_ptr() for t in outs], None, None, ctypes.byref(found), stream)  # noqa: E731
    assert lib.gtsfm_view_graph_cycle_filter_f64(*args(10, need - 1)) == -3 and b"workspace" in lib.gtsfm_last_error()
    # K5 has 10 triplets: a capacity of 9 is refused after the count, which is handed back
    assert lib.gtsfm_view_graph_cycle_filter_f64(*args(9, need)) == -3 and found.value == 10 and b"10 triplets" in lib.gtsfm_last_error()
    torch.cuda.synchronize()
    for t, b in zip(outs, before):
        assert torch.equal(t, b)
    assert lib.gtsfm_view_graph_cycle_filter_f64(*args(10, need)) == 0 and outs[3].cpu().numpy()[:4].tolist() == scenes.expected(sc, 1, 7.0)["counts"][:4].tolist()
    # the engine grows its capacity by itself: one edge row per triplet would not do for K70
    from gtsfm_amd.runtime.view_graph_engine import ViewGraphEngine

    fresh = ViewGraphEngine(dev)
    k70 = {s["name"]: s for s in scenes.all_scenes()}["k70"]
    p70, r70, _ = fresh.upload(k70["pair_images"], k70["rotation"])
    out = fresh.cycle_filter(p70, r70, None, num_images=70, want_triplets=True)
    assert out["counts"]["triplets"] == 54740 > 8 * 2415 and fresh._triplet_capacity == 54740 and len(out["triplets"]) == 54740
    with pytest.raises(TypeError, match="rotation must be a contiguous"):
        fresh.cycle_filter(p70, r70.float(), None, num_images=70)
    with pytest.raises(TypeError, match="pair_images must be a contiguous"):
        fresh.cycle_filter(p70.cpu(), r70, None, num_images=70)


def test_drop_ins_on_the_device(gpu_device):
    """The classes and functions under the reference's names: the known answers, gtsam-like rotation objects, None values."""
    from gtsfm_amd.utils import graph as graph_utils
    from gtsfm_amd.view_graph_estimator import CycleConsistentRotationViewGraphEstimator, EdgeErrorAggregationCriterion

    class Rot:  # what _to_pose_types yields where gtsam is installed
        def __init__(self, m):
            self._m = m

        def matrix(self):
            return self._m

    sc = scenes.five_node_reference_case()
    rotations = {tuple(p): (Rot(r.reshape(3, 3)) if i % 2 else r.reshape(3, 3)) for i, (p, r) in enumerate(zip(sc["pair_images"].tolist(), sc["rotation"]))}
    est = CycleConsistentRotationViewGraphEstimator(EdgeErrorAggregationCriterion.MEDIAN_EDGE_ERROR)
    assert est.run(rotations, {}, [], {}, [], {}) == {(0, 1), (1, 2), (0, 2)}
    assert est.run({**rotations, (1, 3): None}, {}, [], {}, [], {}) == {(0, 1), (1, 2), (0, 2)}
    arrays = est.run_arrays(rotations, want_triplets=True)
    assert arrays["triplets"].tolist() == [[0, 1, 2], [2, 3, 4]] and arrays["num_triplets"].tolist() == [1, 1, 1, 1, 1, 1] and arrays["counts"]["kept_edges"] == 3
    np.testing.assert_allclose(arrays["cycle_error"], [0.0, 15.0], rtol=0, atol=1e-12)
    hubs = {s["name"]: s for s in scenes.all_scenes()}["hubs"]
    rotations = {tuple(p): r.reshape(3, 3) for p, r in zip(hubs["pair_images"].tolist(), hubs["rotation"])}
    thr = hubs["thresholds"][-1]  # the scene asserts that no aggregate lies at it
    for criterion, code in ((EdgeErrorAggregationCriterion.MIN_EDGE_ERROR, ref.MIN_EDGE_ERROR), (EdgeErrorAggregationCriterion.MEDIAN_EDGE_ERROR, ref.MEDIAN_EDGE_ERROR)):
        assert CycleConsistentRotationViewGraphEstimator(criterion, thr).run(rotations, {}, [], {}, [], {}) == ref.run_estimator(rotations, code, thr)
    base = [(0, 1), (1, 2), (2, 3), (1, 3), (3, 4)]
    assert graph_utils.extract_cyclic_triplets_from_edges(base) == [(1, 2, 3)]
    assert graph_utils.extract_cyclic_triplets_from_edges(base + [(5, 1), (3, 5), (1, 5)]) == [(1, 2, 3), (1, 3, 5)]
    assert graph_utils.extract_cyclic_triplets_from_edges(base + [(3, 5), (4, 5)]) == [(1, 2, 3), (3, 4, 5)]
    rng = np.random.default_rng(9)
    pairs = np.sort(rng.integers(0, 40, size=(400, 2)), axis=1)
    edges = [tuple(p) for p in pairs[pairs[:, 0] != pairs[:, 1]].tolist()]
    assert graph_utils.extract_cyclic_triplets_from_edges(edges) == ref.extract_cyclic_triplets_from_edges(edges)
    assert graph_utils.get_nodes_in_largest_connected_component([(2, 4), (3, 4), (4, 7), (7, 6), (1, 5), (8, 9)]) == [2, 3, 4, 6, 7]
    values = {(0, 1): 1, (1, 5): None, (3, 1): 2, (3, 2): 3, (2, 7): None, (4, 6): 4, (6, 7): 5}
    r, u = graph_utils.prune_to_largest_connected_component(values, dict(values), relative_pose_priors={})
    assert list(r) == list(u) == [(0, 1), (3, 1), (3, 2)]
    # a prior joins the two halves, and a None key between two nodes of the component comes along
    r, _ = graph_utils.prune_to_largest_connected_component(values, dict(values), relative_pose_priors={(2, 7): object()})
    assert list(r) == [k for k in values if k != (1, 5)]
