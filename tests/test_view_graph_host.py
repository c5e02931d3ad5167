"""CPU: the specification of the device's view-graph stage (tests/view_graph_reference.py) against what it restates -- the reference's known
answers, a brute-force triplet search, the reference's own functions loaded live where its checkout is present (gtsam and the other modules
that are not installed replaced by a minimal stand-in whose Rot3 is a 3 x 3 float64 matrix), scipy's rotation-vector norm and a 50-digit
evaluation of the cycle angle -- and the parts of the drop-ins that need no GPU."""

import importlib.abc
import importlib.machinery
import importlib.util
import os
import sys
import types
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import yaml

from tests import view_graph_reference as ref
from tests import view_graph_scenes as scenes
from tests.conftest import REPO

REFERENCE = Path(os.environ.get("GTSFM_REFERENCE", "/root/reference"))
LIVE = ("gtsfm.utils.graph", "gtsfm.utils.geometry_comparisons", "gtsfm.view_graph_estimator.cycle_consistent_rotation_estimator")


# ---- the reference's known answers

def test_estimator_known_answer():
    """The reference's test_filter_to_cycle_consistent_edges: the (2, 4) edge off by 15 degrees about y."""
    sc = scenes.five_node_reference_case()
    rotations = {tuple(p): r.reshape(3, 3) for p, r in zip(sc["pair_images"].tolist(), sc["rotation"])}
    assert ref.run_estimator(rotations, ref.MEDIAN_EDGE_ERROR) == {(0, 1), (1, 2), (0, 2)}
    out = ref.cycle_filter(sc["pair_images"], sc["rotation"], None, 5, ref.MEDIAN_EDGE_ERROR, 7.0)
    np.testing.assert_allclose(out["cycle_error"], [0.0, 15.0], rtol=0, atol=1e-12)
    assert out["triplets"].tolist() == [[0, 1, 2], [2, 3, 4]]


def test_triplet_and_adjacency_known_answers():
    """tests/utils/test_graph_utils.py of the reference: one cycle; two cycles sharing an edge; two sharing a node; the adjacency list."""
    base = [(0, 1), (1, 2), (2, 3), (1, 3), (3, 4)]
    assert ref.extract_cyclic_triplets_from_edges(base) == [(1, 2, 3)]
    assert sorted(ref.extract_cyclic_triplets_from_edges(base + [(1, 5), (3, 5)])) == [(1, 2, 3), (1, 3, 5)]
    assert sorted(ref.extract_cyclic_triplets_from_edges(base + [(3, 5), (4, 5)])) == [(1, 2, 3), (3, 4, 5)]
    assert ref.extract_cyclic_triplets_from_edges([(2, 1), (3, 2), (1, 3), (1, 2)]) == [(1, 2, 3)]  # reversed and repeated edges
    assert ref.extract_cyclic_triplets_from_edges([]) == []
    adj = ref.create_adjacency_list(base + [(3, 5), (4, 5)])
    assert adj == {0: {1}, 1: {0, 2, 3}, 2: {1, 3}, 3: {1, 2, 4, 5}, 4: {3, 5}, 5: {3, 4}}


def test_component_known_answers():
    edges = [(2, 4), (3, 4), (4, 7), (7, 6)] + [(1, 5), (8, 9)]
    assert ref.get_nodes_in_largest_connected_component(edges) == [2, 3, 4, 6, 7]
    assert ref.get_nodes_in_largest_connected_component([]) == []
    # equal sizes: the component of the first edge listed
    assert ref.get_nodes_in_largest_connected_component([(5, 6), (0, 1)]) == [5, 6]
    assert ref.get_nodes_in_largest_connected_component([(0, 1), (5, 6)]) == [0, 1]
    assert ref.get_nodes_in_largest_connected_component([(0, 1), (5, 6), (6, 7), (1, 2)]) == [0, 1, 2]


def brute_force_triplets(edges):
    """The reference's extract_triplets_brute_force: a triple loop over the nodes."""
    edge_set = {(min(a, b), max(a, b)) for a, b in edges}
    nodes = sorted({v for e in edge_set for v in e})
    return {(a, b, c) for i, a in enumerate(nodes) for j, b in enumerate(nodes[i + 1:], i + 1) if (a, b) in edge_set for c in nodes[j + 1:]
            if (b, c) in edge_set and (a, c) in edge_set}


@pytest.mark.parametrize("num_pairs,num_nodes", [(100, 200), (400, 40)])
def test_triplets_against_brute_force(num_pairs, num_nodes):
    pairs = np.sort(np.random.default_rng(num_pairs).integers(0, num_nodes, size=(num_pairs, 2)), axis=1)
    edges = [tuple(p) for p in pairs[pairs[:, 0] != pairs[:, 1]].tolist()]
    got = ref.extract_cyclic_triplets_from_edges(edges)
    assert len(got) == len(set(got)) and got == sorted(got) and set(got) == brute_force_triplets(edges)
    assert num_nodes > 40 or len(got) > 50


# ---- the cycle angle

def sample_triplets(count=200, seed=0):
    rng = np.random.default_rng(seed)
    rots = scenes.rotvec_to_matrix(rng.normal(size=(3 * count, 3))).reshape(count, 3, 3, 3)
    rots[: count // 2, 2] = np.matmul(rots[: count // 2, 1], rots[: count // 2, 0])  # consistent up to ...
    rots[: count // 2, 2] = np.matmul(rots[: count // 2, 2], scenes.rotvec_to_matrix(rng.normal(size=(count // 2, 3)) * np.logspace(-9, -1, count // 2)[:, None]))
    return rots[:, 0], rots[:, 1], rots[:, 2]  # i1Ri0, i2Ri1, i2Ri0


def test_cycle_angle_against_scipy_and_50_digits():
    """The restatement takes the angle as 2 atan2(|q_xyz|, |q_w|); scipy's Rotation.from_matrix(M).as_rotvec() norm is the reference's route
    (geometry_comparisons.py:156-158). Near zero acos of the trace loses half the digits; this form does not."""
    from scipy.spatial.transform import Rotation

    r10, r21, r20 = sample_triplets()
    got = ref.cycle_errors(r10, r21, r20)
    m = np.matmul(np.matmul(r20.transpose(0, 2, 1), r21), r10)
    via_scipy = np.rad2deg(np.linalg.norm(Rotation.from_matrix(m).as_rotvec(), axis=1))
    exact = np.array([ref.cycle_error_mp(a, b, c) for a, b, c in zip(r10, r21, r20)])
    print(f"restatement from scipy {np.abs(got - via_scipy).max():.3e}, from 50 digits {np.abs(got - exact).max():.3e} degrees; smallest angle {exact.min():.3e}")
    assert np.abs(got - via_scipy).max() < 1e-13 and np.abs(got - exact).max() < 1e-13
    small = exact < 1e-3
    trace = m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2]
    via_acos = np.rad2deg(np.arccos(np.clip((trace - 1) / 2, -1, 1)))
    # the entries of M carry about 1e-15 of rounding, which the differences of the atan2 form pass on as they are; acos takes a square root of it
    assert small.sum() > 20 and np.abs(got - exact)[small].max() < 1e-13 < 1e-9 < np.abs(via_acos - exact)[small].max()


def test_rotations_that_are_not_orthonormal_follow_the_definition_not_scipy():
    """The numbers behind the PARITY UNPINNED sentence of include/gtsfm_amd.h: scipy's from_matrix re-orthogonalises, the stated definition
    takes the matrix as it is. On 30 degrees scaled by 1.01 scipy answers 30.000 and the definition 30.076; scipy raises on a non-positive
    determinant where the definition answers; on hard_cycles_skewed (rows times 1 + N(0, 1e-6)) the two differ by about 1e-4 degrees while the
    restatement stays within 2.9e-14 degrees of the 50-digit evaluation of the definition."""
    from scipy.spatial.transform import Rotation

    eye = np.eye(3)
    scaled = scenes.axis_angle((0.36, 0.48, 0.8), 30.0) * 1.01
    via_scipy = np.rad2deg(Rotation.from_matrix(scaled).magnitude())
    defined, exact = ref.cycle_errors(scaled[None], eye[None], eye[None])[0], ref.cycle_error_mp(scaled, eye, eye)
    print(f"30 degrees scaled by 1.01: scipy {via_scipy:.3f}, the definition {defined:.3f} degrees (50 digits {exact:.3f})")
    assert f"{via_scipy:.3f}" == "30.000" and f"{defined:.3f}" == f"{exact:.3f}" == "30.076" and abs(defined - exact) < 1e-13
    mirror = np.diag([1.0, 1.0, -1.0])
    with pytest.raises(ValueError, match="Non-positive determinant"):
        Rotation.from_matrix(mirror)
    assert ref.cycle_errors(mirror[None], eye[None], eye[None])[0] == ref.cycle_error_mp(mirror, eye, eye) == 180.0
    skewed = scenes.measured_tolerance("hard_cycles_skewed")
    print(f"hard_cycles_skewed: M M^T off the identity by {skewed['orthonormality']:.3e}; scipy differs from the restatement by {skewed['scipy']:.3e} degrees, "
          f"the restatement from 50 digits by {skewed['restatement']:.3e} degrees")
    assert 5e-5 < skewed["scipy"] < 2e-4 and skewed["restatement"] < 1e-13


def test_hard_scenes_keep_their_own_tolerance():
    """The first scenes' measured distance is the one recorded with them (measured_tolerance asserts it) and no hard scene enters it; each hard
    scene is held to 8 x its own distance over all its triplets."""
    first = scenes.measured_tolerance()
    assert f"{first['restatement']:.3e}" == scenes.FIRST_SCENES_RESTATEMENT and first["tolerance"] == 8 * first["restatement"]
    assert {k[6:] for k in first if k.startswith("scene:")} <= set(scenes.FIRST_SCENES)
    for name in scenes.HARD_SCENES:
        tol = scenes.measured_tolerance(name)
        print(f"{name}: " + ", ".join(f"{k} {v}" for k, v in tol.items()))
        assert tol["tolerance"] == 8 * tol["restatement"] and tol["exact_zero"]
    assert scenes.measured_tolerance("hard_cycles")["restatement"] > first["restatement"]  # it would have loosened the first scenes' tolerance


def test_median_and_min_are_numpys():
    sc = {s["name"]: s for s in scenes.all_scenes()}["hubs"]
    for criterion, fn in ((ref.MIN_EDGE_ERROR, np.amin), (ref.MEDIAN_EDGE_ERROR, np.median)):
        out = ref.cycle_filter(sc["pair_images"], sc["rotation"], None, sc["num_images"], criterion, 7.0)
        assert {len(v) for v in out["lists"].values()} >= {63, 64, 65, 255, 256, 257}
        for row, errors in out["lists"].items():
            assert out["aggregate_error"][row] == fn(errors) and out["num_triplets"][row] == len(errors)
        assert np.isnan(out["aggregate_error"][out["num_triplets"] == 0]).all() and out["keep"][out["num_triplets"] == 0].all()


def test_palace_fixture_is_what_the_restatement_computes():
    z = np.load(scenes.PALACE)
    pairs, n = z["pair_images"], int(z["num_images"])
    assert len(pairs) == 4139 and n == 281 and (pairs[:, 0] < pairs[:, 1]).all() and len(np.unique(pairs, axis=0)) == 4139
    tol = scenes.measured_tolerance()["tolerance"]
    for name, criterion in (("min", ref.MIN_EDGE_ERROR), ("median", ref.MEDIAN_EDGE_ERROR)):
        out = ref.cycle_filter(pairs, z["rotation"], None, n, criterion, 7.0)
        np.testing.assert_array_equal(out["keep"], z[f"keep_{name}"])
        np.testing.assert_allclose(out["aggregate_error"], z[f"aggregate_{name}"], rtol=0, atol=tol, equal_nan=True)
    np.testing.assert_array_equal(out["num_triplets"], z["num_triplets"])
    np.testing.assert_array_equal(out["triplets"], z["triplets"])
    num = out["num_triplets"]
    assert len(out["triplets"]) == 28583 and num.max() == 31 and (num == 0).sum() == 4 and ((num % 2 == 0) & (num > 0)).sum() == 2186
    assert np.bincount(pairs.reshape(-1)).max() == 37 and ref.largest_component(pairs, None, n)["counts"][:3].tolist() == [281, 4139, 1]


# ---- the reference itself, loaded live

class Rot3:
    """The stand-in: a 3 x 3 float64 matrix with gtsam's between (inverse times) and compose."""

    def __init__(self, m=None):
        self._m = np.eye(3) if m is None else np.asarray(m, np.float64).reshape(3, 3)

    def matrix(self):
        return self._m

    def between(self, other):
        return Rot3(self._m.T @ other._m)

    def compose(self, other):
        return Rot3(self._m @ other._m)


class _Anything:
    """Whatever a missing module's function or object is asked to be."""

    def __call__(self, *args, **kwargs):
        return _Anything()

    def __getattr__(self, name):
        return _Anything()

    def __getitem__(self, item):
        return _Anything()


class _StubModule(types.ModuleType):
    __path__ = []  # a package, so that its submodules are looked up too

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        if self.__name__ == "gtsam" and name == "Rot3":
            return Rot3
        if name[0].isupper():  # a type: annotations subscript it, classes derive from it
            return type(name, (), {"__class_getitem__": classmethod(lambda cls, item: cls)})
        return _Anything()


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, fullname, path=None, target=None):
        if fullname.split(".")[0] in ("gtsam", "gtsfm", "dask"):
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        return _StubModule(spec.name)

    def exec_module(self, module):
        pass


@pytest.fixture(scope="module")
def live():
    """The reference's three modules, executed from its checkout with the stand-ins in place; sys.modules is put back afterwards so that
    nothing else in the process ever sees a stand-in."""
    if not (REFERENCE / "gtsfm" / "utils" / "graph.py").exists():
        pytest.skip("the reference checkout is not present")
    before = dict(sys.modules)
    finder = _StubFinder()
    sys.meta_path.insert(0, finder)
    loaded = {}
    try:
        for name in LIVE:
            spec = importlib.util.spec_from_file_location(name, REFERENCE / (name.replace(".", "/") + ".py"))
            module = importlib.util.module_from_spec(spec)
            sys.modules[name] = module
            parent, _, leaf = name.rpartition(".")
            setattr(importlib.import_module(parent), leaf, module)  # ``import gtsfm.utils.graph as graph_utils`` walks the attributes
            spec.loader.exec_module(module)
            loaded[name] = module
    finally:
        sys.meta_path.remove(finder)
        for name in set(sys.modules) - set(before):
            del sys.modules[name]
    return SimpleNamespace(graph=loaded[LIVE[0]], comparisons=loaded[LIVE[1]], estimator=loaded[LIVE[2]])


def test_live_graph_functions(live):
    rng = np.random.default_rng(5)
    for num_pairs, num_nodes in ((100, 200), (300, 30), (60, 12)):
        pairs = np.sort(rng.integers(0, num_nodes, size=(num_pairs, 2)), axis=1)
        edges = [tuple(p) for p in pairs[pairs[:, 0] != pairs[:, 1]].tolist()]
        assert sorted(live.graph.extract_cyclic_triplets_from_edges(edges)) == ref.extract_cyclic_triplets_from_edges(edges)
        assert dict(live.graph.create_adjacency_list(edges)) == ref.create_adjacency_list(edges)
        assert sorted(live.graph.get_nodes_in_largest_connected_component(edges)) == ref.get_nodes_in_largest_connected_component(edges)
    for edges in ([(5, 6), (0, 1)], [(0, 1), (5, 6)], [(7, 8), (8, 9), (1, 2), (2, 3), (4, 5)]):  # ties
        assert sorted(live.graph.get_nodes_in_largest_connected_component(edges)) == ref.get_nodes_in_largest_connected_component(edges)
    rotations = {(0, 1): 1, (1, 5): None, (3, 1): 2, (3, 2): 3, (2, 7): None, (4, 6): 4, (6, 7): 5}
    r, u = live.graph.prune_to_largest_connected_component(rotations, dict(rotations), relative_pose_priors={})
    assert sorted(r) == sorted(u) == [(0, 1), (3, 1), (3, 2)]


@pytest.mark.parametrize("name", ["five_node", "k5", "hubs", "gaps"])
def test_live_estimator(live, name):
    """``run`` of the reference on the scene's edges, Rot3 being the stand-in: the same edge set for both criteria, and the same cycle errors
    to the measured tolerance (the stand-in multiplies with numpy's matmul, the restatement states the order of its sums)."""
    sc = {s["name"]: s for s in scenes.all_scenes()}[name]
    rotations = {tuple(p): Rot3(r) for p, r in zip(sc["pair_images"].tolist(), sc["rotation"])}
    reports = {k: SimpleNamespace(R_error_deg=None) for k in rotations}
    for criterion, code in ((live.estimator.EdgeErrorAggregationCriterion.MIN_EDGE_ERROR, ref.MIN_EDGE_ERROR),
                            (live.estimator.EdgeErrorAggregationCriterion.MEDIAN_EDGE_ERROR, ref.MEDIAN_EDGE_ERROR)):
        got = live.estimator.CycleConsistentRotationViewGraphEstimator(criterion).run(rotations, dict(rotations), [], {}, [], reports)
        exp = ref.cycle_filter(sc["pair_images"], sc["rotation"], None, sc["num_images"], code, 7.0)
        assert got == {tuple(p) for p in sc["pair_images"][exp["keep"] == 1].tolist()}
    trip = exp["triplets"][:: max(1, len(exp["triplets"]) // 200)]
    row_of = {tuple(p): r for r, p in enumerate(sc["pair_images"].tolist())}
    r10, r21, r20, _ = ref.triplet_rotations(trip.astype(np.int64), row_of, sc["rotation"])
    theirs = np.array([live.comparisons.compute_cyclic_rotation_error(Rot3(a), Rot3(b), Rot3(c)) for a, b, c in zip(r10, r21, r20)])
    assert np.abs(theirs - ref.cycle_errors(r10, r21, r20)).max() <= scenes.measured_tolerance()["tolerance"]


# ---- the drop-ins' paths that need no GPU

def test_drop_in_early_paths():
    from gtsfm_amd.utils import graph as graph_utils
    from gtsfm_amd.view_graph_estimator import CycleConsistentRotationViewGraphEstimator, EdgeErrorAggregationCriterion, ViewGraphEstimatorBase
    from gtsfm_amd.runtime.view_graph_engine import criterion_code

    assert [c.value for c in EdgeErrorAggregationCriterion] == ["MIN_EDGE_ERROR", "MEDIAN_EDGE_ERROR"] and EdgeErrorAggregationCriterion.MIN_EDGE_ERROR == "MIN_EDGE_ERROR"
    assert criterion_code(EdgeErrorAggregationCriterion.MIN_EDGE_ERROR) == 0 and criterion_code("MEDIAN_EDGE_ERROR") == 1 and criterion_code(1) == 1
    with pytest.raises(ValueError):
        criterion_code("MEAN_EDGE_ERROR")
    with pytest.raises(TypeError):
        ViewGraphEstimatorBase()  # run is abstract
    est = CycleConsistentRotationViewGraphEstimator("MEDIAN_EDGE_ERROR")
    assert est._edge_error_aggregation_criterion is EdgeErrorAggregationCriterion.MEDIAN_EDGE_ERROR and est._error_threshold == 7.0 and est._engine is None
    eye = np.eye(3)
    rotations = {(0, 1): eye, (2, 1): eye, (1, 2): None, (1, 3): eye, (2, 3): eye, (3, 4): eye}
    directions = {(0, 1): eye[0], (2, 1): eye[0], (1, 2): eye[0], (1, 3): None, (3, 4): eye[0]}
    assert est._get_valid_input_edges(rotations, directions) == [(0, 1), (3, 4)]
    four = est._filter_with_edges(rotations, {**directions, (2, 3): eye[1]}, {k: np.zeros((0, 2)) for k in rotations}, {k: k for k in rotations}, {(0, 1), (2, 3)})
    assert [sorted(d) for d in four] == [[(0, 1), (2, 3)]] * 4 and four[3][(2, 3)] == (2, 3)
    # nothing to do: no device is touched
    assert est.run({}, {}, [], {}, [], {}) == set() and est.run({(0, 1): None}, {}, [], {}, [], {}) == set() and est._engine is None
    with pytest.raises(ValueError, match="incorrectly ordered"):
        est.run_arrays({(2, 1): eye})
    assert graph_utils.extract_cyclic_triplets_from_edges([]) == [] and graph_utils.get_nodes_in_largest_connected_component([]) == []
    assert graph_utils.create_adjacency_list([(0, 1), (1, 2)]) == {0: {1}, 1: {0, 2}, 2: {1}}
    assert graph_utils.normalise_edges([(2, 1), (1, 2), (0, 5)]).tolist() == [[0, 5], [1, 2]]
    assert graph_utils.prune_to_largest_connected_component({(0, 1): None}, {(0, 1): None}, {}) == ({}, {})


def test_view_graph_config_instantiates():
    from gtsfm_amd.view_graph_estimator import CycleConsistentRotationViewGraphEstimator, EdgeErrorAggregationCriterion
    from tests.test_config_hook import instantiate

    node = yaml.safe_load((REPO / "gtsfm_amd" / "configs" / "deep_front_end_amd_view_graph.yaml").read_text())
    two_view = yaml.safe_load((REPO / "gtsfm_amd" / "configs" / "deep_front_end_amd_two_view.yaml").read_text())
    assert {k: v for k, v in node.items() if k != "view_graph_estimator"} == two_view
    est = instantiate(node["view_graph_estimator"])
    assert isinstance(est, CycleConsistentRotationViewGraphEstimator) and est._edge_error_aggregation_criterion is EdgeErrorAggregationCriterion.MEDIAN_EDGE_ERROR
    assert est._error_threshold == 7.0
    import pickle

    assert pickle.loads(pickle.dumps(est))._error_threshold == 7.0
