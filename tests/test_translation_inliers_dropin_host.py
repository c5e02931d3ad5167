"""CPU: the host side of the ``TranslationAveraging1DSFM`` drop-in (gtsfm_amd/averaging/translation/averaging_1dsfm.py): constructor defaults,
module constants and enum values against the reference's source text (read with ``ast`` where the checkout is present), the three sampling
modes against numpy's and scipy's own streams, the host functions against the restatement and the reference's known answers, the refusals,
and the config. No device is touched: everything here runs before an engine exists."""

import ast
import os
import pickle
from pathlib import Path

import numpy as np
import pytest
import yaml

from tests import translation_inliers_reference as ref
from tests.conftest import REPO

REFERENCE = Path(os.environ.get("GTSFM_REFERENCE", "/root/reference"))
SOURCE = REFERENCE / "gtsfm" / "averaging" / "translation" / "averaging_1dsfm.py"


@pytest.mark.skipif(not SOURCE.exists(), reason="reference tree not present")
def test_defaults_constants_and_enum_equal_the_reference_source():
    from gtsfm_amd.averaging.translation import averaging_1dsfm as mod

    tree = ast.parse(SOURCE.read_text())
    constants = {t.id: ast.literal_eval(node.value) for node in tree.body if isinstance(node, ast.Assign) and isinstance(node.value, ast.Constant)
                 for t in node.targets if isinstance(t, ast.Name)}
    assert set(constants) >= {"MAX_PROJECTION_DIRECTIONS", "OUTLIER_WEIGHT_THRESHOLD", "TRACKS_MEASUREMENTS_PER_CAMERA", "MIN_TRACK_MEASUREMENTS_FOR_AVERAGING", "MAX_DELAYED_CALLS"}
    for name, value in constants.items():
        assert getattr(mod, name) == value, name
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "TranslationAveraging1DSFM")
    enum = next(n for n in cls.body if isinstance(n, ast.ClassDef) and n.name == "ProjectionSamplingMethod")
    members = {t.id: ast.literal_eval(n.value) for n in enum.body if isinstance(n, ast.Assign) for t in n.targets}
    assert {m.name: m.value for m in mod.TranslationAveraging1DSFM.ProjectionSamplingMethod} == members and len(members) == 3
    init = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__init__")
    names = [a.arg for a in init.args.args[1:]]
    defaults = [ast.unparse(d) for d in init.args.defaults]
    import inspect

    ours = inspect.signature(mod.TranslationAveraging1DSFM.__init__).parameters
    assert list(ours)[1:1 + len(names)] == names  # the reference's arguments first, in its order
    for name, text in zip(names, defaults):
        expect = {"MAX_DELAYED_CALLS": constants["MAX_DELAYED_CALLS"]}.get(text)
        if text.startswith("ProjectionSamplingMethod."):
            expect = mod.TranslationAveraging1DSFM.ProjectionSamplingMethod[text.split(".")[1]]
        elif expect is None:
            expect = ast.literal_eval(text)
        assert ours[name].default == expect, name
    select = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "_select_tracks_for_averaging")
    assert [a.arg for a in select.args.args] == list(inspect.signature(mod.TranslationAveraging1DSFM._select_tracks_for_averaging).parameters)


def test_sampling_modes_reproduce_the_generators_streams():
    from scipy import stats

    from gtsfm_amd.averaging.translation import TranslationAveraging1DSFM

    methods = TranslationAveraging1DSFM.ProjectionSamplingMethod
    measurements = ref.unit(np.random.default_rng(5).normal(size=(50, 3)))
    np.random.seed(123)
    obj = TranslationAveraging1DSFM()  # the constructor seeds the global generator with 0, as the reference's does
    got = obj.sample_projection_directions(measurements)
    np.random.seed(0)
    assert got.shape == (2000, 3) and got.tobytes() == ref.unit(np.random.normal(size=(2000, 3))).tobytes()

    obj = TranslationAveraging1DSFM(projection_sampling_method="SAMPLE_INPUT_MEASUREMENTS")
    assert obj._projection_sampling_method is methods.SAMPLE_INPUT_MEASUREMENTS
    got = obj.sample_projection_directions(measurements)
    np.random.seed(0)
    assert got.tobytes() == measurements[np.random.choice(50, 50, replace=False)].tobytes()
    obj._max_1dsfm_projection_directions = 20
    np.random.seed(0)
    got = obj.sample_projection_directions(measurements)
    np.random.seed(0)
    assert got.tobytes() == measurements[np.random.choice(50, 20, replace=False)].tobytes()

    obj = TranslationAveraging1DSFM(projection_sampling_method=methods.SAMPLE_WITH_INPUT_DENSITY)
    got = obj.sample_projection_directions(measurements)
    np.random.seed(0)
    spherical = np.column_stack((np.arctan2(measurements[:, 0], measurements[:, 2]), np.arccos(measurements[:, 1])))
    sampled = stats.gaussian_kde(spherical.T).resample(size=2000).T
    expect = np.column_stack((np.sin(sampled[:, 0]) * np.sin(sampled[:, 1]), np.cos(sampled[:, 1]), np.cos(sampled[:, 0]) * np.sin(sampled[:, 1])))
    assert got.shape == (2000, 3) and got.tobytes() == ref.unit(expect).tobytes()
    np.testing.assert_allclose(np.sqrt((got * got).sum(1)), 1.0, rtol=0, atol=4e-16)
    with pytest.raises(ValueError):
        TranslationAveraging1DSFM(projection_sampling_method="SAMPLE_SOMETHING")


class _Rot:
    def __init__(self, m):
        self._m = np.asarray(m, np.float64).reshape(3, 3)

    def matrix(self):
        return self._m


def test_host_functions_equal_the_restatement_and_the_known_answers():
    from gtsfm_amd.averaging.translation.averaging_1dsfm import C, L, TranslationAveraging1DSFM, get_valid_measurements_in_world_frame, select_tracks_csr
    from gtsfm_amd.common.calibration import PinholeIntrinsics
    from gtsfm_amd.common.sfm_track import SfmMeasurement, SfmTrack2d

    obj = TranslationAveraging1DSFM()
    assert obj._engine is None and pickle.loads(pickle.dumps(obj))._outlier_weight_threshold == 0.125
    # test_select_tracks_for_averaging
    cameras = [[0, 1, 2, 3, 5, 6], [1, 2, 3], [0, 1, 3, 4], [0, 2], [0, 1, 2], [2, 3, 4], [0, 3, 1, 5]]
    tracks = [SfmTrack2d([SfmMeasurement(i, np.array([20.0, 20.0])) for i in cams]) for cams in cameras]
    cal = PinholeIntrinsics(20.0, 0.0, 0.0)
    selected = obj._select_tracks_for_averaging(tracks, {0, 1, 2, 3}, [cal] * 7, measurements_per_camera=3)
    assert len(selected) == 4
    for track in selected:
        assert [m.i for m in track.measurements] in [[0, 1, 2, 3], [1, 2, 3], [0, 1, 3], [0, 1, 2], [0, 3, 1]]
    track_off, image = np.concatenate([[0], np.cumsum([len(c) for c in cameras])]), np.concatenate(cameras)
    expect = ref.select_tracks(track_off, image, {0, 1, 2, 3}, 3)
    got = select_tracks_csr(track_off, image, {0, 1, 2, 3}, 3)
    assert got[0].tolist() == expect[0].tolist() and got[1].tolist() == expect[1].tolist()
    assert [[m.i for m in t.measurements] for t in selected] == [[c for c in cameras[j] if c in {0, 1, 2, 3}] for j in expect[2]]
    everything = TranslationAveraging1DSFM(use_all_tracks_for_averaging=True)._select_tracks_for_averaging(tracks, {0, 1, 2, 3}, [cal] * 7)
    assert len(everything) == 5
    # test_get_landmark_directions; a rotation with .matrix() and a plain array
    for rot in (_Rot(np.diag([1.0, -1.0, 1.0])), np.diag([1.0, -1.0, 1.0])):
        directions = obj._get_landmark_directions([SfmTrack2d([SfmMeasurement(0, np.array([20.0, 20.0]))])], [cal], [rot])
        assert list(directions) == [(0, 0)]
        np.testing.assert_allclose(directions[(0, 0)], np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0), rtol=4e-16, atol=0)
    exp, _ = ref.world_landmark_directions([0, 1], [0], [[20.0, 20.0]], [1], None, np.diag([1.0, -1.0, 1.0]).reshape(1, 9), [1], [[20.0, 20.0, 0.0, 0.0]])
    assert directions[(0, 0)].tobytes() == exp[0].tobytes()
    # test_binary_measurements_from_dict
    pairs = {(0, 1): np.eye(3)[0], (0, 2): np.eye(3)[1], (1, 2): np.eye(3)[2]}
    assert set(obj._binary_measurement_keys(pairs, pairs)) == {(C(i2), C(i1)) for i1, i2 in pairs} | {(C(i2), L(i1)) for i1, i2 in pairs}
    assert C(0) < C(5) < L(0)  # gtsam's key order
    # get_valid_measurements_in_world_frame: the quirk, and the restatement's bytes
    rot = np.asarray([[0.36, 0.48, -0.8, -0.8, 0.6, 0.0, 0.48, 0.64, 0.6]] * 3)
    i2Ui1 = {(0, 1): np.array([0.0, 0.6, 0.8]), (1, 2): np.array([1.0, 0.0, 0.0]), (0, 2): None}  # noqa: N806
    world, valid = get_valid_measurements_in_world_frame(i2Ui1, [None, _Rot(rot[1]), None])
    assert list(world) == [(0, 1)] and valid == {0, 1}
    exp, _ = ref.world_pair_directions([(0, 1)], [[0.0, 0.6, 0.8]], None, rot, [0, 1, 0])
    assert world[(0, 1)].tobytes() == exp[0].tobytes()


def test_refusals_raise_before_any_device_is_touched():
    from gtsfm_amd.averaging.translation.averaging_1dsfm import GtsamMissingError, TranslationAveraging1DSFM
    from gtsfm_amd.common.sfm_track import SfmMeasurement, SfmTrack2d

    class Fisheye:  # not of the pinhole family
        def K(self):  # noqa: N802
            return np.eye(3)

    obj = TranslationAveraging1DSFM()
    track = [SfmTrack2d([SfmMeasurement(0, np.array([1.0, 2.0]))])]
    with pytest.raises(NotImplementedError, match="pinhole"):
        obj._get_landmark_directions(track, [Fisheye()], [np.eye(3)])
    with pytest.raises(AssertionError, match="valid rotation"):
        obj._get_landmark_directions(track, [None], [None])
    with pytest.raises(ValueError, match="Tracks must be provided"):
        obj.run_translation_averaging(2, {(0, 1): np.array([1.0, 0.0, 0.0])}, [np.eye(3)] * 2)
    with pytest.raises(ValueError, match="intrinsics"):
        obj.run_translation_averaging(2, {(0, 1): np.array([1.0, 0.0, 0.0])}, [np.eye(3)] * 2, tracks_2d=[], intrinsics=[None])
    with pytest.raises(ValueError, match="ordered"):
        obj.compute_inliers_arrays([(1, 0)], [[1.0, 0.0, 0.0]])
    assert obj.compute_inliers({}, {}) == ({}, {}, set()) and obj._engine is None  # nothing to do: no device
    assert TranslationAveraging1DSFM.run_mfas({}, {}, [np.array([1.0, 0.0, 0.0])]) == [{}]
    # the stage with outlier rejection off and a recovery of the caller's: steps 1-5 run on the host
    seen = {}

    def recovery(num_images, pairs, tracks, wRi_list, i2Ti1_priors, absolute_pose_priors, scale_factor, robust):  # noqa: N803
        seen.update(pairs=pairs, tracks=tracks, scale=scale_factor, robust=robust)
        return [np.zeros(3), np.ones(3), None]

    off = TranslationAveraging1DSFM(reject_outliers=False, translation_recovery=recovery)
    poses, metrics, inliers = off.run_translation_averaging(3, {(0, 1): np.array([0.0, 0.6, 0.8]), (1, 2): None}, [np.eye(3), np.eye(3), None], tracks_2d=[], intrinsics=[None] * 3)
    assert inliers == [(0, 1)] and metrics is None and poses[2] is None and poses[1][1].tolist() == [1.0, 1.0, 1.0] and seen["tracks"] == {} and seen["robust"] is True
    try:
        import gtsam  # noqa: F401
    except Exception:  # noqa: BLE001
        with pytest.raises(GtsamMissingError, match="gtsam") as info:
            TranslationAveraging1DSFM(reject_outliers=False).run_translation_averaging(2, {(0, 1): np.array([1.0, 0.0, 0.0])}, [np.eye(3)] * 2, tracks_2d=[], intrinsics=[None] * 2)
        assert isinstance(info.value, ImportError)


def test_translation_config_instantiates():
    from gtsfm_amd.averaging.translation import TranslationAveraging1DSFM
    from tests.test_config_hook import instantiate

    node = yaml.safe_load((REPO / "gtsfm_amd" / "configs" / "deep_front_end_amd_translation.yaml").read_text())
    view_graph = yaml.safe_load((REPO / "gtsfm_amd" / "configs" / "deep_front_end_amd_view_graph.yaml").read_text())
    assert {k: v for k, v in node.items() if k != "translation_averaging_module"} == view_graph
    obj = instantiate(node["translation_averaging_module"])
    assert isinstance(obj, TranslationAveraging1DSFM) and obj._projection_sampling_method is TranslationAveraging1DSFM.ProjectionSamplingMethod.SAMPLE_INPUT_MEASUREMENTS
    assert obj._reject_outliers is False and obj._use_all_tracks_for_averaging is True and obj._use_relative_camera_poses is True and obj._robust_measurement_noise is True
    assert pickle.loads(pickle.dumps(obj))._use_all_tracks_for_averaging is True
    reference = REFERENCE / "gtsfm" / "configs" / "deep_front_end.yaml"
    if reference.exists():
        def find(n):
            if isinstance(n, dict):
                if str(n.get("_target_", "")).endswith("TranslationAveraging1DSFM"):
                    return n
                for v in n.values():
                    hit = find(v)
                    if hit:
                        return hit
            return None

        theirs = find(yaml.safe_load(reference.read_text()))
        ours = node["translation_averaging_module"]
        assert {k: v for k, v in theirs.items() if k != "_target_"} == {k: v for k, v in ours.items() if k != "_target_"}
