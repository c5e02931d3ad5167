"""Drop-in for ``gtsfm/averaging/translation/averaging_1dsfm.py``: ``TranslationAveraging1DSFM`` with the reference's constructor arguments,
whose outlier rejection (``compute_inliers``, ``run_mfas``: gtsam's MFAS over ``MAX_PROJECTION_DIRECTIONS`` projections) runs on the device
(``gtsfm_translation_inliers_f64``, gtsfm_amd/csrc/translation_kernels.hip). The host parts are the reference's: the three sampling modes draw
from numpy's global generator exactly as the reference calls it, the track selection is its sequential greedy.

Directions are 3-vectors or anything with ``.point3()``; rotations are 3 x 3 arrays or anything with ``.matrix()``; calibrations are of the
pure pinhole family of ``gtsfm_amd.common.calibration.pinhole_parameters`` (anything else raises ``NotImplementedError``).

``run_translation_averaging`` hands the inliers to a ``translation_recovery`` callable. The default is a thin wrapper around gtsam's
``TranslationRecovery`` (it needs gtsam and is not tested here); ``translation_recovery="device"`` selects ``device_translation_recovery``,
which solves the same robust chordal problem on the device (``gtsfm_translation_recovery_f64``, gtsfm_amd/csrc/translation_recovery_kernels.hip;
``recover_arrays`` is the same over arrays). Out of scope: relative and absolute pose priors, ``rig_1dsfm.py``, the Dask graph and the
ground-truth metrics. PARITY UNPINNED: gtsam's MFAS picks among several roots or tied scores in the order of an ``unordered_map`` (here: the
smallest node id); ``Unit3``'s normalisation in the last bits; distortion models; of the recovery, gtsam's Levenberg-Marquardt path and its
seeded random start (here a deterministic linear start), its soft prior on the first key (here a hard anchor), ``Unit3`` and the
2-dimensional noise model of the reference's gtsam version (here the 3-vector chordal residual with the same sigma). No local-minimum
guarantee is claimed."""

from __future__ import annotations

import logging
from enum import Enum
from typing import Any, Callable, Dict, List, Optional, Sequence, Set, Tuple

import numpy as np

from gtsfm_amd.common.calibration import pinhole_parameters
from gtsfm_amd.frontend.registry import GTSFMProcess, UiMetadata

logger = logging.getLogger("gtsfm_amd")

# Hyperparameters for 1D-SFM
MAX_PROJECTION_DIRECTIONS = 2000
OUTLIER_WEIGHT_THRESHOLD = 0.125
NOISE_MODEL_DIMENSION = 2
NOISE_MODEL_SIGMA = 0.01
HUBER_LOSS_K = 1.3
MAX_INLIER_MEASUREMENT_ERROR_DEG = 5.0
MIN_TRACK_MEASUREMENTS_FOR_AVERAGING = 3
TRACKS_MEASUREMENTS_PER_CAMERA = 12
MAX_DELAYED_CALLS = 16
MAX_KDE_SAMPLES = 2000

Pair = Tuple[int, int]


def C(i: int) -> int:  # noqa: N802 - gtsam's symbol_shorthand.A
    return (ord("a") << 56) + int(i)


def L(j: int) -> int:  # noqa: N802 - gtsam's symbol_shorthand.B
    return (ord("b") << 56) + int(j)


class GtsamMissingError(ImportError):
    """``TranslationRecovery`` needs gtsam."""


def vector3(direction) -> np.ndarray:
    point3 = getattr(direction, "point3", None)
    return np.asarray(point3() if callable(point3) else direction, dtype=np.float64).reshape(3)


def matrix3(rotation) -> np.ndarray:
    matrix = getattr(rotation, "matrix", None)
    return np.asarray(matrix() if callable(matrix) else rotation, dtype=np.float64).reshape(3, 3)


def unit_rows(v: np.ndarray) -> np.ndarray:
    """v / sqrt((x x + y y) + z z) per row: the device's normalisation."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    n = np.sqrt((x * x + y * y) + z * z)
    return np.stack([x / n, y / n, z / n], axis=1)


def rotate_unit(rotation: np.ndarray, v: np.ndarray) -> np.ndarray:
    """unit(R v), each row of the product summed as (r0 x + r1 y) + r2 z."""
    r = matrix3(rotation)
    return unit_rows(np.array([(r[k, 0] * v[0] + r[k, 1] * v[1]) + r[k, 2] * v[2] for k in range(3)]))[0]


def sample_random_directions(num_samples: int) -> np.ndarray:
    return unit_rows(np.random.normal(size=(num_samples, 3)))


def sample_kde_directions(measurements: np.ndarray, num_samples: int, max_kde_samples: int = MAX_KDE_SAMPLES) -> np.ndarray:
    """``sampling_utils.sample_kde_directions``: a Gaussian kernel density over (azimuth, elevation), resampled."""
    from scipy import stats

    measurements = np.asarray(measurements, dtype=np.float64).reshape(-1, 3)
    if len(measurements) > max_kde_samples:
        measurements = measurements[np.random.choice(len(measurements), max_kde_samples, replace=False).tolist()]
    spherical = np.column_stack((np.arctan2(measurements[:, 0], measurements[:, 2]), np.arccos(measurements[:, 1])))
    sampled = stats.gaussian_kde(spherical.T).resample(size=num_samples).T
    azimuth, elevation = sampled[:, 0], sampled[:, 1]
    return unit_rows(np.column_stack((np.sin(azimuth) * np.sin(elevation), np.cos(elevation), np.cos(azimuth) * np.sin(elevation))))


def get_valid_measurements_in_world_frame(i2Ui1_dict: Dict[Pair, Any], wRi_list: Sequence[Any]) -> Tuple[Dict[Pair, np.ndarray], Set[int]]:  # noqa: N803
    """The measurements whose direction and wRi2 are present, rotated to the world frame, and the cameras they touch. wRi1 is not looked at,
    yet i1 enters the camera set, as in the reference."""
    world: Dict[Pair, np.ndarray] = {}
    valid_cameras: Set[int] = set()
    for (i1, i2), i2Ui1 in i2Ui1_dict.items():  # noqa: N806
        if i2Ui1 is None or wRi_list[i2] is None:
            continue
        world[(i1, i2)] = rotate_unit(wRi_list[i2], vector3(i2Ui1))
        valid_cameras.update((i1, i2))
    return world, valid_cameras


def greedy_track_subset(cameras_per_track: List[List[int]], valid_cameras: Set[int], measurements_per_camera: int = TRACKS_MEASUREMENTS_PER_CAMERA) -> List[int]:
    """The sequential greedy of ``_select_tracks_for_averaging`` over the filtered tracks' camera lists: repeatedly the track that covers
    the most still-uncovered cameras (``np.argmax``: the first maximum), until every camera sees ``measurements_per_camera`` tracks. Returns
    the chosen tracks' indices in the order of selection."""
    remaining = {c: measurements_per_camera for c in valid_cameras}
    improvement = [len(cams) for cams in cameras_per_track]
    seen_by: Dict[int, List[int]] = {c: [] for c in valid_cameras}
    for k, cams in enumerate(cameras_per_track):
        for c in cams:
            seen_by[c].append(k)
    subset: List[int] = []
    for _ in range(len(cameras_per_track)):
        best = int(np.argmax(improvement))
        if improvement[best] <= 0:
            break
        subset.append(best)
        improvement[best] = 0
        for c in cameras_per_track[best]:
            if remaining[c] == 0:
                continue
            remaining[c] -= 1
            if remaining[c] == 0:  # covered: every track that sees this camera adds one less
                for k in seen_by[c]:
                    improvement[k] = improvement[k] - 1 if improvement[k] > 0 else 0
    return subset


def select_tracks_csr(track_off: np.ndarray, image: np.ndarray, valid_cameras: Set[int], measurements_per_camera: int = TRACKS_MEASUREMENTS_PER_CAMERA,
                      use_all_tracks: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """``_select_tracks_for_averaging`` on the track builder's CSR arrays, as masks for the device: (track_enable [T] uint8, meas_enable [S]
    uint8). A measurement is enabled when its camera is in ``valid_cameras``; a track when it keeps at least 3 and the greedy chose it."""
    track_off, image = np.asarray(track_off, np.int64), np.asarray(image, np.int64)
    meas_ok = np.isin(image, np.fromiter(valid_cameras, np.int64, len(valid_cameras)))
    running = np.concatenate([[0], np.cumsum(meas_ok.astype(np.int64))])
    kept = running[track_off[1:]] - running[track_off[:-1]]
    filtered = np.flatnonzero(kept >= MIN_TRACK_MEASUREMENTS_FOR_AVERAGING)
    if use_all_tracks:
        chosen = filtered
    else:
        cams = [image[track_off[j]:track_off[j + 1]][meas_ok[track_off[j]:track_off[j + 1]]].tolist() for j in filtered]
        chosen = filtered[greedy_track_subset(cams, valid_cameras, measurements_per_camera)] if len(filtered) else filtered
    track_enable = np.zeros(len(track_off) - 1, np.uint8)
    track_enable[chosen] = 1
    return track_enable, meas_ok.astype(np.uint8)


def default_translation_recovery(num_images, w_i2Ui1_dict, w_iUj_dict_tracks, wRi_list, i2Ti1_priors, absolute_pose_priors, scale_factor, robust_measurement_noise):  # noqa: N803
    """gtsam's ``TranslationRecovery`` on the inlier measurements (``averaging_1dsfm.py:439-495``). Needs gtsam; its result is not tested in
    this package and relative pose priors are not handled."""
    try:
        import gtsam  # type: ignore
    except Exception as exc:  # noqa: BLE001
        raise GtsamMissingError("TranslationRecovery needs gtsam, which cannot be imported here: pass translation_recovery= to TranslationAveraging1DSFM, "
                                "or use compute_inliers / VerifiedScene.translation_inliers for the outlier rejection alone") from exc
    if len(i2Ti1_priors) > 0:
        raise NotImplementedError("relative pose priors are not handled by the default translation_recovery")
    noise = gtsam.noiseModel.Isotropic.Sigma(NOISE_MODEL_DIMENSION, NOISE_MODEL_SIGMA)
    if robust_measurement_noise:
        noise = gtsam.noiseModel.Robust.Create(gtsam.noiseModel.mEstimator.Huber.Create(HUBER_LOSS_K), noise)
    measurements = gtsam.BinaryMeasurementsUnit3()
    for (i1, i2), w in w_i2Ui1_dict.items():
        measurements.append(gtsam.BinaryMeasurementUnit3(C(i2), C(i1), gtsam.Unit3(vector3(w)), noise))
    for (j, i), w in w_iUj_dict_tracks.items():
        measurements.append(gtsam.BinaryMeasurementUnit3(C(i), L(j), gtsam.Unit3(vector3(w)), noise))
    values = gtsam.TranslationRecovery().run(measurements, scale_factor)
    return [values.atPoint3(C(i)) if wRi_list[i] is not None and values.exists(C(i)) else None for i in range(num_images)]


_recovery_engines: Dict[str, Any] = {}


def recovery_engine(device=None):
    """The process's ``TranslationRecoveryEngine`` for ``device`` (None: the current one)."""
    key = str(device)
    if key not in _recovery_engines:
        from gtsfm_amd.runtime.translation_recovery_engine import TranslationRecoveryEngine

        _recovery_engines[key] = TranslationRecoveryEngine(device)
    return _recovery_engines[key]


def device_translation_recovery(num_images, w_i2Ui1_dict, w_iUj_dict_tracks, wRi_list, i2Ti1_priors, absolute_pose_priors, scale_factor, robust_measurement_noise,  # noqa: N803
                                device=None, **options):
    """``TranslationRecovery`` on the device, with the signature of ``default_translation_recovery``: the inlier measurements as dicts in, a
    list of ``wti`` (or None for a camera without a rotation or outside the first measurement's component, as the reference's
    ``values.exists`` check gives) out. sigma and Huber's k are the reference's; ``options``: further keys of the engine's ``DEFAULTS``."""
    if len(i2Ti1_priors) > 0:
        raise NotImplementedError("relative pose priors are not handled by device_translation_recovery")
    _, _, pairs, world_pair, track_off, image, world_meas = TranslationAveraging1DSFM._dicts_to_arrays(w_i2Ui1_dict, w_iUj_dict_tracks)
    if len(pairs) + len(image) == 0:
        return [None] * num_images
    eng = recovery_engine(device)
    dev = eng.upload(pairs, world_pair, None, track_off, image, world_meas, None)
    out = eng.recover(*dev, num_images=num_images, scale_factor=scale_factor, sigma=NOISE_MODEL_SIGMA, huber_k=HUBER_LOSS_K if robust_measurement_noise else 0.0, **options)
    wti, valid = out["translation"][0].cpu().numpy(), out["node_valid"][0].cpu().numpy()
    return [wti[i].copy() if wRi_list[i] is not None and valid[i] else None for i in range(num_images)]


class TranslationAverages:
    """What ``VerifiedScene.translation_averaging`` returns: ``wti_list`` (a position or None per image), ``wTi_list`` ((wRi, wti) or None),
    ``landmarks`` [T, 3] (NaN for a track that took no part), ``inliers`` (the ``TranslationInliers`` of the rejection, whose ``.edges``
    feeds ``tracks()``), ``status``, ``counters``, ``costs``. ``read_back()`` downloads the rows the recovery ran on."""

    def __init__(self, wRi_list, wti_list, landmarks, inliers, status, counters, costs, device_rows=None) -> None:  # noqa: N803
        self.wRi_list, self.wti_list, self.landmarks, self.inliers = wRi_list, wti_list, landmarks, inliers
        self.status, self.counters, self.costs, self._device_rows = status, counters, costs, device_rows
        self.wTi_list = [(matrix3(r), t) if r is not None and t is not None else None for r, t in zip(wRi_list, wti_list)]

    @classmethod
    def empty(cls, inliers: "TranslationInliers") -> "TranslationAverages":
        """The result for a scene without rows."""
        from gtsfm_amd.runtime.translation_recovery_engine import COST_FIELDS, COUNTER_FIELDS

        return cls([], [], np.zeros((0, 3)), inliers, "NO_VALID_ROW", dict.fromkeys(COUNTER_FIELDS, 0), dict.fromkeys(COST_FIELDS, float("nan")))

    def cameras(self, intrinsics) -> Dict[int, Any]:
        """{image: PinholeCamera} of the images with a pose and a calibration: the ``cameras`` argument of ``triangulate``."""
        from gtsfm_amd.common.calibration import PinholeCamera

        return {i: PinholeCamera(p[0], p[1], intrinsics[i]) for i, p in enumerate(self.wTi_list) if p is not None and i < len(intrinsics) and intrinsics[i] is not None}

    def read_back(self) -> Dict[str, np.ndarray]:
        """Host copies of the recovery's inputs: ``pair_images``, ``world_pair``, ``pair_enable``, ``track_off``, ``image``, ``world_meas``, ``meas_enable``."""
        return {k: (None if v is None else v.cpu().numpy()) for k, v in (self._device_rows or {}).items()}


class TranslationInliers:
    """What ``compute_inliers_arrays`` and ``VerifiedScene.translation_inliers`` return: ``pairs`` the pair rows, ``pair_weight`` their mean
    outlier weights (NaN for a row that did not take part), ``pair_inlier`` the mask; ``edges`` the inlier pairs in row order (the ``edges=``
    argument of ``tracks()`` / ``triangulate()``), ``inlier_cameras``; ``meas_weight`` / ``meas_inlier`` per track measurement, ``counts``."""

    def __init__(self, pairs: List[Pair], pair_weight: np.ndarray, pair_inlier: np.ndarray, camera_inlier: np.ndarray, meas_weight: np.ndarray, meas_inlier: np.ndarray,
                 counts: Dict[str, int], tracks: Optional[Dict[str, np.ndarray]] = None) -> None:
        self.pairs, self.pair_weight, self.pair_inlier, self.camera_inlier = pairs, pair_weight, pair_inlier, camera_inlier
        self.meas_weight, self.meas_inlier, self.counts, self.tracks = meas_weight, meas_inlier, counts, tracks
        self.edges = [p for p, k in zip(pairs, pair_inlier.tolist()) if k]
        self.inlier_cameras = set(np.flatnonzero(camera_inlier).tolist())
        self.mean_weights = {p: float(w) for p, w in zip(pairs, pair_weight.tolist())}

    @classmethod
    def empty(cls) -> "TranslationInliers":
        """The result for a scene without rows."""
        from gtsfm_amd.runtime.translation_engine import COUNT_FIELDS

        return cls([], np.zeros(0), np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(0), np.zeros(0, np.uint8), dict.fromkeys(COUNT_FIELDS, 0))


class TranslationAveraging1DSFM(GTSFMProcess):
    """1D-SFM translation averaging with outlier rejection."""

    class ProjectionSamplingMethod(str, Enum):
        """How the projection directions of 1DSfM are sampled (string values, for the configs)."""

        SAMPLE_INPUT_MEASUREMENTS = "SAMPLE_INPUT_MEASUREMENTS"
        SAMPLE_WITH_INPUT_DENSITY = "SAMPLE_WITH_INPUT_DENSITY"
        SAMPLE_WITH_UNIFORM_DENSITY = "SAMPLE_WITH_UNIFORM_DENSITY"

    @staticmethod
    def get_ui_metadata() -> UiMetadata:
        return UiMetadata(display_name="Translation Averaging", input_products=("View-Graph Relative Translations", "Global Rotations", "Tracks"),
                          output_products=("Global Translations", "Inlier Pairs"), parent_plate="Sparse Reconstruction")

    def __init__(self, robust_measurement_noise: bool = True, use_tracks_for_averaging: bool = True, reject_outliers: bool = True,
                 projection_sampling_method: "TranslationAveraging1DSFM.ProjectionSamplingMethod" = ProjectionSamplingMethod.SAMPLE_WITH_UNIFORM_DENSITY,
                 max_delayed_calls: int = MAX_DELAYED_CALLS, use_all_tracks_for_averaging: bool = False, use_relative_camera_poses: bool = True,
                 translation_recovery: Optional[Callable[..., List[Optional[np.ndarray]]]] = None, device=None) -> None:
        self._robust_measurement_noise = robust_measurement_noise
        self._max_1dsfm_projection_directions = MAX_PROJECTION_DIRECTIONS
        self._outlier_weight_threshold = OUTLIER_WEIGHT_THRESHOLD
        self._reject_outliers = reject_outliers
        self._projection_sampling_method = TranslationAveraging1DSFM.ProjectionSamplingMethod(projection_sampling_method)
        self._use_tracks_for_averaging = use_tracks_for_averaging
        self._max_delayed_calls = max_delayed_calls  # kept for the signature: the directions are one device call, not Dask tasks
        self._use_relative_camera_poses = use_relative_camera_poses
        self._use_all_tracks_for_averaging = use_all_tracks_for_averaging
        if translation_recovery == "device":
            translation_recovery = device_translation_recovery
        self._translation_recovery = translation_recovery or default_translation_recovery
        self._recovery_options: Dict[str, Any] = {}  # keys of the recovery engine's DEFAULTS, for the device's recovery
        self._device = device
        self._engine = None
        np.random.seed(0)

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_engine"] = None
        return state

    def engine(self):
        if self._engine is None:
            from gtsfm_amd.runtime.translation_engine import TranslationInliersEngine

            self._engine = TranslationInliersEngine(self._device)
        return self._engine

    # ---- host parts ----

    def sample_projection_directions(self, w_measurements: np.ndarray) -> np.ndarray:
        """[D, 3] unit vectors by the configured method, from numpy's global generator as the reference draws them."""
        w_measurements = np.asarray(w_measurements, dtype=np.float64).reshape(-1, 3)
        method, methods = self._projection_sampling_method, TranslationAveraging1DSFM.ProjectionSamplingMethod
        if method == methods.SAMPLE_INPUT_MEASUREMENTS:
            num_samples = min(len(w_measurements), self._max_1dsfm_projection_directions)
            return w_measurements[np.random.choice(len(w_measurements), num_samples, replace=False)]
        if method == methods.SAMPLE_WITH_INPUT_DENSITY:
            return sample_kde_directions(w_measurements, self._max_1dsfm_projection_directions)
        if method == methods.SAMPLE_WITH_UNIFORM_DENSITY:
            return sample_random_directions(self._max_1dsfm_projection_directions)
        raise ValueError("Unsupported sampling method!")

    @staticmethod
    def _binary_measurement_keys(w_i2Ui1_dict: Dict[Pair, Any], w_iUj_dict_tracks: Dict[Pair, Any]) -> List[Tuple[int, int]]:  # noqa: N803
        """The (key1, key2) of ``_binary_measurements_from_dict``: (C(i2), C(i1)) per pair, then (C(i), L(j)) per track measurement."""
        return [(C(i2), C(i1)) for i1, i2 in w_i2Ui1_dict] + [(C(i), L(j)) for j, i in w_iUj_dict_tracks]

    def _select_tracks_for_averaging(self, tracks: List[Any], valid_cameras: Set[int], intrinsics: List[Any],
                                     measurements_per_camera: int = TRACKS_MEASUREMENTS_PER_CAMERA) -> List[Any]:
        """Drops the measurements of cameras outside ``valid_cameras`` and the tracks left with fewer than 3, then takes the track that covers
        the most still-uncovered cameras until every camera sees ``measurements_per_camera`` tracks (a sequential greedy, on the host)."""
        filtered = [t for t in (track.select_for_cameras(camera_idxs=valid_cameras) for track in tracks)
                    if t.number_measurements() >= MIN_TRACK_MEASUREMENTS_FOR_AVERAGING]
        if self._use_all_tracks_for_averaging:
            return filtered
        return [filtered[k] for k in greedy_track_subset([[int(m.i) for m in t.measurements] for t in filtered], valid_cameras, measurements_per_camera)]

    def _get_landmark_directions(self, tracks_2d: List[Any], intrinsics: List[Any], wRi_list: List[Any]) -> Dict[Pair, np.ndarray]:  # noqa: N803
        """{(track_id, camera): unit(wRi unit((x, y, 1)))} for every measurement of every track."""
        directions: Dict[Pair, np.ndarray] = {}
        params: Dict[int, Tuple[float, float, float, float]] = {}
        for track_id, track in enumerate(tracks_2d):
            for m in track.measurements:
                cam = int(m.i)
                assert wRi_list[cam] is not None, "Camera must have valid rotation to use tracks for averaging."
                assert intrinsics[cam] is not None, "Camera must be calibrated to use tracks for averaging."
                if cam not in params:
                    fx, fy, cx, cy, pure = pinhole_parameters(intrinsics[cam])
                    if not pure:
                        raise NotImplementedError(f"camera {cam}: {type(intrinsics[cam]).__name__} is not a pure pinhole calibration")
                    params[cam] = (fx, fy, cx, cy)
                fx, fy, cx, cy = params[cam]
                u, v = np.float64(np.float32(m.uv[0])), np.float64(np.float32(m.uv[1]))  # the device's table is float32
                ray = unit_rows(np.array([(u - cx) / fx, (v - cy) / fy, 1.0]))[0]
                directions[(track_id, cam)] = rotate_unit(wRi_list[cam], ray)
        return directions

    # ---- the device call ----

    def compute_inliers_arrays(self, pair_images, world_pair, track_off=None, image=None, world_meas=None, num_images: Optional[int] = None, directions=None,
                               want_position: bool = False) -> Dict[str, Any]:
        """``compute_inliers`` over arrays: pair rows ``pair_images`` [E, 2] (i1 < i2) with world directions ``world_pair`` [E, 3], tracks as
        CSR (``track_off`` [T + 1], ``image`` [S]) with world directions ``world_meas`` [S, 3]; ``directions`` [D, 3] (default: sampled by the
        configured method from the measurements, pairs first). Returns host arrays ``pair_weight``, ``pair_inlier``, ``meas_weight``,
        ``meas_inlier``, ``camera_inlier``, ``directions``, ``counts`` (and ``position`` with ``want_position``)."""
        pairs = np.asarray(pair_images, np.int32).reshape(-1, 2)
        world_pair = np.asarray(world_pair, np.float64).reshape(-1, 3)
        track_off = np.zeros(1, np.int64) if track_off is None else np.asarray(track_off, np.int64)
        image = np.zeros(0, np.int32) if image is None else np.asarray(image, np.int32)
        world_meas = np.zeros((0, 3)) if world_meas is None else np.asarray(world_meas, np.float64).reshape(-1, 3)
        if len(pairs) and (pairs[:, 0] >= pairs[:, 1]).any():
            raise ValueError("incorrectly ordered pair: i1 < i2 is required")
        if num_images is None:
            num_images = int(max(pairs.max(initial=-1), image.max(initial=-1))) + 1
        if directions is None:
            directions = self.sample_projection_directions(np.concatenate([world_pair, world_meas]))
        directions = np.asarray(directions, np.float64).reshape(-1, 3)
        if len(pairs) + len(image) == 0:
            return {"pair_weight": np.zeros(0), "pair_inlier": np.zeros(0, np.uint8), "meas_weight": np.zeros(0), "meas_inlier": np.zeros(0, np.uint8),
                    "camera_inlier": np.zeros(num_images, np.uint8), "directions": directions, "counts": dict.fromkeys(_count_fields(), 0)}
        eng = self.engine()
        t = len(track_off) - 1
        dev = eng.upload(pairs, None, None, None, np.ones(num_images, np.uint8), None, track_off, image, None, np.ones(t, np.uint8), None, directions)
        out = eng.inliers(*dev, threshold=self._outlier_weight_threshold, world=eng.upload_world(world_pair, world_meas), want_position=want_position)
        res = {k: out[k].cpu().numpy() for k in ("pair_weight", "pair_inlier", "meas_weight", "meas_inlier", "camera_inlier")}
        res.update(directions=directions, counts=out["counts"])
        if want_position:
            res["position"] = out["position"].cpu().numpy()
        return res

    def recover_arrays(self, pair_images, world_pair, track_off=None, image=None, world_meas=None, pair_enable=None, meas_enable=None, num_images: Optional[int] = None,
                       anchor: int = -1, scale_factor: float = 1.0, **options) -> Dict[str, Any]:
        """``TranslationRecovery`` over arrays, beside ``compute_inliers_arrays``: the pair rows with their world directions, the tracks as CSR
        with theirs, the two masks (normally ``pair_inlier`` / ``meas_inlier``). Returns host arrays ``translation`` [N + T, 3] (cameras, then
        landmarks; NaN outside the anchor's component), ``node_valid``, and ``status``, ``counters``, ``costs``."""
        from gtsfm_amd.runtime.translation_recovery_engine import COST_FIELDS, COUNTER_FIELDS

        pairs = np.asarray(pair_images, np.int32).reshape(-1, 2)
        image = np.zeros(0, np.int32) if image is None else np.asarray(image, np.int32)
        if num_images is None:
            num_images = int(max(pairs.max(initial=-1), image.max(initial=-1))) + 1
        eng = recovery_engine(self._device)
        dev = eng.upload(pairs, world_pair, pair_enable, np.zeros(1, np.int64) if track_off is None else track_off, image, np.zeros((0, 3)) if world_meas is None else world_meas,
                         meas_enable)
        opts = dict(sigma=NOISE_MODEL_SIGMA, huber_k=HUBER_LOSS_K if self._robust_measurement_noise else 0.0)
        opts.update(getattr(self, "_recovery_options", {}), **options)
        out = eng.recover(*dev, num_images=num_images, anchor=anchor, scale_factor=scale_factor, **opts)
        return {"translation": out["translation"][0].cpu().numpy(), "node_valid": out["node_valid"][0].cpu().numpy(), "status": out["status"][0],
                "counters": dict(zip(COUNTER_FIELDS, (int(x) for x in out["counters"][0]))), "costs": dict(zip(COST_FIELDS, (float(x) for x in out["costs"][0])))}

    @staticmethod
    def _dicts_to_arrays(w_i2Ui1_dict: Dict[Pair, Any], w_iUj_dict_tracks: Dict[Pair, Any]):  # noqa: N803
        pair_keys, meas_keys = list(w_i2Ui1_dict), list(w_iUj_dict_tracks)
        world_pair = np.array([vector3(w_i2Ui1_dict[k]) for k in pair_keys]).reshape(-1, 3)
        order = sorted(range(len(meas_keys)), key=lambda k: meas_keys[k][0])  # stable: CSR by track id
        meas_keys = [meas_keys[k] for k in order]
        num_tracks = max((j for j, _ in meas_keys), default=-1) + 1
        track_off = np.zeros(num_tracks + 1, np.int64)
        for j, _ in meas_keys:
            track_off[j + 1] += 1
        track_off = np.cumsum(track_off)
        image = np.array([i for _, i in meas_keys], np.int32)
        world_meas = np.array([vector3(w_iUj_dict_tracks[k]) for k in meas_keys]).reshape(-1, 3)
        return pair_keys, meas_keys, np.asarray(pair_keys, np.int32).reshape(-1, 2), world_pair, track_off, image, world_meas

    def compute_inliers(self, w_i2Ui1_dict: Dict[Pair, Any], w_iUj_dict_tracks: Dict[Pair, Any]) -> Tuple[Dict[Pair, Any], Dict[Pair, Any], Set[int]]:  # noqa: N803
        """The inlier camera-camera measurements, the inlier camera-landmark measurements (of inlier cameras only) and the inlier cameras."""
        pair_keys, meas_keys, pairs, world_pair, track_off, image, world_meas = self._dicts_to_arrays(w_i2Ui1_dict, w_iUj_dict_tracks)
        # the reference samples from the measurements in dict order, pairs first
        combined = np.array([vector3(v) for v in list(w_i2Ui1_dict.values()) + list(w_iUj_dict_tracks.values())]).reshape(-1, 3)
        directions = self.sample_projection_directions(combined)
        res = self.compute_inliers_arrays(pairs, world_pair, track_off, image, world_meas, directions=directions)
        inlier_pairs = {k: w_i2Ui1_dict[k] for k, keep in zip(pair_keys, res["pair_inlier"].tolist()) if keep}
        inlier_cameras = {c for k in inlier_pairs for c in k}
        inlier_tracks = {k: w_iUj_dict_tracks[k] for k, keep in zip(meas_keys, res["meas_inlier"].tolist()) if keep}
        inlier_tracks = {k: w_iUj_dict_tracks[k] for k in w_iUj_dict_tracks if k in inlier_tracks}  # the input's order
        return inlier_pairs, inlier_tracks, inlier_cameras

    @staticmethod
    def run_mfas(w_i2Ui1_dict: Dict[Pair, Any], w_iUj_dict_tracks: Dict[Pair, Any], directions: Sequence[Any], device=None) -> List[Dict[Tuple[int, int], float]]:  # noqa: N803
        """MFAS on a batch of directions: per direction {(key1, key2): outlier weight} with gtsam's symbol keys (C(i2), C(i1)) / (C(i), L(j))."""
        self = TranslationAveraging1DSFM.__new__(TranslationAveraging1DSFM)
        self._device, self._engine, self._outlier_weight_threshold = device, None, OUTLIER_WEIGHT_THRESHOLD
        pair_keys, meas_keys, pairs, world_pair, track_off, image, world_meas = self._dicts_to_arrays(w_i2Ui1_dict, w_iUj_dict_tracks)
        dirs = np.array([vector3(d) for d in directions]).reshape(-1, 3)
        if len(dirs) == 0 or len(pairs) + len(image) == 0:
            return [{} for _ in dirs]
        num_images = int(max(pairs.max(initial=-1), image.max(initial=-1))) + 1
        res = self.compute_inliers_arrays(pairs, world_pair, track_off, image, world_meas, num_images=num_images, directions=dirs, want_position=True)
        track = np.repeat(np.arange(len(track_off) - 1), np.diff(track_off))
        key1 = np.concatenate([pairs[:, 1], image]).astype(np.int64)
        key2 = np.concatenate([pairs[:, 0], num_images + track]).astype(np.int64)
        m = np.concatenate([world_pair, world_meas])
        names = [(C(i2), C(i1)) for i1, i2 in pair_keys] + [(C(i), L(j)) for j, i in meas_keys]
        out = []
        for d, position in zip(dirs, res["position"]):
            w = (m[:, 0] * d[0] + m[:, 1] * d[1]) + m[:, 2] * d[2]
            forward = ~(w < 0)
            src, dst = np.where(forward, key1, key2), np.where(forward, key2, key1)
            weight = np.where(position[src] > position[dst], np.abs(w), 0.0)
            out.append({k: float(x) for k, x in zip(names, weight)})
        return out

    # ---- the whole stage ----

    def run_translation_averaging(self, num_images: int, i2Ui1_dict: Dict[Pair, Any], wRi_list: List[Any], tracks_2d: Optional[List[Any]] = None,  # noqa: N803
                                  intrinsics: Optional[List[Any]] = None, absolute_pose_priors: Sequence[Any] = (), i2Ti1_priors: Optional[Dict[Pair, Any]] = None,
                                  scale_factor: float = 1.0, gt_wTi_list: Sequence[Any] = ()):
        """World-frame measurements, track selection, landmark directions, outlier rejection on the device, then ``translation_recovery``
        (on the device too with ``translation_recovery="device"``). Returns (wTi_list, None, the inlier pairs); wTi is (wRi as a 3 x 3
        array, wti) or None. The metrics group is out of scope."""
        w_i2Ui1_dict, valid_cameras = get_valid_measurements_in_world_frame(i2Ui1_dict, wRi_list)
        if not self._use_relative_camera_poses:
            w_i2Ui1_dict = {}
        if self._use_tracks_for_averaging:
            if tracks_2d is None:
                raise ValueError("Tracks must be provided when they are to be used in translation averaging.")
            if intrinsics is None or len(intrinsics) != len(wRi_list):
                raise ValueError("Number of intrinsics must match number of cameras when tracks are provided.")
            selected = self._select_tracks_for_averaging(tracks_2d, valid_cameras, intrinsics)
            w_iUj_dict_tracks = self._get_landmark_directions(selected, intrinsics, wRi_list)
        else:
            w_iUj_dict_tracks = {}
        if self._reject_outliers:
            inlier_pairs, inlier_tracks, _ = self.compute_inliers(w_i2Ui1_dict, w_iUj_dict_tracks)
        else:
            inlier_pairs, inlier_tracks = w_i2Ui1_dict, w_iUj_dict_tracks
        extra = dict(device=self._device, **self._recovery_options) if self._translation_recovery is device_translation_recovery else {}
        wti_list = self._translation_recovery(num_images, inlier_pairs, inlier_tracks, wRi_list, i2Ti1_priors or {}, list(absolute_pose_priors), scale_factor,
                                              self._robust_measurement_noise, **extra)
        wTi_list = [(matrix3(r), np.asarray(t, np.float64).reshape(3)) if r is not None and t is not None else None for r, t in zip(wRi_list, wti_list)]  # noqa: N806
        return wTi_list, None, list(inlier_pairs.keys())


def _count_fields():
    from gtsfm_amd.runtime.translation_engine import COUNT_FIELDS

    return COUNT_FIELDS


ProjectionSamplingMethod = TranslationAveraging1DSFM.ProjectionSamplingMethod
