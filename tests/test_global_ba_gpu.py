"""GPU: ``gtsfm_global_ba_f64`` on every scene of tests/global_ba_scenes.py against the restatement (tests/global_ba_reference.py). The stage
is float64 + - * / sqrt in one stated order, so the device's cameras, points, reprojection errors, masks, counters and costs are ASSERTED
to be the restatement's bytes on every scene: that is the contract the documents state. Equal bytes run to run, alone against batched
(P = 3) and under a permutation of each track's measurements; inputs untouched; offsets that are not ascending refused with nothing
written; a short workspace is GTSFM_ERR_WORKSPACE; the drop-in entry points agree with the engine and raise for what is not restated.
``-s`` prints the lines of profiles/global_ba_gpu_tests.txt. Were float64 sqrt or / not correctly rounded on the device, the byte
assertions here would fail: that is a finding to report, not a tolerance to widen."""

import pickle

import numpy as np
import pytest

from tests import global_ba_reference as ref
from tests import global_ba_scenes as scenes

pytestmark = pytest.mark.gpu

KEYS = ("cameras", "point", "reproj_error", "track_valid", "camera_kept", "node_valid", "counters", "costs")


@pytest.fixture(scope="module")
def engine(gpu_device):
    from gtsfm_amd.runtime.global_ba_engine import GlobalBAEngine

    return GlobalBAEngine(gpu_device)


def host(out, p=0):
    res = {k: out[k].cpu().numpy() for k in ("point", "reproj_error", "track_valid")}
    res.update({k: out[k][p].cpu().numpy() for k in ("cameras", "camera_kept", "node_valid")})
    res.update(counters=out["counters"][p], costs=out["costs"][p])
    return res


def run_device(engine, sc, **override):
    opts = dict(sc["options"], **override)
    anchor = opts.pop("anchor", sc["anchor"])
    dev = engine.upload(*scenes.arrays_of(sc))
    keep = [None if t is None else t.clone() for t in dev]
    out = engine.adjust(*dev, anchor=anchor, **opts)
    for before, after in zip(keep, dev):
        assert before is None or before.cpu().numpy().tobytes() == after.cpu().numpy().tobytes(), "an input was changed"
    return host(out)


def same_bytes(a, b, keys=KEYS):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


def restated(want):
    return {**{k: want[k] for k in KEYS[:6]}, "counters": np.array([want["counters"][k] for k in ref.COUNTER_FIELDS], np.int32),
            "costs": np.array([want["costs"][k] for k in ref.COST_FIELDS], np.float64)}


@pytest.mark.parametrize("name", scenes.SCENE_NAMES)
def test_device_bytes_are_the_restatements(engine, name):
    sc, want = scenes.get(name), scenes.expected(name)
    assert sc["check"](want), "the scene does not contain what it is named for"
    got = run_device(engine, sc)
    c = dict(zip(ref.COUNTER_FIELDS, (int(x) for x in got["counters"])))
    w = restated(want)
    equal = {k: np.asarray(got[k]).tobytes() == np.asarray(w[k]).tobytes() for k in KEYS}
    with np.errstate(invalid="ignore"):
        far = float(np.nanmax(np.abs(got["point"] - want["point"]), initial=0.0))
    print(f"\nglobal_ba {name}: status {ref.STATUS_NAMES[c['status']]} cameras {c['cameras']} points {c['points']} measurements {c['valid_measurements']} accepted {c['accepted_steps']} "
          f"solves {c['solves_tried']} cg {c['cg_iterations']} cost {got['costs'][0]:.6e} -> {got['costs'][1]:.6e} |g|_inf {got['costs'][2]:.3e} lambda {got['costs'][3]:.0e} "
          f"kept {int(got['track_valid'].sum())}/{len(got['track_valid'])} | device-restatement {far:.3e}, bytes equal {equal}")
    assert all(equal.values()), equal
    assert same_bytes(got, run_device(engine, sc)), "two runs differ"


def test_batch_equals_alone(engine):
    """P = 3 over ranges of the same arrays: every problem gives the bytes it gives alone, and the restatement's."""
    arrays, off, parts = scenes.batch()
    out = engine.adjust(*engine.upload(*arrays), problem_off=off)
    for p, sc in enumerate(parts):
        tlo, thi = int(off[p]), int(off[p + 1])
        mlo, mhi = int(arrays[1][tlo]), int(arrays[1][thi])
        alone = run_device(engine, dict(sc, options={}, anchor=-1))
        inside = host(out, p)
        m = len(alone["node_valid"])
        inside.update(point=inside["point"][tlo:thi], reproj_error=inside["reproj_error"][mlo:mhi], track_valid=inside["track_valid"][tlo:thi])
        assert not inside["node_valid"][m:].any()
        inside["node_valid"] = inside["node_valid"][:m]
        assert same_bytes(alone, inside), f"problem {p}"
        assert same_bytes(alone, restated(ref.solve(arrays[0], *ref.problem_arrays(*arrays[1:], off, p)))), f"problem {p} against the restatement"


@pytest.mark.parametrize("name", ["planted_noise", "gaps", "long_track", "outliers_huber"])
def test_measurement_permutation(engine, name):
    """The order of a track's measurements changes no byte but the places of the reprojection errors."""
    sc = scenes.get(name)
    moved = scenes.permuted(sc)
    a, b = run_device(engine, sc), run_device(engine, moved)
    assert same_bytes(a, b, [k for k in KEYS if k != "reproj_error"])
    key = lambda x, e: sorted(zip(np.repeat(np.arange(len(x["track_off"]) - 1), np.diff(x["track_off"])).tolist(), x["image"].tolist(), e.view(np.int64).tolist()))  # noqa: E731
    assert key(sc, a["reproj_error"]) == key(moved, b["reproj_error"])


def raw_call(engine, arrays, problem_off, ws_bytes=None, anchor=-1, max_tracks=None, **override):
    """The C call with outputs filled with 7: (rc, outputs untouched, the error text)."""
    import torch

    from gtsfm_amd.runtime import lib as L

    dev = engine.upload(*arrays)
    n, t, s = len(arrays[0]), len(arrays[1]) - 1, len(arrays[2])
    off = np.asarray(problem_off, np.int64).reshape(-1)
    p = len(off) - 1
    t_max = min(max(int(np.diff(off).max()), 0), t) if max_tracks is None else max_tracks
    off_dev = torch.from_numpy(off).to(engine.device)
    lib = L.load()
    need = int(lib.gtsfm_global_ba_workspace_bytes(s, n, t, t_max, p))
    ws = torch.zeros((need if ws_bytes is None else ws_bytes) + 256, dtype=torch.uint8, device=engine.device)
    full = lambda shape, dt: torch.full(shape, 7, dtype=dt, device=engine.device)  # noqa: E731
    outs = [full((p, n, 17), torch.float64), full((t, 3), torch.float64), full((s,), torch.float64), full((t,), torch.uint8), full((p, n), torch.uint8),
            full((p, n + t_max), torch.uint8), full((p, 8), torch.int32), full((p, 4), torch.float64)]
    o = dict(ref.DEFAULTS, **override)
    rc = lib.gtsfm_global_ba_f64(dev[0].data_ptr(), n, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(), None, None, t, s, off_dev.data_ptr(), p, t_max, anchor,
                                 o["min_track_length"], o["measurement_sigma"], o["huber_k"], o["reproj_error_threshold"], o["rel_tol"], o["abs_tol"], o["cg_forcing"], o["max_iterations"],
                                 o["max_inner"], ws.data_ptr(), need if ws_bytes is None else ws_bytes, *[x.data_ptr() for x in outs], torch.cuda.current_stream(engine.device).cuda_stream)
    torch.cuda.synchronize()
    return rc, all(bool((x == 7).all()) for x in outs), lib.gtsfm_last_error()


@pytest.mark.parametrize("case", ["track_offsets", "track_total", "track_first", "problem_offsets", "problem_total", "problem_tracks", "anchor", "sigma", "threshold"])
def test_invalid_input_is_refused_with_nothing_written(engine, case):
    sc = scenes.get("two_cameras_eight_points")
    arrays = list(scenes.arrays_of(sc))
    off = {"track_offsets": [0, 2, 6, 4, 8, 10, 12, 14, 16], "track_total": [0, 2, 4, 6, 8, 10, 12, 14, 15], "track_first": [1, 2, 4, 6, 8, 10, 12, 14, 16]}.get(case)
    if off is not None:
        arrays[1] = np.asarray(off, np.int64)
    problem_off = {"problem_offsets": [0, 5, 3, 8], "problem_total": [0, 4, 7], "problem_tracks": [0, 2, 8]}.get(case, [0, 8])
    extra = {"sigma": {"measurement_sigma": 0.0}, "threshold": {"reproj_error_threshold": 0.0}}.get(case, {})
    rc, untouched, err = raw_call(engine, tuple(arrays), problem_off, anchor=5 if case == "anchor" else -1, max_tracks=3 if case == "problem_tracks" else None, **extra)
    assert rc == -1 and err
    assert untouched, "an output was written"


def test_short_workspace(engine):
    from gtsfm_amd.runtime import lib as L

    sc = scenes.get("two_cameras_eight_points")
    arrays = scenes.arrays_of(sc)
    need = int(L.load().gtsfm_global_ba_workspace_bytes(16, 2, 8, 8, 1))
    assert need > 0 and int(L.load().gtsfm_global_ba_workspace_bytes(16, 2, 8, 9, 1)) == 0 and int(L.load().gtsfm_global_ba_workspace_bytes(-1, 2, 8, 8, 1)) == 0
    rc, untouched, err = raw_call(engine, arrays, [0, 8], ws_bytes=need - 1)
    assert rc == -3 and untouched and b"workspace" in err
    rc, untouched, _ = raw_call(engine, arrays, [0, 8], ws_bytes=need)
    assert rc == 0 and not untouched


def test_drop_in_agrees_with_the_engine(engine, gpu_device):
    """``run_ba_arrays`` and ``run_ba`` (cameras and SfmTracks in, optimised and filtered data out) give the engine's bytes; the object pickles."""
    from gtsfm_amd.bundle.bundle_adjustment import BundleAdjustmentOptimizer, RobustBAMode
    from gtsfm_amd.bundle.global_ba import GlobalBundleAdjustment
    from gtsfm_amd.common.calibration import PinholeCamera, PinholeIntrinsics
    from gtsfm_amd.data_association.point3d_initializer import SfmTrack

    sc = scenes.get("outliers_huber")
    got = run_device(engine, sc, reproj_error_threshold=3.0)
    obj = GlobalBundleAdjustment(reproj_error_thresholds=[10, 5, 3], robust_ba_mode="HUBER", measurement_noise_sigma=1.0, device=gpu_device)
    assert isinstance(obj, BundleAdjustmentOptimizer) and obj._robust_ba_mode is RobustBAMode.HUBER
    obj = pickle.loads(pickle.dumps(obj))
    res = obj.run_ba_arrays(*scenes.arrays_of(sc))
    assert same_bytes(got, res)
    assert pickle.loads(pickle.dumps(obj))._engine is None
    cams = {i: PinholeCamera(row[5:14].reshape(3, 3), row[14:17], PinholeIntrinsics(row[1], row[3], row[4], row[2])) for i, row in enumerate(sc["cameras"])}
    tracks = []
    for j in range(len(sc["point"])):
        t = SfmTrack(sc["point"][j])
        for s in range(int(sc["track_off"][j]), int(sc["track_off"][j + 1])):
            t.addMeasurement(int(sc["image"][s]), sc["uv"][s])
        tracks.append(t)
    (opt_cams, opt_tracks), (kept_cams, kept_tracks), mask = obj.run_ba(cams, tracks)
    assert np.stack([t.point3() for t in opt_tracks]).tobytes() == got["point"].tobytes()
    assert np.stack([np.asarray(opt_cams[i].pose().rotation().matrix()).reshape(9) for i in range(len(cams))]).tobytes() == np.ascontiguousarray(got["cameras"][:, 5:14]).tobytes()
    assert np.stack([np.asarray(opt_cams[i].pose().translation()).reshape(3) for i in range(len(cams))]).tobytes() == np.ascontiguousarray(got["cameras"][:, 14:17]).tobytes()
    assert mask == [bool(v) for v in got["track_valid"]] and len(kept_tracks) == int(got["track_valid"].sum()) and sorted(kept_cams) == list(range(len(cams)))
    assert all(t.numberMeasurements() == 8 for t in kept_tracks)
    none = BundleAdjustmentOptimizer(reproj_error_thresholds=[None], device=gpu_device)  # RobustBAMode.NONE, no filter
    res = none.run_ba_arrays(*scenes.arrays_of(sc))
    assert same_bytes(run_device(engine, sc, huber_k=np.inf, reproj_error_threshold=np.inf, measurement_sigma=2.0), res)


def test_what_is_not_restated_raises():
    from gtsfm_amd.bundle.bundle_adjustment import BundleAdjustmentOptimizer, RobustBAMode
    from gtsfm_amd.common.calibration import PinholeCamera, PinholeIntrinsics

    for kw, word in (({"robust_ba_mode": RobustBAMode.GMC}, "robust_ba_mode"), ({"robust_ba_mode": "TLS"}, "robust_ba_mode"), ({"use_gnc": True}, "use_gnc"),
                     ({"shared_calib": True}, "shared_calib"), ({"use_pose_prior": True}, "use_pose_prior"), ({"use_first_point_prior": True}, "use_first_point_prior")):
        with pytest.raises(NotImplementedError, match=word):
            BundleAdjustmentOptimizer(**kw)
    obj = BundleAdjustmentOptimizer(use_karcher_mean_factor=True, use_calibration_prior=False, ordering_type="COLAMD", print_summary=True)  # accepted and ignored
    cams = {0: PinholeCamera(np.eye(3), np.zeros(3), PinholeIntrinsics(500.0, 10.0, 10.0))}
    with pytest.raises(NotImplementedError, match="relative_pose_priors"):
        obj.run_ba(cams, [], relative_pose_priors={(0, 1): object()})
    with pytest.raises(NotImplementedError, match="absolute_pose_priors"):
        obj.run_ba(cams, [], absolute_pose_priors=[object()])

    class Fisheye:
        def K(self):  # noqa: N802
            return np.eye(3)

    class Cam:
        def calibration(self):
            return Fisheye()

    with pytest.raises(NotImplementedError, match="Fisheye"):
        obj.run_ba({0: Cam()}, [])
