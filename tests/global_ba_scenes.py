"""The scenes of the global bundle adjustment tests: the smallest shapes at which the kernel can go wrong. Each is a dict of the arrays
``gtsfm_global_ba_f64`` takes (the camera table, the track CSR, the points, the two masks), ``anchor``, ``options``, the planted geometry
``truth`` (camera centres [N, 3] and points [T, 3]; NaN where there is none) and ``check``, which says on the restatement's result that the
scene holds what it is named for. Every scene is built with a fixed seed, and ``expected`` asserts that no reprojection error of the
restatement lies within 1e-6 px of the scene's threshold, so that no track may be excused."""

import functools

import numpy as np

from tests import global_ba_reference as ref


def look_at(centre, target, roll_deg=0.0):
    z = np.asarray(target, np.float64) - centre
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    c, s = np.cos(np.deg2rad(roll_deg)), np.sin(np.deg2rad(roll_deg))
    return np.stack([x, np.cross(z, x), z], axis=1) @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def small_rotation(rng, sigma_rad):
    w = rng.normal(0.0, sigma_rad, 3)
    k = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    u, _, vt = np.linalg.svd(np.eye(3) + k + 0.5 * k @ k)
    return u @ vt


def geometry(n_cam, n_pts, seed, cam_seed=0, focal=(800.0, 800.0), unit=1.0):
    """Cameras on an arc ten units from a slab of points (``unit`` scales the world), looking at it."""
    rng = np.random.default_rng(5000 + cam_seed)
    ang = np.linspace(-0.6, 0.6, n_cam) if n_cam > 1 else np.zeros(1)
    centre = np.stack([10.0 * np.sin(ang), rng.uniform(-1.0, 1.0, n_cam), 10.0 - 10.0 * np.cos(ang) + rng.uniform(-0.5, 0.5, n_cam)], 1)
    rot = np.stack([look_at(centre[i], [rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 10.0], rng.uniform(-5.0, 5.0)) for i in range(n_cam)])
    intr = np.stack([np.full(n_cam, focal[0]) + 10.0 * np.arange(n_cam), np.full(n_cam, focal[1]) + 10.0 * np.arange(n_cam), 320.0 + 2.0 * np.arange(n_cam),
                     240.0 - np.arange(n_cam)], 1)
    prng = np.random.default_rng(6000 + seed)
    points = np.stack([prng.uniform(-3.0, 3.0, n_pts), prng.uniform(-2.0, 2.0, n_pts), prng.uniform(8.5, 11.5, n_pts)], 1)
    return intr, rot, centre * unit, points * unit


def project(intr, rot, centre, x):
    q = (x - centre) @ rot
    return np.stack([intr[0] * q[:, 0] / q[:, 2] + intr[2], intr[1] * q[:, 1] / q[:, 2] + intr[3]], 1)


def converged(r):
    return r["counters"]["status"] == ref.CONVERGED


def status_is(status, **counters):
    return lambda r: r["counters"]["status"] == status and all(r["counters"][k] == v for k, v in counters.items())


def scene(name, intr, rot, centre, points, views, seed, noise=0.0, start=(0.01, 0.05, 0.05), unit=1.0, options=None, anchor=-1, check=None, outliers=0,
          outlier_px=40.0):
    """``views``: per point the cameras that see it. ``start``: the perturbation of the start (radians, camera centres, points; the last two in
    ``unit``). ``outliers``: that many tracks get one measurement moved by ``outlier_px``."""
    rng = np.random.default_rng(7000 + seed)
    n_cam, n_pts = len(intr), len(points)
    track_off = np.concatenate([[0], np.cumsum([len(v) for v in views])]).astype(np.int64)
    image = np.asarray([c for v in views for c in v], np.int32)
    track = np.repeat(np.arange(n_pts), [len(v) for v in views])
    uv = np.zeros((len(image), 2))
    for i in range(n_cam):
        at = image == i
        if at.any():
            uv[at] = project(intr[i], rot[i], centre[i], points[track[at]])
    uv = uv + rng.normal(0.0, 1.0, uv.shape) * noise
    outlier_tracks = np.sort(rng.choice(n_pts, outliers, replace=False)) if outliers else np.zeros(0, np.int64)
    for j in outlier_tracks:
        ang = rng.uniform(0.0, 2.0 * np.pi)
        uv[track_off[j] + rng.integers(0, len(views[j]))] += outlier_px * np.array([np.cos(ang), np.sin(ang)])
    cameras = np.zeros((n_cam, 17))
    cameras[:, 0], cameras[:, 1:5] = 1.0, intr
    for i in range(n_cam):
        cameras[i, 5:14] = (rot[i] @ small_rotation(rng, start[0])).reshape(-1)
        cameras[i, 14:17] = centre[i] + rng.normal(0.0, start[1] * unit, 3)
    point = points + rng.normal(0.0, start[2] * unit, points.shape)
    return {"name": name, "cameras": cameras, "track_off": track_off, "image": image, "uv": uv.astype(np.float32), "point": point, "track_enable": None, "meas_enable": None,
            "anchor": anchor, "options": dict(options or {}), "truth": (centre.copy(), points.copy()), "outlier_tracks": outlier_tracks, "check": check or converged}


def planted(name, n_cam, n_pts, seed, per_point=0, cam_seed=0, focal=(800.0, 800.0), unit=1.0, **kw):
    """Every point is seen by ``per_point`` cameras (0: by all)."""
    intr, rot, centre, points = geometry(n_cam, n_pts, seed, cam_seed, focal, unit)
    rng = np.random.default_rng(8000 + seed)
    if per_point:
        views = [sorted(((j + np.arange(per_point)) % n_cam).tolist()) if j < n_cam else sorted(rng.choice(n_cam, per_point, replace=False).tolist()) for j in range(n_pts)]
    else:
        views = [list(range(n_cam))] * n_pts
    return scene(name, intr, rot, centre, points, views, seed, unit=unit, **kw)


def recovered(r, sc, tol):
    """The planted geometry up to a similarity: cameras' centres and points together."""
    centre, points = sc["truth"]
    got = np.concatenate([r["cameras"][:, 14:17], r["point"]])
    want = np.concatenate([centre, points])
    on = np.concatenate([r["node_valid"][:len(centre)], r["node_valid"][len(centre):]]) != 0
    fit, _, _ = ref.fit_similarity(np.where(on[:, None], got, np.nan), want)
    return float(np.nanmax(np.linalg.norm(fit - want, axis=1))) < tol


def rejected(r):
    return sum(1 for e in r["log"] if not e["accepted"])


@functools.lru_cache(maxsize=None)
def all_scenes():
    s = []
    s.append(planted("two_cameras_eight_points", 2, 8, 1, noise=0.3, check=lambda r: converged(r) and r["counters"]["cameras"] == 2 and r["counters"]["points"] == 8))
    sc = planted("planted_noise_free", 6, 40, 2)
    sc["check"] = lambda r, sc=sc: converged(r) and r["costs"]["final_cost"] < 1e-6 and recovered(r, sc, 1e-5)
    s.append(sc)
    from tests import multi_view_scene as mv

    g = mv.planted_scene()
    sc = scene("planted_noise", g["intrinsics"], g["wRi"], g["centre"], g["points"], [list(range(mv.NUM_IMAGES))] * mv.NUM_POINTS, 3, noise=mv.NOISE_PX)
    sc["check"] = lambda r, sc=sc: (converged(r) and r["counters"]["cameras"] == 10 and r["counters"]["points"] == 260 and int((r["graph"].node == 0).sum()) > 256
                                    and recovered(r, sc, 0.05) and r["track_valid"].all())
    s.append(sc)
    # 5 % gross outliers: both Huber branches, the outlier tracks fail the filter, every inlier track passes
    sc = planted("outliers_huber", 8, 60, 4, noise=0.3, outliers=3)

    def huber_check(r, sc=sc):
        bad = np.zeros(60, bool)
        bad[sc["outlier_tracks"]] = True
        w = r["initial_weights"]
        return converged(r) and (w < 1).any() and (w == 1).any() and not r["track_valid"][bad].any() and r["track_valid"][~bad].all() and r["camera_kept"].all()

    sc["check"] = huber_check
    s.append(sc)
    s.append(dict(sc, name="outliers_no_huber", options={"huber_k": np.inf}, check=lambda r: converged(r) and (r["initial_weights"] == 1).all()))
    # lane ownership and tree padding: 255 / 256 / 257 compact nodes, cut after three accepted steps
    for pts in (250, 251, 252):
        s.append(planted(f"nodes{5 + pts}", 5, pts, 5, per_point=3, noise=0.3, options={"max_iterations": 3},
                         check=lambda r, pts=pts: r["counters"]["cameras"] + r["counters"]["points"] == 5 + pts and r["counters"]["accepted_steps"] == 3))
    # a track seen by every camera beside tracks of two
    intr, rot, centre, points = geometry(8, 30, 6)
    views = [list(range(8))] + [sorted([j % 8, (j + 1) % 8]) for j in range(29)]
    s.append(scene("long_track", intr, rot, centre, points, views, 6, noise=0.3,
                   check=lambda r: converged(r) and int((r["graph"].node == 8).sum()) == 8 and int((r["graph"].node == 9).sum()) == 2))
    # invalid and partial data
    intr, rot, centre, points = geometry(7, 30, 7)
    base = scene("gaps", intr, rot, centre, points, [list(range(7))] * 30, 7, noise=0.3)
    ids = np.asarray([3 * k + 2 for k in range(7)], np.int32)
    cams = np.zeros((24, 17))
    cams[ids] = base["cameras"]
    cams[4, :], cams[4, 0] = base["cameras"][1], 0.0  # not estimated, and measurements name it
    image = ids[base["image"]]
    image[[5, 40]] = 4
    image[12], image[50] = 99, -1  # outside the table: not estimated, not refused
    track_enable = np.ones(30, np.uint8)
    track_enable[[3, 17]] = 0
    point = base["point"].copy()
    point[9, 1] = np.nan
    meas_enable = np.ones(len(image), np.uint8)
    meas_enable[[0, 30, 31]] = 0
    meas_enable[7 * 20 + 1:7 * 21] = 0  # track 20 is left with one valid measurement
    uv = base["uv"].copy()
    uv[66, 0] = np.nan
    truth_c = np.full((24, 3), np.nan)
    truth_c[ids] = base["truth"][0]
    s.append(dict(base, cameras=cams, image=image, track_enable=track_enable, point=point, meas_enable=meas_enable, uv=uv, truth=(truth_c, base["truth"][1]),
                  check=lambda r: (converged(r) and r["counters"]["anchor"] == 2 and r["counters"]["cameras"] == 7 and r["counters"]["points"] == 30 - 4
                                   and r["counters"]["valid_measurements"] == 7 * 26 - 4 - 3 and not r["node_valid"][24 + 20] and np.isnan(r["reproj_error"][[5, 12, 50, 66]]).all())))
    intr, rot, centre, points = geometry(9, 40, 8)
    views = [[0, 1, 2, 3, 4]] * 22 + [[5, 6, 7, 8]] * 18
    sc = scene("two_components_anchor", intr, rot, centre, points, views, 8, noise=0.3, anchor=6)
    sc["check"] = lambda r, sc=sc: (converged(r) and r["node_valid"].tolist() == [0] * 5 + [1] * 4 + [0] * 22 + [1] * 18 and r["cameras"][:5].tobytes() == sc["cameras"][:5].tobytes()
                                    and r["point"][:22].tobytes() == sc["point"][:22].tobytes() and not r["track_valid"][:22].any() and np.isnan(r["reproj_error"][:110]).all())
    s.append(sc)
    s.append(dict(sc, name="two_components", anchor=-1, check=lambda r: converged(r) and r["counters"]["anchor"] == 0 and r["node_valid"].tolist() == [1] * 5 + [0] * 4 + [1] * 22 + [0] * 18))
    intr, rot, centre, points = geometry(5, 20, 9)
    sc = scene("camera_without_tracks", intr, rot, centre, points, [[0, 1, 3, 4]] * 20, 9, noise=0.3)
    sc["check"] = lambda r, sc=sc: converged(r) and r["node_valid"][:5].tolist() == [1, 1, 0, 1, 1] and r["cameras"][2].tobytes() == sc["cameras"][2].tobytes() and not r["camera_kept"][2]
    s.append(sc)
    sc = scene("empty", intr, rot, centre, np.zeros((0, 3)), [], 9)
    sc["check"] = lambda r, sc=sc: r["counters"]["status"] == ref.NO_VALID_ROW and r["cameras"].tobytes() == sc["cameras"].tobytes() and not r["node_valid"].any()
    s.append(sc)
    sc = planted("anchor_without_measurement", 5, 20, 9, per_point=3, anchor=2)
    sc["meas_enable"] = (sc["image"] != 2).astype(np.uint8)
    sc["check"] = status_is(ref.NO_VALID_ROW, anchor=2)
    s.append(sc)
    sc = planted("non_finite", 4, 12, 10, noise=0.3)
    sc["cameras"][1, 1] = np.nan  # a focal length: a NaN pose would count as a point behind the camera
    sc["check"] = lambda r, sc=sc: r["counters"]["status"] == ref.NON_FINITE and r["cameras"].tobytes() == sc["cameras"].tobytes() and not r["track_valid"].any() and not r["node_valid"].any()
    s.append(sc)
    # cheirality: a point that starts behind one of its cameras
    sc = planted("behind_camera", 5, 24, 11, noise=0.3)
    c0 = sc["cameras"][4]
    sc["point"][7] = c0[14:17] - 0.5 * c0[5:14].reshape(3, 3)[:, 2]
    sc["check"] = lambda r: r["counters"]["status"] != ref.NON_FINITE and r["initial_behind"] >= 1 and r["costs"]["final_cost"] < r["costs"]["init_cost"]
    s.append(sc)
    # every branch of the outer and inner loop
    far = dict(noise=0.3, start=(0.3, 2.0, 2.0))
    s.append(planted("rejected_steps", 6, 40, 12, check=lambda r: converged(r) and rejected(r) >= 3 and max(e["lambda"] for e in r["log"]) > 1e-4, **far))
    for k in (1, 2, 3, 5):  # the fifth accepted step comes after seven rejected trials
        s.append(planted(f"max_iterations_{k}", 6, 40, 12, options={"max_iterations": k}, check=status_is(ref.MAX_ITERATIONS, accepted_steps=k), **far))
    s.append(planted("lambda_bound", 4, 16, 13, noise=0.3, options={"measurement_sigma": 1e-160},
                     check=lambda r: r["counters"]["status"] == ref.LAMBDA_BOUND and r["counters"]["accepted_steps"] == 0 and r["counters"]["solves_tried"] == 11 and np.isinf(r["costs"]["init_cost"])))
    s.append(planted("cg_cap", 6, 40, 14, noise=0.3, options={"max_inner": 2},
                     check=lambda r: r["counters"]["status"] in (ref.CONVERGED, ref.MAX_ITERATIONS) and any(e["accepted"] and e["cg"] == 2 for e in r["log"]) and all(e["cg"] <= 2 for e in r["log"])))
    s.append(planted("cg_forcing_zero", 4, 16, 15, noise=0.3, options={"cg_forcing": 0.0, "max_inner": 60}, check=lambda r: converged(r) and all(e["cg"] > 2 for e in r["log"])))
    # calibration and scale
    s.append(planted("anisotropic", 5, 30, 16, noise=0.3, focal=(700.0, 1100.0)))
    s.append(planted("focal_3000", 5, 30, 17, noise=0.3, focal=(3000.0, 3000.0)))
    s.append(planted("unit_1e-3", 5, 30, 18, noise=0.3, unit=1e-3))
    s.append(planted("unit_1e3", 5, 30, 19, noise=0.3, unit=1e3))
    # the filter: tracks with errors on both sides of 10 / 5 / 3 px
    for thr in (10.0, 5.0, 3.0):
        s.append(planted(f"threshold_{thr:g}", 6, 50, 20, noise=2.2, outliers=6, outlier_px=12.0, options={"reproj_error_threshold": thr},
                         check=lambda r: r["counters"]["status"] in (ref.CONVERGED, ref.MAX_ITERATIONS) and r["track_valid"].any() and not r["track_valid"].all()))
    names = [x["name"] for x in s]
    assert len(set(names)) == len(names)
    return s


SCENE_NAMES = tuple(x["name"] for x in all_scenes())
SMALL = ("two_cameras_eight_points", "planted_noise_free", "outliers_huber", "long_track", "anisotropic")  # what the arbiter runs on
ARRAYS = ("cameras", "track_off", "image", "uv", "point", "track_enable", "meas_enable")


def get(name):
    return next(x for x in all_scenes() if x["name"] == name)


def arrays_of(sc):
    return tuple(sc[k] for k in ARRAYS)


def options_of(sc):
    return dict(ref.DEFAULTS, **sc["options"])


def solve(sc, **override):
    opts = dict(sc["options"], **override)
    anchor = opts.pop("anchor", sc["anchor"])
    return ref.solve(*arrays_of(sc), anchor=anchor, **opts)


@functools.lru_cache(maxsize=None)
def expected(name):
    sc = get(name)
    r = solve(sc)
    thr = options_of(sc)["reproj_error_threshold"]
    assert ref.filter_margin(r, thr) > ref.FILTER_MARGIN_PX, f"{name}: a reprojection error within {ref.FILTER_MARGIN_PX} px of {thr}"
    return r


def permuted(sc, seed=5):
    """The same problem with each track's measurements in another order."""
    rng = np.random.default_rng(seed)
    perm = np.concatenate([lo + rng.permutation(hi - lo) for lo, hi in zip(sc["track_off"][:-1], sc["track_off"][1:])]).astype(np.int64)
    take = lambda x: None if x is None else x[perm]  # noqa: E731
    return dict(sc, image=sc["image"][perm], uv=sc["uv"][perm], meas_enable=take(sc["meas_enable"]))


@functools.lru_cache(maxsize=None)
def batch():
    """Three problems over ranges of one set of arrays and one camera table: (arrays, problem_off [4], the parts)."""
    parts = [planted("batch0", 6, 40, 21, noise=0.3), planted("batch1", 6, 25, 22, per_point=3, noise=0.3), planted("batch2", 6, 33, 23, noise=0.3, outliers=2)]
    parts[1]["meas_enable"] = np.ones(len(parts[1]["image"]), np.uint8)
    parts[1]["meas_enable"][[4, 9]] = 0
    cams = parts[0]["cameras"]
    parts = [dict(x, cameras=cams) for x in parts]
    cat = lambda k: np.concatenate([x[k] for x in parts])  # noqa: E731
    track_off = np.concatenate([[0]] + [x["track_off"][1:] + sum(len(y["image"]) for y in parts[:i]) for i, x in enumerate(parts)]).astype(np.int64)
    meas_enable = np.concatenate([np.ones(len(x["image"]), np.uint8) if x["meas_enable"] is None else x["meas_enable"] for x in parts])
    off = np.concatenate([[0], np.cumsum([len(x["point"]) for x in parts])]).astype(np.int64)
    return (cams, track_off, cat("image"), cat("uv"), cat("point"), None, meas_enable), off, parts
