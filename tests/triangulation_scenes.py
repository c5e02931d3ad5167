"""Seeded synthetic scenes for the triangulation tests: the smallest shapes at which the kernels take another path."""

from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from tests import triangulation_reference as ref

NUM_CAMERAS = 80
INVALID = (3, 7)  # images without an estimated camera
LOOSE = dict(threshold=10.0, num_hypotheses=100)


def cameras(seed: int = 5) -> np.ndarray:
    rng = np.random.default_rng(seed)
    table = np.zeros((NUM_CAMERAS + 2, 17))  # two more rows than cameras: images 80 and 81 exist but have no estimate
    for i in range(NUM_CAMERAS):
        th = 2.0 * np.pi * i / NUM_CAMERAS * 0.6
        eye = np.array([10.0 * np.cos(th), 10.0 * np.sin(th), 0.0]) + rng.normal(0.0, 0.3, 3)
        table[i] = ref.lookat_camera(eye, rng.normal(0.0, 0.3, 3), [0.0, 0.0, 1.0], 800.0 + 3.0 * i, 640.0, 480.0)
        table[i, 2] = table[i, 1] * 1.01  # fy != fx
    for i in INVALID:
        table[i, 0] = 0.0
    return table


def _measure(table: np.ndarray, image: int, x: np.ndarray, rng, noise: float = 0.5) -> np.ndarray:
    u, v, _ = ref.project(table[image], x)
    return np.array([u, v]) + rng.normal(0.0, noise, 2)


def small_shapes(seed: int = 11) -> Dict[str, np.ndarray]:
    """CSR tracks: lengths 0, 1, 2, 3, 14, 15 and 75 (1, 3, 91 hypotheses; 105 > 100 and 2 775 > 2 749 pairs exercise the sampler), a
    first measurement without a camera, no camera at all, an image index outside the table, two measurements in one image, outliers,
    crossed measurements (a point behind the cameras), and short filler tracks up to a count that is no multiple of the 256 tracks of
    a workgroup; the hypothesis segments of the long tracks straddle wave and workgroup boundaries."""
    rng = np.random.default_rng(seed)
    table = cameras()
    valid = [i for i in range(NUM_CAMERAS) if i not in INVALID]
    tracks: List[List[Tuple[int, np.ndarray]]] = []

    def track(images, outliers=(), noise=0.5):
        x = rng.uniform(-2.0, 2.0, 3)
        meas = [(int(i), _measure(table, int(i), x, rng, noise) if table[int(i), 0] else rng.uniform(0.0, 900.0, 2)) for i in images]
        for k in outliers:
            meas[k] = (meas[k][0], meas[k][1] + rng.choice([-1.0, 1.0], 2) * rng.uniform(40.0, 80.0, 2))
        tracks.append(meas)

    for n in (2, 3, 14, 15, 14, 15, 3, 2):
        track(sorted(rng.choice(valid, n, replace=False)))
    track(sorted(rng.choice(valid, 15, replace=False)), outliers=(4,))
    track(sorted(rng.choice(valid, 14, replace=False)), outliers=(0, 13))
    track(sorted(rng.choice(valid, 6, replace=False)), outliers=(2,))
    track([3, 10, 20, 30])            # the first measurement's camera is not estimated
    track([3, 7])                     # no camera at all
    track([3, 12])                    # one camera: POSES_UNDERCONSTRAINED without RANSAC
    track([5, 81, 40])                # an image beyond the cameras that exist
    track([9, 30, 9, 50])             # two measurements in one image
    tracks.append([])                 # an empty track
    track([15])                       # a single measurement
    track([20, 21])                   # crossed: each camera gets the other's pixel, the rays meet behind the cameras
    tracks[-1] = [(20, tracks[-1][1][1]), (21, tracks[-1][0][1])]
    track([40, 41], noise=0.0)        # neighbours: a small triangulation angle
    track([0, 79], noise=0.0)         # the ends of the arc: a large one
    track([i for i in range(78) if i not in INVALID][:75], outliers=(10, 50))
    while len(tracks) < 301:
        track(sorted(rng.choice(valid, int(rng.integers(2, 5)), replace=False)), outliers=(0,) if rng.random() < 0.15 else ())
    order = rng.permutation(len(tracks))  # the long tracks do not sit at the front
    tracks = [tracks[j] for j in order]
    off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    image = np.array([m[0] for t in tracks for m in t], dtype=np.int32)
    uv = np.array([m[1] for t in tracks for m in t], dtype=np.float32).reshape(-1, 2)
    return {"cameras": table, "track_off": off, "image": image, "uv": uv}


def reversed_tracks(off: np.ndarray, image: np.ndarray, uv: np.ndarray):
    idx = np.concatenate([np.arange(a, b)[::-1] for a, b in zip(off[:-1], off[1:])] + [np.zeros(0, np.int64)]).astype(np.int64)
    return image[idx], uv[idx], idx


def reversal_tolerance(scene: Dict[str, np.ndarray], factor: float = 8.0) -> Tuple[float, float]:
    """The fixture's recipe on this scene: ``factor`` x the largest difference between the restatement on each track's measurements in
    forward and in reversed order (relative point distance, average error in px), over NO_RANSAC without a threshold and over
    RANSAC_SAMPLE_UNIFORM on the tracks whose pairs are all evaluated (a sampled track draws other pairs when reversed)."""
    off, image, uv, table = scene["track_off"], scene["image"], scene["uv"], scene["cameras"]
    rimage, ruv, idx = reversed_tracks(off, image, uv)
    rel, dif = [1e-16], [1e-16]
    for opts in (dict(mode=ref.NO_RANSAC), dict(mode=ref.RANSAC_SAMPLE_UNIFORM, **LOOSE)):
        sampled = np.array([opts["mode"] != ref.NO_RANSAC and (b - a) * (b - a - 1) // 2 > LOOSE["num_hypotheses"] for a, b in zip(off[:-1], off[1:])])
        keep = np.concatenate([[0], np.cumsum(np.where(sampled, 0, np.diff(off)))])
        sel = np.concatenate([np.arange(a, b) for a, b, s in zip(off[:-1], off[1:], sampled) if not s])
        fwd = ref.triangulate_tracks(table, keep, image[sel], uv[sel], **opts)
        rev = ref.triangulate_tracks(table, keep, rimage[sel], ruv[sel], **opts)
        same = (fwd["exit_code"] == rev["exit_code"]) & ~fwd["non_decisive"]
        ok = same & (fwd["exit_code"] == ref.SUCCESS)
        rel.append(float(np.max(np.linalg.norm(fwd["point"][ok] - rev["point"][ok], axis=1) / np.linalg.norm(fwd["point"][ok], axis=1), initial=0.0)))
        fin = same & np.isfinite(fwd["avg_error"]) & np.isfinite(rev["avg_error"])
        dif.append(float(np.max(np.abs(fwd["avg_error"][fin] - rev["avg_error"][fin]), initial=0.0)))
    return factor * max(rel), factor * max(dif)


# ---- hard geometry: candidates for tests/golden/triangulation_hard_scenes.npz (tools/make_triangulation_hard_fixture.py) ----

INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1
OFFSETS = {"0": (0.0, 0.0, 0.0), "1e3": (1e3, 1e3, 1e3), "1e5": (1e5, 1e5, 1e5), "utm": (5e5, 4e6, 100.0)}
RANK_TARGETS = {"1e-6": 1.2e-6, "1e-7": 1.2e-7, "1e-8": 1.2e-8, "1e-10": 1e-10 / 1.2, "1e-11": 1e-11 / 1.2, "1e-12": 1e-12 / 1.2}
RANSAC = dict(mode=ref.RANSAC_SAMPLE_UNIFORM, threshold=10.0, num_hypotheses=100, seed=0)


class _Family:
    def __init__(self, **options):
        self.options, self.cams, self.tracks, self.rung = options, [], [], []

    def add(self, rung: str, cams, uv, images=None) -> None:
        """One track: ``cams`` rows get fresh image indices; ``images`` overrides them per measurement (None keeps the fresh one)."""
        first = len(self.cams)
        self.cams += [np.asarray(c, np.float64) for c in cams]
        idx = list(range(first, first + len(cams))) if images is None else [first + k if i is None else i for k, i in enumerate(images)]
        self.tracks.append((idx, np.asarray(uv, np.float64).reshape(-1, 2)))
        self.rung.append(rung)

    def scene(self, extra_rows: int = 0) -> Dict[str, object]:
        table = np.zeros((len(self.cams) + extra_rows, 17))
        for i, c in enumerate(self.cams):
            table[i] = c
        off = np.concatenate([[0], np.cumsum([len(t[0]) for t in self.tracks])]).astype(np.int64)
        image = np.array([len(table) if i == "num_images" else i for t in self.tracks for i in t[0]], dtype=np.int64).astype(np.int32)
        uv = np.concatenate([t[1] for t in self.tracks] + [np.zeros((0, 2))]).astype(np.float32)
        return {"cameras": table, "track_off": off, "image": image, "uv": uv, "options": dict(self.options), "rung": list(self.rung)}


def _views(rng, n: int, parallax: float, noise: float, offset=(0.0, 0.0, 0.0), unit: float = 1.0, f: float = 800.0, fy_ratio: float = 1.0,
           cx: float = 640.0, cy: float = 480.0):
    """``n`` cameras spread over a baseline of ``parallax`` x depth, all looking at a point ``depth`` in front of them."""
    offset = np.asarray(offset, np.float64)
    depth = unit * rng.uniform(5.0, 20.0)
    x = offset + np.array([rng.uniform(-0.2, 0.2) * depth, rng.uniform(-0.2, 0.2) * depth, depth])
    cams, uv = [], []
    for i in range(n):
        eye = offset + parallax * depth * np.array([i / (n - 1) - 0.5, rng.normal(0.0, 0.1), rng.normal(0.0, 0.1)])
        cam = ref.lookat_camera(eye, x + depth * rng.normal(0.0, 0.05, 3), [0.0, 1.0, 0.0], f, cx, cy)
        cam[2] = f * fy_ratio
        cams.append(cam)
        u, v, _ = ref.project(cam, x)
        uv.append(np.array([u, v]) + (rng.normal(0.0, noise, 2) if noise else 0.0))
    return cams, np.array(uv)


def _ladder(fam: _Family, rng, rung: str, count: int = 8, **kw) -> None:
    for j in range(count):
        fam.add(rung, *_views(rng, 2 if j % 2 == 0 else 5, **kw))


def _axis_camera(z: float, towards: float, roll: float, x: float = 0.0, f: float = 50.0) -> np.ndarray:
    """A camera at (x, 0, z) looking along +z or -z (``towards`` = +1 / -1), rolled about its axis; principal point (0, 0)."""
    c, s = np.cos(roll), np.sin(roll)
    rot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    if towards < 0:
        rot = np.diag([1.0, -1.0, -1.0]) @ rot
    return ref.pack_camera(f, f, 0.0, 0.0, rot, [x, 0.0, z])


def _rank_track(kind: str, eps: float, geo) -> Tuple[List[np.ndarray], np.ndarray]:
    if kind == "facing":  # two cameras facing each other along the z axis, the point ``eps`` off the axis
        cams, x = [_axis_camera(-geo[0], 1.0, geo[2]), _axis_camera(geo[1], -1.0, geo[3])], np.array([eps, 0.0, 0.0])
    elif kind == "rotation":  # (nearly) equal centres: the second camera rolled, ``eps`` beside the first
        cams, x = [_axis_camera(0.0, 1.0, geo[2]), _axis_camera(0.0, 1.0, geo[3], x=eps)], np.array([0.0, 0.0, geo[0]])
    else:  # five cameras on the z axis, on both sides of the point, which lies ``eps`` off the axis
        cams = [_axis_camera(-geo[0], 1.0, geo[2]), _axis_camera(geo[1], -1.0, geo[3]), _axis_camera(-2.0 * geo[0], 1.0, geo[3] + 1.0),
                _axis_camera(1.5 * geo[1], -1.0, geo[2] - 1.0), _axis_camera(-0.5 * geo[0], 1.0, 0.3)]
        x = np.array([eps, 0.0, 0.0])
    uv = np.array([ref.project(c, x)[:2] for c in cams]).astype(np.float32).astype(np.float64)
    return cams, uv


def _bisect_rank(kind: str, target: float, geo) -> Tuple[List[np.ndarray], np.ndarray]:
    """The track of ``kind`` whose exact sigma_3 (arbiter) is ``target``, by bisection on the perturbation in log space."""
    from tests import triangulation_arbiter as arbiter

    def sigma3(eps: float) -> float:
        cams, uv = _rank_track(kind, eps, geo)
        return float(arbiter.dlt([arbiter.Cam(c) for c in cams], [arbiter._mp_uv(p) for p in uv])[0][2])

    lo, hi = -25.0, 0.0
    for _ in range(48):
        mid = 0.5 * (lo + hi)
        if sigma3(10.0**mid) < target:
            lo = mid
        else:
            hi = mid
    return _rank_track(kind, 10.0 ** (0.5 * (lo + hi)), geo)


def _circle(rng, x, noise: float = 0.05, f: float = 50.0):
    table, uv = [], []
    for i in range(8):
        th = 2.0 * np.pi * i / 8
        cam = ref.lookat_camera([40.0 * np.cos(th), 40.0 * np.sin(th), 0.0], np.zeros(3), [0.0, 0.0, 1.0], f)
        table.append(cam)
        uv.append(np.array(ref.project(cam, x)[:2]) + rng.normal(0.0, noise, 2))
    return table, np.array(uv)


def select_pairs_reversed_ties(table, images, uv, mode, num_hypotheses, seed):
    """``ref.select_pairs`` with every tie rule reversed (top-k ties to the SMALLER index, the others to the larger): the sampler
    families must give other outputs under it, or they would not pin the rule."""
    import itertools
    import math

    n = len(images)
    total = n * (n - 1) // 2
    h = min(int(num_hypotheses), total)
    if h >= total:
        return list(range(total))
    tkey = ref.track_key(images[0], uv[0])
    keys = np.empty(total)
    for p, (k1, k2) in enumerate(itertools.combinations(range(n), 2)):
        w = ref.baseline(ref._camera(table, images[k1]), ref._camera(table, images[k2]))
        u = (float(ref.pair_hash(seed, tkey, p) >> 11) + 0.5) * 2.0**-53
        keys[p] = float(ref.pair_hash(seed, tkey, p) >> 11) if mode == ref.RANSAC_SAMPLE_UNIFORM else -w if mode == ref.RANSAC_TOPK_BASELINES else (
            -math.log(u) / w if w > 0.0 else math.inf)
    tie = np.arange(total) if mode == ref.RANSAC_TOPK_BASELINES else -np.arange(total)
    return sorted(int(p) for p in np.lexsort((tie, keys))[:h])


def hard_scenes(seed: int = 23) -> Dict[str, Dict[str, object]]:
    """Candidate families {name: scene}; a scene has cameras, track_off, image, uv (float32), options and a rung label per track. Every
    track has cameras of its own. tools/make_triangulation_hard_fixture.py keeps the decisive tracks on which the design holds."""
    rng = np.random.default_rng(seed)
    out: Dict[str, Dict[str, object]] = {}

    fam = _Family(**RANSAC)
    for parallax in ("1e-1", "1e-2", "1e-3", "1e-4", "1e-5"):
        for noise in (0.0, 0.5):
            _ladder(fam, rng, f"parallax {parallax} {'noisy' if noise else 'clean'}", parallax=float(parallax), noise=noise)
    out["parallax"] = fam.scene()

    for name, offset in OFFSETS.items():  # a family each: the port-to-arbiter difference grows with the offset
        fam = _Family(**RANSAC)
        for parallax in ("1e-1", "1e-3"):
            _ladder(fam, rng, f"offset {name} parallax {parallax}", parallax=float(parallax), noise=0.5, offset=offset)
        out[f"offset_{name}"] = fam.scene()

    fam = _Family(**RANSAC)
    for unit in ("1e-3", "1e0", "1e4"):
        for f in (50.0, 5000.0):  # fx : fy = 2 : 1, the principal point far off-centre
            _ladder(fam, rng, f"scale {unit} f {f:g}", parallax=0.1, noise=0.5, unit=float(unit), f=f, fy_ratio=0.5, cx=5000.0, cy=-3000.0)
    out["scale"] = fam.scene()

    facing, rotation, final = _Family(**RANSAC), _Family(**RANSAC), _Family(mode=ref.NO_RANSAC, threshold=10.0)
    for name, target in RANK_TARGETS.items():
        for j in range(4):
            geo = (rng.uniform(10.0, 40.0), rng.uniform(10.0, 40.0), rng.uniform(0.0, 6.0), rng.uniform(0.0, 6.0))
            facing.add(f"rank facing {name}", *_bisect_rank("facing", target, geo))
            rotation.add(f"rank rotation {name}", *_bisect_rank("rotation", target, geo))
            final.add(f"rank final {name}", *_bisect_rank("final", target, geo))
    out["rank_facing"], out["rank_rotation"], out["rank_final"] = facing.scene(), rotation.scene(), final.scene()

    fam = _Family(mode=ref.NO_RANSAC)
    for zeta in (1e-3, 1e-6):
        for side in (1.0, -1.0):  # the point just in front of / just behind the second camera, a normal point for the first
            for j in range(3):
                c1 = ref.lookat_camera([0.0, -10.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], 800.0, 640.0, 480.0)
                c2 = ref.lookat_camera([2.0, 0.5 * j, 1.0], [2.0, 10.0, 1.0], [0.0, 0.0, 1.0], 800.0, 640.0, 480.0)
                x = c2[14:17] + c2[5:14].reshape(3, 3) @ (zeta * np.array([0.3 + 0.1 * j, 0.2, side]))
                fam.add(f"depth {zeta:g} {'front' if side > 0 else 'behind'}", [c1, c2], [ref.project(c1, x)[:2], ref.project(c2, x)[:2]])
    for disparity in (1e-30, 0.0):  # parallel axes: the null vector's w -> 0
        fam.add(f"depth infinity disparity {disparity:g}", [_axis_camera(0.0, 1.0, 0.0), _axis_camera(0.0, 1.0, 0.0, x=1.0)], [[disparity, 0.0], [0.0, 0.0]])
    out["depth"] = fam.scene()

    # sampler ties, with more pairs than hypotheses
    for name, mode, hyp in (("ties_topk10", ref.RANSAC_TOPK_BASELINES, 10), ("ties_biased10", ref.RANSAC_SAMPLE_BIASED_BASELINE, 10),
                            ("ties_topk1", ref.RANSAC_TOPK_BASELINES, 1), ("ties_uniform0", ref.RANSAC_SAMPLE_UNIFORM, 0)):
        fam = _Family(mode=mode, threshold=5.0, num_hypotheses=hyp, seed=3)
        for j in range(8):  # the circle of 8: equal chords tie; measurements 0, 1, 2 are outliers, so the tie rule decides the winner
            cams, uv = _circle(rng, np.array([3.0, -2.0, 1.0]) + rng.normal(0.0, 0.5, 3))
            for k in (0, 1, 2) if hyp > 1 else (0,):
                uv[k] += rng.choice([-1.0, 1.0], 2) * rng.uniform(15.0, 30.0, 2)
            fam.add(f"{name} circle", cams, uv)
        out[name] = fam.scene()
    for name, mode in (("ties_missing_topk5", ref.RANSAC_TOPK_BASELINES), ("ties_missing_biased5", ref.RANSAC_SAMPLE_BIASED_BASELINE)):
        fam = _Family(mode=mode, threshold=5.0, num_hypotheses=5, seed=3)
        for j in range(4):  # 6 measurements, 3 of them without a camera: 12 of the 15 pairs have baseline 0
            cams, uv = _circle(rng, np.array([3.0, -2.0, 1.0]) + rng.normal(0.0, 0.5, 3))
            keep = sorted(rng.choice(8, 6, replace=False).tolist())
            cams, uv = [cams[k] for k in keep], uv[keep]
            for k in rng.choice(6, 3, replace=False):
                cams[k] = np.zeros(17)
            fam.add(f"{name} three cameras missing", cams, uv)
        for j in range(2):  # two measurements in one image: a pair with two estimated cameras and baseline 0
            cams, uv = _circle(rng, np.array([3.0, -2.0, 1.0]) + rng.normal(0.0, 0.5, 3))
            first = len(fam.cams)
            fam.add(f"{name} one image twice", cams[:6], np.vstack([uv[:6], uv[2] + [1.5, -2.0]]), images=[None] * 6 + [first + 2])
        out[name] = fam.scene()

    for name, options in (("hostile_no_ransac", dict(mode=ref.NO_RANSAC, threshold=10.0)), ("hostile_ransac", RANSAC)):
        fam = _Family(**options)
        for bad in (-1, INT32_MIN, INT32_MAX, "num_images"):
            for at in (0, 1, 3):
                cams, uv = _views(rng, 4, parallax=0.1, noise=0.5)
                fam.add(f"hostile image {bad} at {at}", cams, uv, images=[bad if k == at else None for k in range(4)])
        out[name] = fam.scene()
    return out
