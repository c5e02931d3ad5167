"""The scenes of the translation-recovery tests: the smallest shapes at which the kernel can go wrong. Each is a dict of the arrays
``gtsfm_translation_recovery_f64`` takes (pair rows, track CSR, world directions, the two masks), ``num_images``, ``anchor``, ``options``, the
planted positions ``truth`` [N + T, 3] (None where there is none) and ``check``, which says on the restatement's result that the scene holds
what it is named for. A pair row (i1, i2) carries unit(x_i1 - x_i2), a measurement of camera i on landmark j unit(x_j - x_i)."""

import functools
from pathlib import Path

import numpy as np

from tests import translation_recovery_reference as ref

GOLDEN = Path(__file__).resolve().parent / "golden"


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def perturb(z, rng, noise_rad):
    """Unit vectors turned by about noise_rad in a random direction."""
    return z if noise_rad == 0 else unit(z + noise_rad * rng.normal(size=z.shape))


def scene(name, num_images, pairs, cams, land, views, seed, noise=0.0, wrong=0, options=None, anchor=-1, check=None):
    """``views``: per landmark the cameras that see it. ``wrong``: that many rows get a random direction."""
    rng = np.random.default_rng(seed)
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    cams, land = np.asarray(cams, np.float64).reshape(-1, 3), np.asarray(land, np.float64).reshape(-1, 3)
    world_pair = perturb(unit(cams[pairs[:, 0]] - cams[pairs[:, 1]]), rng, noise) if len(pairs) else np.zeros((0, 3))
    track_off = np.concatenate([[0], np.cumsum([len(v) for v in views])]).astype(np.int64)
    image = np.asarray([c for v in views for c in v], np.int32)
    track = np.repeat(np.arange(len(views)), [len(v) for v in views])
    world_meas = perturb(unit(land[track] - cams[image]), rng, noise) if len(image) else np.zeros((0, 3))
    wrong_rows = np.sort(rng.choice(np.arange(1, len(pairs) + len(image)), wrong, replace=False)) if wrong else np.zeros(0, np.int64)
    for r in wrong_rows:
        if r < len(pairs):
            world_pair[r] = unit(rng.normal(size=3))
        else:
            world_meas[r - len(pairs)] = unit(rng.normal(size=3))
    return {"name": name, "pair_images": pairs, "world_pair": world_pair, "pair_enable": None, "track_off": track_off, "image": image, "world_meas": world_meas,
            "meas_enable": None, "num_images": num_images, "anchor": anchor, "options": dict(options or {}), "truth": np.concatenate([cams, land]), "wrong_rows": wrong_rows,
            "check": check or converged}


def converged(r):
    return r["counters"]["status"] == ref.CONVERGED


def status_is(status, **counters):
    return lambda r: r["counters"]["status"] == status and all(r["counters"][k] == v for k, v in counters.items())


def ring(n, step=(1,)):
    return sorted({(min(i, (i + s) % n), max(i, (i + s) % n)) for i in range(n) for s in step})


def planted(name, n_cam, n_land, seed, per_land=4, pairs=None, **kw):
    """Cameras in a box of side 10, landmarks in a box of side 6 ten units in front; a window graph of pairs; every landmark seen by per_land cameras."""
    rng = np.random.default_rng(1000 + seed)
    cams = rng.uniform(-5, 5, size=(n_cam, 3))
    land = rng.uniform(-3, 3, size=(n_land, 3)) + [0.0, 0.0, 10.0]
    if pairs is None:
        pairs = ring(n_cam, (1, 2, 3))
    views = [sorted(rng.choice(n_cam, min(per_land, n_cam), replace=False).tolist()) for _ in range(n_land)]
    return scene(name, n_cam, pairs, cams, land, views, seed, **kw)


def circle(n, radius):
    ang = 2 * np.pi * np.arange(n) / n
    return np.stack([radius * np.cos(ang), radius * np.sin(ang), np.zeros(n)], 1)


@functools.lru_cache(maxsize=None)
def all_scenes():
    s = []
    none = np.zeros((0, 3))
    s.append(scene("no_rows", 3, [], np.zeros((3, 3)), none, [], 0, check=lambda r: r["counters"]["status"] == ref.NO_VALID_ROW and not r["node_valid"].any()))
    s.append(scene("one_pair", 2, [(0, 1)], [[1.0, 2.0, 2.0], [0.0, 0.0, 0.0]], none, [], 0, options={"scale_factor": 3.0},
                   check=lambda r: converged(r) and r["counters"]["anchor"] == 1 and r["translation"][0].tobytes() == (3.0 * unit([1.0, 2.0, 2.0])).tobytes()))
    # the reference's known scenes (tests/averaging/translation/test_averaging_1dsfm.py), restated as arrays
    s.append(scene("circle4_all_edges", 4, [(i, j) for i in range(4) for j in range(i + 1, 4)], circle(4, 5.0), none, [], 1))
    s.append(scene("circle8_two_edges", 8, ring(8, (1, 2)), circle(8, 40.0), none, [], 2))
    door = np.load(GOLDEN / "triangulation_lund_door.npz")["cameras"][:, 14:17]
    s.append(scene("door12_exhaustive", 12, [(i, j) for i in range(12) for j in range(i + 1, 12)], door, none, [], 3))
    # planted scenes with landmarks
    s.append(planted("planted_noise_free", 30, 80, 4))
    s.append(planted("planted_noise", 30, 80, 4, noise=0.01))
    s.append(planted("planted_wrong_huber", 30, 80, 4, noise=0.01, wrong=8))
    s.append(planted("planted_wrong_no_huber", 30, 80, 4, noise=0.01, wrong=8, options={"huber_k": 0.0}))
    # lane ownership and tree padding: the component sizes around 256 and 512, cut after three iterations
    for nodes in (255, 256, 257, 513):
        n_cam = nodes // 4
        s.append(planted(f"nodes{nodes}", n_cam, nodes - n_cam, 5, noise=0.01, options={"max_outer": 3},
                         check=lambda r, nodes=nodes: r["counters"]["component_size"] == nodes and r["counters"]["outer_iterations"] == 3))
    rng = np.random.default_rng(6)
    hub_cams = np.concatenate([[[0.0, 0.0, 0.0]], unit(rng.normal(size=(300, 3))) * rng.uniform(2, 9, size=(300, 1))])
    s.append(scene("hub300", 301, [(0, k) for k in range(1, 301)] + [(k, k + 1) for k in range(1, 300, 7)], hub_cams, none, [], 6, noise=0.01,
                   check=lambda r: converged(r) and int((r["graph"].node == 0).sum()) == 300))
    s.append(planted("pairs_only", 20, 0, 7, noise=0.01, check=lambda r: converged(r) and r["counters"]["anchor"] == 1))
    s.append(planted("tracks_only", 12, 40, 8, noise=0.01, pairs=[], check=lambda r: converged(r) and r["counters"]["anchor"] < 12 and r["counters"]["component_size"] == 52))
    # a leaf camera (one pair row, no landmark) and a landmark left with one measurement
    sc = planted("leaves", 10, 12, 9, noise=0.01, pairs=ring(9, (1, 2)) + [(4, 9)])
    sc["meas_enable"] = np.ones(len(sc["image"]), np.uint8)
    sc["meas_enable"][sc["image"] == 9] = 0
    of5 = np.arange(int(sc["track_off"][5]), int(sc["track_off"][6]))
    sc["meas_enable"][of5[sc["image"][of5] != 9][1:]] = 0
    sc["check"] = lambda r: (converged(r) and r["counters"]["component_size"] == 22 and int((r["graph"].node == 9).sum()) == 1
                             and int((r["graph"].node == 10 + 5).sum()) == 1)
    s.append(sc)
    # rows that are not valid: disabled and NaN, the first row too; camera ids with gaps; a second component
    sc = planted("masked_rows", 16, 20, 10, noise=0.01)
    sc["pair_enable"] = np.ones(len(sc["pair_images"]), np.uint8)
    sc["pair_enable"][[0, 5]] = 0
    sc["world_pair"][0] = np.nan
    sc["world_pair"][7, 1] = np.nan
    sc["world_pair"][9, 2] = np.inf
    sc["meas_enable"] = np.ones(len(sc["image"]), np.uint8)
    sc["meas_enable"][[3, 11]] = 0
    sc["world_meas"][20, 0] = np.nan
    sc["check"] = lambda r: converged(r) and r["counters"]["valid_rows"] == len(r["graph"].row) // 2 == 16 * 3 - 4 + 80 - 3 and r["counters"]["anchor"] == 2
    s.append(sc)
    base = planted("gaps", 14, 10, 11, noise=0.01)
    ids = np.asarray([3 * k + 2 for k in range(14)], np.int32)
    sc = dict(base, pair_images=ids[base["pair_images"]], image=ids[base["image"]], num_images=45)
    truth = np.full((45 + 10, 3), np.nan)
    truth[ids], truth[45:] = base["truth"][:14], base["truth"][14:]
    sc["truth"] = truth
    sc["check"] = lambda r: converged(r) and r["counters"]["component_size"] == 24 and int(r["node_valid"].sum()) == 24
    s.append(sc)
    two = ring(9, (1, 2)) + [(10 + a, 10 + b) for a, b in ring(6, (1, 2))]
    cams17 = np.random.default_rng(12).uniform(-5, 5, size=(17, 3))
    s.append(scene("two_components", 17, two[::-1], cams17, none, [], 12, check=lambda r: r["counters"]["component_size"] == 6 and r["node_valid"].tolist() == [0] * 10 + [1] * 6 + [0]
                   and np.isnan(r["translation"][:10]).all()))
    s.append(scene("two_components_anchor", 17, two, cams17, none, [], 12, anchor=4, check=lambda r: r["counters"]["component_size"] == 9 and r["node_valid"].tolist() == [1] * 9 + [0] * 8))
    s.append(planted("scale_2_5", 12, 20, 13, noise=0.01, options={"scale_factor": 2.5}))
    s.append(planted("sigma_0_5", 12, 20, 13, noise=0.01, options={"sigma": 0.5}))
    for k in (1, 2, 3):
        s.append(planted(f"max_outer_{k}", 30, 80, 4, noise=0.01, wrong=8, options={"max_outer": k}, check=status_is(ref.MAX_ITERATIONS, outer_iterations=k)))
    # two coincident nodes: without an initialisation every node sits on the anchor, |d| = 0 on every row
    s.append(planted("non_finite", 10, 12, 14, options={"init_max_iterations": 0}, check=lambda r: r["counters"]["status"] == ref.NON_FINITE and not r["node_valid"].any()
                     and np.isnan(r["translation"]).all()))
    names = [x["name"] for x in s]
    assert len(set(names)) == len(names)
    return s


SCENE_NAMES = tuple(x["name"] for x in all_scenes())
NOISE_FREE = ("circle4_all_edges", "circle8_two_edges", "door12_exhaustive", "planted_noise_free")
BATCH = ("planted_noise", "gaps", "tracks_only", "masked_rows")  # a batch of four problems


def get(name):
    return next(x for x in all_scenes() if x["name"] == name)


ARRAYS = ("pair_images", "world_pair", "pair_enable", "track_off", "image", "world_meas", "meas_enable")


def arrays_of(sc):
    return tuple(sc[k] for k in ARRAYS)


def solve(sc, **override):
    opts = dict(sc["options"], **override)
    anchor = opts.pop("anchor", sc["anchor"])
    return ref.solve(*arrays_of(sc), num_images=sc["num_images"], anchor=anchor, **opts)


@functools.lru_cache(maxsize=None)
def expected(name):
    return solve(get(name))


def options_of(sc):
    return dict(ref.DEFAULTS, **sc["options"])


def permuted(sc, seed=5):
    """The same problem with its pair rows and each track's measurements in another order; row 0 (the scale row of the default anchor) stays."""
    rng = np.random.default_rng(seed)
    e = len(sc["pair_images"])
    perm = np.concatenate([[0], 1 + rng.permutation(e - 1)]) if e else np.zeros(0, np.int64)
    mperm = np.concatenate([lo + (rng.permutation(hi - lo) if (e or lo) else np.concatenate([[0], 1 + rng.permutation(hi - lo - 1)]))
                            for lo, hi in zip(sc["track_off"][:-1], sc["track_off"][1:])]).astype(np.int64) if len(sc["image"]) else np.zeros(0, np.int64)
    take = lambda x, p: None if x is None else x[p]  # noqa: E731
    return dict(sc, pair_images=sc["pair_images"][perm], world_pair=sc["world_pair"][perm], pair_enable=take(sc["pair_enable"], perm), image=sc["image"][mperm],
                world_meas=sc["world_meas"][mperm], meas_enable=take(sc["meas_enable"], mperm))


def batch(names=BATCH):
    return batch_of([get(n) for n in names])


def batch_of(parts):
    """The scenes as one call: concatenated arrays, problem_row_off [P + 1, 2], the common num_images and the parts."""
    n = max(x["num_images"] for x in parts)
    cat = lambda k, fill: np.concatenate([np.full(len(x["pair_images"] if k == "pair_enable" else x["image"]), 1, np.uint8) if x[k] is None and fill else x[k] for x in parts])  # noqa: E731
    track_off = np.concatenate([[0]] + [x["track_off"][1:] + sum(len(y["image"]) for y in parts[:i]) for i, x in enumerate(parts)]).astype(np.int64)
    off = np.zeros((len(parts) + 1, 2), np.int64)
    off[1:, 0] = np.cumsum([len(x["pair_images"]) for x in parts])
    off[1:, 1] = np.cumsum([len(x["track_off"]) - 1 for x in parts])
    arrays = (cat("pair_images", False), cat("world_pair", False), cat("pair_enable", True), track_off, cat("image", False), cat("world_meas", False), cat("meas_enable", True))
    return arrays, off, n, parts
