"""Scenes for the rotation-averaging stage: the smallest shapes that reach each path of tests/rotation_averaging_reference.py, shared by the
host-build test (bytes), the device test and the CPU tests. A scene is a dict of arrays plus ``check``, a predicate on the restatement's
result that asserts the scene contains what it is named for. ``expected(name)`` computes the restatement once per process.

The reference's known answers (tests/averaging/rotation/test_shonan.py, tests/data/sample_poses.py) are restated as arrays: the rotations
are written out from their Euler angles; gtsam's ``SFMdata.posesOnCircle`` is restated as four cameras a quarter turn apart about the
vertical axis behind a fixed tilt (the rotations it gives were not observed: gtsam cannot be imported here)."""

from __future__ import annotations

import functools
from typing import Dict, List

import numpy as np

from tests import rotation_averaging_reference as ref
from tests.conftest import REPO

PALACE = REPO / "tests" / "golden" / "view_graph_palace_edges.npz"


def rodrigues(v) -> np.ndarray:
    v = np.asarray(v, dtype=np.float64)
    t = float(np.linalg.norm(v))
    if t == 0.0:
        return np.eye(3)
    k = v / t
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * kx + (1 - np.cos(t)) * (kx @ kx)


def rx(deg):
    return rodrigues([np.radians(deg), 0, 0])


def ry(deg):
    return rodrigues([0, np.radians(deg), 0])


def rz(deg):
    return rodrigues([0, 0, np.radians(deg)])


def random_rotations(rng, n):
    v = rng.standard_normal((n, 3))
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0, np.pi, (n, 1))
    return np.stack([rodrigues(x) for x in v])


def scene(name, pairs, rotation, weight, num_images, *, enable=None, anchor=-1, truth=None, check=None, options=None, known_tol_deg=None) -> Dict[str, object]:
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    return {"name": name, "pair_images": pairs, "rotation": np.ascontiguousarray(np.asarray(rotation, dtype=np.float64).reshape(-1, 9)),
            "weight": np.ascontiguousarray(np.asarray(weight, dtype=np.float64).reshape(-1)), "pair_enable": None if enable is None else np.asarray(enable, np.uint8),
            "num_images": int(num_images), "anchor": int(anchor), "truth": truth, "check": check or (lambda r: True), "options": dict(options or {}),
            "known_tol_deg": known_tol_deg}


def relative(truth, pairs, rng=None, noise_deg=0.0):
    """i2Ri1 = wRi2^T wRi1 of each (i1, i2), followed by a rotation of about ``noise_deg`` per axis."""
    out = []
    for i1, i2 in pairs:
        m = truth[i2].T @ truth[i1]
        if noise_deg:
            m = m @ rodrigues(np.radians(noise_deg) * rng.standard_normal(3))
        out.append(m)
    return np.stack(out) if len(out) else np.zeros((0, 3, 3))


def planted(name, n, pairs, seed, *, noise_deg=2.0, outliers=(), weights="wide", **kw):
    rng = np.random.default_rng(seed)
    truth = random_rotations(rng, n)
    m = relative(truth, pairs, rng, noise_deg)
    for k in outliers:
        m[k] = random_rotations(rng, 1)[0]
    w = rng.uniform(15, 600, len(pairs)) ** 2 if weights == "wide" else np.ones(len(pairs))
    return scene(name, pairs, m, w, n, truth=truth, **kw)


def ring(n):
    return [(i, (i + 1) % n) for i in range(n)]


def chain(n):
    return [(i, i + 1) for i in range(n - 1)]


def status_is(code, **counters):
    def check(r):
        c = r["counters"]
        return c["status"] == code and all(c[k] == v for k, v in counters.items())

    return check


@functools.lru_cache(maxsize=None)
def all_scenes() -> List[Dict[str, object]]:
    s = []
    conv = status_is(ref.CONVERGED)
    s.append(scene("empty", np.zeros((0, 2)), np.zeros((0, 9)), np.zeros(0), 3, check=status_is(ref.NO_VALID_ROW, component_size=0)))
    s.append(scene("one_row", [(0, 1)], [ry(30)], [4.0], 2, truth=np.stack([ry(30), np.eye(3)]), check=status_is(ref.CONVERGED, component_size=2, anchor=1), known_tol_deg=1e-6))
    # the reference's known answers; the weights are its dummy correspondence counts (i1 + i2) squared
    r01, r12 = ry(30), rz(20)
    s.append(scene("simple", [(1, 0), (2, 1)], [r01, r12], [1.0, 9.0], 3, truth=np.stack([np.eye(3), r01, r01 @ r12]), check=conv, known_tol_deg=2.0))
    s.append(scene("simple_with_prior", [(1, 0), (2, 0)], [ry(30), rx(30)], [1.0, 1e5], 3, truth=np.stack([np.eye(3), ry(30), rx(30)]), check=conv, known_tol_deg=2.0))
    s.append(scene("nonconsecutive", [(1, 2), (2, 3), (1, 3)], [np.eye(3)] * 3, [9.0, 25.0, 16.0], 4, truth=np.stack([np.eye(3)] * 4),
                   check=lambda r: r["counters"]["status"] == ref.CONVERGED and r["node_valid"].tolist() == [0, 1, 1, 1], known_tol_deg=0.1))
    circle = np.stack([rz(90.0 * k) @ rx(-100.0) for k in range(4)])
    line = np.stack([ry(10)] * 3)
    pano = np.stack([ry(-30), np.eye(3), ry(30)])
    for name, truth, pairs in (("circle_two_edges", circle, [(1, 0), (2, 1), (3, 2), (0, 3)]), ("circle_all_edges", circle, [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]),
                               ("line_large_edges", line, [(0, 1), (0, 2), (1, 2)]), ("panorama", pano, [(0, 1), (0, 2), (1, 2)])):
        w = [float(max(a + b, 1)) ** 2 for a, b in pairs]
        s.append(scene(name, pairs, relative(truth, pairs), w, len(truth), truth=truth, check=conv, known_tol_deg=2.0))
    # chains and rings across the lane count and the tree's powers of two
    s.append(planted("chain63", 63, chain(63), 11, check=status_is(ref.CONVERGED, component_size=63)))
    s.append(planted("ring64", 64, ring(64), 12, check=status_is(ref.CONVERGED, component_size=64)))
    s.append(planted("ring65", 65, ring(65), 13, check=status_is(ref.CONVERGED, component_size=65)))
    s.append(planted("chain257", 257, chain(257)[::-1], 14, anchor=256, check=status_is(ref.CONVERGED, component_size=257)))
    s.append(planted("ring257", 257, ring(257), 15, check=status_is(ref.CONVERGED, component_size=257)))
    hub = [(0, k) if k % 2 else (k, 0) for k in range(1, 301)] + [(k, k + 1) for k in range(1, 300, 7)]
    s.append(planted("hub300", 301, hub, 16, check=lambda r: r["counters"]["status"] == ref.CONVERGED and int((r["graph"].node == 0).sum()) == 300))
    window = [(i, j) for i in range(120) for j in range(i + 1, min(i + 7, 120))]
    rng = np.random.default_rng(17)
    s.append(planted("window120x6_outliers", 120, window, 17, outliers=sorted(rng.choice(len(window), 20, replace=False).tolist()),
                     check=lambda r: r["counters"]["status"] == ref.CONVERGED and r["counters"]["valid_rows"] == len(window)))
    gap_ids = [3 * k + 2 for k in range(14)]
    gp = [(gap_ids[a], gap_ids[b]) for a, b in ring(14) + [(0, 5), (3, 9)]]
    sc = planted("gaps", 45, gp, 18, check=lambda r: r["counters"]["status"] == ref.CONVERGED and r["counters"]["component_size"] == 14 and int(r["node_valid"].sum()) == 14)
    s.append(sc)
    # rows that are not valid: disabled, NaN, zero and negative weight; the ring stays connected without them
    base = ring(20) + [(0, 7), (3, 12), (5, 15), (8, 18), (2, 9), (4, 14)]
    sc = planted("masked_rows", 20, base, 19, check=lambda r: r["counters"]["status"] == ref.CONVERGED and r["counters"]["valid_rows"] == 20 and r["counters"]["anchor"] == 2)
    sc["pair_enable"] = np.ones(len(base), np.uint8)
    sc["pair_enable"][[20, 21]] = 0
    sc["rotation"][22, 4] = np.nan
    sc["rotation"][23, 0] = np.inf
    sc["weight"][24], sc["weight"][25] = 0.0, -3.0
    sc["pair_enable"][0] = 0  # the first row too: the anchor is the i2 of the first VALID row, (1, 2)
    sc["rotation"][0] = np.nan
    sc["check"] = lambda r: r["counters"]["status"] == ref.CONVERGED and r["counters"]["valid_rows"] == 19 and r["counters"]["anchor"] == 2 and r["counters"]["component_size"] == 20
    s.append(sc)
    two = ring(9) + [(10 + a, 10 + b) for a, b in ring(6)]
    s.append(planted("two_components", 17, two[::-1], 20, check=lambda r: r["counters"]["component_size"] == 6 and r["node_valid"].tolist() == [0] * 10 + [1] * 6 + [0]))
    s.append(planted("two_components_anchor", 17, two, 20, anchor=4, check=lambda r: r["counters"]["component_size"] == 9 and r["node_valid"].tolist() == [1] * 9 + [0] * 8))
    dup = ring(12) + [(3, 4), (4, 3), (7, 6), (0, 1)]
    s.append(planted("duplicate_pairs", 12, dup, 21, check=lambda r: r["counters"]["status"] == ref.CONVERGED and r["counters"]["valid_rows"] == 16))
    sc = planted("weights_span", 30, ring(30) + [(i, (i + 5) % 30) for i in range(0, 30, 3)], 22, check=conv)
    sc["weight"] = np.geomspace(1.0, 600.0 ** 2, len(sc["weight"]))[np.random.default_rng(22).permutation(len(sc["weight"]))]
    s.append(sc)
    s.append(planted("noise_free", 40, ring(40) + [(i, (i + 9) % 40) for i in range(0, 40, 4)], 23, noise_deg=0.0,
                     check=lambda r: r["counters"]["status"] == ref.CONVERGED and r["costs"]["final_cost"] < 1e-18))
    s.append(planted("max_iterations", 65, ring(65), 13, options={"max_outer": 1}, check=status_is(ref.MAX_ITERATIONS, outer_iterations=1)))
    s.append(planted("non_finite", 12, ring(12), 24, options={"chordal_max_iterations": 0}, check=lambda r: r["counters"]["status"] == ref.NON_FINITE and not r["node_valid"].any()))
    s.append(planted("unweighted", 50, ring(50) + [(i, (i + 11) % 50) for i in range(0, 50, 5)], 25, weights="ones", check=conv))
    z = np.load(PALACE)
    n_pal = int(z["num_images"])
    wp = (10.0 + np.arange(len(z["pair_images"])) % 97) ** 2
    s.append(scene("palace", z["pair_images"], z["rotation"], wp, n_pal, enable=z["keep_median"], check=lambda r: r["counters"]["status"] in (ref.CONVERGED, ref.MAX_ITERATIONS)))
    # the point reached from the chordal start is a critical point that is provably NOT the global minimum: lambda_min(S) far below gtsam's -1e-4
    s.append(dict(not_global_scene(NOT_GLOBAL_SEED), check=lambda r: r["counters"]["status"] == ref.CONVERGED and r["decisive"]
                  and ref.dense_certificate(r) < 100 * ref.GTSAM_OPTIMALITY_THRESHOLD))
    names = [x["name"] for x in s]
    assert len(set(names)) == len(names)
    return s


NOT_GLOBAL_SEED = 0  # the first seed tried; lambda_min(S) = -67.9 there


def not_global_scene(seed):
    """A ring of 257 with chords (i, i + 7) for every fifth i, 2 degrees of noise, 3 random-rotation edges, weights U[15, 600)^2."""
    pairs = ring(257) + [(i, (i + 7) % 257) for i in range(0, 257, 5)]
    rng = np.random.default_rng(1000 + seed)
    out = sorted(rng.choice(len(pairs), 3, replace=False).tolist())
    return planted("not_global", 257, pairs, seed, outliers=out)


SCENE_NAMES = tuple(x["name"] for x in all_scenes())
SMALL_SCENES = tuple(x["name"] for x in all_scenes() if x["num_images"] <= 65)  # the mpmath arbiter's (tests/rotation_averaging_arbiter.py: MP_MAX_NODES)


def get(name):
    return next(x for x in all_scenes() if x["name"] == name)


def solve(sc, **override):
    opts = dict(sc["options"], **override)
    anchor = opts.pop("anchor", sc["anchor"])
    return ref.solve(sc["pair_images"], sc["rotation"], sc["weight"], sc["pair_enable"], num_images=sc["num_images"], anchor=anchor, **opts)


@functools.lru_cache(maxsize=None)
def expected(name):
    return solve(get(name))


def options_of(sc):
    return dict(ref.DEFAULTS, **sc["options"])
