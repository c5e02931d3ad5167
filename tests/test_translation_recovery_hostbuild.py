"""CPU: the translation-recovery solver itself (trec_validate and trec_solve of gtsfm_amd/csrc/translation_recovery_kernels.hip, the functions the
kernels run), compiled for the host into the stand-alone program tools/translation_recovery_host_main.cpp -- once plain and once with the
host's address and undefined-behaviour sanitizers -- on every scene of tests/translation_recovery_scenes.py. The program solves each scene
with one lane over zeroed memory and with the device's 256-lane partition, last lane first, over memory filled with 0xFF, and every problem
of a batch alone as well; all must be byte-equal to each other and to the restatement (tests/translation_recovery_reference.py): positions,
mask, counters and costs. The program runs as its own process; no sanitizer is loaded into Python and no GPU is involved."""

import shutil
import struct

import numpy as np
import pytest

from gtsfm_amd.csrc.build import HIPCC
from tests import translation_recovery_reference as ref
from tests import translation_recovery_scenes as scenes
from tests.conftest import REPO
from tests.hostbuild_program import build_program, run

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc is not installed")

SOURCE = REPO / "tools" / "translation_recovery_host_main.cpp"
MAGIC = 0x3143455254524D46


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    return build_program(tmp_path_factory, SOURCE, request.param == "sanitized")


def write_scene(path, arrays, num_images, row_off, anchor, opts):
    pair_images, world_pair, pair_enable, track_off, image, world_meas, meas_enable = arrays
    pair_images = np.zeros((0, 2), np.int32) if pair_images is None else np.asarray(pair_images).reshape(-1, 2)
    track_off = np.zeros(1, np.int64) if track_off is None else np.asarray(track_off)
    image = np.zeros(0, np.int32) if image is None else np.asarray(image)
    e, t, s = len(pair_images), len(track_off) - 1, len(image)
    row_off = np.asarray(row_off, np.int64).reshape(-1, 2)
    p = len(row_off) - 1
    max_tracks = min(max(int(np.diff(row_off[:, 1]).max()), 0), t)
    with open(path, "wb") as f:
        f.write(struct.pack("<16q", MAGIC, e, t, s, num_images, p, max_tracks, anchor, opts["init_max_iterations"], opts["max_outer"], opts["max_inner"], *[0] * 5))
        f.write(struct.pack("<16d", opts["scale_factor"], opts["sigma"], opts["huber_k"], opts["init_tol"], opts["delta0"], opts["kappa_cg"], opts["gradient_tol"], opts["rel_tol"],
                            opts["abs_tol"], *[0.0] * 7))
        for a, dt in ((pair_images, np.int32), (np.zeros((0, 3)) if world_pair is None else world_pair, np.float64), (np.ones(e) if pair_enable is None else pair_enable, np.uint8),
                      (track_off, np.int64), (image, np.int32), (np.zeros((0, 3)) if world_meas is None else world_meas, np.float64),
                      (np.ones(s) if meas_enable is None else meas_enable, np.uint8), (row_off, np.int64)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    return p, num_images + max_tracks


def run_program(program, arrays, num_images, row_off, anchor, opts, expect_status=0):
    exe, d = program
    path, out_path = d / "scene.bin", d / "out.bin"
    p, m = write_scene(path, arrays, num_images, row_off, anchor, opts)
    out_path.unlink(missing_ok=True)
    done = run(exe, [path, out_path], expect_status)
    if expect_status:
        return done.stderr
    raw = out_path.read_bytes()
    out, at = {}, 0
    for key, dt, shape in (("translation", np.float64, (p, m, 3)), ("node_valid", np.uint8, (p, m)), ("counters", np.int32, (p, 8)), ("costs", np.float64, (p, 4))):
        count = int(np.prod(shape))
        out[key] = np.frombuffer(raw, dtype=dt, count=count, offset=at).reshape(shape)
        at += count * np.dtype(dt).itemsize
    assert at == len(raw)
    return out


def assert_equals_restatement(out, p, want, what):
    m = len(want["translation"])
    assert out["translation"][p][:m].tobytes() == want["translation"].tobytes(), f"{what}: positions"
    assert out["node_valid"][p][:m].tobytes() == want["node_valid"].tobytes(), f"{what}: node_valid"
    assert not out["node_valid"][p][m:].any() and np.isnan(out["translation"][p][m:]).all(), f"{what}: nodes the problem does not have"
    assert out["counters"][p].tolist() == [want["counters"][k] for k in ref.COUNTER_FIELDS], f"{what}: counters"
    assert out["costs"][p].tobytes() == np.array([want["costs"][k] for k in ref.COST_FIELDS], np.float64).tobytes(), f"{what}: costs"


def whole(sc):
    return [[0, 0], [len(sc["pair_images"]), len(sc["track_off"]) - 1]]


@pytest.mark.parametrize("name", scenes.SCENE_NAMES)
def test_host_build_equals_the_restatement(program, name):
    sc = scenes.get(name)
    want = scenes.expected(name)
    assert sc["check"](want), "the scene does not contain what it is named for"
    out = run_program(program, scenes.arrays_of(sc), sc["num_images"], whole(sc), sc["anchor"], scenes.options_of(sc))
    assert_equals_restatement(out, 0, want, name)


def test_host_build_batch(program):
    """Four problems over ranges of the same arrays: each equals the restatement of its own rows (and the program itself holds each to its solo run)."""
    arrays, off, n, parts = scenes.batch()
    out = run_program(program, arrays, n, off, -1, dict(ref.DEFAULTS))
    for p in range(len(parts)):
        want = ref.solve(*ref.problem_arrays(*arrays, off, p), num_images=n)
        assert_equals_restatement(out, p, want, f"problem {p}")


def test_host_build_permutation_with_the_anchor_given(program):
    """With the anchor given, the order of the pair rows and of a track's measurements changes no byte (row 0, the scale row, stays)."""
    sc = scenes.get("planted_noise")
    anchor = scenes.expected("planted_noise")["counters"]["anchor"]
    a = run_program(program, scenes.arrays_of(sc), sc["num_images"], whole(sc), anchor, scenes.options_of(sc))
    b = run_program(program, scenes.arrays_of(scenes.permuted(sc)), sc["num_images"], whole(sc), anchor, scenes.options_of(sc))
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.mark.parametrize("case", ["unordered_pair", "self_pair", "out_of_range", "negative", "camera", "track_offsets", "track_total", "problem_offsets", "problem_tracks", "anchor", "sigma"])
def test_host_build_refuses_bad_input(program, case):
    pairs = {"unordered_pair": [(1, 0), (1, 2)], "self_pair": [(0, 1), (2, 2)], "out_of_range": [(0, 1), (1, 5)], "negative": [(-1, 1), (1, 2)]}.get(case, [(0, 1), (1, 2)])
    z = np.tile([0.0, 0.0, 1.0], (2, 1))
    track_off = {"track_offsets": [0, 2, 1, 3], "track_total": [0, 1, 2, 2]}.get(case, [0, 1, 2, 3])
    image = [0, 7, 2] if case == "camera" else [0, 1, 2]
    row_off = {"problem_offsets": [[0, 0], [3, 3]], "problem_tracks": [[0, 0], [1, 1], [2, 3]]}.get(case, [[0, 0], [2, 3]])
    opts = dict(ref.DEFAULTS, sigma=0.0) if case == "sigma" else dict(ref.DEFAULTS)
    arrays = (np.asarray(pairs, np.int32), z, None, track_off, image, np.tile([0.0, 1.0, 0.0], (3, 1)), None)
    if case == "problem_tracks":  # the header says one track per problem at the most
        arrays, row_off = arrays[:3] + ([0, 1, 2, 3, 3], image, arrays[5], None), [[0, 0], [1, 1], [2, 2], [2, 4]]
        exe, d = program
        p, m = write_scene(d / "scene.bin", arrays, 3, row_off, -1, opts)
        raw = bytearray((d / "scene.bin").read_bytes())
        raw[6 * 8:7 * 8] = struct.pack("<q", 1)
        (d / "scene.bin").write_bytes(bytes(raw))
        done = run(exe, [d / "scene.bin", d / "out.bin"], 3)
        assert "refused" in done.stderr
        return
    err = run_program(program, arrays, 3, row_off, 9 if case == "anchor" else -1, opts, expect_status=3)
    assert "refused" in err
