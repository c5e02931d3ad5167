"""CPU: the 1DSfM kernels' own per-lane functions (the GTSFM_HD functions of gtsfm_amd/csrc/translation_kernels.hip), compiled for the host into
the stand-alone program tools/translation_inliers_host_main.cpp -- once plain and once with the host's address and undefined-behaviour
sanitizers -- on every scene of tests/translation_inliers_scenes.py. The program runs each scene twice -- one lane, ascending indices, zeroed
memory; the device's 256-lane partition, descending indices, memory filled with 0xFF -- and the two outputs must be byte-equal to each other
and to the restatement (tests/translation_inliers_reference.py), positions included. The program runs as its own process; no sanitizer is
loaded into Python and no GPU is involved."""

import shutil
import struct

import numpy as np
import pytest

from gtsfm_amd.csrc.build import HIPCC
from tests import translation_inliers_scenes as scenes
from tests.conftest import REPO
from tests.hostbuild_program import build_program, run

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc is not installed")

SOURCE = REPO / "tools" / "translation_inliers_host_main.cpp"
MAGIC = 0x31534E4952544D46


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    return build_program(tmp_path_factory, SOURCE, request.param == "sanitized")


def write_scene(path, sc):
    e, s, n, t, d = len(sc["pair_images"]), len(sc["image"]), int(sc["num_images"]), len(sc["track_off"]) - 1, len(sc["directions"])
    given = sc["world"] is not None
    world = sc["world"] if given else (np.zeros((e, 3)), np.zeros((s, 3)))
    with open(path, "wb") as f:
        f.write(struct.pack("<16q", MAGIC, e, s, n, t, d, 0 if sc["pair_enable"] is None else 1, 0 if sc["meas_enable"] is None else 1, 1 if given else 0, *[0] * 7))
        f.write(struct.pack("<8d", sc["threshold"], *[0.0] * 7))
        for a, dt in ((sc["pair_images"], np.int32), (sc["pair_direction"], np.float64), (np.ones(e) if sc["pair_enable"] is None else sc["pair_enable"], np.uint8),
                      (sc["rotation"], np.float64), (sc["rotation_valid"], np.uint8), (sc["intrinsics"], np.float64), (sc["track_off"], np.int64), (sc["image"], np.int32),
                      (sc["uv"], np.float32), (sc["track_enable"], np.uint8), (np.ones(s) if sc["meas_enable"] is None else sc["meas_enable"], np.uint8),
                      (sc["directions"], np.float64), (world[0], np.float64), (world[1], np.float64)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    return e, s, n, t, d


def run_program(program, sc, expect_status=0):
    exe, d = program
    path, out_path = d / "scene.bin", d / "out.bin"
    e, s, n, t, dn = write_scene(path, sc)
    out_path.unlink(missing_ok=True)
    done = run(exe, [path, out_path], expect_status)
    if expect_status:
        return done.stderr
    raw = out_path.read_bytes()
    assert len(raw) % 2 == 0 and raw[: len(raw) // 2] == raw[len(raw) // 2:], "the two runs differ"
    out, at = {}, 0
    for key, dt, shape in (("world_pair", np.float64, (e, 3)), ("world_meas", np.float64, (s, 3)), ("pair_weight", np.float64, (e,)), ("meas_weight", np.float64, (s,)),
                           ("pair_inlier", np.uint8, (e,)), ("meas_inlier", np.uint8, (s,)), ("camera_inlier", np.uint8, (n,)), ("position", np.int32, (dn, n + t)),
                           ("counts", np.int32, (8,))):
        count = int(np.prod(shape))
        out[key] = np.frombuffer(raw, dtype=dt, count=count, offset=at).reshape(shape)
        at += count * np.dtype(dt).itemsize
    assert 2 * at == len(raw)
    return out


@pytest.mark.parametrize("name", scenes.SCENE_NAMES)
def test_host_build_equals_the_restatement(program, name):
    scenes.assert_bytes_equal(name, run_program(program, scenes.get(name)), scenes.expected(name))


@pytest.mark.parametrize("case", ["reversed", "duplicate", "out_of_range", "negative", "duplicate_measurement", "camera_out_of_range", "camera_without_rotation", "no_direction"])
def test_host_build_refuses_bad_rows(program, case):
    pairs = {"reversed": [(0, 1), (2, 1)], "duplicate": [(0, 1), (1, 2), (0, 1)], "out_of_range": [(0, 1), (1, 5)], "negative": [(-1, 1), (1, 2)]}.get(case, [(0, 1), (1, 2)])
    tracks = {"duplicate_measurement": [[0, 1, 1]], "camera_out_of_range": [[0, 1, 3]], "camera_without_rotation": [[0, 1, 2]]}.get(case, [])
    valid = [1, 1, 0] if case == "camera_without_rotation" else [1, 1, 1]
    sc = scenes.scene(case, [(0, 1)] * len(pairs), np.tile([0.0, 0.6, 0.8], (len(pairs), 1)), 3, np.zeros((0, 3)) if case == "no_direction" else [[1.0, 0.0, 0.0]], tracks=tracks,
                      rotation_valid=valid)
    sc["pair_images"] = np.asarray(pairs, np.int32)
    assert "refused" in run_program(program, sc, expect_status=3)
