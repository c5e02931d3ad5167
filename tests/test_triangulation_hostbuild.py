"""CPU: the triangulation kernels' own per-track arithmetic (the TRI_HD functions of gtsfm_amd/csrc/triangulation_kernels.hip), compiled
for the host into the stand-alone program tools/triangulation_host_main.cpp -- once plain and once with the host's address and
undefined-behaviour sanitizers -- and held to the rule the device is held to (``arbiter.accept`` against the hard-scene fixture; the
restatement's existing rule on ``small_shapes()``). The program itself requires its two lane partitions (one lane; the device's
select / grid-stride pattern over a workspace filled with 0xFF) to give byte-equal outputs. No GPU is involved."""

import shutil
import struct

import numpy as np
import pytest

from gtsfm_amd.csrc.build import HIPCC
from tests import triangulation_reference as ref
from tests import triangulation_scenes as scenes
from tests.conftest import REPO
from tests.hostbuild_program import build_program, run
from tests.test_triangulation_arbiter_host import FAMILIES, held_to_rule

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc is not installed")

SOURCE = REPO / "tools" / "triangulation_host_main.cpp"
MAGIC = 0x3149525453464754


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    return build_program(tmp_path_factory, SOURCE, request.param == "sanitized")


def run_program(program, scene, expect_status=0, **opts):
    exe, d = program
    off, image, uv, table = scene["track_off"], scene["image"], scene["uv"], scene["cameras"]
    t, s = len(off) - 1, len(image)
    path, out_path = d / "scene.bin", d / "out.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<8q", MAGIC, t, s, len(table), opts.get("mode", 0), opts.get("num_hypotheses", 2749), opts.get("seed", 0), 0))
        f.write(struct.pack("<2d", opts.get("threshold", np.inf), opts.get("min_angle_deg", 0.0)))
        for a, dt in ((off, np.int64), (image, np.int32), (uv, np.float32), (table, np.float64)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    out_path.unlink(missing_ok=True)
    done = run(exe, [path, out_path], expect_status)
    if expect_status:
        return done.stderr
    raw = out_path.read_bytes()
    assert len(raw) % 2 == 0 and raw[: len(raw) // 2] == raw[len(raw) // 2 :], "the two lane partitions differ"
    out, at = {}, 0
    for k, dt, n in (("point", np.float64, 3 * t), ("avg_error", np.float64, t), ("exit_code", np.int32, t), ("inlier_mask", np.uint8, s), ("stats", np.int32, 4 * t)):
        out[k] = np.frombuffer(raw, dtype=dt, count=n, offset=at)
        at += n * np.dtype(dt).itemsize
    assert 2 * at == len(raw)
    out["point"], out["stats"] = out["point"].reshape(t, 3), out["stats"].reshape(t, 4)
    return out


@pytest.mark.parametrize("name", list(FAMILIES))
def test_host_build_on_the_hard_fixture(program, name):
    """Includes the hostile-index families: under the sanitizers a read outside the camera table is a report."""
    fam = FAMILIES[name]
    out = run_program(program, fam, **fam["options"])
    held_to_rule(fam, out, f"host build ({program[0].parent.name}), {name}")


@pytest.fixture(scope="module")
def small():
    scene = scenes.small_shapes()
    scene["tolerance"] = scenes.reversal_tolerance(scene)
    return scene


SMALL_CASES = [dict(mode=ref.NO_RANSAC), dict(mode=ref.NO_RANSAC, threshold=10.0, min_angle_deg=3.0), dict(mode=ref.RANSAC_SAMPLE_UNIFORM, min_angle_deg=3.0, seed=9, **scenes.LOOSE),
               dict(mode=ref.RANSAC_SAMPLE_BIASED_BASELINE, **scenes.LOOSE), dict(mode=ref.RANSAC_TOPK_BASELINES, **scenes.LOOSE)]


@pytest.mark.parametrize("case", range(len(SMALL_CASES)))
def test_host_build_on_small_shapes(program, small, case):
    """The GPU suite's rule for this scene (tests/test_triangulation_gpu.py), against the live restatement."""
    from tests.test_triangulation_gpu import assert_matches

    opts = SMALL_CASES[case]
    key = tuple(sorted(opts.items()))
    if key not in small:
        small[key] = ref.triangulate_tracks(small["cameras"], small["track_off"], small["image"], small["uv"], **opts)
    out = run_program(program, small, **opts)
    assert_matches(out, small[key], small["track_off"], small[key]["non_decisive"], *small["tolerance"], f"host build, small shapes {opts}")


def test_host_build_grid_stride_and_flags(program, small):
    """527 800 hypotheses: more than 2048 x 256 lanes, so the device partition's stride loop runs twice (the program compares it with the
    one-lane run). 5 800 copies of a 14-measurement track, all 91 pairs each: the sampler's quadratic ranking would dominate with the
    75-measurement track. Offsets that do not ascend, and a track longer than 65 535, end with the first error flag's status."""
    j = int(np.where(np.diff(small["track_off"]) == 14)[0][0])
    a, b = small["track_off"][j : j + 2]
    copies = 5800
    scene = {"cameras": small["cameras"], "track_off": np.arange(copies + 1, dtype=np.int64) * (b - a), "image": np.tile(small["image"][a:b], copies),
             "uv": np.tile(small["uv"][a:b], (copies, 1))}
    out = run_program(program, scene, mode=ref.RANSAC_SAMPLE_UNIFORM, **scenes.LOOSE)
    assert (out["stats"][:, 0] == 91).all() and out["stats"][:, 0].sum() > 2048 * 256
    for k in ("point", "avg_error", "exit_code", "stats"):
        assert out[k].tobytes() == out[k][:1].tobytes() * copies, k
    assert out["inlier_mask"].tobytes() == out["inlier_mask"][: b - a].tobytes() * copies and out["exit_code"][0] == ref.SUCCESS
    bad = dict(small)
    bad["track_off"] = small["track_off"].copy()
    bad["track_off"][5] = bad["track_off"][4] - 1
    run_program(program, bad, expect_status=3)
    long = {"cameras": small["cameras"], "track_off": np.array([0, 65536], np.int64), "image": np.zeros(65536, np.int32), "uv": np.zeros((65536, 2), np.float32)}
    run_program(program, long, expect_status=3)
