"""CPU: the view-graph kernels' own per-index functions (the GTSFM_HD functions of gtsfm_amd/csrc/view_graph_kernels.hip), compiled for the host
into the stand-alone program tools/view_graph_host_main.cpp -- once plain and once with the host's address and undefined-behaviour
sanitizers -- on every scene of tests/view_graph_scenes.py, held to the rule the device is held to (tests/test_view_graph_gpu.py): the
discrete outputs equal the restatement's, the values lie within the measured tolerance. The program itself requires its two runs to give
byte-equal outputs: ascending indices with one lane per edge over zeroed memory against descending indices with 64 lanes per edge over
memory filled with 0xFF. No GPU is involved. The distances go to profiles/view_graph_host_tests.txt by hand (``-s`` shows them)."""

import shutil
import struct

import numpy as np
import pytest

from gtsfm_amd.csrc.build import HIPCC
from tests import view_graph_reference as ref
from tests import view_graph_scenes as scenes
from tests.conftest import REPO
from tests.hostbuild_program import build_program, run

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc is not installed")

SOURCE = REPO / "tools" / "view_graph_host_main.cpp"
MAGIC = 0x3148505247574956


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    return build_program(tmp_path_factory, SOURCE, request.param == "sanitized")


def run_program(program, sc, criterion, threshold, expect_status=0):
    exe, d = program
    pairs, rot = np.ascontiguousarray(sc["pair_images"], np.int32), np.ascontiguousarray(sc["rotation"], np.float64)
    e, n = len(pairs), int(sc["num_images"])
    enable = np.ones(e, np.uint8) if sc["enable"] is None else np.ascontiguousarray(sc["enable"], np.uint8)
    path, out_path = d / "scene.bin", d / "out.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<8q", MAGIC, e, n, 0 if sc["enable"] is None else 1, criterion, 0, 0, 0))
        f.write(struct.pack("<8d", threshold, 0, 0, 0, 0, 0, 0, 0))
        f.write(pairs.tobytes() + rot.tobytes() + enable.tobytes())
    out_path.unlink(missing_ok=True)
    done = run(exe, [path, out_path], expect_status)
    if expect_status:
        return done.stderr
    raw = out_path.read_bytes()
    assert len(raw) % 2 == 0 and raw[: len(raw) // 2] == raw[len(raw) // 2:], "the two runs differ"
    out, at = {}, 0

    def take(key, dt, count):
        nonlocal at
        out[key] = np.frombuffer(raw, dtype=dt, count=count, offset=at)
        at += count * np.dtype(dt).itemsize

    take("num_triplets", np.int32, e), take("aggregate_error", np.float64, e), take("keep", np.uint8, e), take("counts", np.int32, 8), take("total", np.int64, 1)
    t = int(out["total"][0])
    take("triplets", np.int32, 3 * t), take("cycle_error", np.float64, t), take("node_mask", np.uint8, n), take("pair_keep", np.uint8, e), take("component_counts", np.int32, 8)
    assert 2 * at == len(raw)
    return out


@pytest.mark.parametrize("name", scenes.SCENE_NAMES)
def test_host_build_against_the_restatement(program, name):
    sc = {s["name"]: s for s in scenes.all_scenes()}[name]
    tol = scenes.measured_tolerance(name)  # a hard scene is held to its own measured distance, every other scene to that of the first scenes
    for criterion in (ref.MIN_EDGE_ERROR, ref.MEDIAN_EDGE_ERROR):
        for thr in sc["thresholds"]:
            got = run_program(program, sc, criterion, thr)
            dist = scenes.check_outputs(f"{name}/{criterion}/{thr}", got, scenes.expected(sc, criterion, thr), tol["tolerance"], exact_zero=tol["exact_zero"])
            print(f"{name} criterion {criterion} threshold {thr:.6g}: {len(sc['pair_images'])} edges, {int(got['total'][0])} triplets, aggregate within {dist['aggregate_error']:.3e}, "
                  f"cycle error within {dist['cycle_error']:.3e} degrees (restatement from 50 digits {tol['restatement']:.3e}, tolerance {tol['tolerance']:.3e})")
    if name in scenes.HARD_SCENES:
        print(f"{name}: " + ", ".join(f"{k} {v}" for k, v in tol.items() if k not in ("restatement", "tolerance", "exact_zero")))


@pytest.mark.parametrize("case", ["reversed", "duplicate", "out_of_range", "negative"])
def test_host_build_refuses_bad_edges(program, case):
    pairs = {"reversed": [(0, 1), (2, 1), (0, 2)], "duplicate": [(0, 1), (1, 2), (0, 1)], "out_of_range": [(0, 1), (1, 5)], "negative": [(-1, 1), (1, 2)]}[case]
    sc = scenes.scene(case, [(0, 1)] * len(pairs), num_images=3)
    sc["pair_images"] = np.asarray(pairs, np.int32)
    assert "refused" in run_program(program, sc, ref.MEDIAN_EDGE_ERROR, 7.0, expect_status=3)
