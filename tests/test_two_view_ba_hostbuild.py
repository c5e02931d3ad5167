"""CPU: the two-view bundle adjustment kernels' own arithmetic (the TVBA_HD functions of gtsfm_amd/csrc/two_view_ba_kernels.hip, lane
loops and lane-0 decisions included), compiled for the host into the stand-alone program tools/two_view_ba_host_main.cpp -- once plain and
once with the host's address and undefined-behaviour sanitizers -- and held to the rule the device is held to
(tests/test_two_view_ba_gpu.py, against the live restatement). The program itself requires its two lane partitions to give byte-equal
outputs: ONE lane that walks each pair's rows in row order and adds every point into the slot of the lane that owns it on the device
(row j -> slot j % 256) over zeroed memory, against the device's 256 lanes per pair, each with the kernel's own lane loop, run in
descending order over memory filled with 0xFF; both combine the 256 slots by the device's tree, which defines the sum. No GPU is
involved."""

import shutil
import struct

import numpy as np
import pytest

from gtsfm_amd.csrc.build import HIPCC
from tests import two_view_ba_reference as ref
from tests import two_view_ba_scenes as scenes
from tests.conftest import REPO
from tests.hostbuild_program import build_program, run

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc is not installed")

SOURCE = REPO / "tools" / "two_view_ba_host_main.cpp"
MAGIC = 0x3141425657544754


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    return build_program(tmp_path_factory, SOURCE, request.param == "sanitized")


def run_program(program, layout, expect_status=0, trace=False, **options):
    """``trace``: also ``out["trace"]``, the lines of the program's trace of rejected trials and stops."""
    exe, d = program
    opt = {**ref.DEFAULTS, **options}
    p, m = len(layout["kp_off1"]), len(layout["match_idx"])
    path, out_path = d / "scene.bin", d / "out.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<8q", MAGIC, p, m, len(layout["kp_xy"]), opt["max_iterations"], opt["min_verified"], int(opt["allow_indeterminate"]), 1))
        f.write(struct.pack("<8d", opt["reproj_error_threshold"], opt["huber_k"], opt["measurement_sigma"], opt["pose_prior_sigma"], opt["point_prior_sigma"],
                            opt["triangulation_threshold"], opt["triangulation_min_angle_deg"], 0.0))
        for k, dt in (("kp_xy", np.float32), ("kp_off1", np.int64), ("kp_off2", np.int64), ("match_idx", np.int32), ("match_off", np.int64), ("match_count", np.int32),
                      ("inlier_mask", np.uint8), ("intrinsics", np.float64), ("rotation", np.float64), ("translation", np.float64)):
            f.write(np.ascontiguousarray(layout[k], dtype=dt).tobytes())
    out_path.unlink(missing_ok=True)
    done = run(exe, [path, out_path, *([str(d / "trace.txt")] if trace else [])], expect_status)
    if expect_status:
        return done.stderr
    raw = out_path.read_bytes()
    assert len(raw) % 2 == 0 and raw[: len(raw) // 2] == raw[len(raw) // 2 :], "the two runs differ"
    out, at = {}, 0
    for k, dt, n in (("rotation", np.float64, 9 * p), ("translation", np.float64, 3 * p), ("valid_mask", np.uint8, m), ("point", np.float64, 3 * m), ("cost", np.float64, 2 * p),
                     ("stats", np.int32, 8 * p)):
        out[k] = np.frombuffer(raw, dtype=dt, count=n, offset=at)
        at += n * np.dtype(dt).itemsize
    assert 2 * at == len(raw)
    out["rotation"], out["translation"], out["point"] = out["rotation"].reshape(p, 3, 3), out["translation"].reshape(p, 3), out["point"].reshape(m, 3)
    out["cost"], out["stats"] = out["cost"].reshape(p, 2), out["stats"].reshape(p, 8)
    if trace:
        out["trace"] = [line.split() for line in (d / "trace.txt").read_text().splitlines()]
    return out


@pytest.fixture(scope="module")
def scene():
    from tests.test_two_view_ba_gpu import scene_pairs

    names, pairs = scene_pairs()
    return {"names": names, "pairs": pairs, "layout": scenes.capacity_layout(pairs)}


def test_host_build_against_the_restatement(program, scene):
    """The GPU suite's rule (tests/test_two_view_ba_gpu.py) for the whole scene: every status, the lane-count boundaries, the door pair.
    Rows past match_count hold index -1 and a mask of 1: under the sanitizers, reading a keypoint through them is a report."""
    from tests.test_two_view_ba_gpu import compare_pair, expected_and_tolerance

    if "expected" not in scene:  # shared by the two builds: their outputs are the same bytes
        entering = run_program(program, scene["layout"], max_iterations=0)["point"]
        scene["expected"], scene["tolerance"] = expected_and_tolerance(scene["names"], scene["pairs"], scene["layout"], entering)
        scene["entering"] = entering
    out = run_program(program, scene["layout"])
    assert run_program(program, scene["layout"], max_iterations=0)["point"].tobytes() == scene["entering"].tobytes()
    assert sum(e["non_decisive"] for e in scene["expected"]) <= len(scene["pairs"]) // 16
    failures = []
    for p, (name, rows, exp) in enumerate(zip(scene["names"], scene["layout"]["rows"], scene["expected"])):
        try:
            compare_pair(name, out, p, rows, exp, scene["tolerance"])
        except AssertionError as e:
            failures.append(f"{name}: {e}")
    assert not failures, "\n".join(failures)


def test_host_build_flags_bad_offsets(program, scene):
    layout = dict(scenes.capacity_layout(scene["pairs"][2:4]))
    layout["match_off"] = layout["match_off"].copy()
    layout["match_off"][1] = layout["match_off"][2] + 1
    run_program(program, layout, expect_status=3)


# ---- the catalogue of hard pairs: proven here before a GPU sees it

HARD_CACHE = {}  # the restatement runs, shared by the two builds: their entering points are the same bytes


@pytest.fixture(scope="module")
def hard():
    return scenes.hard_pairs()


@pytest.mark.parametrize("family", scenes.HARD_FAMILIES)
def test_host_build_hard_family(program, hard, family):
    """tests/test_two_view_ba_gpu.py's rule for one family of the catalogue, the tolerance measured on that family."""
    from tests.test_two_view_ba_gpu import check_non_finite_family, run_family

    records = run_family(lambda layout, **o: run_program(program, layout, **o), family, hard[family], cache=HARD_CACHE)
    if family == "non_finite":
        check_non_finite_family(records)


def test_host_build_dud_rows(program, hard):
    """A verified row without a keypoint index or with a NaN pixel: under the sanitizers, reading a keypoint through index -1 is a report."""
    from tests.test_two_view_ba_gpu import check_dud_rows

    run = lambda layout, **o: run_program(program, layout, **o)  # noqa: E731
    check_dud_rows(run, hard["rejections"][0]["pair"])
    check_dud_rows(run, scenes.make_pair(102, 14), verified_decides=True)


def test_host_build_rejection_routes(program, hard):
    """Which way each rejected trial goes in the kernel's arithmetic, from the program's trace. On the non-finite pair the restatement
    rejects all 11 trials by a trial cost that is not finite (its weights k / inf = 0 are applied first, so its blocks are exact zeros and its
    step is zero); the kernel's arithmetic applies the weight last, 0 x inf = NaN poisons the sums, and all 11 go by the failed solve. Only
    the discrete outputs have to agree, and do (test_host_build_hard_family). A far start is rejected by the fidelity test in both."""
    entry = hard["non_finite"][0]
    out = run_program(program, scenes.capacity_layout([entry["pair"]]), trace=True, **entry["options"])
    print("non_finite:", out["trace"])
    assert [line[3] for line in out["trace"][:-1]] == ["poisoned"] * 11 and out["trace"][-1] == ["0", "stop", "lambda_bound"]
    assert float(out["trace"][0][2]) == ref.LAMBDA_INITIAL
    assert float(out["trace"][-2][2]) <= ref.LAMBDA_UPPER < float(out["trace"][-2][2]) * ref.LAMBDA_FACTOR
    entry = hard["rejections"][0]
    layout = scenes.capacity_layout([entry["pair"]])
    out = run_program(program, layout, trace=True)
    entering = run_program(program, layout, max_iterations=0)["point"]
    pair = entry["pair"]
    exp = ref.two_view_ba(pair["k1"], pair["k2"], pair["uv1"], pair["uv2"], pair["R"], pair["t"], initial_points=entering[layout["rows"][0]])
    assert not exp["non_decisive"] and exp["rejected"]["fidelity"] == sum(exp["rejected"].values()) >= 10
    assert [line[3] for line in out["trace"][:-1]] == ["fidelity"] * exp["rejected"]["fidelity"] and out["trace"][-1] == ["0", "stop", exp["stop"]]
