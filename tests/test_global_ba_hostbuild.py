"""CPU: the global bundle adjustment itself (gba_validate and gba_solve of gtsfm_amd/csrc/global_ba_kernels.hip, the functions the kernels
run), compiled for the host into the stand-alone program tools/global_ba_host_main.cpp -- once plain and once with the host's address and
undefined-behaviour sanitizers -- on every scene of tests/global_ba_scenes.py. The program solves each scene with one lane over zeroed memory
and with the device's 256-lane partition, last lane first, over memory filled with 0xFF, and every problem of a batch alone as well; all must
be byte-equal to each other and to the restatement (tests/global_ba_reference.py) in every output. The program runs as its own process; no
sanitizer is loaded into Python and no GPU is involved."""

import shutil
import struct

import numpy as np
import pytest

from gtsfm_amd.csrc.build import HIPCC
from tests import global_ba_reference as ref
from tests import global_ba_scenes as scenes
from tests.conftest import REPO
from tests.hostbuild_program import build_program, run

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc is not installed")

SOURCE = REPO / "tools" / "global_ba_host_main.cpp"
MAGIC = 0x3141424C47524D46
OUTPUTS = ("cameras", "point", "reproj_error", "track_valid", "camera_kept", "node_valid")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    return build_program(tmp_path_factory, SOURCE, request.param == "sanitized")


def write_scene(path, arrays, problem_off, anchor, opts, max_tracks=None):
    cameras, track_off, image, uv, point, track_enable, meas_enable = arrays
    n, t, s = len(cameras), len(track_off) - 1, len(image)
    problem_off = np.asarray(problem_off, np.int64).reshape(-1)
    p = len(problem_off) - 1
    if max_tracks is None:
        max_tracks = min(max(int(np.diff(problem_off).max()), 0), t)
    with open(path, "wb") as f:
        f.write(struct.pack("<16q", MAGIC, n, t, s, p, max_tracks, anchor, opts["min_track_length"], opts["max_iterations"], opts["max_inner"], *[0] * 6))
        f.write(struct.pack("<16d", opts["measurement_sigma"], opts["huber_k"], opts["reproj_error_threshold"], opts["rel_tol"], opts["abs_tol"], opts["cg_forcing"], *[0.0] * 10))
        for a, dt in ((cameras, np.float64), (track_off, np.int64), (image, np.int32), (uv, np.float32), (point, np.float64), (np.ones(t) if track_enable is None else track_enable, np.uint8),
                      (np.ones(s) if meas_enable is None else meas_enable, np.uint8), (problem_off, np.int64)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    return p, n, n + max_tracks, t, s


def run_program(program, arrays, problem_off, anchor, opts, expect_status=0, max_tracks=None):
    exe, d = program
    path, out_path = d / "scene.bin", d / "out.bin"
    p, n, m, t, s = write_scene(path, arrays, problem_off, anchor, opts, max_tracks)
    out_path.unlink(missing_ok=True)
    done = run(exe, [path, out_path], expect_status)
    if expect_status:
        return done.stderr
    raw = out_path.read_bytes()
    out, at = {}, 0
    for key, dt, shape in (("cameras", np.float64, (p, n, 17)), ("point", np.float64, (t, 3)), ("reproj_error", np.float64, (s,)), ("track_valid", np.uint8, (t,)),
                           ("camera_kept", np.uint8, (p, n)), ("node_valid", np.uint8, (p, m)), ("counters", np.int32, (p, 8)), ("costs", np.float64, (p, 4))):
        count = int(np.prod(shape))
        out[key] = np.frombuffer(raw, dtype=dt, count=count, offset=at).reshape(shape)
        at += count * np.dtype(dt).itemsize
    assert at == len(raw)
    return out


def assert_equals_restatement(out, p, want, what, tlo=0, mlo=0):
    t, s, m = len(want["point"]), len(want["reproj_error"]), len(want["node_valid"])
    got = {"cameras": out["cameras"][p], "point": out["point"][tlo:tlo + t], "reproj_error": out["reproj_error"][mlo:mlo + s], "track_valid": out["track_valid"][tlo:tlo + t],
           "camera_kept": out["camera_kept"][p], "node_valid": out["node_valid"][p][:m]}
    for k in OUTPUTS:
        assert got[k].tobytes() == want[k].tobytes(), f"{what}: {k}"
    assert not out["node_valid"][p][m:].any(), f"{what}: nodes the problem does not have"
    assert out["counters"][p].tolist() == [want["counters"][k] for k in ref.COUNTER_FIELDS], f"{what}: counters"
    assert out["costs"][p].tobytes() == np.array([want["costs"][k] for k in ref.COST_FIELDS], np.float64).tobytes(), f"{what}: costs {out['costs'][p]} {want['costs']}"


def whole(sc):
    return [0, len(sc["track_off"]) - 1]


@pytest.mark.parametrize("name", scenes.SCENE_NAMES)
def test_host_build_equals_the_restatement(program, name):
    sc = scenes.get(name)
    want = scenes.expected(name)
    assert sc["check"](want), "the scene does not contain what it is named for"
    out = run_program(program, scenes.arrays_of(sc), whole(sc), sc["anchor"], scenes.options_of(sc))
    assert_equals_restatement(out, 0, want, name)


def test_host_build_batch(program):
    """Three problems over ranges of the same arrays: each equals the restatement of its own tracks (and the program itself holds each to its solo run)."""
    arrays, off, parts = scenes.batch()
    out = run_program(program, arrays, off, -1, dict(ref.DEFAULTS))
    for p in range(len(parts)):
        want = ref.solve(arrays[0], *ref.problem_arrays(*arrays[1:], off, p))
        assert want["counters"]["status"] == ref.CONVERGED
        assert_equals_restatement(out, p, want, f"problem {p}", tlo=int(off[p]), mlo=int(arrays[1][off[p]]))


@pytest.mark.parametrize("name", ["planted_noise", "gaps", "long_track"])
def test_host_build_measurement_permutation(program, name):
    """The order of a track's measurements changes no byte but the places of the reprojection errors."""
    sc = scenes.get(name)
    moved = scenes.permuted(sc)
    a = run_program(program, scenes.arrays_of(sc), whole(sc), sc["anchor"], scenes.options_of(sc))
    b = run_program(program, scenes.arrays_of(moved), whole(sc), sc["anchor"], scenes.options_of(sc))
    assert all(a[k].tobytes() == b[k].tobytes() for k in a if k != "reproj_error")
    key = lambda x, e: sorted(zip(np.repeat(np.arange(len(x["track_off"]) - 1), np.diff(x["track_off"])).tolist(), x["image"].tolist(), e.view(np.int64).tolist()))  # noqa: E731
    assert key(sc, a["reproj_error"]) == key(moved, b["reproj_error"])


@pytest.mark.parametrize("case", ["track_offsets", "track_total", "track_first", "problem_offsets", "problem_total", "problem_tracks", "anchor", "sigma", "threshold"])
def test_host_build_refuses_bad_input(program, case):
    sc = scenes.get("two_cameras_eight_points")
    arrays = list(scenes.arrays_of(sc))
    off = {"track_offsets": [0, 2, 6, 4, 8, 10, 12, 14, 16], "track_total": [0, 2, 4, 6, 8, 10, 12, 14, 15], "track_first": [1, 2, 4, 6, 8, 10, 12, 14, 16]}.get(case)
    if off is not None:
        arrays[1] = np.asarray(off, np.int64)
    problem_off = {"problem_offsets": [0, 5, 3, 8], "problem_total": [0, 4, 7], "problem_tracks": [0, 2, 8]}.get(case, [0, 8])
    opts = dict(ref.DEFAULTS, **{"sigma": {"measurement_sigma": 0.0}, "threshold": {"reproj_error_threshold": 0.0}}.get(case, {}))
    err = run_program(program, tuple(arrays), problem_off, 5 if case == "anchor" else -1, opts, expect_status=3, max_tracks=3 if case == "problem_tracks" else None)
    assert "refused" in err
