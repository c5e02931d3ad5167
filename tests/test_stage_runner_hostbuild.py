"""CPU: the host side of the stage runner (gtsfm_amd/csrc/stage_runner.h: HostRunner's each, group, scan, fetch and zero), compiled for the
host into the stand-alone program tools/stage_runner_host_main.cpp -- once plain and once with the host's address and undefined-behaviour
sanitizers. The program runs each under both host settings (ascending with one lane per group; descending with the stage's lane count) on
arrays of their exact size: ``each`` over 0, 1, 255, 256 and 257 indices; ``group`` over (1, 1), (3, 64) and (0, 64); ``scan`` over 0, 1,
4096 and 4097 values against a plain loop of its own; ``fetch`` and ``zero`` with guarded neighbours. It runs as its own process; no
sanitizer is loaded into Python and no GPU is involved. The device side is held at the same sizes through the existing entry points
(tests/test_view_graph_gpu.py, tests/test_translation_inliers_gpu.py)."""

import shutil

import pytest

from gtsfm_amd.csrc.build import HIPCC
from tests.conftest import REPO
from tests.hostbuild_program import build_program, run

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc is not installed")

SOURCE = REPO / "tools" / "stage_runner_host_main.cpp"


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "sanitized"])
def test_host_runner_equals_plain_loops(tmp_path_factory, sanitized):
    exe, _ = build_program(tmp_path_factory, SOURCE, sanitized)
    done = run(exe, [])
    assert "equal the plain loops" in done.stdout
