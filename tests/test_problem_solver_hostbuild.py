"""CPU: the scaffold the per-problem solvers share (gtsfm_amd/csrc/problem_solver.h: solver_scan, solver_tree and the per-node reductions,
solver_build_lists, solver_component), compiled for the host into the stand-alone program tools/problem_solver_host_main.cpp -- once plain
and once with the host's address and undefined-behaviour sanitizers. The program runs each on tiny inputs (scans of 0, 1, 255, 256 and 257
values; trees of 1, 2 and 5 nodes; lists over 6 nodes with a node of degree 0, a repeated pair and an invalid row; the component of an
anchor without a row, of a path of 5 nodes and with two components) with one lane, 256 lanes last lane first and 64 lanes, and compares
every output byte for byte with plain loops of its own. It runs as its own process; no sanitizer is loaded into Python and no GPU is
involved."""

import shutil

import pytest

from gtsfm_amd.csrc.build import HIPCC
from tests.conftest import REPO
from tests.hostbuild_program import build_program, run

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc is not installed")

SOURCE = REPO / "tools" / "problem_solver_host_main.cpp"


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "sanitized"])
def test_shared_scaffold_equals_plain_loops(tmp_path_factory, sanitized):
    exe, _ = build_program(tmp_path_factory, SOURCE, sanitized)
    done = run(exe, [])
    assert "equal the plain loops" in done.stdout
