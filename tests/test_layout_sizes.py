"""Host only: every size function of the image models, SuperPoint, the two-way matcher and the learned matchers returns what
``tests/golden/layout_sizes.json`` recorded (``tools/record_layout_sizes.py``, run against the library as it was before the layouts
moved onto ``WorkspaceCarver`` and ``vgg_trunk.h``), and the packed NetVLAD / D2-Net blobs of the seeded weights hash as they did. A
workspace piece that moved or changed size, or a blob offset that shifted, shows here without a GPU."""

from __future__ import annotations

import importlib.util
import json
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location("record_layout_sizes", REPO / "tools" / "record_layout_sizes.py")
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

GOLDEN = json.loads(rec.GOLDEN.read_text())


@pytest.fixture(autouse=True)
def _default_environment(monkeypatch):
    """The matcher sizes were recorded with no ``GTSFM_*`` switch set (the attention and GEMM modes change what the matchers park in
    the workspace); ``GTSFM_LIB`` only chooses which library is asked."""
    import os

    for name in [n for n in os.environ if n.startswith("GTSFM_") and n != "GTSFM_LIB"]:
        monkeypatch.delenv(name)


def test_the_recording_covers_the_tools_cases():
    assert {name: [args for args, _ in rows] for name, rows in GOLDEN["sizes"].items()} == rec.cases()
    assert 100 <= sum(len(rows) for rows in GOLDEN["sizes"].values()) <= 500


@pytest.mark.parametrize("name", sorted(GOLDEN["sizes"]))
def test_size_function_returns_the_recorded_sizes(name):
    from gtsfm_amd.runtime import lib as _lib

    lib = _lib.load()
    got = [[args, rec.call(lib, name, args)] for args, _ in GOLDEN["sizes"][name]]
    assert got == GOLDEN["sizes"][name]


def test_packed_blobs_hash_as_recorded():
    assert rec.blob_hashes() == GOLDEN["blobs"]
