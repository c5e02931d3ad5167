"""Write tests/golden/twoway_lund_door_sift.npz: the Lund-door SIFT descriptors GTSfM ships as test data
(``tests/data/set1_lund_door/features/descriptors_{0,1}.npy`` in a GTSfM checkout, float32 holding integers 0..221) stored as uint8
(lossless), and the expected TwoWayMatcher output for ratio_test_threshold 0.8 and None from the restatement in
tests/twoway_reference.py (exact for integer descriptors).

Usage: python tools/make_twoway_fixture.py <gtsfm checkout>
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from tests.twoway_reference import twoway_match  # noqa: E402

OUT = REPO / "tests" / "golden" / "twoway_lund_door_sift.npz"


def main(gtsfm_root: str) -> None:
    feats = Path(gtsfm_root) / "tests" / "data" / "set1_lund_door" / "features"
    desc = []
    for i in (0, 1):
        d = np.load(feats / f"descriptors_{i}.npy")
        assert d.dtype == np.float32 and np.array_equal(d, np.round(d)) and d.min() >= 0 and d.max() <= 255, "expected integer SIFT"
        desc.append(d.astype(np.uint8))
    assert all(np.array_equal(u.astype(np.float32), np.load(feats / f"descriptors_{i}.npy")) for i, u in enumerate(desc))
    f0, f1 = (d.astype(np.float32) for d in desc)
    expected_r08 = twoway_match(f0, f1, ratio=0.8)
    expected_none = twoway_match(f0, f1, ratio=None)
    np.savez_compressed(OUT, descriptors_0=desc[0], descriptors_1=desc[1], expected_ratio_0_8=expected_r08, expected_no_ratio=expected_none)
    print(f"{OUT}: {OUT.stat().st_size} bytes; {len(expected_r08)} matches (ratio 0.8), {len(expected_none)} (no ratio test)")


if __name__ == "__main__":
    main(sys.argv[1])
