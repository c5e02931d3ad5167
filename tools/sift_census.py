"""Prints the census of ``tests/sift_constructed.py`` (events of the numpy restatement of SIFT) for the constructed images and for the five
images of the goldens: ``python tools/sift_census.py > profiles/sift_constructed_census.txt``. CPU only; the two photographs take minutes."""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tests"))
import sift_agreement  # noqa: E402
import sift_constructed as C  # noqa: E402

GOLDEN = REPO / "tests" / "golden"


def main() -> None:
    constructed = {name: C.census(image, C.half_mask(image.shape, 1))[0] for name, image in C.images().items()}
    print("Events of the numpy restatement (tests/sift_reference.py) per image, counted by tests/sift_constructed.py: census() on the CPU.")
    print("The constructed images (with the seeded half mask of the tests):")
    print(C.table(constructed))
    existing = {}
    for name in ("40x48", "123x157", "240x320"):
        g = np.load(GOLDEN / f"sift_{name}.npz")
        existing[name] = C.census(g["gray"], g["mask"] if "mask" in g.files else None)[0]
    for index in (0, 1):
        gray, _ = sift_agreement.load_lund_door(GOLDEN, index)
        existing[f"lund_door_{index}"] = C.census(gray, None)[0]
    print()
    print("The five images of the goldens (three crops, two photographs of 1936 x 1296; every oriented keypoint is described):")
    print(C.table(existing))


if __name__ == "__main__":
    main()
