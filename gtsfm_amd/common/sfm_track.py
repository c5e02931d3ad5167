"""``SfmMeasurement`` / ``SfmTrack2d`` boundary types.

When GTSfM is importable, ``gtsfm.common.sfm_track`` is re-exported unchanged, so the track estimators hand the rest of the pipeline
the reference's own classes. GTSfM cannot be imported in the build container (cv2 / gtsam are missing); the stand-ins
below restate the interface (``gtsfm/common/sfm_track.py:17-112``): the fields ``i`` / ``uv`` and ``measurements``, the accessors, and
an equality that ignores the order of a track's measurements.
"""

from __future__ import annotations

from typing import Iterable, List, NamedTuple

import numpy as np

try:  # pragma: no cover - exercised only where GTSfM is installed
    from gtsfm.common.sfm_track import SfmMeasurement, SfmTrack2d  # type: ignore  # noqa: F401
except Exception:  # noqa: BLE001 - any import failure (cv2, gtsam, ...) selects the stand-ins

    class SfmMeasurement(NamedTuple):  # type: ignore[no-redef]
        """A keypoint of image ``i`` at pixel ``uv``."""

        i: int
        uv: np.ndarray

        def __eq__(self, other: object) -> bool:
            return isinstance(other, SfmMeasurement) and self.i == other.i and bool(np.allclose(self.uv, other.uv))

        def __ne__(self, other: object) -> bool:
            return not self == other

    class SfmTrack2d(NamedTuple):  # type: ignore[no-redef]
        """The 2-D measurements of one 3-D point."""

        measurements: List[SfmMeasurement]

        def number_measurements(self) -> int:
            return len(self.measurements)

        def measurement(self, idx: int) -> SfmMeasurement:
            return self.measurements[idx]

        def select_subset(self, idxs: Iterable[int]) -> "SfmTrack2d":
            return SfmTrack2d([self.measurements[j] for j in idxs])

        def select_for_cameras(self, camera_idxs) -> "SfmTrack2d":
            return SfmTrack2d([m for m in self.measurements if m.i in camera_idxs])

        def __eq__(self, other: object) -> bool:
            if not isinstance(other, SfmTrack2d) or len(self.measurements) != len(other.measurements):
                return False
            return all(any(m == o for o in other.measurements) for m in self.measurements)

        def __ne__(self, other: object) -> bool:
            return not self == other

        def validate_unique_cameras(self) -> bool:
            cams = [m.i for m in self.measurements]
            return len(set(cams)) == len(cams)
