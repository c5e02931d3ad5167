"""``DataAssociation.run_triangulation`` (``gtsfm/data_association/data_assoc.py:205-273``) on the device: the reference's three lists,
in track order, from one launch instead of a Python loop over tracks split into Dask tasks."""

from __future__ import annotations

import logging
from typing import Dict, List, Optional, Sequence, Tuple

from gtsfm_amd.common.sfm_track import SfmTrack2d
from gtsfm_amd.data_association.point3d_initializer import Point3dInitializer, SfmTrack, TriangulationExitCode

logger = logging.getLogger(__name__)


def run_triangulation(cameras: Dict[int, object], tracks_2d: Sequence[SfmTrack2d], options, seed: int = 0,
                      device=None) -> Tuple[List[Optional[SfmTrack]], List[Optional[float]], List[TriangulationExitCode]]:
    """(sfm_tracks, avg_track_reproj_errors, triangulation_exit_codes); empty lists, with the reference's warnings, without cameras or
    tracks."""
    if len(cameras) == 0:
        logger.warning("No cameras found, skipping triangulation.")
        return [], [], []
    if len(tracks_2d) == 0:
        logger.warning("No tracks found, skipping triangulation.")
        return [], [], []
    results = Point3dInitializer(cameras, options, seed=seed, device=device).triangulate_batch(tracks_2d)
    return [r[0] for r in results], [r[1] for r in results], [r[2] for r in results]
