"""Writes tests/golden/view_graph_palace_edges.npz: the pair graph of the reference's palace scene (its tests/data/palace/visibility_graph.csv,
data only: 4 139 unique edges i < j over 281 images in one component, 28 583 triplets, at most 31 per edge, 4 edges without one) with seeded
rotations (tests/view_graph_scenes.py: about 1 degree on inliers, 20 to 90 degrees on about 10 % of the edges) and what the restatement
(tests/view_graph_reference.py) computes from them for both criteria at the default threshold.

Usage: python tools/make_view_graph_fixture.py [path to visibility_graph.csv]   (default: under $GTSFM_REFERENCE or /root/reference)"""

import os
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from tests import view_graph_reference as ref  # noqa: E402
from tests import view_graph_scenes as scenes  # noqa: E402

SEED = 8


def main(csv_path: str) -> None:
    rows = np.loadtxt(csv_path, delimiter=",", skiprows=1, dtype=np.int64).reshape(-1, 2)
    pairs = np.unique(np.stack([rows.min(axis=1), rows.max(axis=1)], axis=1), axis=0)
    pairs = pairs[pairs[:, 0] < pairs[:, 1]]
    pairs = pairs[np.random.default_rng(SEED).permutation(len(pairs))].astype(np.int32)  # rows in no particular order, as a scene's launches leave them
    num_images = int(pairs.max()) + 1
    rotation = scenes.seeded_rotations(pairs, SEED)
    out = {"pair_images": pairs, "num_images": np.int64(num_images), "rotation": rotation}
    for name, criterion in (("min", ref.MIN_EDGE_ERROR), ("median", ref.MEDIAN_EDGE_ERROR)):
        res = ref.cycle_filter(pairs, rotation, None, num_images, criterion, 7.0)
        out[f"aggregate_{name}"], out[f"keep_{name}"] = res["aggregate_error"], res["keep"]
    out["num_triplets"], out["triplets"], out["counts_median"] = res["num_triplets"], res["triplets"], res["counts"]
    comp = ref.largest_component(pairs, None, num_images)
    print(f"{len(pairs)} edges, {num_images} ids, {int(comp['counts'][0])} nodes in the largest of {int(comp['counts'][2])} components, {len(res['triplets'])} triplets, "
          f"at most {int(res['num_triplets'].max())} per edge, {int((res['num_triplets'] == 0).sum())} edges without one, "
          f"{int(((res['num_triplets'] % 2 == 0) & (res['num_triplets'] > 0)).sum())} with an even count, largest degree "
          f"{int(np.bincount(pairs.reshape(-1)).max())}; kept {int(out['keep_min'].sum())} (min) / {int(out['keep_median'].sum())} (median)")
    target = REPO / "tests" / "golden" / "view_graph_palace_edges.npz"
    np.savez_compressed(target, **out)
    print(target, target.stat().st_size, "bytes")


if __name__ == "__main__":
    default = Path(os.environ.get("GTSFM_REFERENCE", "/root/reference")) / "tests" / "data" / "palace" / "visibility_graph.csv"
    main(sys.argv[1] if len(sys.argv) > 1 else str(default))
