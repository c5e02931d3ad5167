"""Agreement of a SIFT output with OpenCV's recorded output for the same image (``tests/golden/sift_lund_door_*.npz``): the figures
the host test, the GPU test and ``tools/make_sift_fixture.py`` all compute, and the caps they hold them to."""

from __future__ import annotations

from typing import Dict

import numpy as np

MATCH_PX = 0.01
# caps: at most 0.5 % of the recorded keypoints unmatched; of the matched ones at least 99 % agree in size and in response (relative
# 1e-4) and in the number of orientations; at least 98 % of the descriptors within +-1 per element and at least 85 % identical
CAPS = {"unmatched_share_max": 0.005, "size_share_min": 0.99, "response_share_min": 0.99, "orientation_share_min": 0.99,
        "descriptor_within1_share_min": 0.98, "descriptor_identical_share_min": 0.85}


def agreement(rec_xy, rec_size, rec_resp, rec_desc, xy, size, resp, desc) -> Dict[str, float]:
    """``rec_*``: the recorded keypoints (N, 2), (N,), (N,) and descriptors (N, 128); the others: the output under test, which may hold
    more keypoints than the recording (the recording is a top-k cut, and the two cut at slightly different responses)."""
    rec_xy, xy = np.asarray(rec_xy, dtype=np.float64), np.asarray(xy, dtype=np.float64)
    rec_desc, desc = np.asarray(rec_desc).astype(np.int16), np.asarray(desc).astype(np.int16)
    n = len(rec_xy)
    nearest = np.empty(n, dtype=np.int64)
    dist = np.empty(n, dtype=np.float64)
    for s in range(0, n, 512):  # blocks keep the distance matrix small
        d = np.abs(rec_xy[s : s + 512, None, :] - xy[None, :, :]).max(axis=2)
        nearest[s : s + 512] = d.argmin(axis=1)
        dist[s : s + 512] = d.min(axis=1)
    matched = dist <= MATCH_PX
    m = np.flatnonzero(matched)
    rel = lambda a, b: np.abs(a - b) / np.abs(b)  # noqa: E731
    size_ok = rel(np.asarray(size, dtype=np.float64)[nearest[m]], np.asarray(rec_size, dtype=np.float64)[m]) <= 1e-4
    resp_ok = rel(np.asarray(resp, dtype=np.float64)[nearest[m]], np.asarray(rec_resp, dtype=np.float64)[m]) <= 1e-4
    # orientations per location: how many keypoints of either output sit within MATCH_PX of the recorded keypoint
    ori_ok = np.empty(len(m), dtype=bool)
    within1 = np.empty(len(m), dtype=bool)
    identical = np.empty(len(m), dtype=bool)
    for t, i in enumerate(m):
        mine = np.flatnonzero(np.abs(xy - rec_xy[i]).max(axis=1) <= MATCH_PX)
        theirs = np.flatnonzero(np.abs(rec_xy - rec_xy[i]).max(axis=1) <= MATCH_PX)
        ori_ok[t] = len(mine) == len(theirs)
        worst = np.abs(desc[mine] - rec_desc[i][None, :]).max(axis=1).min()  # the closest descriptor of this location
        within1[t], identical[t] = worst <= 1, worst == 0
    share = lambda a: float(a.mean()) if len(a) else 0.0  # noqa: E731
    return {"recorded": float(n), "unmatched": float(n - len(m)), "unmatched_share": float(n - len(m)) / n, "size_share": share(size_ok),
            "response_share": share(resp_ok), "orientation_share": share(ori_ok), "descriptor_within1_share": share(within1),
            "descriptor_identical_share": share(identical)}


def check_caps(fig: Dict[str, float]) -> None:
    assert fig["unmatched_share"] <= CAPS["unmatched_share_max"], fig
    for k in ("size_share", "response_share", "orientation_share", "descriptor_within1_share", "descriptor_identical_share"):
        assert fig[k] >= CAPS[k + "_min"], (k, fig)


def load_lund_door(golden_dir, index: int):
    """``(gray (H, W) uint8, golden)`` of full-size image ``index``: the gray image is stored in row strips of less than 1 MB each."""
    golden = dict(np.load(golden_dir / f"sift_lund_door_{index}.npz"))
    strips = sorted(golden_dir.glob(f"sift_lund_door_{index}_gray*.npz"), key=lambda p: int(p.stem.rsplit("gray", 1)[1]))
    parts = [np.load(p) for p in strips]
    gray = np.concatenate([p["rows"] for p in parts], axis=0)
    assert gray.shape[0] == int(parts[0]["height"]) and [int(p["first_row"]) for p in parts] == list(np.cumsum([0] + [len(p["rows"]) for p in parts[:-1]]))
    return np.ascontiguousarray(gray), golden


def stored_figures(golden) -> Dict[str, float]:
    return dict(zip((str(k) for k in golden["agreement_names"]), (float(v) for v in golden["agreement_values"])))
