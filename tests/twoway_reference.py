"""NumPy restatement of GTSfM's TwoWayMatcher (``gtsfm/frontend/matcher/twoway_matcher.py``) -- the oracle of the two-way tests.

Contract, as ``cv.BFMatcher`` + the reference's Python around it behave:
* either descriptor array empty -> ``np.array([])``; rows holding a NaN are dropped and the indices mapped back afterwards;
* one-way A->B: each row of A takes its nearest row of B by the float32 distance (EUCLIDEAN: correctly rounded sqrtf of the sum of
  squares; HAMMING: popcount of a XOR b), ties to the lower index; with a ratio test r the row is kept iff
  float64(d1st) <= r * float64(d2nd), d2nd = the second entry of the top-2 (duplicates count), and a single-row B raises ValueError;
  kept matches are sorted by distance, stably (row order breaks ties);
* two-way: (i, j) of the 1->2 list is kept iff 2->1 maps j back to i; the 1->2 order is kept; (K, 2) uint32, ``np.array([])`` if K = 0.

The float64 squared distances are exact for integer-valued descriptors (SIFT, ORB, BRISK as OpenCV emits them), so there the
restatement is the reference bit for bit. For real-valued data ``oneway`` also returns each decision's relative margin.
"""

from __future__ import annotations

from typing import Dict, Optional

import numpy as np

HAMMING = 1
EUCLIDEAN = 2


def squared_distances(a: np.ndarray, b: np.ndarray, metric: int = EUCLIDEAN) -> np.ndarray:
    """[N1, N2] float64: sum (a - b)^2 (EUCLIDEAN) or popcount(a XOR b) (HAMMING, uint8 rows)."""
    if metric == HAMMING:
        bits_a = np.unpackbits(a.astype(np.uint8), axis=1).astype(np.float64)
        bits_b = np.unpackbits(b.astype(np.uint8), axis=1).astype(np.float64)
        return bits_a @ (1 - bits_b).T + (1 - bits_a) @ bits_b.T
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    if a.shape[0] * b.shape[0] * a.shape[1] <= 2_000_000:
        return ((a64[:, None, :] - b64[None, :, :]) ** 2).sum(-1)
    e = (a64 * a64).sum(1)[:, None] + (b64 * b64).sum(1)[None, :] - 2.0 * (a64 @ b64.T)
    return np.maximum(e, 0.0)


def float32_distances(e: np.ndarray, metric: int = EUCLIDEAN) -> np.ndarray:
    """The distances OpenCV reports: float32 (EUCLIDEAN: sqrtf of the float32 sum, correctly rounded)."""
    if metric == HAMMING:
        return e.astype(np.float32)
    return np.sqrt(e.astype(np.float32))


def oneway(dist: np.ndarray, ratio: Optional[float], dist64: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """One-way matching over a [N1, N2] float32 distance matrix. Returns nn [N1], keep [N1] (bool), order (kept rows in the
    reference's distance order) and, with ``dist64`` (float64 distances), margin [N1]: the relative gap of the nearest-neighbour
    choice and, with a ratio test, of the ratio decision (the smaller of the two)."""
    n1, n2 = dist.shape
    rows = np.arange(n1)
    nn = np.argmin(dist, axis=1)
    d1 = dist[rows, nn]
    keep = np.ones(n1, dtype=bool)
    if ratio is not None:
        if n2 < 2:
            raise ValueError("not enough values to unpack (expected 2, got 1)")
        rest = dist.copy()
        rest[rows, nn] = np.inf
        d2 = rest[rows, np.argmin(rest, axis=1)]
        keep = d1.astype(np.float64) <= ratio * d2.astype(np.float64)
    order = rows[keep][np.argsort(d1[keep], kind="stable")]
    out = {"nn": nn, "keep": keep, "order": order, "dist": d1}
    if dist64 is not None:
        s = np.sort(dist64, axis=1)
        tiny = 1e-30
        margin = (s[:, 1] - s[:, 0]) / np.maximum(s[:, 0], tiny) if n2 > 1 else np.full(n1, np.inf)
        if ratio is not None:
            margin = np.minimum(margin, np.abs(s[:, 0] - ratio * s[:, 1]) / np.maximum(s[:, 0], tiny))
        out["margin"] = margin
    return out


def twoway_valid(d1: np.ndarray, d2: np.ndarray, metric: int = EUCLIDEAN, ratio: Optional[float] = None, with_margins: bool = False):
    """Two-way matching of NaN-free, non-empty descriptor arrays: (K, 2) int64 in the reference's order, and with ``with_margins``
    the per-row confidence of that decision (row i of d1: min of its own margin and its nearest column's)."""
    e = squared_distances(d1, d2, metric)
    dist = float32_distances(e, metric)
    d64 = np.sqrt(e) if with_margins else None
    ab = oneway(dist, ratio, d64)
    ba = oneway(dist.T, ratio, None if d64 is None else d64.T)
    back = np.where(ba["keep"], ba["nn"], -1)
    out = np.array([(i, ab["nn"][i]) for i in ab["order"] if back[ab["nn"][i]] == i], dtype=np.int64).reshape(-1, 2)
    if not with_margins:
        return out
    return out, np.minimum(ab["margin"], ba["margin"][ab["nn"]])


def twoway_match(descriptors_i1: np.ndarray, descriptors_i2: np.ndarray, metric: int = EUCLIDEAN, ratio: Optional[float] = None) -> np.ndarray:
    """The reference's ``TwoWayMatcher.match`` output for these descriptors (empty and NaN conventions included)."""
    if descriptors_i1.size == 0 or descriptors_i2.size == 0:
        return np.array([])
    valid_1 = np.nonzero(~(np.isnan(descriptors_i1).any(axis=1)))[0]
    valid_2 = np.nonzero(~(np.isnan(descriptors_i2).any(axis=1)))[0]
    if len(valid_1) == 0 or len(valid_2) == 0:
        return np.array([])
    if ratio is not None and min(len(valid_1), len(valid_2)) < 2:
        raise ValueError("not enough values to unpack (expected 2, got 1)")
    m = twoway_valid(descriptors_i1[valid_1], descriptors_i2[valid_2], metric, ratio)
    if m.size == 0:
        return np.array([])
    return np.stack([valid_1[m[:, 0]], valid_2[m[:, 1]]], axis=1).astype(np.uint32)
