"""Torch restatement of GTSfM's D2-Net detector-descriptor, single scale (``thirdparty/d2net/lib/{model_test,pyramid,utils}.py``,
``gtsfm/frontend/detector_descriptor/d2net.py``) -- the oracle of the D2-Net tests.

* ``normalise`` is the reference's numpy preprocessing (float32 division by 255, float64 mean / std, rounded to float32).
* ``dense_map`` runs the feature extractor with torch's CPU convolutions and pools (ReLU after every convolution, the last included).
* ``head`` is the detection head in an EXPLICIT operation order (the one ``include/gtsfm_amd.h`` states): channel maximum, 3 x 3
  local maximum, Hessian edge test, Newton step, ``|step| < 0.5``, valid corners; then bilinear descriptors, normalisation and the
  coordinate upscaling. With float32 tensors the whole path equals the reference bit for bit (``tools/make_d2net_fixture.py``
  checks that against the reference's modules, ``process_multiscale(scales=[1])`` and ``D2NetDetDesc.detect_and_describe``); with
  float64 tensors it is the arbiter of the accuracy tests.
* The candidates are ordered by (score descending; channel, i, j ascending). The reference's ``np.argsort(-scores)`` is not stable,
  so equal scores are unpinned towards it.
* ``seeded_weights`` / ``seeded_image`` make the synthetic model and inputs the fixtures are built from.
"""

from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

CONV_LAYER_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21)
CONVS = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512)]
POOL_AFTER = {1, 3}  # conv indices followed by a 2 x 2 max-pool
FIRST_DILATED = 7    # AvgPool2d(2, stride=1) sits in front of it
EDGE_THRESHOLD = 5


def key(i: int, part: str) -> str:
    return f"dense_feature_extraction.model.{CONV_LAYER_INDEX[i]}.{part}"


def seeded_weights(seed: int = 0) -> Dict[str, torch.Tensor]:
    """Synthetic D2-Net weights under the checkpoint's keys: Kaiming-normal convolutions (activations keep their scale through the
    ten layers; with torch's default init they decay), bias N(0, 0.1)."""
    g = torch.Generator().manual_seed(seed)
    w: Dict[str, torch.Tensor] = {}
    for i, (cin, cout) in enumerate(CONVS):
        w[key(i, "weight")] = torch.randn((cout, cin, 3, 3), generator=g) * float(np.sqrt(2.0 / (9 * cin)))
        w[key(i, "bias")] = torch.randn((cout,), generator=g) * 0.1
    return w


def seeded_image(seed: int, height: int, width: int) -> np.ndarray:
    """(H, W, 3) uint8: 8 x 8 blocks of a random colour at weight 0.7 plus per-pixel noise at weight 0.3."""
    rng = np.random.default_rng(seed)
    blocks = rng.random(((height + 7) // 8, (width + 7) // 8, 3))
    blocks = np.repeat(np.repeat(blocks, 8, axis=0), 8, axis=1)[:height, :width]
    noise = rng.random((height, width, 3))
    return np.round(255.0 * (0.7 * blocks + 0.3 * noise)).astype(np.uint8)


def normalise(image: np.ndarray) -> np.ndarray:
    """(H, W, 3) or (H, W) array -> (3, H, W) float32, as ``resize_image`` (gray -> three equal channels), ``preprocess_image(.., 'torch')``
    and the ``astype(np.float32)`` of d2net.py:78 make it."""
    if image.ndim == 2:
        image = np.repeat(image[:, :, np.newaxis], 3, -1)
    x = image.astype(np.float32)
    x = np.transpose(x, [2, 0, 1])
    x /= 255.0
    mean = np.array([0.485, 0.456, 0.406])
    std = np.array([0.229, 0.224, 0.225])
    x = (x - mean.reshape([3, 1, 1])) / std.reshape([3, 1, 1])
    return x.astype(np.float32)


def dense_map(weights: Dict[str, torch.Tensor], x: torch.Tensor, stages: Optional[dict] = None) -> torch.Tensor:
    """(1, 3, H, W) normalised image -> (1, 512, H2, W2); the dtype of ``x`` sets the arithmetic. ``stages`` receives 'conv1_1' and
    'conv3_3' (after ReLU) and 'dense'."""
    dt = x.dtype
    for i in range(len(CONVS)):
        if i == FIRST_DILATED:
            x = F.avg_pool2d(x, 2, stride=1)
        d = 2 if i >= FIRST_DILATED else 1
        x = F.relu(F.conv2d(x, weights[key(i, "weight")].to(dt), weights[key(i, "bias")].to(dt), padding=d, dilation=d))
        if stages is not None and i == 0:
            stages["conv1_1"] = x
        if stages is not None and i == FIRST_DILATED - 1:
            stages["conv3_3"] = x
        if i in POOL_AFTER:
            x = F.max_pool2d(x, 2, stride=2)
    if stages is not None:
        stages["dense"] = x
    return x


def head(dense: torch.Tensor, max_keypoints: Optional[int] = None) -> Dict[str, np.ndarray]:
    """The detection head on a (512, h, w) map in the explicit operation order. Returns numpy arrays: ``cand`` (n, 3) int64 (channel, i, j),
    ``steps`` (n, 2), ``cand_scores`` (n,) -- every candidate, sorted -- and ``keypoints`` (k, 2) (x, y), ``scores`` (k,), ``descriptors``
    (k, 512) of the first k = min(n, max_keypoints)."""
    c, h, w = dense.shape
    x = dense
    xp = F.pad(x, (1, 1, 1, 1))
    nb = lambda dy, dx: xp[:, 1 + dy : 1 + dy + h, 1 + dx : 1 + dx + w]  # noqa: E731
    up, down, left, right = nb(-1, 0), nb(1, 0), nb(0, -1), nb(0, 1)
    is_depth_max = x == x.max(dim=0)[0]
    is_local_max = x == F.max_pool2d(x[None], 3, stride=1, padding=1)[0]
    dii = (up - 2 * x) + down
    djj = (left - 2 * x) + right
    dij = 0.25 * (((nb(-1, -1) - nb(-1, 1)) - nb(1, -1)) + nb(1, 1))
    det = dii * djj - dij * dij
    tr = dii + djj
    threshold = (EDGE_THRESHOLD + 1) ** 2 / EDGE_THRESHOLD
    not_edge = (det > 0) & (tr * tr / det <= threshold)
    di = 0.5 * down - 0.5 * up
    dj = 0.5 * right - 0.5 * left
    h00, h01, h11 = djj / det, -dij / det, dii / det
    step_i = -(h00 * di + h01 * dj)
    step_j = -(h01 * di + h11 * dj)
    detected = is_depth_max & is_local_max & not_edge & (step_i.abs() < 0.5) & (step_j.abs() < 0.5)
    pos = torch.nonzero(detected)  # (n, 3): channel, i, j
    ci, ii, jj = pos[:, 0], pos[:, 1], pos[:, 2]
    si, sj = step_i[ci, ii, jj], step_j[ci, ii, jj]
    pi, pj = ii.to(x.dtype) + si, jj.to(x.dtype) + sj
    i0, j0, i1, j1 = torch.floor(pi).long(), torch.floor(pj).long(), torch.ceil(pi).long(), torch.ceil(pj).long()
    valid = (i0 >= 0) & (j0 >= 0) & (i1 < h) & (j1 < w)
    ci, ii, jj, si, sj, pi, pj, i0, j0, i1, j1 = (t[valid] for t in (ci, ii, jj, si, sj, pi, pj, i0, j0, i1, j1))
    scores = x[ci, ii, jj]
    order = np.lexsort((jj.numpy(), ii.numpy(), ci.numpy(), -scores.numpy()))
    out = {"cand": torch.stack([ci, ii, jj], 1).numpy()[order], "steps": torch.stack([si, sj], 1).numpy()[order], "cand_scores": scores.numpy()[order]}
    keep = torch.from_numpy(order[: len(order) if max_keypoints is None else max_keypoints].copy())
    ci, pi, pj, i0, j0, i1, j1 = (t[keep] for t in (ci, pi, pj, i0, j0, i1, j1))
    dist_i, dist_j = pi - i0.to(x.dtype), pj - j0.to(x.dtype)
    w_tl, w_tr, w_bl, w_br = (1 - dist_i) * (1 - dist_j), (1 - dist_i) * dist_j, dist_i * (1 - dist_j), dist_i * dist_j
    desc = w_tl * x[:, i0, j0] + w_tr * x[:, i0, j1] + w_bl * x[:, i1, j0] + w_br * x[:, i1, j1]
    desc = F.normalize(desc, dim=0)
    up2 = lambda p: (p * 2 + 0.5) * 2 + 0.5  # noqa: E731  upscale_positions(scaling_steps=2)
    out["keypoints"] = torch.stack([up2(pj), up2(pi)], 1).numpy()
    out["scores"] = scores[keep].numpy()
    out["descriptors"] = desc.t().contiguous().numpy()
    return out


def forward(weights: Dict[str, torch.Tensor], image: np.ndarray, max_keypoints: Optional[int] = None, dtype=torch.float32,
            stages: Optional[dict] = None) -> Dict[str, np.ndarray]:
    """One image (uint8 or float, (H, W, 3) or (H, W)) through the single-scale path. ``dtype=torch.float64`` evaluates the same path
    in double precision from the same float32-normalised input."""
    x = torch.from_numpy(normalise(image))[None].to(dtype)
    with torch.no_grad():
        dense = dense_map(weights, x, stages)
        return head(dense[0], max_keypoints)
