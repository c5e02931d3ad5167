"""Torch restatement of GTSfM's NetVLAD global descriptor (``thirdparty/hloc/netvlad.py``), its ``.mat`` checkpoint parse and the
similarity retriever's ``pairs_from_score_matrix`` (``gtsfm/retriever/similarity_retriever.py``) -- the oracle of the NetVLAD and
retrieval tests.

* ``forward`` runs the reference's operations in its order on the CPU: preprocessing ``clamp(x * 255, 0, 255) - mean`` (std 1),
  VGG16 conv1_1 .. conv5_3 (ReLU after every convolution but the last, 2 x 2 max-pools after conv1_2 / 2_2 / 3_3 / 4_3), per-pixel
  ``F.normalize``, ``softmax(conv1d(x, score_w))``, the residual sum over the (B, 512, 64, HW) difference tensor, intra- and global
  normalisation and the optional whitening. With float32 tensors it equals the reference bit for bit
  (``tools/make_netvlad_fixture.py`` checks that); with float64 tensors it is the arbiter of the accuracy tests.
* ``load_mat`` parses a checkpoint in the reference's layout (``scipy.io.loadmat(struct_as_record=False, squeeze_me=True)``).
* ``seeded_weights`` / ``seeded_images`` / ``write_mat`` make the synthetic model and inputs the fixtures are built from.
"""

from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-6
# VGG16 ``features`` up to conv5_3 (torchvision's layer list without the last ReLU and max-pool): (kind, cin, cout)
VGG16_CONVS = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
               (512, 512), (512, 512), (512, 512)]
POOL_AFTER = {1, 3, 6, 9}  # conv indices followed by a max-pool
# index of each convolution among the 29 backbone children (conv / ReLU / pool), which is its index in the checkpoint's layer list
CONV_CHILD_INDEX = [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
NETVLAD_LAYER, WHITEN_LAYER = 30, 33


def backbone_layer_kinds() -> List[str]:
    """The 29 children of ``nn.Sequential(*list(vgg16().features.children())[:-2])``: 'conv', 'relu' or 'pool'."""
    kinds: List[str] = []
    for ci in range(len(VGG16_CONVS)):
        kinds += ["conv", "relu"]
        if ci in POOL_AFTER:
            kinds.append("pool")
    return kinds[:-1]  # conv5_3 has no ReLU


def seeded_weights(seed: int = 0, whiten: bool = True, centre_scale: float = 1.0) -> Dict[str, torch.Tensor]:
    """Synthetic NetVLAD weights in torch layouts (He-scaled convolutions so that activations keep their scale through 13 layers).
    ``centre_scale`` < 1 shrinks the cluster centres, so that the residuals, and with them the descriptors, depend more on the image."""
    g = torch.Generator().manual_seed(seed)
    w: Dict[str, torch.Tensor] = {}
    for i, (cin, cout) in enumerate(VGG16_CONVS):
        w[f"conv{i}.weight"] = torch.randn((cout, cin, 3, 3), generator=g) * float(np.sqrt(2.0 / (9 * cin)))
        w[f"conv{i}.bias"] = torch.randn((cout,), generator=g) * 0.1
    w["score_w"] = torch.randn((64, 512), generator=g) * 5.0
    w["centers"] = torch.randn((512, 64), generator=g) * float(centre_scale / np.sqrt(512))
    w["mean"] = torch.tensor([123.68, 116.779, 103.939], dtype=torch.float32) + torch.rand((3,), generator=g)
    if whiten:
        w["whiten.weight"] = torch.randn((4096, 32768), generator=g) * float(1 / np.sqrt(32768))
        w["whiten.bias"] = torch.randn((4096,), generator=g) * 0.01
    return w


def seeded_images(seed: int, batch: int, height: int, width: int) -> torch.Tensor:
    """(B, 3, H, W) float32 in [0, 1] as the loader's batch transform makes it: uint8 / 255."""
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (batch, 3, height, width), generator=g, dtype=torch.uint8)
    # smooth the noise a little (a box blur of the uint8 image) so that the features are image-like
    f = F.avg_pool2d(u8.float(), 5, stride=1, padding=2, count_include_pad=False).round().clamp(0, 255).to(torch.uint8)
    return f.type(torch.float32) / 255.0


def forward(weights: Dict[str, torch.Tensor], image: torch.Tensor, whiten: bool = True, stages: Optional[dict] = None) -> torch.Tensor:
    """NetVLAD.forward (netvlad.py:166-202). ``image``: (B, 3, H, W) in [0, 1]; the dtype of ``image`` sets the arithmetic (the
    weights are cast to it). ``stages`` (optional dict) receives 'conv1_1' (after ReLU), 'conv5_3' and 'vlad' (pre-whitening)."""
    dt = image.dtype
    W = {k: v.to(dt) for k, v in weights.items()}
    assert image.shape[1] == 3
    assert image.min() >= -EPS and image.max() <= 1 + EPS
    x = torch.clamp(image * 255, 0.0, 255.0)
    x = x - x.new_tensor(W["mean"].numpy() if dt == torch.float32 else W["mean"].double().numpy()).view(1, -1, 1, 1)
    x = x / x.new_tensor(np.array([1, 1, 1], dtype=np.float32)).view(1, -1, 1, 1)
    for i in range(len(VGG16_CONVS)):
        x = F.conv2d(x, W[f"conv{i}.weight"], W[f"conv{i}.bias"], padding=1)
        if i != len(VGG16_CONVS) - 1:
            x = F.relu(x)
        if i == 0 and stages is not None:
            stages["conv1_1"] = x
        if i in POOL_AFTER:
            x = F.max_pool2d(x, 2, 2)
    if stages is not None:
        stages["conv5_3"] = x
    b, c = x.shape[:2]
    x = x.view(b, c, -1)
    x = F.normalize(x, dim=1)
    scores = F.softmax(F.conv1d(x, W["score_w"].unsqueeze(-1)), dim=1)
    diff = x.unsqueeze(2) - W["centers"].unsqueeze(0).unsqueeze(-1)
    desc = (scores.unsqueeze(1) * diff).sum(dim=-1)
    desc = F.normalize(desc, dim=1)
    desc = F.normalize(desc.view(b, -1), dim=1)
    if stages is not None:
        stages["vlad"] = desc
    if whiten:
        desc = F.normalize(F.linear(desc, W["whiten.weight"], W["whiten.bias"]), dim=1)
    return desc


# ---------------------------------------------------------------------------------------------------------------------------------
# The checkpoint: VGG16-NetVLAD-Pitts30K.mat as exported by netvlad_tf_open's net_class2struct.m
# ---------------------------------------------------------------------------------------------------------------------------------


def write_mat(path: Path, weights: Dict[str, torch.Tensor]) -> None:
    """A ``.mat`` file in the checkpoint's layout holding ``weights``: ``net.layers`` (conv layers: S x S x IN x OUT and OUT; layer 30:
    score weights D x K and the NEGATED centres; layer 33: 1 x 1 x IN x OUT and OUT) and ``net.meta.normalization.averageImage``
    (H x W x 3, every pixel the mean)."""
    import scipy.io

    empty = np.empty((0,), dtype=object)
    layers = [{"weights": empty} for _ in range(WHITEN_LAYER + 1)]
    for i, li in enumerate(CONV_CHILD_INDEX):
        wl = np.empty((2,), dtype=object)
        wl[0] = weights[f"conv{i}.weight"].numpy().transpose(2, 3, 1, 0).copy()
        wl[1] = weights[f"conv{i}.bias"].numpy().copy()
        layers[li] = {"weights": wl}
    wl = np.empty((2,), dtype=object)
    wl[0] = weights["score_w"].numpy().T.copy()
    wl[1] = (-weights["centers"]).numpy().copy()
    layers[NETVLAD_LAYER] = {"weights": wl}
    if "whiten.weight" in weights:
        wl = np.empty((2,), dtype=object)
        wl[0] = weights["whiten.weight"].numpy().T.copy()[None, None]
        wl[1] = weights["whiten.bias"].numpy().copy()
        layers[WHITEN_LAYER] = {"weights": wl}
    cells = np.empty((len(layers),), dtype=object)
    for i, layer in enumerate(layers):
        cells[i] = layer
    avg = np.broadcast_to(weights["mean"].numpy().astype(np.float32), (4, 5, 3)).copy()
    net = {"layers": cells, "meta": {"normalization": {"averageImage": avg}}}
    scipy.io.savemat(str(path), {"net": net}, do_compression=False)


def load_mat(path: Path, whiten: bool = True) -> Dict[str, torch.Tensor]:
    """The reference's parse (netvlad.py:125-163): conv weights S x S x IN x OUT -> OUT x IN x S x S matched to the backbone children by
    index, layer 30's weights[0] (D x K) transposed for the score projection, centres = -weights[1], layer 33 for the whitening,
    averageImage[0, 0] as the mean. Tensors are returned as the reference holds them (permuted views included)."""
    import scipy.io

    path = Path(path)
    if not path.exists():
        raise FileNotFoundError(f"NetVLAD checkpoint not found: {path}")
    mat = scipy.io.loadmat(str(path), struct_as_record=False, squeeze_me=True)
    layers = mat["net"].layers
    out: Dict[str, torch.Tensor] = {}
    ci = 0
    for kind, mat_layer in zip(backbone_layer_kinds(), layers):
        if kind == "conv":
            out[f"conv{ci}.weight"] = torch.tensor(mat_layer.weights[0]).float().permute([3, 2, 0, 1])
            out[f"conv{ci}.bias"] = torch.tensor(mat_layer.weights[1]).float()
            ci += 1
    out["score_w"] = torch.tensor(layers[NETVLAD_LAYER].weights[0]).float().permute([1, 0])
    out["centers"] = torch.tensor(-layers[NETVLAD_LAYER].weights[1]).float()
    if whiten:
        out["whiten.weight"] = torch.tensor(layers[WHITEN_LAYER].weights[0]).float().squeeze().permute([1, 0])
        out["whiten.bias"] = torch.tensor(layers[WHITEN_LAYER].weights[1].squeeze()).float()
    out["mean"] = torch.from_numpy(np.asarray(mat["net"].meta.normalization.averageImage[0, 0]).astype(np.float32))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Retrieval
# ---------------------------------------------------------------------------------------------------------------------------------

MAX_NUM_IMAGES = 10000


def similarity_matrix(descriptors: Sequence[np.ndarray], blocksize: int = 50) -> torch.Tensor:
    """compute_similarity_matrix: (N, N) float32, blocks (bi, bj) with bj >= bi filled with einsum('id,jd->ij'), zeros elsewhere."""
    n = len(descriptors)
    if n > MAX_NUM_IMAGES:
        raise RuntimeError("Cannot construct similarity matrix of this size.")
    sim = torch.zeros((n, n))
    nb = (n + blocksize - 1) // blocksize
    for bi in range(nb):
        for bj in range(bi, nb):
            i0, i1 = bi * blocksize, min((bi + 1) * blocksize, n)
            j0, j1 = bj * blocksize, min((bj + 1) * blocksize, n)
            a = torch.from_numpy(np.array(descriptors[i0:i1]))
            b = torch.from_numpy(np.array(descriptors[j0:j1]))
            sim[i0:i1, j0:j1] = torch.einsum("id,jd->ij", a, b)
    return sim


def pairs_from_score_matrix(scores: torch.Tensor, num_select: int, min_score: Optional[float] = None) -> list:
    """pairs_from_score_matrix with the retriever's mask (j <= i invalid) on a COPY of ``scores``: (i, j) pairs, row-major over
    (i, rank), ranks in descending score order. Equal scores are ranked by the lower column index (the documented rule of the device
    kernel; torch.topk makes no promise), which is the only place this differs from the reference."""
    s = scores.clone()
    n = s.shape[0]
    num_select = min(num_select, n)
    invalid = torch.from_numpy(~np.triu(np.ones((n, n), dtype=bool), k=1))
    if min_score is not None:
        invalid |= s < min_score
    s.masked_fill_(invalid, float("-inf"))
    pairs = []
    for i in range(n):
        row = s[i].numpy()
        order = np.lexsort((np.arange(n), -row.astype(np.float64)))[:num_select]  # descending score, then ascending column
        pairs += [(i, int(j)) for j in order if np.isfinite(row[j])]
    return pairs


def sequential_pairs(num_images: int, max_frame_lookahead: int) -> list:
    """SequentialRetriever.get_image_pairs."""
    return [(i1, i2) for i1 in range(num_images) for i2 in range(i1 + 1, min(i1 + max_frame_lookahead + 1, num_images))]


def decision_margin(desc64: np.ndarray, num_select: int, min_score: Optional[float]) -> float:
    """Smallest float64 distance of any retrieval decision from its boundary: every candidate's score from ``min_score``, and the
    gaps between consecutive ranked scores up to rank ``num_select`` (the boundary rank included). Pair lists of two float32
    evaluations can only differ where this is below their error."""
    s = desc64 @ desc64.T
    n = len(s)
    margin = np.inf
    for i in range(n - 1):
        row = s[i, i + 1 :]
        if min_score is not None:
            margin = min(margin, np.abs(row - min_score).min())
            row = row[row >= min_score]
        top = np.sort(row)[::-1][: num_select + 1]
        if len(top) > 1 and num_select > 0:
            margin = min(margin, np.diff(top[::-1]).min())
    return float(margin)


def assert_margins(desc64: np.ndarray, num_select: int, min_score: Optional[float], bound: float = 1e-5) -> None:
    m = decision_margin(desc64, num_select, min_score)
    assert m >= bound, f"a retrieval decision lies within {m:.2e} of its boundary (fixture too close to call)"


def end_to_end_images(seed: int = 21, groups: int = 3, per_group: int = 4, height: int = 96, width: int = 128) -> torch.Tensor:
    """(groups * per_group, 3, H, W) in [0, 1]: noisy uint8 variants of a few seeded base images, interleaved (image i belongs to group
    i % groups), so that retrieval has clear neighbours."""
    g = torch.Generator().manual_seed(seed)
    bases = (seeded_images(seed, groups, height, width) * 255).round()
    out = []
    for v in range(per_group):
        for b in range(groups):
            noise = torch.randn((3, height, width), generator=g) * 12.0
            out.append((bases[b] + noise).round().clamp(0, 255))
    return torch.stack(out).to(torch.uint8).type(torch.float32) / 255.0


def cache_sample(seed: int):
    """Input batch and global descriptors of the recorded global-descriptor cache entries (``tools/record_global_descriptor_cache.py``):
    a (2, 3, 12, 16) float32 batch in [0, 1] and two float32 (4096,) unit rows."""
    rng = np.random.default_rng(seed)
    images = torch.from_numpy((rng.integers(0, 256, size=(2, 3, 12, 16)) / 255.0).astype(np.float32))
    desc = rng.standard_normal((2, 4096))
    desc = (desc / np.linalg.norm(desc, axis=1, keepdims=True)).astype(np.float32)
    return images, [d for d in desc]
