"""Host side of the MegaLoc global descriptor: the checkpoint parse, the weight packing, the position table and
``gtsfm_megaloc_forward`` (``gtsfm_amd/csrc/megaloc_kernels.hip``). PyTorch provides device memory and streams only; every stage of the
model runs in the library, and there is no fallback.

The checkpoint is the file the reference downloads, ``megaloc.torch``: a ``state_dict`` of ``MegaLocModel``
(``thirdparty/megaloc/megaloc.py``) with ``backbone.model.*`` in ``torch.hub`` DINOv2 naming and ``aggregator.*``. It is never
downloaded: a missing file raises ``FileNotFoundError``. The key names are upstream's published layout; no real file was available to
check them against. Weights travel as a dictionary of float32 arrays under those names; ``from_hf_state_dict`` maps the ``transformers``
port's names to the same dictionary."""

from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Dict, List, Optional, Union

import numpy as np

from gtsfm_amd.runtime.engine_base import EngineBase

HIDDEN, PATCH, FF, TABLE = 768, 14, 3072, 37
MLP_DIM, CLUSTERS, CLUSTER_DIM, TOKEN_DIM = 512, 64, 256, 256
SALAD_DIM = TOKEN_DIM + CLUSTERS * CLUSTER_DIM  # 16640
BB, AGG = "backbone.model.", "aggregator."
_BLOCK = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias", "ls1.gamma", "norm2.weight",
          "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias", "ls2.gamma")
_BLOCK_SHAPES = ((HIDDEN,), (HIDDEN,), (3 * HIDDEN, HIDDEN), (3 * HIDDEN,), (HIDDEN, HIDDEN), (HIDDEN,), (HIDDEN,), (HIDDEN,), (HIDDEN,),
                 (FF, HIDDEN), (FF,), (HIDDEN, FF), (HIDDEN,), (HIDDEN,))
_HEAD = (("agg.token_features.0", (MLP_DIM, HIDDEN)), ("agg.token_features.2", (TOKEN_DIM, MLP_DIM)), ("agg.cluster_features.0", (MLP_DIM, HIDDEN)),
         ("agg.cluster_features.3", (CLUSTER_DIM, MLP_DIM)), ("agg.score.0", (MLP_DIM, HIDDEN)), ("agg.score.3", (CLUSTERS, MLP_DIM)))


def _f32(a) -> np.ndarray:
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32)


def depth_of(weights) -> int:
    ids = [int(k[len(BB + "blocks."):].split(".")[0]) for k in weights if k.startswith(BB + "blocks.")]
    if not ids:
        raise KeyError("MegaLoc weights hold no backbone.model.blocks.* entries")
    return 1 + max(ids)


def tensor_order(depth: int) -> List[str]:
    """Names in the order of ``gtsfm_megaloc_pack_weights`` (the position table travels separately)."""
    names = [BB + "patch_embed.proj.weight", BB + "patch_embed.proj.bias", BB + "cls_token"]
    names += [f"{BB}blocks.{i}.{n}" for i in range(depth) for n in _BLOCK]
    names += [BB + "norm.weight", BB + "norm.bias"]
    names += [f"{AGG}{n}.{p}" for n, _ in _HEAD for p in ("weight", "bias")]
    return names + [AGG + "agg.dust_bin", AGG + "linear.weight", AGG + "linear.bias"]


def expected_shapes(depth: int, feat_dim: int) -> Dict[str, tuple]:
    """Shapes after squeezing the 1 x 1 convolution kernels and the leading ones of cls_token."""
    shapes = {BB + "patch_embed.proj.weight": (HIDDEN, 3, PATCH, PATCH), BB + "patch_embed.proj.bias": (HIDDEN,), BB + "cls_token": (HIDDEN,),
              BB + "pos_embed": (1, 1 + TABLE * TABLE, HIDDEN), BB + "norm.weight": (HIDDEN,), BB + "norm.bias": (HIDDEN,),
              AGG + "agg.dust_bin": (1,), AGG + "linear.weight": (feat_dim, SALAD_DIM), AGG + "linear.bias": (feat_dim,)}
    for i in range(depth):
        for n, s in zip(_BLOCK, _BLOCK_SHAPES):
            shapes[f"{BB}blocks.{i}.{n}"] = s
    for n, s in _HEAD:
        shapes[f"{AGG}{n}.weight"], shapes[f"{AGG}{n}.bias"] = s, (s[0],)
    return shapes


def normalise_weights(weights: Dict[str, object]) -> Dict[str, np.ndarray]:
    """Float32 arrays in the packer's shapes (1 x 1 convolutions as matrices, cls_token and dust_bin flat); raises ``KeyError`` for a missing
    entry and ``ValueError`` for a wrong shape. Unknown entries (``mask_token``) are dropped."""
    depth = depth_of(weights)
    if AGG + "linear.bias" not in weights:
        raise KeyError(f"MegaLoc weights are missing ['{AGG}linear.bias']")
    feat_dim = int(np.asarray(_f32(weights[AGG + "linear.bias"])).size)
    shapes = expected_shapes(depth, feat_dim)
    missing = [n for n in shapes if n not in weights]
    if missing:
        raise KeyError(f"MegaLoc weights are missing {missing}")
    out = {}
    for n, shape in shapes.items():
        a = _f32(weights[n])
        if tuple(d for d in a.shape if d != 1) != tuple(d for d in shape if d != 1):  # (1 x 1 kernels, cls_token's and dust_bin's unit axes aside)
            raise ValueError(f"MegaLoc weight {n} has shape {a.shape}, expected {shape}")
        out[n] = a.reshape(shape)
    if feat_dim % 64:
        raise ValueError(f"MegaLoc feat_dim must be a multiple of 64 (got {feat_dim})")
    return out


def load_checkpoint(path: Union[str, Path]) -> Dict[str, np.ndarray]:
    """``megaloc.torch`` -> the weight dictionary. Never downloaded: a missing file raises ``FileNotFoundError``."""
    import torch

    path = Path(path)
    if not path.exists():
        raise FileNotFoundError(f"MegaLoc checkpoint not found: {path} (gtsfm_amd never downloads weights)")
    sd = torch.load(str(path), map_location="cpu", weights_only=True)
    return normalise_weights(sd)


def from_hf_state_dict(backbone_sd: Dict[str, object], head_sd: Dict[str, object]) -> Dict[str, np.ndarray]:
    """``transformers``' ``Dinov2Model.state_dict()`` (query / key / value fused into qkv, ``layer_scale1.lambda1`` -> ``ls1.gamma``, ...) plus the
    ``aggregator.*`` entries in the reference's naming -> the weight dictionary."""
    w: Dict[str, object] = {k: v for k, v in head_sd.items() if k.startswith(AGG)}
    w[BB + "cls_token"] = backbone_sd["embeddings.cls_token"]
    w[BB + "pos_embed"] = backbone_sd["embeddings.position_embeddings"]
    w[BB + "patch_embed.proj.weight"] = backbone_sd["embeddings.patch_embeddings.projection.weight"]
    w[BB + "patch_embed.proj.bias"] = backbone_sd["embeddings.patch_embeddings.projection.bias"]
    w[BB + "norm.weight"], w[BB + "norm.bias"] = backbone_sd["layernorm.weight"], backbone_sd["layernorm.bias"]
    depth = 1 + max(int(k.split(".")[2]) for k in backbone_sd if k.startswith("encoder.layer."))
    for i in range(depth):
        b, h = f"{BB}blocks.{i}.", f"encoder.layer.{i}."
        for p in ("weight", "bias"):
            w[f"{b}attn.qkv.{p}"] = np.concatenate([_f32(backbone_sd[f"{h}attention.attention.{n}.{p}"]) for n in ("query", "key", "value")], axis=0)
            for src, dst in (("attention.output.dense", "attn.proj"), ("norm1", "norm1"), ("norm2", "norm2"), ("mlp.fc1", "mlp.fc1"), ("mlp.fc2", "mlp.fc2")):
                w[f"{b}{dst}.{p}"] = backbone_sd[f"{h}{src}.{p}"]
        w[b + "ls1.gamma"], w[b + "ls2.gamma"] = backbone_sd[h + "layer_scale1.lambda1"], backbone_sd[h + "layer_scale2.lambda1"]
    return normalise_weights(w)


def pack_weights(weights: Dict[str, object]) -> np.ndarray:
    """Named weights -> the packed float32 blob of ``gtsfm_megaloc_pack_weights`` (LayerScale folded into attn.proj / mlp.fc2)."""
    from gtsfm_amd.runtime import lib as _lib

    lib = _lib.load()
    w = normalise_weights(weights)
    depth, feat_dim = depth_of(w), int(w[AGG + "linear.bias"].size)
    arrays = [w[n] for n in tensor_order(depth)]
    ptrs = (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
    out = np.empty(lib.gtsfm_megaloc_packed_weight_floats(depth, feat_dim), dtype=np.float32)
    _lib.check(lib.gtsfm_megaloc_pack_weights(ptrs, depth, feat_dim, out.ctypes.data), "gtsfm_megaloc_pack_weights")
    return out


def position_table(pos_embed: np.ndarray, gh: int, gw: int) -> np.ndarray:
    """The 37 x 37 position table at a gh x gw grid, (1 + gh gw, 768) float32, with the call the ``transformers`` port makes: the table itself at
    37 x 37, else ``interpolate(size=(gh, gw), mode="bicubic", align_corners=False)`` in float32. Host-side weight preparation, once per grid."""
    import torch

    pos = torch.from_numpy(np.ascontiguousarray(pos_embed, dtype=np.float32)).reshape(1, 1 + TABLE * TABLE, HIDDEN)
    if (gh, gw) != (TABLE, TABLE):
        patch = pos[:, 1:].reshape(1, TABLE, TABLE, HIDDEN).permute(0, 3, 1, 2)
        patch = torch.nn.functional.interpolate(patch, size=(gh, gw), mode="bicubic", align_corners=False)
        pos = torch.cat((pos[:, :1], patch.permute(0, 2, 3, 1).reshape(1, -1, HIDDEN)), dim=1)
    return np.ascontiguousarray(pos[0].numpy())


class MegaLocEngine(EngineBase):
    """Packed weights resident on one device, position tables cached per grid, a cached workspace; one instance per process / GPU."""

    WS_SLACK = "exact"

    def __init__(self, weights: Dict[str, object], device=None):
        super().__init__(device)
        w = normalise_weights(weights)
        self.depth, self.feat_dim = depth_of(w), int(w[AGG + "linear.bias"].size)
        self._pos_embed = w[BB + "pos_embed"]
        self._weights = self._torch.from_numpy(pack_weights(w)).to(self.device)
        self._pos: Dict[tuple, object] = {}
        self._flag = self._torch.zeros(1, dtype=self._torch.int32, device=self.device)

    @classmethod
    def from_checkpoint(cls, path: Union[str, Path], device=None) -> "MegaLocEngine":
        return cls(load_checkpoint(path), device)

    def _position(self, gh: int, gw: int):
        if (gh, gw) not in self._pos:
            self._pos[(gh, gw)] = self._torch.from_numpy(position_table(self._pos_embed, gh, gw)).to(self.device)
        return self._pos[(gh, gw)]

    def _workspace(self, b: int, h: int, w: int):
        need = int(self._lib.gtsfm_megaloc_workspace_bytes(b, h, w, self.feat_dim))
        if need == 0:
            raise ValueError(f"MegaLoc needs height and width that are multiples of {PATCH} and more than {CLUSTERS} patches (got a batch of {b} x {h} x {w})")
        return self._grow(need)

    def _prepare(self, images):
        """(B, 3, H, W), normalised float (any float dtype: converted to float32) or raw uint8, CPU or device -> (device tensor, layout, B, H, W).
        Raises ``ValueError`` before any launch for H or W not a multiple of 14 (the reference resizes there) and for 64 patches or fewer (the
        reference's log(n - 64) is undefined)."""
        torch = self._torch
        if images.dim() != 4 or images.shape[1] != 3:
            raise AssertionError(f"MegaLoc takes a (B, 3, H, W) batch (got shape {tuple(images.shape)})")
        b, _, h, w = (int(v) for v in images.shape)
        if h % PATCH or w % PATCH:
            raise ValueError(f"MegaLoc takes heights and widths that are multiples of {PATCH} (got {h} x {w})")
        if (h // PATCH) * (w // PATCH) <= CLUSTERS:
            raise ValueError(f"MegaLoc needs more than {CLUSTERS} patches (got {h} x {w}: {(h // PATCH) * (w // PATCH)})")
        layout = 1 if images.dtype == torch.uint8 else 0
        if layout == 0:
            images = images.to(torch.float32)
        return images.to(self.device, non_blocking=True).contiguous(), layout, b, h, w

    def describe(self, images):
        """Descriptors of a batch as a device tensor (B, feat_dim). A batch of any size runs in chunks of at most 64 images inside the library.
        Raises ``ValueError`` when a float image holds a non-finite value; the check reads one flag after the call."""
        torch = self._torch
        if images.dim() == 4 and images.shape[0] == 0:
            return torch.empty((0, self.feat_dim), dtype=torch.float32, device=self.device)
        images, layout, b, h, w = self._prepare(images)
        out = torch.empty((b, self.feat_dim), dtype=torch.float32, device=self.device)
        ws = self._workspace(b, h, w)
        self._flag.zero_()
        rc = self._lib.gtsfm_megaloc_forward(self._weights.data_ptr(), self.depth, self.feat_dim, self._position(h // PATCH, w // PATCH).data_ptr(),
                                             images.data_ptr(), layout, b, h, w, out.data_ptr(), self._flag.data_ptr(), ws.data_ptr(), ws.numel(),
                                             self._L.current_stream_handle())
        self._L.check(rc, "gtsfm_megaloc_forward")
        if layout == 0 and int(self._flag.item()) != 0:
            raise ValueError("MegaLoc input holds a non-finite value")
        return out

    def stage(self, images, stage: int):
        """Stage-wise outputs (device): 0 = tokens after patch embedding + cls + positions, 1 = output of block 0, 2 = the final LayerNorm's tokens
        (each (B, 1 + n, 768)), 3 = the SALAD vector (B, 16640)."""
        torch = self._torch
        images, layout, b, h, w = self._prepare(images)
        if stage not in (0, 1, 2, 3):
            raise ValueError(f"stage must be 0, 1, 2 or 3 (got {stage})")
        shape = (b, SALAD_DIM) if stage == 3 else (b, 1 + (h // PATCH) * (w // PATCH), HIDDEN)
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        ws = self._workspace(b, h, w)
        rc = self._lib.gtsfm_megaloc_stage(self._weights.data_ptr(), self.depth, self.feat_dim, self._position(h // PATCH, w // PATCH).data_ptr(),
                                           images.data_ptr(), layout, b, h, w, stage, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                           self._L.current_stream_handle())
        self._L.check(rc, "gtsfm_megaloc_stage")
        return out
