"""CPU restatement of the MegaLoc global descriptor (``thirdparty/megaloc/megaloc.py``): DINOv2 ViT-B/14 backbone, SALAD aggregation,
linear layer, L2 norm. torch on the CPU, float32 or float64 by the input's dtype. Test helper and fixture source
(``tools/make_megaloc_fixture.py``); never on a hot path.

Pins: the SALAD head, the linear layer and the norms are written against the reference's own ``Aggregator`` / ``L2Norm`` and equal them
bit for bit in float32 (``tests/test_megaloc_host.py``). The backbone is written against the ``transformers`` port
(``transformers.models.dinov2.modeling_dinov2.Dinov2Model``), because the reference takes DINOv2 from ``torch.hub`` and that source is
not in its checkout: parity is unpinned towards ``torch.hub``'s DINOv2 (notably its position-table interpolation with a +0.1 offset).

Weights are a dictionary in the naming of the published ``megaloc.torch`` state_dict (``backbone.model.*`` in ``torch.hub`` DINOv2 naming,
``aggregator.*``)."""

from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

HIDDEN, HEADS, PATCH, FF = 768, 12, 14, 3072
MLP_DIM, CLUSTERS, CLUSTER_DIM, TOKEN_DIM = 512, 64, 256, 256
SALAD_DIM = TOKEN_DIM + CLUSTERS * CLUSTER_DIM  # 16640
TABLE = 37  # the position table is 37 x 37 (518 / 14) + the class position
LN_EPS = 1e-6
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
BB, AGG = "backbone.model.", "aggregator."


def seeded_weights(seed: int, depth: int = 12, feat_dim: int = 8448) -> Dict[str, torch.Tensor]:
    """A live network: products scaled by 1 / sqrt(fan-in) with gains above the usual 0.02 initialisation (with that, every image gives
    nearly the same descriptor), LayerNorm gains around 1, LayerScale around 0.5."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape, s=1.0: torch.randn(shape, generator=g) * s  # noqa: E731
    w: Dict[str, torch.Tensor] = {}

    def linear(name, out_f, in_f, gain=1.0, shape=None, bias=0.05):
        w[name + ".weight"] = (rn(out_f, in_f, s=gain / math.sqrt(in_f))).reshape(shape or (out_f, in_f))
        w[name + ".bias"] = rn(out_f, s=bias)

    def norm(name):
        w[name + ".weight"] = 1.0 + rn(HIDDEN, s=0.1)
        w[name + ".bias"] = rn(HIDDEN, s=0.05)

    w[BB + "cls_token"] = rn(1, 1, HIDDEN, s=0.5)
    w[BB + "pos_embed"] = rn(1, 1 + TABLE * TABLE, HIDDEN, s=0.5)
    linear(BB + "patch_embed.proj", HIDDEN, 3 * PATCH * PATCH, 1.0, (HIDDEN, 3, PATCH, PATCH))
    for i in range(depth):
        b = f"{BB}blocks.{i}."
        norm(b + "norm1")
        linear(b + "attn.qkv", 3 * HIDDEN, HIDDEN, 1.5)
        linear(b + "attn.proj", HIDDEN, HIDDEN, 1.0)
        w[b + "ls1.gamma"] = 0.5 + rn(HIDDEN, s=0.1)
        norm(b + "norm2")
        linear(b + "mlp.fc1", FF, HIDDEN, 1.0)
        linear(b + "mlp.fc2", HIDDEN, FF, 1.0)
        w[b + "ls2.gamma"] = 0.5 + rn(HIDDEN, s=0.1)
    norm(BB + "norm")
    a = AGG + "agg."
    linear(a + "token_features.0", MLP_DIM, HIDDEN, 1.4)
    linear(a + "token_features.2", TOKEN_DIM, MLP_DIM, 1.4)
    linear(a + "cluster_features.0", MLP_DIM, HIDDEN, 1.4, (MLP_DIM, HIDDEN, 1, 1))
    linear(a + "cluster_features.3", CLUSTER_DIM, MLP_DIM, 1.4, (CLUSTER_DIM, MLP_DIM, 1, 1))
    linear(a + "score.0", MLP_DIM, HIDDEN, 1.4, (MLP_DIM, HIDDEN, 1, 1))
    linear(a + "score.3", CLUSTERS, MLP_DIM, 2.0, (CLUSTERS, MLP_DIM, 1, 1))
    w[a + "dust_bin"] = torch.tensor(1.0)
    linear(AGG + "linear", feat_dim, SALAD_DIM, 1.0, bias=1e-4)  # (its input is a unit vector: entries ~ 1 / 129)
    return w


def depth_of(weights) -> int:
    return 1 + max(int(k[len(BB + "blocks.") :].split(".")[0]) for k in weights if k.startswith(BB + "blocks."))


def seeded_images(seed: int, batch: int, height: int, width: int) -> torch.Tensor:
    """(B, 3, H, W) uint8: smooth seeded colour fields plus noise, so that images differ at every scale."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand((batch, 3, max(height // 28, 2), max(width // 28, 2)), generator=g)
    smooth = F.interpolate(coarse, size=(height, width), mode="bilinear", align_corners=False)
    noise = torch.randn((batch, 3, height, width), generator=g) * 0.08
    return ((smooth + noise) * 255.0).round().clamp(0, 255).to(torch.uint8)


def normalise(images_u8: torch.Tensor) -> torch.Tensor:
    """The reference's batch transform: ``x.type(torch.float32) / 255.0``, then torchvision's ``Normalize``: ``(x - mean) / std`` with float32 mean / std."""
    x = images_u8.type(torch.float32) / 255.0
    mean = torch.as_tensor(MEAN, dtype=torch.float32).view(-1, 1, 1)
    std = torch.as_tensor(STD, dtype=torch.float32).view(-1, 1, 1)
    return (x - mean) / std


def position_table(pos_embed: torch.Tensor, gh: int, gw: int) -> torch.Tensor:
    """The transformers port's ``interpolate_pos_encoding``: the table itself at 37 x 37, else bicubic in float32, align_corners=False. (1, 1 + gh gw, 768) float32."""
    pos_embed = pos_embed.to(torch.float32)
    if gh == TABLE and gw == TABLE:
        return pos_embed
    patch = pos_embed[:, 1:].reshape(1, TABLE, TABLE, HIDDEN).permute(0, 3, 1, 2)
    patch = F.interpolate(patch, size=(gh, gw), mode="bicubic", align_corners=False)
    return torch.cat((pos_embed[:, :1], patch.permute(0, 2, 3, 1).reshape(1, -1, HIDDEN)), dim=1)


def backbone(weights, images: torch.Tensor, stages: Optional[dict] = None) -> torch.Tensor:
    """Normalised (B, 3, H, W) images -> the final LayerNorm's tokens (B, 1 + n, 768) (row 0 ``x_norm_clstoken``, the rest ``x_norm_patchtokens``)."""
    dt = images.dtype
    w = {k: v.to(dt) for k, v in weights.items() if k.startswith(BB)}
    bsz, _, height, width = images.shape
    assert height % PATCH == 0 and width % PATCH == 0
    x = F.conv2d(images, w[BB + "patch_embed.proj.weight"], w[BB + "patch_embed.proj.bias"], stride=PATCH).flatten(2).transpose(1, 2)
    x = torch.cat((w[BB + "cls_token"].expand(bsz, -1, -1), x), dim=1)
    x = x + position_table(weights[BB + "pos_embed"], height // PATCH, width // PATCH).to(dt)
    if stages is not None:
        stages["tokens"] = x
    for i in range(depth_of(weights)):
        b = f"{BB}blocks.{i}."
        h = F.layer_norm(x, (HIDDEN,), w[b + "norm1.weight"], w[b + "norm1.bias"], LN_EPS)
        qkv = F.linear(h, w[b + "attn.qkv.weight"], w[b + "attn.qkv.bias"]).view(bsz, -1, 3, HEADS, HIDDEN // HEADS)
        q, k, v = (qkv[:, :, j].transpose(1, 2) for j in range(3))
        att = F.softmax(torch.matmul(q, k.transpose(2, 3)) * (HIDDEN // HEADS) ** -0.5, dim=-1)
        ctx = torch.matmul(att, v).transpose(1, 2).reshape(bsz, -1, HIDDEN)
        x = F.linear(ctx, w[b + "attn.proj.weight"], w[b + "attn.proj.bias"]) * w[b + "ls1.gamma"] + x
        h = F.layer_norm(x, (HIDDEN,), w[b + "norm2.weight"], w[b + "norm2.bias"], LN_EPS)
        h = F.linear(F.gelu(F.linear(h, w[b + "mlp.fc1.weight"], w[b + "mlp.fc1.bias"])), w[b + "mlp.fc2.weight"], w[b + "mlp.fc2.bias"])
        x = h * w[b + "ls2.gamma"] + x
        if stages is not None and i == 0:
            stages["block0"] = x
    x = F.layer_norm(x, (HIDDEN,), w[BB + "norm.weight"], w[BB + "norm.bias"], LN_EPS)
    if stages is not None:
        stages["norm"] = x
    return x


def matching_probs(scores: torch.Tensor, dustbin_score: torch.Tensor, num_iters: int = 3) -> torch.Tensor:
    """The reference's ``get_matching_probs`` + ``log_otp_solver`` (reg = 1), restated: log-space Sinkhorn over the (m + 1) x n score matrix
    whose last row is the dustbin, returning ``log P - norm``. Written in this helper's own form; what it shares with the reference is the
    sequence of torch operations on the values, which a bit-exact restatement must share (``tests/test_megaloc_host.py`` holds it to
    ``np.array_equal`` against the reference run live). Two properties of the reference are kept on purpose: the marginals are float32 tensors
    whatever the dtype of ``scores`` (``norm`` is made by ``torch.tensor`` of a Python float), and the dustbin's mass is added to one float32
    element by a Python float."""
    bsz, m, n = scores.size()
    cost = torch.cat((scores, dustbin_score.to(scores.dtype).expand(bsz, 1, n)), dim=1)  # (B, m + 1, n)
    norm = -torch.tensor(math.log(n + m))
    row_mass = torch.full((m + 1,), float(norm))  # float32: log of the mass of every cluster row ...
    row_mass[m] += math.log(n - m)                # ... and of the dustbin row
    col_mass = torch.full((n,), float(norm))
    u = torch.zeros(bsz, m + 1)
    v = torch.zeros(bsz, n)
    for _ in range(num_iters):
        u = row_mass.expand(bsz, -1) - torch.logsumexp(cost + v[:, None, :], dim=2)
        v = col_mass.expand(bsz, -1) - torch.logsumexp(cost + u[:, :, None], dim=1)
    return cost + u[:, :, None] + v[:, None, :] - norm


def salad(weights, feature_map: torch.Tensor, token: torch.Tensor) -> torch.Tensor:
    """``SALAD.forward`` in eval mode: (B, 768, gh, gw) patch features and the (B, 768) class token -> (B, 16640)."""
    dt = feature_map.dtype
    a = AGG + "agg."
    w = {k: v.to(dt) for k, v in weights.items() if k.startswith(a)}
    conv = lambda x, name: F.conv2d(x, w[a + name + ".weight"], w[a + name + ".bias"])  # noqa: E731
    f = conv(F.relu(conv(feature_map, "cluster_features.0")), "cluster_features.3").flatten(2)
    p = conv(F.relu(conv(feature_map, "score.0")), "score.3").flatten(2)
    t = F.linear(F.relu(F.linear(token, w[a + "token_features.0.weight"], w[a + "token_features.0.bias"])), w[a + "token_features.2.weight"],
                 w[a + "token_features.2.bias"])
    p = torch.exp(matching_probs(p, w[a + "dust_bin"], 3))[:, :-1, :]
    agg = (f.unsqueeze(2) * p.unsqueeze(1)).sum(dim=-1)  # (B, 256, 64): the reference multiplies two repeated (B, 256, 64, n) tensors
    out = torch.cat([F.normalize(t, p=2, dim=-1), F.normalize(agg, p=2, dim=1).flatten(1)], dim=-1)
    return F.normalize(out, p=2, dim=-1)


def head(weights, feature_map: torch.Tensor, token: torch.Tensor, stages: Optional[dict] = None) -> torch.Tensor:
    """``Aggregator`` + ``L2Norm``: SALAD, the linear layer, the final normalisation."""
    dt = feature_map.dtype
    s = salad(weights, feature_map, token)
    if stages is not None:
        stages["salad"] = s
    return F.normalize(F.linear(s, weights[AGG + "linear.weight"].to(dt), weights[AGG + "linear.bias"].to(dt)), p=2.0, dim=1)


def forward(weights, images: torch.Tensor, stages: Optional[dict] = None) -> torch.Tensor:
    """Normalised (B, 3, H, W) float32 / float64 images -> (B, feat_dim) descriptors. ``stages`` (optional dict) receives ``tokens``, ``block0``,
    ``norm`` (each (B, 1 + n, 768)) and ``salad`` (B, 16640)."""
    with torch.no_grad():
        bsz, _, height, width = images.shape
        x = backbone(weights, images, stages)
        fmap = x[:, 1:].reshape(bsz, height // PATCH, width // PATCH, HIDDEN).permute(0, 3, 1, 2)
        return head(weights, fmap, x[:, 0], stages)


def to_hf_state_dict(weights) -> Dict[str, torch.Tensor]:
    """The backbone part in the naming of ``transformers``' ``Dinov2Model`` (fused qkv split into query / key / value)."""
    out = {
        "embeddings.cls_token": weights[BB + "cls_token"],
        "embeddings.mask_token": torch.zeros(1, HIDDEN),
        "embeddings.position_embeddings": weights[BB + "pos_embed"],
        "embeddings.patch_embeddings.projection.weight": weights[BB + "patch_embed.proj.weight"],
        "embeddings.patch_embeddings.projection.bias": weights[BB + "patch_embed.proj.bias"],
        "layernorm.weight": weights[BB + "norm.weight"],
        "layernorm.bias": weights[BB + "norm.bias"],
    }
    for i in range(depth_of(weights)):
        b, h = f"{BB}blocks.{i}.", f"encoder.layer.{i}."
        for j, name in enumerate(("query", "key", "value")):
            out[f"{h}attention.attention.{name}.weight"] = weights[b + "attn.qkv.weight"][j * HIDDEN : (j + 1) * HIDDEN].clone()
            out[f"{h}attention.attention.{name}.bias"] = weights[b + "attn.qkv.bias"][j * HIDDEN : (j + 1) * HIDDEN].clone()
        for src, dst in (("attn.proj", "attention.output.dense"), ("norm1", "norm1"), ("norm2", "norm2"), ("mlp.fc1", "mlp.fc1"), ("mlp.fc2", "mlp.fc2")):
            out[f"{h}{dst}.weight"], out[f"{h}{dst}.bias"] = weights[f"{b}{src}.weight"], weights[f"{b}{src}.bias"]
        out[h + "layer_scale1.lambda1"], out[h + "layer_scale2.lambda1"] = weights[b + "ls1.gamma"], weights[b + "ls2.gamma"]
    return out


def hf_model(weights, dtype=torch.float32):
    """``Dinov2Model`` of the installed ``transformers`` with the seeded backbone weights."""
    from transformers import Dinov2Config, Dinov2Model

    cfg = Dinov2Config(hidden_size=HIDDEN, num_hidden_layers=depth_of(weights), num_attention_heads=HEADS, mlp_ratio=4, image_size=518, patch_size=PATCH,
                       layerscale_value=1.0, layer_norm_eps=LN_EPS)
    model = Dinov2Model(cfg).eval()
    model.load_state_dict(to_hf_state_dict(weights), strict=True)
    return model.to(dtype)


def sample_indices(seed: int, count: int, total: int) -> np.ndarray:
    return np.sort(np.random.default_rng(seed).choice(total, size=min(count, total), replace=False))


STAGES = ("tokens", "block0", "norm", "salad")
SAMPLE = 4096  # stage values kept per golden


def case_record(weight_seed: int, depth: int, feat_dim: int, seed: int, batch: int, height: int, width: int) -> dict:
    """What a golden file holds (tools/make_megaloc_fixture.py): seeds; the descriptors in float64 and float32; per stage a seeded sample of
    the float64 and the float32 restatement's values, ``err_<stage>`` = max |float32 - float64| over the WHOLE stage and its largest magnitude."""
    weights = seeded_weights(weight_seed, depth, feat_dim)
    x = normalise(seeded_images(seed, batch, height, width))
    s32, s64 = {}, {}
    d32, d64 = forward(weights, x, s32), forward(weights, x.double(), s64)
    rec = {"weight_seed": weight_seed, "depth": depth, "feat_dim": feat_dim, "seed": seed, "batch": batch, "height": height, "width": width,
           "descriptors_f64": d64.numpy(), "descriptors_f32": d32.numpy(), "err_descriptors": float((d32.double() - d64).abs().max())}
    for i, st in enumerate(STAGES):
        idx = sample_indices(seed * 10 + i, SAMPLE, s64[st].numel())
        take = torch.from_numpy(idx)
        rec.update({f"{st}_idx": idx.astype(np.int64), f"{st}_f64": s64[st].reshape(-1)[take].numpy(), f"{st}_f32": s32[st].reshape(-1)[take].numpy(),
                    f"err_{st}": float((s32[st].double() - s64[st]).abs().max()), f"max_{st}": float(s64[st].abs().max())})
    return rec


def assert_record_matches(today: dict, golden) -> None:
    """A golden equals what the restatement produces today. Not bit for bit: torch's CPU products sum in an order that depends on the thread count, so
    two runs of the same code differ in the last bits. Bounds by reasoning, not by observation: a float64 evaluation in another summation order
    moves by ~1e-16 x magnitude (< 10) x the depth of the sums, orders of magnitude under 1e-10, while any change of the helper (an operation, a
    seed, a scale) moves values by far more than the float32 rounding level of 1e-7; a float32 evaluation in another order stays at its own
    rounding distance from float64: within 4 x the recorded distance (+ 1e-7) of the recorded float64 value, and its own distance within a
    factor 4 of the recorded one (the factor the GPU tests grant another summation order)."""
    for key in ("weight_seed", "depth", "feat_dim", "seed", "batch", "height", "width"):
        assert int(today[key]) == int(golden[key]), key
    for st in STAGES + ("descriptors",):
        if st != "descriptors":
            assert np.array_equal(today[f"{st}_idx"], golden[f"{st}_idx"]), st
        f64, err = np.asarray(golden[f"{st}_f64"]), float(golden[f"err_{st}"])
        assert np.abs(today[f"{st}_f64"] - f64).max() <= 1e-10, (st, np.abs(today[f"{st}_f64"] - f64).max())
        for f32 in (today[f"{st}_f32"], np.asarray(golden[f"{st}_f32"])):
            assert np.abs(f32.astype(np.float64) - f64).max() <= 4 * err + 1e-7, st
        assert 0.25 * err <= today[f"err_{st}"] <= 4 * err, (st, today[f"err_{st}"], err)


def end_to_end_images(seed: int = 32, groups: int = 6, per_group: int = 4, size: int = 322) -> torch.Tensor:
    """(groups * per_group, 3, size, size) uint8: noisy variants of a few seeded base images, interleaved (image i belongs to group i % groups)."""
    g = torch.Generator().manual_seed(seed)
    bases = seeded_images(seed, groups, size, size).float()
    out = []
    for _ in range(per_group):
        for b in range(groups):
            out.append((bases[b] + torch.randn((3, size, size), generator=g) * 10.0).round().clamp(0, 255))
    return torch.stack(out).to(torch.uint8)
