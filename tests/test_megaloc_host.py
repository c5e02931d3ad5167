"""CPU: the MegaLoc restatement against its pins (the reference's Aggregator / L2Norm where its tree is present, ``transformers``' Dinov2Model)
and its goldens; the checkpoint loaders; the weight packer; the plugin's host contract (registry, pickling, transforms); the new config."""

from __future__ import annotations

import ctypes as C
import os
import pickle
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from tests import megaloc_reference as mr
from tests.conftest import REPO

GOLDEN = REPO / "tests" / "golden"
REFERENCE = Path(os.environ.get("GTSFM_REFERENCE", "/root/reference"))
CASES = sorted(p.stem for p in GOLDEN.glob("megaloc_*.npz"))  # every golden, the depth-12 / 8448 one included (~20 s: 230 M seeded weights, a float32 and a float64 pass)


@pytest.fixture(scope="module")
def weights():
    return mr.seeded_weights(1, depth=2, feat_dim=512)


@pytest.mark.skipif(not (REFERENCE / "thirdparty" / "megaloc" / "megaloc.py").exists(), reason="reference tree not present")
def test_head_equals_live_reference_bit_for_bit():
    """SALAD + linear + L2 norm of the restatement == the reference's Aggregator + L2Norm, ``np.array_equal`` in float32 (tools/make_megaloc_fixture.py
    imports the reference's file by path in a child process)."""
    subprocess.run([sys.executable, str(REPO / "tools" / "make_megaloc_fixture.py"), "--head-only", "--reference", str(REFERENCE)], check=True, cwd=str(REPO))


@pytest.mark.parametrize("shape", [(2, 322, 322), (2, 224, 308)])
def test_backbone_equals_transformers_port(weights, shape):
    """The restatement multiplies by the fused qkv matrix (the checkpoint's layout), the port by three matrices: not the same bits. Bound: 4 x the
    port's own float32-vs-float64 distance, measured here. (Parity towards torch.hub's DINOv2 is unpinned.)"""
    pytest.importorskip("transformers")
    b, h, w = shape
    x = mr.normalise(mr.seeded_images(7, b, h, w))
    m32, m64 = mr.hf_model(weights), mr.hf_model(weights, torch.float64)
    with torch.no_grad():
        ours = mr.backbone(weights, x)
        hf32, hf64 = m32(pixel_values=x).last_hidden_state, m64(pixel_values=x.double()).last_hidden_state
    own = float((hf32.double() - hf64).abs().max())
    dist = float((ours.double() - hf64).abs().max())
    print(f"{h} x {w}: restatement {dist:.3e} from the port's float64; the port's float32 {own:.3e}")
    assert tuple(ours.shape) == (b, 1 + (h // 14) * (w // 14), 768)
    assert 0 < own and dist <= 4 * own
    # float64 against float64: the same model
    assert float((mr.backbone(weights, x.double()) - hf64).abs().max()) < 1e-12


def test_every_golden_is_covered():
    assert {"megaloc_d12_322x322_b2", "megaloc_d2_322x322_b3", "megaloc_d2_224x308_b2", "megaloc_d2_126x126_b2"} <= set(CASES)


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_goldens(name):
    """Fixtures cannot drift from the helper: seeds -> today's restatement against the recorded values, float64 to 1e-10, float32 and its recorded
    distance to the float32 rounding level (``assert_record_matches`` says why not bit for bit: the CPU's summation order follows the thread count)."""
    g = np.load(GOLDEN / f"{name}.npz")
    today = mr.case_record(*(int(g[k]) for k in ("weight_seed", "depth", "feat_dim", "seed", "batch", "height", "width")))
    mr.assert_record_matches(today, g)
    changed = dict(today)
    changed["norm_f64"] = today["norm_f64"] * (1 + 1e-6)  # a drift at the float32 level is caught
    with pytest.raises(AssertionError):
        mr.assert_record_matches(changed, g)


def test_goldens_are_small_and_live():
    for p in GOLDEN.glob("megaloc_*.npz"):
        assert p.stat().st_size < 1024 * 1024, p
        d = np.load(p)["descriptors_f64"]
        sim = d @ d.T
        assert np.allclose(np.diag(sim), 1.0) and sim[0, 1] < 0.99, (p.name, sim)  # different images give different descriptors


def test_checkpoint_round_trip_and_errors(weights, tmp_path):
    from gtsfm_amd.runtime import megaloc_engine as me

    path = tmp_path / "megaloc.torch"
    extra = dict(weights)
    extra[mr.BB + "mask_token"] = torch.zeros(1, 768)  # torch.hub's DINOv2 carries one; unused
    torch.save(extra, path)
    loaded = me.load_checkpoint(path)
    assert mr.BB + "mask_token" not in loaded and set(loaded) == set(weights)
    for k, v in loaded.items():
        assert v.dtype == np.float32 and np.array_equal(v.reshape(-1), weights[k].numpy().reshape(-1)), k
    assert me.depth_of(loaded) == 2 and loaded[mr.AGG + "linear.weight"].shape == (512, 16640)
    assert loaded[mr.AGG + "agg.score.3.weight"].shape == (64, 512) and loaded[mr.BB + "cls_token"].shape == (768,)
    with pytest.raises(FileNotFoundError, match="nope.torch"):
        me.load_checkpoint(tmp_path / "nope.torch")
    bad = dict(weights)
    bad[mr.BB + "blocks.1.mlp.fc1.weight"] = torch.zeros(3072, 767)
    torch.save(bad, path)
    with pytest.raises(ValueError, match="blocks.1.mlp.fc1.weight"):
        me.load_checkpoint(path)
    del bad[mr.BB + "blocks.1.mlp.fc1.weight"]
    with pytest.raises(KeyError, match="blocks.1.mlp.fc1.weight"):
        me.normalise_weights(bad)


def test_hf_named_state_dict_loads_to_the_same_arrays(weights, tmp_path):
    """The second loader: ``Dinov2Model.state_dict()`` names (query / key / value, ``layer_scale1.lambda1``, ...) -> the dictionary ``megaloc.torch`` gives."""
    pytest.importorskip("transformers")
    from gtsfm_amd.runtime import megaloc_engine as me

    torch.save(dict(weights), tmp_path / "megaloc.torch")
    loaded = me.load_checkpoint(tmp_path / "megaloc.torch")
    hf = me.from_hf_state_dict(mr.hf_model(weights).state_dict(), {k: v for k, v in weights.items() if k.startswith(mr.AGG)})
    assert set(loaded) == set(hf)
    for k, v in loaded.items():
        assert hf[k].dtype == np.float32 and np.array_equal(v, hf[k]), k


def test_position_table_is_the_ports_interpolation(weights):
    from gtsfm_amd.runtime import megaloc_engine as me

    pos = weights[mr.BB + "pos_embed"]
    for gh, gw in ((23, 23), (16, 22), (37, 37), (9, 9)):
        assert np.array_equal(me.position_table(pos.numpy(), gh, gw), mr.position_table(pos, gh, gw)[0].numpy())
    assert np.array_equal(me.position_table(pos.numpy(), 37, 37), pos[0].numpy())


def test_weight_packing(weights):
    """Every parameter lands once (LayerScale folded into attn.proj / mlp.fc2 in float32), padding is zero."""
    from gtsfm_amd.runtime import lib as _lib
    from gtsfm_amd.runtime import megaloc_engine as me

    lib = _lib.load()
    packed = me.pack_weights(weights)
    assert packed.size == lib.gtsfm_megaloc_packed_weight_floats(2, 512) and packed.size % 64 == 0
    assert lib.gtsfm_megaloc_packed_weight_floats(0, 512) == 0 and lib.gtsfm_megaloc_packed_weight_floats(2, 500) == 0
    w = me.normalise_weights(weights)
    total, count = 0.0, 0
    for name in me.tensor_order(2):
        a = w[name].astype(np.float64)
        for ls, lin in (("ls1.gamma", "attn.proj"), ("ls2.gamma", "mlp.fc2")):
            if name.endswith(ls):
                a = np.zeros(0)  # folded
            elif name.endswith(lin + ".weight"):
                a = (w[name.replace(lin + ".weight", ls)][:, None] * w[name]).astype(np.float64)  # float32 product, as the packer's
            elif name.endswith(lin + ".bias"):
                a = (w[name.replace(lin + ".bias", ls)] * w[name]).astype(np.float64)
        total += a.sum()
        count += a.size
    assert np.count_nonzero(packed) <= count and packed.size - count < 64 * 8  # (the patch weights and dust_bin are padded to 64 floats)
    assert abs(packed.astype(np.float64).sum() - total) <= 1e-9 * np.abs(packed).astype(np.float64).sum()
    # fields sit where the layout says: the patch embedding first, the output projection's bias last
    assert np.array_equal(packed[: 768 * 588], w[mr.BB + "patch_embed.proj.weight"].reshape(-1))
    assert np.array_equal(packed[-512:], w[mr.AGG + "linear.bias"])
    assert lib.gtsfm_megaloc_workspace_bytes(1, 322, 322, 512) > 0
    for b, h, wd in ((1, 322, 320), (1, 112, 112), (0, 322, 322)):
        assert lib.gtsfm_megaloc_workspace_bytes(b, h, wd, 512) == 0
    assert lib.gtsfm_megaloc_workspace_bytes(400, 322, 322, 512) == lib.gtsfm_megaloc_workspace_bytes(64, 322, 322, 512)  # chunks of 64
    assert lib.gtsfm_megaloc_pack_weights(None, 2, 512, packed.ctypes.data_as(C.c_void_p)) != 0


def test_plugin_contract_without_a_device(tmp_path):
    from gtsfm_amd.frontend import global_descriptor as gd
    from gtsfm_amd.frontend.global_descriptor.global_descriptor_base import GlobalDescriptorBase
    from gtsfm_amd.frontend.global_descriptor.megaloc_global_descriptor import MegaLocGlobalDescriptor

    assert gd.MegaLoc is MegaLocGlobalDescriptor and gd.MegaLocGlobalDescriptor is MegaLocGlobalDescriptor
    assert MegaLocGlobalDescriptor.__name__ == "MegaLocGlobalDescriptor" and issubclass(MegaLocGlobalDescriptor, GlobalDescriptorBase)
    assert {"MegaLoc", "MegaLocGlobalDescriptor", "NetVLAD"} <= set(dir(gd))
    plugin = MegaLocGlobalDescriptor()  # no arguments, no device, no file touched
    plugin._model = object()
    clone = pickle.loads(pickle.dumps(plugin))
    assert clone._model is None and clone._weights_path == plugin._weights_path
    resize, batch = plugin.get_preprocessing_transforms()
    rng = np.random.default_rng(3)
    hwc = rng.integers(0, 256, size=(480, 640, 3), dtype=np.uint8)
    chw = resize(hwc)
    assert chw.dtype == torch.uint8 and tuple(chw.shape) == (3, 322, 322)
    expect = torch.nn.functional.interpolate(torch.from_numpy(hwc).permute(2, 0, 1)[None].float(), size=(322, 322), mode="bilinear", antialias=True,
                                             align_corners=False).round().clamp(0, 255).to(torch.uint8)[0]
    assert torch.equal(chw, expect)
    same = resize(rng.integers(0, 256, size=(322, 322, 3), dtype=np.uint8))
    assert same.dtype == torch.uint8 and tuple(same.shape) == (3, 322, 322)
    x = batch(torch.stack([chw, same]))
    mean, std = torch.tensor([0.485, 0.456, 0.406]).view(-1, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(-1, 1, 1)
    assert x.dtype == torch.float32 and torch.equal(x, (torch.stack([chw, same]).type(torch.float32) / 255.0 - mean) / std)
    assert torch.equal(x, mr.normalise(torch.stack([chw, same])))
    assert plugin.describe_batch(torch.zeros((0, 3, 322, 322))) == []
    with pytest.raises(AssertionError):
        plugin.describe_batch(torch.zeros((3, 322, 322)))


def test_megaloc_config_instantiates_and_pickles():
    from gtsfm_amd.frontend.cacher.global_descriptor_cacher import GlobalDescriptorCacher
    from gtsfm_amd.frontend.global_descriptor import MegaLocGlobalDescriptor
    from gtsfm_amd.retriever import Similarity
    from tests.test_config_hook import instantiate

    cfg = yaml.safe_load((REPO / "gtsfm_amd" / "configs" / "deep_front_end_amd_megaloc.yaml").read_text())
    assert cfg["_target_"] == "gtsfm.retriever.image_pairs_generator.ImagePairsGenerator" and cfg["batch_size"] == 16
    base = yaml.safe_load((REPO / "gtsfm_amd" / "configs" / "deep_front_end_amd_retrieval.yaml").read_text())
    assert cfg["retriever"] == base["retriever"]
    gd, retriever = instantiate(cfg["global_descriptor"]), instantiate(cfg["retriever"])
    assert isinstance(gd, GlobalDescriptorCacher) and isinstance(gd._global_descriptor, MegaLocGlobalDescriptor)
    assert isinstance(retriever, Similarity)
    pickle.loads(pickle.dumps(gd))
    resize, batch = gd.get_preprocessing_transforms()
    assert callable(resize) and callable(batch)
