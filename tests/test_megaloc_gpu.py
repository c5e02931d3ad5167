"""GPU: MegaLoc on libgtsfm_amd.so against the goldens of tests/megaloc_reference.py (SALAD head and output projection pinned to the reference's
code bit for bit on the CPU, the backbone to the ``transformers`` port; parity unpinned towards ``torch.hub``'s DINOv2), stage by stage; batch /
run-to-run identity; the uint8 path; the input checks; a batch past 2^31 bytes of hidden activations; the plugin end to end; the cacher.

Tolerance, every stage: the golden records ``err`` = max |float32 restatement - float64 restatement| measured on the CPU when it was written; the
GPU must be within 4 x err + 1e-7 of the float64 value (the rule of ``test_netvlad_gpu.py::test_accuracy_against_float64``: another summation order
in the same precision may cost a small multiple of the reference's own rounding distance, not more)."""

from __future__ import annotations

import pickle
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import megaloc_reference as mr
from tests import netvlad_reference as nr

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
CASES = sorted(p.stem for p in GOLDEN.glob("megaloc_*.npz"))
STAGES = ("tokens", "block0", "norm", "salad")
# the plugin's end-to-end case (tools/make_megaloc_fixture.py: E2E)
E2E = {"weight_seed": 2, "depth": 2, "feat_dim": 512, "num_matched": 5, "min_score": 0.985}

_engines: dict = {}


def _engine(weight_seed: int, depth: int, feat_dim: int):
    """One engine per seeded model; the depth-12 one (0.9 GB of weights) is dropped again when a shallow one is asked for."""
    from gtsfm_amd.runtime.megaloc_engine import MegaLocEngine

    key = (weight_seed, depth, feat_dim)
    if key not in _engines:
        _engines.clear()
        torch.cuda.empty_cache()
        _engines[key] = MegaLocEngine(mr.seeded_weights(weight_seed, depth, feat_dim))
    return _engines[key]


@pytest.fixture()
def shallow():
    return _engine(1, 2, 512)


def _golden(name):
    g = np.load(GOLDEN / f"{name}.npz")
    images = mr.seeded_images(int(g["seed"]), int(g["batch"]), int(g["height"]), int(g["width"]))
    return g, images


def test_goldens_present():
    assert {"megaloc_d12_322x322_b2", "megaloc_d2_322x322_b3", "megaloc_d2_224x308_b2", "megaloc_d2_126x126_b2"} <= set(CASES)


@pytest.mark.parametrize("name", CASES)
def test_stages_match_goldens(name):
    g, u8 = _golden(name)
    engine = _engine(int(g["weight_seed"]), int(g["depth"]), int(g["feat_dim"]))
    images = mr.normalise(u8)
    n = (u8.shape[2] // 14) * (u8.shape[3] // 14)
    failures = []
    for k, stage in enumerate(STAGES):
        out = engine.stage(images, k)
        assert tuple(out.shape) == ((u8.shape[0], mr.SALAD_DIM) if stage == "salad" else (u8.shape[0], 1 + n, 768))
        got = out.cpu().reshape(-1).numpy().astype(np.float64)[g[f"{stage}_idx"]]
        err, tol = np.abs(got - g[f"{stage}_f64"]).max(), 4 * float(g[f"err_{stage}"]) + 1e-7
        print(f"{name} {stage}: GPU {err:.3e} from float64, fp32 restatement {float(g[f'err_{stage}']):.3e}, bound {tol:.3e}, magnitude {float(g[f'max_{stage}']):.3g}")
        if not err <= tol:
            failures.append((stage, err, tol))
    desc = engine.describe(images).cpu().numpy().astype(np.float64)
    assert desc.shape == g["descriptors_f64"].shape
    err, tol = np.abs(desc - g["descriptors_f64"]).max(), 4 * float(g["err_descriptors"]) + 1e-7
    print(f"{name} descriptors: GPU {err:.3e} from float64, fp32 restatement {float(g['err_descriptors']):.3e}, bound {tol:.3e}")
    if not err <= tol:
        failures.append(("descriptors", err, tol))
    assert not failures, failures
    assert np.abs(np.linalg.norm(desc, axis=1) - 1).max() < 1e-6


@pytest.mark.parametrize("batch", [1, 3, 16])
def test_batched_equals_single_and_repeatable(shallow, batch):
    images = mr.normalise(mr.seeded_images(50 + batch, batch, 322, 322))
    out = shallow.describe(images)
    assert torch.equal(out, shallow.describe(images)), "two runs differ"
    for i in range(batch):
        assert torch.equal(out[i : i + 1], shallow.describe(images[i : i + 1])), f"image {i}: batched != alone"
    if batch == 3:
        for k in range(4):
            assert torch.equal(shallow.stage(images, k)[1:2], shallow.stage(images[1:2], k)), f"stage {k}"


def test_uint8_path_equals_float_path(shallow):
    _, u8 = _golden("megaloc_d2_224x308_b2")
    images = mr.normalise(u8)  # (u8.float() / 255 - mean) / std on the CPU, float32
    assert torch.equal(shallow.stage(u8, 0), shallow.stage(images, 0))
    assert torch.equal(shallow.describe(u8), shallow.describe(images))


def test_device_input_and_checks(shallow):
    _, u8 = _golden("megaloc_d2_126x126_b2")
    images = mr.normalise(u8)
    assert torch.equal(shallow.describe(images.cuda()), shallow.describe(images))
    assert torch.equal(shallow.describe(u8.cuda()), shallow.describe(images))
    for value in (float("nan"), float("inf")):
        bad = images.clone()
        bad[1, 2, 5, 7] = value
        with pytest.raises(ValueError, match="non-finite"):
            shallow.describe(bad)
        with pytest.raises(ValueError, match="non-finite"):
            shallow.describe(bad.cuda())
    shallow.describe(images)  # the flag is cleared per call
    with pytest.raises(AssertionError):
        shallow.describe(images[:, :2])
    for shape in ((1, 3, 322, 320), (2, 3, 125, 126)):
        with pytest.raises(ValueError, match="multiples of 14"):
            shallow.describe(torch.zeros(shape))
    with pytest.raises(ValueError, match="more than 64 patches"):
        shallow.describe(torch.zeros((1, 3, 112, 112)))  # n = 64: log(n - 64) in the reference
    with pytest.raises(ValueError, match="more than 64 patches"):
        shallow.stage(torch.zeros((1, 3, 56, 140)), 3)
    assert tuple(shallow.describe(torch.zeros((0, 3, 322, 322))).shape) == (0, 512)


@pytest.mark.parametrize("height,width,n", [(168, 714, 612), (350, 350, 625)])
def test_score_matrix_at_and_past_the_lds_limit(shallow, height, width, n):
    """The SALAD kernel keeps the 65 x n matrix in LDS while (512 + ceil64(n) + 65 n) floats fit in the CU's 160 KiB: n = 612 (168 x 714) is the last
    such size, 163 728 of 163 840 bytes with 1024 threads, the largest allocation the code permits; at n = 625 (350 x 350) the same kernel keeps the
    matrix in the workspace. Same rule for both: within 4 x the float32 restatement's own distance from float64 (+ 1e-7), computed here."""
    assert (height // 14) * (width // 14) == n
    assert ((512 + (n + 63) // 64 * 64 + 65 * n) * 4 <= 160 * 1024) == (n == 612)
    u8 = mr.seeded_images(61, 2, height, width)
    images = mr.normalise(u8)
    weights = mr.seeded_weights(1, 2, 512)
    s32, s64 = {}, {}
    d32, d64 = mr.forward(weights, images, s32), mr.forward(weights, images.double(), s64)
    for got, f32, f64, what in ((shallow.stage(images, 3), s32["salad"], s64["salad"], "salad"), (shallow.describe(images), d32, d64, "descriptors")):
        err, own = float((got.cpu().double() - f64).abs().max()), float((f32.double() - f64).abs().max())
        print(f"{height} x {width} {what}: GPU {err:.3e} from float64, fp32 restatement {own:.3e}")
        assert err <= 4 * own + 1e-7, what
    out = shallow.describe(images)
    assert torch.equal(out[1:2], shallow.describe(images[1:2])) and torch.equal(out, shallow.describe(u8))


def test_batch_past_2_31_bytes_of_hidden_activations(shallow):
    """400 images at 322 x 322: 400 * 530 tokens * 3072 * 4 bytes > 2^31. The library runs the batch in chunks of at most 64 images through
    one workspace; the first and the last image equal themselves alone."""
    b = 400
    assert b * 530 * 3072 * 4 > 2**31
    gen = torch.Generator(device="cuda").manual_seed(5)
    u8 = torch.randint(0, 256, (b, 3, 322, 322), generator=gen, device="cuda", dtype=torch.uint8)
    out = shallow.describe(u8)
    for i in (0, 63, 64, b - 1):
        assert torch.equal(out[i : i + 1], shallow.describe(u8[i : i + 1].clone())), f"image {i}"
    del u8, out
    shallow._ws = None
    torch.cuda.empty_cache()


def test_plugin_end_to_end(tmp_path):
    """24 seeded images -> MegaLoc().describe_batch in batches of 16 (unified_megaloc.yaml's batch_size) -> Similarity(5, 0.985): the pair list of
    the CPU restatement's descriptors. No decision of the float64 restatement lies within 1e-5 of its boundary (asserted)."""
    from gtsfm_amd.frontend.global_descriptor import MegaLoc
    from gtsfm_amd.retriever import Similarity

    weights = mr.seeded_weights(E2E["weight_seed"], E2E["depth"], E2E["feat_dim"])
    ckpt = tmp_path / "megaloc.torch"
    torch.save(weights, ckpt)
    plugin = MegaLoc(weights_path=ckpt)
    retriever = Similarity(num_matched=E2E["num_matched"], min_score=E2E["min_score"])
    plugin, retriever = pickle.loads(pickle.dumps(plugin)), pickle.loads(pickle.dumps(retriever))
    _, batch_transform = plugin.get_preprocessing_transforms()
    u8 = mr.end_to_end_images()
    assert len(u8) == 24
    descs, ref32, ref64 = [], [], []
    for i in range(0, len(u8), 16):
        batch = batch_transform(u8[i : i + 16])
        out = plugin.describe_batch(batch)
        assert all(isinstance(d, np.ndarray) and d.dtype == np.float32 and d.shape == (E2E["feat_dim"],) for d in out)
        descs.extend(out)
        ref32.extend(mr.forward(weights, batch).numpy())
        ref64.extend(mr.forward(weights, batch.double()).numpy())
    nr.assert_margins(np.array(ref64), E2E["num_matched"], E2E["min_score"])
    fnames = [f"img{i}.jpg" for i in range(len(u8))]
    pairs = retriever.get_image_pairs(descs, fnames)
    expect = nr.pairs_from_score_matrix(nr.similarity_matrix(ref32), E2E["num_matched"], E2E["min_score"])
    assert pairs == expect and len(pairs) >= 24
    assert plugin.describe_batch(torch.zeros((0, 3, 322, 322))) == []
    with pytest.raises(FileNotFoundError, match="nope.torch"):
        MegaLoc(weights_path=tmp_path / "nope.torch").describe_batch(batch_transform(u8[:1]))


def test_global_descriptor_cacher_round_trip(tmp_path):
    """GlobalDescriptorCacher keys its entries by the wrapped object's class name: ``MegaLocGlobalDescriptor``. A second cacher over the same
    directory answers from the cache (its plugin has no checkpoint to load)."""
    from gtsfm_amd.frontend.cacher import global_descriptor_cacher as gdc
    from gtsfm_amd.frontend.global_descriptor import MegaLocGlobalDescriptor

    weights = mr.seeded_weights(E2E["weight_seed"], E2E["depth"], E2E["feat_dim"])
    torch.save(weights, tmp_path / "megaloc.torch")
    plugin = MegaLocGlobalDescriptor(weights_path=tmp_path / "megaloc.torch")
    batch = mr.normalise(mr.seeded_images(9, 2, 126, 126))
    first = gdc.GlobalDescriptorCacher(plugin, cache_root=tmp_path / "cache").describe_batch(batch)
    assert list((tmp_path / "cache" / "global_descriptor").glob("MegaLocGlobalDescriptor_*.pbz2"))
    assert type(plugin).__name__ == "MegaLocGlobalDescriptor" and len(first) == 2 and first[0].shape == (E2E["feat_dim"],)
    again = gdc.GlobalDescriptorCacher(MegaLocGlobalDescriptor(weights_path=tmp_path / "nope.torch"), cache_root=tmp_path / "cache").describe_batch(batch)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
