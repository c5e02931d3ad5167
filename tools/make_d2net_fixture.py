"""Regenerate tests/golden/d2net_*.npz from seeds, after checking that the torch restatement (tests/d2net_reference.py) is the
reference's own D2-Net bit for bit.

Runs only where the GTSfM reference tree is present (``--reference``, default ``$GTSFM_REFERENCE`` or /root/reference), with the
reference on ``sys.path`` (packages that are not installed and that this path never touches are replaced by inert modules). Per case
it checks, bit for bit:
  * the dense map against ``DenseFeatureExtractionModule``, the detections against ``HardDetectionModule`` and the steps at every
    detection against ``HandcraftedLocalizationModule`` (torch's CPU ``F.conv2d`` with the 3 x 3 derivative filters);
  * keypoints, scores and descriptors against ``process_multiscale(scales=[1])``;
  * the plugin's output against ``D2NetDetDesc.detect_and_describe`` reading a seeded checkpoint ``{"model": state_dict}``.
The goldens hold outputs only: keypoints, scores, descriptors (a seeded column sample when there are many keypoints), the candidates'
(channel, i, j), seeded samples of relu(conv1_1), relu(conv3_3) and the dense map, the float64 evaluation's results as differences to
the float32 ones, and the float32-to-float64 distances the tests' tolerances derive from. Inputs and weights are regenerated from seeds.

Usage: python tools/make_d2net_fixture.py [--reference DIR] [--check-only]
"""

from __future__ import annotations

import argparse
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "oracle"))

from tests import d2net_reference as dr  # noqa: E402

WEIGHT_SEED = 0
SAMPLE = 4096       # stage values kept per file
DESC_COLUMNS = 128  # descriptor columns kept when a case has more than DESC_FULL_ROWS keypoints
DESC_FULL_ROWS = 100
# (name, image seed, height, width)
CASES = [("d2net_64x80", 21, 64, 80), ("d2net_123x157", 22, 123, 157), ("d2net_240x320", 23, 240, 320), ("d2net_16x16", 24, 16, 16)]
EXTRA_COUNT_SHAPES = [(25, 480, 640)]  # keypoint count and closest adjacent scores only (INTEGRATION.md quotes them)


def stage_sample(x: torch.Tensor, seed: int) -> tuple:
    """Seeded sample of an NCHW stage output, as (flat NHWC indices, values)."""
    nhwc = x.permute(0, 2, 3, 1).contiguous().reshape(-1)
    idx = np.sort(np.random.default_rng(seed).choice(nhwc.numel(), size=min(SAMPLE, nhwc.numel()), replace=False))
    return idx.astype(np.int64), nhwc[torch.from_numpy(idx)].numpy()


def rel_err(a: torch.Tensor, b64: torch.Tensor) -> float:
    return float((a.double() - b64).abs().max() / b64.abs().max())


def match_by_candidate(ca: np.ndarray, cb: np.ndarray):
    """Rows of ``ca`` and ``cb`` (n, 3) that name the same (channel, i, j): (indices into a, indices into b)."""
    index = {tuple(r): k for k, r in enumerate(cb.tolist())}
    pairs = [(k, index[tuple(r)]) for k, r in enumerate(ca.tolist()) if tuple(r) in index]
    return np.array([p[0] for p in pairs], dtype=np.int64), np.array([p[1] for p in pairs], dtype=np.int64)


def check_against_reference(weights, image, ours, stages, reference_modules) -> None:
    D2Net, process_multiscale = reference_modules
    model = D2Net(model_file=None, use_relu=True, use_cuda=False).eval()
    model.load_state_dict(weights)
    x = torch.from_numpy(dr.normalise(image))[None]
    with torch.no_grad():
        dense = model.dense_feature_extraction(x)
        assert torch.equal(dense, stages["dense"]), "dense map differs from DenseFeatureExtractionModule"
        detected = model.detection(dense)[0]
        steps = model.localization(dense)[0]
        kps, scores, desc = process_multiscale(x, model, scales=[1])
    c, i, j = ours["cand"].T
    assert bool(detected[c, i, j].all()), "a candidate is not a detection of HardDetectionModule"
    assert np.array_equal(steps[0][c, i, j].numpy(), ours["steps"][:, 0]) and np.array_equal(steps[1][c, i, j].numpy(), ours["steps"][:, 1]), \
        "steps differ from HandcraftedLocalizationModule"
    assert kps.shape == (len(c), 3) and scores.shape == (len(c),) and desc.shape == (len(c), 512), (kps.shape, len(c))
    # process_multiscale lists its keypoints in torch.nonzero order: (channel, i, j) ascending
    order = np.lexsort((j, i, c))
    assert np.array_equal(kps[:, [1, 0]], ours["keypoints"][order]) and np.all(kps[:, 2] == 1), "keypoints differ from process_multiscale"
    assert np.array_equal(scores, ours["scores"][order]), "scores differ from process_multiscale"
    assert np.array_equal(desc, ours["descriptors"][order]), "descriptors differ from process_multiscale"


def check_plugin(reference_plugin, checkpoint: Path, image, ours, max_keypoints) -> None:
    ref_d2, Image = reference_plugin
    plugin = ref_d2.D2NetDetDesc(max_keypoints=max_keypoints, model_path=checkpoint, use_cuda=False)
    kps, desc = plugin.detect_and_describe(Image(value_array=image))
    n = min(len(ours["cand"]), max_keypoints)
    assert kps.coordinates.shape == (n, 2) and desc.shape == (n, 512)
    if len(np.unique(ours["cand_scores"])) == len(ours["cand_scores"]):  # distinct scores: the unstable argsort has one answer
        assert np.array_equal(kps.coordinates, ours["keypoints"][:n]) and np.array_equal(kps.responses, ours["scores"][:n]), "plugin keypoints"
        assert np.array_equal(desc, ours["descriptors"][:n]), "plugin descriptors"
    else:
        assert np.array_equal(np.sort(kps.responses)[::-1], ours["scores"][:n]), "plugin scores"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GTSFM_REFERENCE", "/root/reference"))
    ap.add_argument("--check-only", action="store_true")
    args = ap.parse_args()
    reference = Path(args.reference)
    if not (reference / "thirdparty" / "d2net" / "lib" / "model_test.py").exists():
        sys.exit(f"reference tree not found under {reference}")
    from validate_cache_against_reference import _AbsentPackages

    sys.meta_path.insert(0, _AbsentPackages())
    sys.path.insert(0, str(reference))
    import gtsfm.frontend.detector_descriptor.d2net as ref_d2
    from gtsfm.common.image import Image
    from thirdparty.d2net.lib.model_test import D2Net
    from thirdparty.d2net.lib.pyramid import process_multiscale

    assert Path(ref_d2.__file__).is_relative_to(reference)
    assert ref_d2.USE_MULTISCALE is False and ref_d2.USE_RELU is True and ref_d2.PREPROCESSING_METHOD == "torch"
    weights = dr.seeded_weights(WEIGHT_SEED)
    with tempfile.TemporaryDirectory() as tmp:
        checkpoint = Path(tmp) / "d2_tf.pth"
        torch.save({"model": weights}, str(checkpoint))
        for name, seed, h, w in CASES:
            image = dr.seeded_image(seed, h, w)
            stages: dict = {}
            ours = dr.forward(weights, image, stages=stages)
            check_against_reference(weights, image, ours, stages, (D2Net, process_multiscale))
            for cap in (5000, 10):
                check_plugin((ref_d2, Image), checkpoint, image, dr.forward(weights, image, max_keypoints=cap), cap)
            s64: dict = {}
            f64 = dr.forward(weights, image, dtype=torch.float64, stages=s64)
            ia, ib = match_by_candidate(ours["cand"], f64["cand"])
            n, n64 = len(ours["cand"]), len(f64["cand"])
            smax = float(np.abs(f64["scores"]).max()) if n64 else 1.0
            err = {
                "conv1_err64": rel_err(stages["conv1_1"], s64["conv1_1"]), "conv3_err64": rel_err(stages["conv3_3"], s64["conv3_3"]),
                "dense_err64": rel_err(stages["dense"], s64["dense"]),
                "kp_err64": float(np.abs(ours["keypoints"][ia] - f64["keypoints"][ib]).max()) if len(ia) else 0.0,
                "score_err64": float(np.abs(ours["scores"][ia] - f64["scores"][ib]).max() / smax) if len(ia) else 0.0,
                "desc_err64": float(np.abs(ours["descriptors"][ia] - f64["descriptors"][ib]).max()) if len(ia) else 0.0,
            }
            gaps = -np.diff(ours["cand_scores"].astype(np.float64)) / smax if n > 1 else np.array([np.inf])
            print(f"{name}: restatement == reference, bit for bit; map {tuple(stages['dense'].shape[2:])}, {n} keypoints (float64: {n64}, "
                  f"{n - len(ia)} / {n64 - len(ib)} unmatched), map max {float(stages['dense'].max()):.3f}, closest adjacent scores "
                  f"{gaps.min():.2e} of the maximum; " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()), flush=True)
            if args.check_only:
                continue
            cols = np.arange(512) if n <= DESC_FULL_ROWS else np.sort(np.random.default_rng(seed + 400).choice(512, size=DESC_COLUMNS, replace=False))
            i1, v1 = stage_sample(stages["conv1_1"], seed + 100)
            i3, v3 = stage_sample(stages["conv3_3"], seed + 200)
            i4, v4 = stage_sample(stages["dense"], seed + 300)
            d32 = ours["descriptors"][:, cols]
            np.savez_compressed(
                REPO / "tests" / "golden" / f"{name}.npz", seed=seed, height=h, width=w, weight_seed=WEIGHT_SEED,
                keypoints=ours["keypoints"], scores=ours["scores"], desc_cols=cols.astype(np.int16), descriptors=d32, cand=ours["cand"].astype(np.int16),
                steps=ours["steps"], conv1_idx=i1, conv1_val=v1, conv3_idx=i3, conv3_val=v3, conv3_shape=np.array(stages["conv3_3"].shape),
                dense_idx=i4, dense_val=v4, dense_shape=np.array(stages["dense"].shape), dense_max=np.float32(stages["dense"].max()),
                f64_cand=f64["cand"].astype(np.int16), f64_keypoints=f64["keypoints"], f64_scores=f64["scores"],
                f64_desc_minus_f32=(f64["descriptors"][ib][:, cols] - d32[ia].astype(np.float64)).astype(np.float32), f64_match_f32=ia, f64_match_f64=ib,
                **{k: np.float64(v) for k, v in err.items()})
        for seed, h, w in ([] if args.check_only else EXTRA_COUNT_SHAPES):
            ours = dr.forward(weights, dr.seeded_image(seed, h, w))
            f64 = dr.forward(weights, dr.seeded_image(seed, h, w), dtype=torch.float64)
            ia, ib = match_by_candidate(ours["cand"], f64["cand"])
            gaps = -np.diff(ours["cand_scores"].astype(np.float64)) / float(ours["cand_scores"].max())
            print(f"{h}x{w}: {len(ours['cand'])} keypoints (float64: {len(f64['cand'])}, {len(ours['cand']) - len(ia)} / {len(f64['cand']) - len(ib)} unmatched), "
                  f"closest adjacent scores {gaps.min():.2e} of the maximum", flush=True)


if __name__ == "__main__":
    main()
