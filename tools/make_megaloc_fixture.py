"""Regenerate tests/golden/megaloc_*.npz from seeds, after checking the torch restatement (tests/megaloc_reference.py) against its two pins:

* the SALAD head, the linear layer and the final norm against the reference's own ``Aggregator`` / ``L2Norm`` (``thirdparty/megaloc/megaloc.py``),
  bit for bit in float32. The file is imported by path in a child process with ``torchvision`` and ``gtsfm.utils.logger`` stubbed; only
  ``Aggregator`` and ``L2Norm`` are built (``DINOv2`` would reach for ``torch.hub``). Needs the reference tree (``--reference``, default
  ``$GTSFM_REFERENCE`` or /root/reference); skipped with a note when it is absent.
* the backbone against ``transformers``' ``Dinov2Model`` on the same seeded weights, within 4 x the port's own float32-vs-float64 distance
  (the restatement multiplies by a fused qkv matrix, the port by three: not the same bits). Parity towards ``torch.hub``'s DINOv2 is unpinned.

The goldens hold seeds, float64 values of every stage (sampled for the large ones), the float32 restatement's values at the same places and
``err_<stage>`` = max |float32 restatement - float64 restatement| over the whole stage: the GPU test's tolerance is 4 x that + 1e-7.

Usage: python tools/make_megaloc_fixture.py [--reference DIR] [--check-only]
"""

from __future__ import annotations

import argparse
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from tests import megaloc_reference as mr  # noqa: E402
from tests import netvlad_reference as nr  # noqa: E402

# (name, weight seed, depth, feat_dim, image seed, batch, height, width)
CASES = [
    ("megaloc_d12_322x322_b2", 0, 12, 8448, 41, 2, 322, 322),
    ("megaloc_d2_322x322_b3", 1, 2, 512, 42, 3, 322, 322),
    ("megaloc_d2_224x308_b2", 1, 2, 512, 43, 2, 224, 308),
    ("megaloc_d2_126x126_b2", 1, 2, 512, 44, 2, 126, 126),
]
# the plugin's end-to-end case (tests/test_megaloc_gpu.py): weight seed, depth, feat_dim, Similarity(num_matched, min_score)
E2E = {"weight_seed": 2, "depth": 2, "feat_dim": 512, "num_matched": 5, "min_score": 0.985}

_CHILD = r"""
import importlib.util, logging, sys, types
from pathlib import Path
import numpy as np, torch

ref, sd_path, in_path, out_path, feat_dim = sys.argv[1:6]
tv = types.ModuleType("torchvision"); tvt = types.ModuleType("torchvision.transforms"); tv.transforms = tvt
g = types.ModuleType("gtsfm"); gu = types.ModuleType("gtsfm.utils"); gl = types.ModuleType("gtsfm.utils.logger")
gl.get_logger = lambda: logging.getLogger("reference")
g.utils, gu.logger = gu, gl
sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "gtsfm": g, "gtsfm.utils": gu, "gtsfm.utils.logger": gl})
spec = importlib.util.spec_from_file_location("reference_megaloc", str(Path(ref) / "thirdparty" / "megaloc" / "megaloc.py"))
mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
agg = mod.Aggregator(feat_dim=int(feat_dim), agg_config={"num_channels": 768, "num_clusters": 64, "cluster_dim": 256, "token_dim": 256, "mlp_dim": 512},
                     salad_out_dim=64 * 256 + 256).eval()
agg.load_state_dict(torch.load(sd_path), strict=True)
data = np.load(in_path)
with torch.no_grad():
    out = mod.L2Norm()(agg((torch.from_numpy(data["x"]), torch.from_numpy(data["t"]))))
np.save(out_path, out.numpy())
"""


def reference_head(reference: Path, weights, x: torch.Tensor, t: torch.Tensor) -> np.ndarray:
    """The reference's ``L2Norm(Aggregator((x, t)))`` with the seeded ``aggregator.*`` weights."""
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        torch.save({k[len(mr.AGG) :]: v for k, v in weights.items() if k.startswith(mr.AGG)}, tmp / "sd.pt")
        np.savez(tmp / "in.npz", x=x.numpy(), t=t.numpy())
        feat_dim = weights[mr.AGG + "linear.bias"].numel()
        subprocess.run([sys.executable, "-c", _CHILD, str(reference), str(tmp / "sd.pt"), str(tmp / "in.npz"), str(tmp / "out.npy"), str(feat_dim)], check=True)
        return np.load(tmp / "out.npy")


def check_head(reference: Path) -> None:
    weights = mr.seeded_weights(1, depth=1, feat_dim=512)
    g = torch.Generator().manual_seed(5)
    for b, gh, gw in ((2, 23, 23), (1, 16, 22), (3, 9, 9)):
        x, t = torch.randn((b, mr.HIDDEN, gh, gw), generator=g), torch.randn((b, mr.HIDDEN), generator=g)
        with torch.no_grad():
            ours = mr.head(weights, x, t).numpy()
        assert np.array_equal(ours, reference_head(reference, weights, x, t)), f"SALAD + linear + L2: restatement differs from the reference at {b} x {gh} x {gw}"
        print(f"head {b} x {gh} x {gw}: restatement == reference's Aggregator + L2Norm, bit for bit", flush=True)


def check_backbone() -> None:
    weights = mr.seeded_weights(1, depth=2, feat_dim=512)
    m32, m64 = mr.hf_model(weights), mr.hf_model(weights, torch.float64)
    for seed, b, h, w in ((7, 2, 322, 322), (8, 2, 224, 308)):
        x = mr.normalise(mr.seeded_images(seed, b, h, w))
        with torch.no_grad():
            ours = mr.backbone(weights, x)
            hf32, hf64 = m32(pixel_values=x).last_hidden_state, m64(pixel_values=x.double()).last_hidden_state
        own = float((hf32.double() - hf64).abs().max())
        dist = float((ours.double() - hf64).abs().max())
        assert dist <= 4 * own, f"backbone {h} x {w}: restatement {dist:.3e} from the port's float64, the port's own float32 {own:.3e}"
        print(f"backbone {h} x {w}: restatement within {dist:.3e} of Dinov2Model float64 (the port's float32: {own:.3e})", flush=True)


def e2e_check() -> float:
    """The plugin's end-to-end case must not sit on a decision boundary: float64 margins of Similarity(num_matched, min_score)."""
    weights = mr.seeded_weights(E2E["weight_seed"], E2E["depth"], E2E["feat_dim"])
    x = mr.normalise(mr.end_to_end_images())
    d64 = torch.cat([mr.forward(weights, x[i : i + 16].double()) for i in range(0, len(x), 16)]).numpy()
    nr.assert_margins(d64, E2E["num_matched"], E2E["min_score"])
    return nr.decision_margin(d64, E2E["num_matched"], E2E["min_score"])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GTSFM_REFERENCE", "/root/reference"))
    ap.add_argument("--check-only", action="store_true")
    ap.add_argument("--head-only", action="store_true", help="only the check against the reference's Aggregator / L2Norm")
    args = ap.parse_args()
    reference = Path(args.reference)
    if (reference / "thirdparty" / "megaloc" / "megaloc.py").exists():
        check_head(reference)
    else:
        print(f"reference tree not found under {reference}: the SALAD head is NOT re-checked against it")
    if args.head_only:
        return
    check_backbone()
    print(f"end-to-end case: smallest float64 decision margin {e2e_check():.3e}", flush=True)
    for name, *case in CASES:
        rec = mr.case_record(*case)
        path = REPO / "tests" / "golden" / f"{name}.npz"
        print(name, {k: f"{v:.3e}" for k, v in rec.items() if k.startswith("err_")}, flush=True)
        if args.check_only:
            mr.assert_record_matches(rec, np.load(path))
            continue
        np.savez_compressed(path, **rec)


if __name__ == "__main__":
    main()
