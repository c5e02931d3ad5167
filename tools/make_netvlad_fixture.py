"""Regenerate tests/golden/netvlad_*.npz from seeds, after checking that the torch restatement (tests/netvlad_reference.py) is the
reference's own NetVLAD bit for bit.

Runs only where the GTSfM reference tree is present (``--reference``, default ``$GTSFM_REFERENCE`` or /root/reference). The reference's
``thirdparty/hloc/netvlad.py`` is imported by path in a child process, with ``torchvision.models.vgg16`` (VGG16's ``features``
layer list, restated) and ``gtsfm.utils.logger`` (needs dask) stubbed, and reads a seeded checkpoint written in the real file's
layout, so its own parse runs. The goldens hold outputs only: the final descriptors (or the 32768-vector without whitening), the
pre-whitening vector and seeded samples of relu(conv1_1) and conv5_3; inputs and weights are regenerated from the seeds.

Usage: python tools/make_netvlad_fixture.py [--reference DIR] [--check-only]
"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from tests import netvlad_reference as nr  # noqa: E402

WEIGHT_SEED = 0
SAMPLE = 4096  # stage values kept per file
# (name, image seed, batch, height, width, whiten)
CASES = [
    ("netvlad_120x160_b3", 11, 3, 120, 160, True),
    ("netvlad_123x157_b2", 12, 2, 123, 157, True),
    ("netvlad_480x640_b2", 13, 2, 480, 640, True),
    ("netvlad_120x160_b2_nowhiten", 14, 2, 120, 160, False),
]

_CHILD = r"""
import importlib.util, json, logging, sys, types
from pathlib import Path
import numpy as np, torch, torch.nn as nn

ref, mat_dir, case_json, out_path = sys.argv[1:5]
case = json.loads(case_json)

def vgg16():
    cfg = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]
    layers, cin = [], 3
    for v in cfg:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    m = nn.Module()
    m.features = nn.Sequential(*layers)
    return m

tv = types.ModuleType("torchvision"); tvm = types.ModuleType("torchvision.models"); tvm.vgg16 = vgg16; tv.models = tvm
sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, tvm
g = types.ModuleType("gtsfm"); gu = types.ModuleType("gtsfm.utils"); gl = types.ModuleType("gtsfm.utils.logger")
gl.get_logger = lambda: logging.getLogger("reference")
g.utils, gu.logger = gu, gl
sys.modules.update({"gtsfm": g, "gtsfm.utils": gu, "gtsfm.utils.logger": gl})
spec = importlib.util.spec_from_file_location("reference_netvlad", str(Path(ref) / "thirdparty" / "hloc" / "netvlad.py"))
mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
# the reference downloads a missing checkpoint with wget: the seeded file must be there, and no program may be started
assert (Path(mat_dir) / "VGG16-NetVLAD-Pitts30K.mat").exists(), mat_dir
def _no_subprocess(*args, **kwargs):
    raise RuntimeError(f"the reference tried to start {args!r}")
mod.subprocess.run = _no_subprocess
conf = {"model_name": "VGG16-NetVLAD-Pitts30K", "checkpoint_dir": Path(mat_dir), "whiten": case["whiten"]}
model = mod.NetVLAD(conf).eval()
images = torch.from_numpy(np.load(case["images"]))
with torch.no_grad():
    desc = model({"image": images})["global_descriptor"]
np.save(out_path, desc.numpy())
"""


def reference_forward(reference: Path, mat_dir: Path, images: torch.Tensor, whiten: bool) -> np.ndarray:
    with tempfile.TemporaryDirectory() as tmp:
        np.save(Path(tmp) / "images.npy", images.numpy())
        out = Path(tmp) / "out.npy"
        case = json.dumps({"images": str(Path(tmp) / "images.npy"), "whiten": whiten})
        subprocess.run([sys.executable, "-c", _CHILD, str(reference), str(mat_dir), case, str(out)], check=True)
        return np.load(out)


def stage_sample(x: torch.Tensor, seed: int) -> tuple:
    """Seeded sample of an NCHW stage output, as (flat NHWC indices, values)."""
    nhwc = x.permute(0, 2, 3, 1).contiguous().reshape(-1)
    idx = np.sort(np.random.default_rng(seed).choice(nhwc.numel(), size=min(SAMPLE, nhwc.numel()), replace=False))
    return idx.astype(np.int64), nhwc[torch.from_numpy(idx)].numpy()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GTSFM_REFERENCE", "/root/reference"))
    ap.add_argument("--check-only", action="store_true")
    args = ap.parse_args()
    reference = Path(args.reference)
    if not (reference / "thirdparty" / "hloc" / "netvlad.py").exists():
        sys.exit(f"reference tree not found under {reference}")
    weights = nr.seeded_weights(WEIGHT_SEED, whiten=True)
    with tempfile.TemporaryDirectory() as mat_dir:
        mat = Path(mat_dir) / "VGG16-NetVLAD-Pitts30K.mat"
        nr.write_mat(mat, weights)
        parsed = nr.load_mat(mat)
        for k, v in weights.items():
            assert torch.equal(parsed[k], v), f"parse of {k} differs from the seeded tensor"
        for name, seed, b, h, w, whiten in CASES:
            images = nr.seeded_images(seed, b, h, w)
            stages: dict = {}
            with torch.no_grad():
                ours = nr.forward(parsed, images, whiten=whiten, stages=stages)
                ours_seeded = nr.forward(weights, images, whiten=whiten)
            ref = reference_forward(reference, Path(mat_dir), images, whiten)
            assert np.array_equal(ours.numpy(), ref), f"{name}: restatement differs from the reference"
            assert torch.equal(ours, ours_seeded), f"{name}: parsed and seeded weights give different bits"
            print(f"{name}: restatement == reference, bit for bit ({ours.shape})", flush=True)
            if args.check_only:
                continue
            i1, v1 = stage_sample(stages["conv1_1"], seed + 100)
            i5, v5 = stage_sample(stages["conv5_3"], seed + 200)
            np.savez_compressed(REPO / "tests" / "golden" / f"{name}.npz", seed=seed, batch=b, height=h, width=w, whiten=int(whiten),
                                weight_seed=WEIGHT_SEED, descriptors=ours.numpy(), vlad=stages["vlad"].numpy(), conv1_idx=i1, conv1_val=v1,
                                conv5_idx=i5, conv5_val=v5, conv5_shape=np.array(stages["conv5_3"].shape))


if __name__ == "__main__":
    main()
