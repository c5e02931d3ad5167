"""Global-descriptor cache entries interchanged with the REFERENCE'S OWN cacher code, in both directions.

``gtsfm/frontend/cacher/global_descriptor_cacher.py`` cannot normally be imported here: through ``gtsfm.utils.io`` and
``gtsfm.loader.loader_base`` it pulls gtsam, h5py, open3d, dask, torchvision and more. Its caching logic needs none of them, so this
script imports the reference's modules with the ABSENT THIRD-PARTY PACKAGES replaced by inert ``unittest.mock`` modules (nothing of
GTSfM itself is replaced) and lets the reference's code run:

1. the REFERENCE cacher wraps a stand-in plugin named ``NetVLADGlobalDescriptor`` (the class name is the cache namespace) and writes
   the entry of ``cache_sample(1)`` with its own key scheme and ``write_to_bz2_file``;
2. a SECOND PROCESS without the reference on its path reads it through ``gtsfm_amd.frontend.cacher.global_descriptor_cacher``: the
   lookup must HIT (the wrapped plugin raises if it is called) and return the same arrays; it then writes the entry of ``cache_sample(2)``;
3. the REFERENCE cacher reads that entry: HIT (plugin raises if called), same arrays.

``--write`` stores the reference-written file of step 1 under ``tests/golden/reference_global_descriptor_cache/`` so that
``tests/test_global_descriptor_cache.py`` repeats step 2 wherever the tests run.
Usage: python tools/record_global_descriptor_cache.py [--write]   (reference tree: $GTSFM_REFERENCE or /root/reference)
"""

from __future__ import annotations

import argparse
import importlib.abc
import importlib.machinery
import os
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path
from unittest import mock

import numpy as np

REPO = Path(__file__).resolve().parent.parent
REFERENCE = Path(os.environ.get("GTSFM_REFERENCE", "/root/reference"))
GOLDEN = REPO / "tests" / "golden" / "reference_global_descriptor_cache"


class _AbsentPackages(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """Inert modules for third-party packages that are not installed here and that the caching code never touches."""

    ROOTS = {"gtsam", "cv2", "h5py", "open3d", "simplejson", "dask", "distributed", "pycolmap", "trimesh", "hydra", "omegaconf", "pydot",
             "plotly", "networkx", "seaborn", "kornia", "pydegensac", "colour", "torchvision", "graphviz", "rawpy", "imageio", "shapely",
             "pyvista", "PIL"}

    def find_spec(self, name, path, target=None):
        if name.split(".")[0] in self.ROOTS:
            try:
                if importlib.machinery.PathFinder.find_spec(name.split(".")[0]) is not None:
                    return None  # really installed: use it
            except (ImportError, ValueError):
                pass
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        m = mock.MagicMock(name=spec.name)
        m.__name__, m.__path__, m.__spec__, m.__loader__ = spec.name, [], spec, self
        return m

    def exec_module(self, module):
        pass


OURS_SCRIPT = r'''
import sys, numpy as np
sys.path.insert(0, {repo!r})
assert not any("reference" in p for p in sys.path)
from gtsfm_amd.frontend.cacher.global_descriptor_cacher import GlobalDescriptorCacher
from tests.netvlad_reference import cache_sample
root = {root!r}
class NetVLADGlobalDescriptor:
    def __init__(self, data=None): self.data = data
    def describe_batch(self, images):
        if self.data is None: raise AssertionError("cache miss on an entry the reference wrote")
        return self.data
    def get_preprocessing_transforms(self): return None, None
images, desc = cache_sample(1)
got = GlobalDescriptorCacher(NetVLADGlobalDescriptor(), cache_root=root).describe_batch(images)
assert isinstance(got, list) and len(got) == 2 and all(g.dtype == np.float32 and np.array_equal(g, d) for g, d in zip(got, desc))
images, desc = cache_sample(2)
GlobalDescriptorCacher(NetVLADGlobalDescriptor(desc), cache_root=root).describe_batch(images)
print("OURS_OK")
'''


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="store the reference-written entry under tests/golden/reference_global_descriptor_cache/")
    args = ap.parse_args()
    if not (REFERENCE / "gtsfm" / "frontend" / "cacher" / "global_descriptor_cacher.py").exists():
        raise SystemExit(f"reference cacher not found under {REFERENCE}")
    sys.path.insert(0, str(REPO))
    from tests.netvlad_reference import cache_sample

    sys.meta_path.insert(0, _AbsentPackages())
    sys.path.insert(0, str(REFERENCE))
    import gtsfm.frontend.cacher.global_descriptor_cacher as ref_gdc
    from gtsfm.frontend.global_descriptor.global_descriptor_base import GlobalDescriptorBase as RefGDBase

    class NetVLADGlobalDescriptor(RefGDBase):  # the class NAME is the reference's cache namespace (global_descriptor_cacher.py:40)
        def __init__(self, data=None):
            self.data = data

        def describe_batch(self, images):
            if self.data is None:
                raise AssertionError("cache miss on an entry gtsfm_amd wrote")
            return self.data

        def get_preprocessing_transforms(self):
            return None, None

    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp) / "cache"
        ref_gdc.CACHE_ROOT_PATH = root  # the reference derives it from its own location (read-only here)
        # (1) the reference's code writes
        images, desc = cache_sample(1)
        ref_gdc.GlobalDescriptorCacher(NetVLADGlobalDescriptor(desc)).describe_batch(images)
        written = sorted(p.relative_to(root) for p in root.rglob("*.pbz2"))
        assert len(written) == 1 and written[0].parent == Path("global_descriptor"), written
        print("reference wrote:", [str(p) for p in written])
        if args.write:
            if GOLDEN.exists():
                shutil.rmtree(GOLDEN)
            (GOLDEN / written[0].parent).mkdir(parents=True)
            shutil.copy(root / written[0], GOLDEN / written[0])
        # (2) our cacher, in a process that cannot see the reference, reads it and writes its own
        env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
        out = subprocess.run([sys.executable, "-c", OURS_SCRIPT.format(repo=str(REPO), root=str(root))], capture_output=True, text=True, env=env,
                             cwd=str(REPO))
        assert out.returncode == 0 and "OURS_OK" in out.stdout, out.stderr[-3000:]
        print("gtsfm_amd (no reference on its path) read the entry as a hit and wrote one of its own")
        # (3) the reference's code reads ours
        images, desc = cache_sample(2)
        got = ref_gdc.GlobalDescriptorCacher(NetVLADGlobalDescriptor()).describe_batch(images)
        assert len(got) == 2 and all(np.array_equal(g, d) for g, d in zip(got, desc))
        print("the reference's cacher read gtsfm_amd's entry as a hit, same arrays")
    print("OK")


if __name__ == "__main__":
    main()
