"""Disk cache around a global-descriptor plugin, in the reference's format and key scheme (mirror of
``gtsfm/frontend/cacher/global_descriptor_cacher.py:29-112``): key ``<type(obj).__name__>_<sha1 of the batch's bytes>``
(``gtsfm/utils/cache.py``'s ``generate_hash_for_image_batch``: ``images.cpu().numpy().tobytes()``), file
``<root>/global_descriptor/<key>.pbz2`` holding ``{"global_descriptors": list}``."""

from __future__ import annotations

import hashlib
from pathlib import Path
from typing import Optional

from gtsfm_amd.frontend.cacher import cache_format
from gtsfm_amd.frontend.global_descriptor.global_descriptor_base import GlobalDescriptorBase

CACHE_ROOT_PATH = Path(__file__).resolve().parent.parent.parent.parent / "cache"


def generate_hash_for_image_batch(images) -> str:
    return hashlib.sha1(images.cpu().numpy().tobytes()).hexdigest()


def global_descriptor_cache_key(global_descriptor_obj, images) -> str:
    return "{}_{}".format(type(global_descriptor_obj).__name__, generate_hash_for_image_batch(images))


class GlobalDescriptorCacher(GlobalDescriptorBase):
    """Cacher for global-descriptor output on disk, keyed on the input batch."""

    def __init__(self, global_descriptor_obj: GlobalDescriptorBase, cache_root: Optional[Path] = None) -> None:
        self._global_descriptor = global_descriptor_obj
        self._cache_root = Path(cache_root) if cache_root is not None else CACHE_ROOT_PATH

    def _cache_path(self, images) -> Path:
        return self._cache_root / "global_descriptor" / "{}.pbz2".format(global_descriptor_cache_key(self._global_descriptor, images))

    def get_preprocessing_transforms(self):
        if self._global_descriptor is not None:
            return self._global_descriptor.get_preprocessing_transforms()
        import torch

        return (lambda x: torch.from_numpy(x)), None

    def describe_batch(self, images) -> list:
        path = self._cache_path(images)
        cached = cache_format.read_from_bz2_file(path)
        if cached is not None:
            return cached["global_descriptors"]
        global_descriptors = self._global_descriptor.describe_batch(images)
        cache_format.write_to_bz2_file({"global_descriptors": global_descriptors}, path)
        return global_descriptors
