"""``GlobalDescriptorBase``: the reference's class when GTSfM is importable, else a stand-in with the same contract
(``gtsfm/frontend/global_descriptor/global_descriptor_base.py:15-46``)."""

from __future__ import annotations

import abc

try:  # pragma: no cover
    from gtsfm.frontend.global_descriptor.global_descriptor_base import GlobalDescriptorBase  # type: ignore  # noqa: F401
except Exception:  # noqa: BLE001

    class GlobalDescriptorBase:  # type: ignore[no-redef]
        """Assigns one vector to each input image."""

        @abc.abstractmethod
        def describe_batch(self, images):
            """(B, C, H, W) batch -> list of B (D,) numpy arrays."""

        @abc.abstractmethod
        def get_preprocessing_transforms(self):
            """(resize transform, optional batch transform)."""
