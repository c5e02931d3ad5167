"""``RetrieverBase``: the reference's class when GTSfM is importable, else a stand-in with the same contract
(``gtsfm/retriever/retriever_base.py:17-88``)."""

from __future__ import annotations

import abc

from gtsfm_amd.frontend.registry import GTSFMProcess, UiMetadata

try:  # pragma: no cover
    from gtsfm.retriever.retriever_base import RetrieverBase  # type: ignore  # noqa: F401
except Exception:  # noqa: BLE001

    class RetrieverBase(GTSFMProcess):  # type: ignore[no-redef]
        """Base class for image retriever implementations."""

        @staticmethod
        def get_ui_metadata() -> UiMetadata:
            return UiMetadata(
                display_name="Image Retriever",
                input_products=("Image Loader",),
                output_products=("Visibility Graph",),
                parent_plate="Loader and Retriever",
            )

        def set_max_frame_lookahead(self, n) -> None:
            raise AttributeError(f"{type(self).__name__} has no max_frame_lookahead")

        def set_num_matched(self, n) -> None:
            raise AttributeError(f"{type(self).__name__} has no num_matched")

        @abc.abstractmethod
        def get_image_pairs(self, global_descriptors, image_fnames, plots_output_dir=None):
            """List of (i1, i2) image pairs."""

        def save_diagnostics(self, image_fnames, pairs, plots_output_dir) -> None:
            del image_fnames, pairs, plots_output_dir

        def evaluate(self, num_images, visibility_graph):
            """The reference's ``retriever_metrics`` group as a plain dict (GtsfmMetricsGroup needs GTSfM)."""
            return {"retriever_metrics": {"num_input_images": num_images, "num_retrieved_image_pairs": len(visibility_graph)}}
