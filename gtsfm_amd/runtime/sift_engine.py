"""Host side of the SIFT detector-descriptor: image checks, the gray conversion (``gtsfm_prep_rgb_to_gray_u8``) and
``gtsfm_sift_detect_and_describe`` / ``gtsfm_sift_stage`` (``gtsfm_amd/csrc/sift_kernels.hip``). PyTorch provides device memory and
streams only; every stage runs in the library, and there is no fallback.

The algorithm is OpenCV's ``SIFT_create()`` with its defaults, which is all the reference's ``SIFTDetectorDescriptor`` uses
(``gtsfm/frontend/detector_descriptor/sift.py:44-54``); ``tests/sift_reference.py`` restates it in numpy, operation for operation."""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from gtsfm_amd.runtime.engine_base import EngineBase

DESCRIPTOR_DIM = 128
CANDIDATE_WORDS = 4  # int32 octave, layer, row, column
KEYPOINT_WORDS = 8  # the four above, then float32 x, y (octave coordinates), scl, response
ORIENTED_WORDS = 10  # a keypoint, then float32 angle and a zero word
ERR_WORKSPACE = -3  # GTSFM_ERR_WORKSPACE: a list was too small


def check_image(array: np.ndarray) -> None:
    """(H, W), (H, W, 3) and (H, W, 4) pass; anything else raises as the reference's ``rgb_to_gray_cv`` does."""
    if not (array.ndim == 2 or (array.ndim == 3 and array.shape[2] in (3, 4))):
        raise ValueError("Input image dimensions are wrong")
    if array.dtype != np.uint8:
        raise TypeError(f"SIFT takes uint8 images (got {array.dtype})")


def default_capacities(height: int, width: int) -> Tuple[int, int]:
    """Candidate and keypoint records per image: 1/8 and 1/32 of the doubled image's pixels (a 1296 x 1936 photograph has 0.5 % and
    0.25 %); an image that needs more is run again with what it needs."""
    px = 4 * height * width
    return max(px // 8, 4096), max(px // 32, 2048)


def split_keypoints(records: np.ndarray) -> Dict[str, np.ndarray]:
    """(n, 8) or (n, 10) int32 records -> the fields of ``tests/sift_reference.py``'s keypoint dictionaries."""
    a = np.ascontiguousarray(records)
    f = a.view(np.float32)
    out = {"octave": a[:, 0].copy(), "layer": a[:, 1].copy(), "row": a[:, 2].copy(), "column": a[:, 3].copy(), "x": f[:, 4].copy(), "y": f[:, 5].copy(),
           "scl": f[:, 6].copy(), "response": f[:, 7].copy()}
    if a.shape[1] == ORIENTED_WORDS:
        out["angle"] = f[:, 8].copy()
    return out


class SiftEngine(EngineBase):
    """A cached workspace on one device; one instance per process / GPU."""

    WS_SLACK = "exact"

    def __init__(self, device=None):
        super().__init__(device)
        self.relaunches = 0  # calls repeated because a candidate or keypoint list was too small

    def _workspace(self, b: int, h: int, w: int, cand: int, kp: int):
        need = int(self._lib.gtsfm_sift_workspace_bytes(b, h, w, cand, kp))
        if need == 0:
            why = self._lib.gtsfm_last_error().decode("utf-8", "replace")
            raise ValueError(f"SIFT cannot take a batch of {b} x {h} x {w} with capacities {cand} / {kp}: {why}")
        return self._grow(need)

    def _gray(self, images: Sequence[np.ndarray]):
        """Equal-sized uint8 images -> [B][H][W] uint8 on the device; colour goes through ``gtsfm_prep_rgb_to_gray_u8``."""
        torch = self._torch
        images = [np.asarray(im) for im in images]
        if not images:
            raise ValueError("SIFT needs at least one image")
        for im in images:
            check_image(im)
        first = images[0]
        if any(im.shape != first.shape for im in images):
            raise ValueError("the images of a SIFT batch must share their shape")
        dev = torch.from_numpy(np.stack([np.ascontiguousarray(im) for im in images])).to(self.device)
        if first.ndim == 2:
            return dev
        b, h, w, c = dev.shape
        gray = torch.empty((b, h, w), dtype=torch.uint8, device=self.device)
        rc = self._lib.gtsfm_prep_rgb_to_gray_u8(dev.data_ptr(), b * h, w, c, gray.data_ptr(), self._L.current_stream_handle())
        self._L.check(rc, "gtsfm_prep_rgb_to_gray_u8")
        return gray

    def _masks(self, masks, b: int, h: int, w: int):
        if masks is None or all(m is None for m in masks):
            return None
        rows = []
        for m in masks:
            m = np.ones((h, w), dtype=np.uint8) if m is None else (np.asarray(m) != 0).astype(np.uint8)
            if m.shape != (h, w):
                raise ValueError(f"a mask has the image's height and width (got {m.shape} for {h} x {w})")
            rows.append(m)
        if len(rows) != b:
            raise ValueError("one mask (or None) per image")
        return self._torch.from_numpy(np.stack(rows)).to(self.device)

    def _detect_device(self, images, max_keypoints: int, masks, cand_capacity: int = 0, kp_capacity: int = 0):
        """One batch of equal-sized images through ``gtsfm_sift_detect_and_describe``, repeated while a list is too small. Returns
        ``(found [B][4] host counts, k, out_kp [B][k][4], out_de [B][k][128])``; image i's first ``min(found[i, 2], k)`` rows are valid."""
        torch = self._torch
        if max_keypoints < 1:
            raise ValueError(f"max_keypoints must be positive (got {max_keypoints})")
        gray = self._gray(images)
        b, h, w = (int(s) for s in gray.shape)
        mask = self._masks(masks, b, h, w)
        cand, kp = default_capacities(h, w)
        cand, kp = (int(cand_capacity) or cand), (int(kp_capacity) or kp)
        counts = torch.zeros((b, 4), dtype=torch.int32, device=self.device)
        while True:
            k = min(int(max_keypoints), kp)
            ws = self._workspace(b, h, w, cand, kp)
            out_kp = torch.empty((b, k, 4), dtype=torch.float32, device=self.device)
            out_de = torch.empty((b, k, DESCRIPTOR_DIM), dtype=torch.float32, device=self.device)
            rc = self._lib.gtsfm_sift_detect_and_describe(gray.data_ptr(), self._L.ptr(mask), b, h, w, k, cand, kp, counts.data_ptr(), out_kp.data_ptr(),
                                                          out_de.data_ptr(), ws.data_ptr(), ws.numel(), self._L.current_stream_handle())
            found = counts.cpu().numpy()
            if rc == ERR_WORKSPACE:  # a list was too small for at least one image: repeat, never truncate
                cand, kp = max(cand, int(found[:, 0].max())), max(kp, int(found[:, 1:3].max()))
                self.relaunches += 1
                continue
            self._L.check(rc, "gtsfm_sift_detect_and_describe")
            return found, k, out_kp, out_de

    def detect_batch(self, images: Sequence[np.ndarray], max_keypoints: int = 5000, masks: Optional[Sequence[Optional[np.ndarray]]] = None,
                     cand_capacity: int = 0, kp_capacity: int = 0) -> List[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]]:
        """Per image ``(coordinates (N, 2) (x, y), sizes (N,), responses (N,), descriptors (N, 128))``, float32, N <= max_keypoints, by
        response descending (equal responses by octave, layer, row, column, angle). A keypoint whose mask pixel is 0 is dropped before
        the top-k. When an image has more candidates or keypoints than the lists hold, the call is repeated with what it reported."""
        found, k, out_kp, out_de = self._detect_device(images, max_keypoints, masks, cand_capacity, kp_capacity)
        out = []
        for i in range(len(found)):
            n = min(int(found[i, 2]), k)
            rows = out_kp[i, :n].cpu().numpy()
            out.append((rows[:, :2].copy(), rows[:, 2].copy(), rows[:, 3].copy(), out_de[i, :n].cpu().numpy()))
        return out

    def detect_table(self, images: Sequence[np.ndarray], max_keypoints: int = 5000, masks: Optional[Sequence[Optional[np.ndarray]]] = None,
                     image_batch: int = 8) -> Dict[str, object]:
        """Images of any mix of shapes -> one device-resident feature table with ``cap = max_keypoints`` rows per image: ``xy``
        [n][cap][2], ``sizes`` [n][cap], ``responses`` [n][cap] float32, ``descriptors`` [n][cap][128] uint8, ``count`` [n] int32. The
        images are grouped by shape and go through ``detect_batch``'s call in groups of at most ``image_batch``; image i's first
        ``count[i]`` rows are what ``detect_batch`` returns for it (the descriptors after the cast: a value that is not an integer in
        0 .. 255 raises ``RuntimeError``, nothing is clamped). Rows beyond the count are zero."""
        torch = self._torch
        if image_batch < 1:
            raise ValueError(f"image_batch must be positive (got {image_batch})")
        images = [np.asarray(im) for im in images]
        masks = [None] * len(images) if masks is None else list(masks)
        if len(masks) != len(images):
            raise ValueError("one mask (or None) per image")
        n, cap = len(images), int(max_keypoints)
        if cap < 1:
            raise ValueError(f"max_keypoints must be positive (got {max_keypoints})")
        rows = torch.zeros((n, cap, 4), dtype=torch.float32, device=self.device)
        desc = torch.zeros((n, cap, DESCRIPTOR_DIM), dtype=torch.uint8, device=self.device)
        count = np.zeros(n, dtype=np.int32)
        flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        groups: Dict[Tuple[int, ...], List[int]] = {}
        for i, im in enumerate(images):
            groups.setdefault(tuple(im.shape), []).append(i)
        for members in groups.values():
            for g0 in range(0, len(members), image_batch):
                ids = members[g0 : g0 + image_batch]
                found, k, out_kp, out_de = self._detect_device([images[i] for i in ids], cap, [masks[i] for i in ids])
                for b, i in enumerate(ids):
                    c = min(int(found[b, 2]), k)
                    count[i] = c
                    if c == 0:
                        continue
                    rows[i, :c] = out_kp[b, :c]
                    rc = self._lib.gtsfm_pack_rows_f32_to_u8(out_de[b].data_ptr(), c, DESCRIPTOR_DIM, DESCRIPTOR_DIM, desc[i].data_ptr(), DESCRIPTOR_DIM,
                                                             flag.data_ptr(), self._L.current_stream_handle())
                    self._L.check(rc, "gtsfm_pack_rows_f32_to_u8")
        if n and int(flag.cpu()[0]) != 0:
            raise RuntimeError("a SIFT descriptor value is not an integer in 0 .. 255: the uint8 table cannot hold it")
        return {"xy": rows[:, :, :2].contiguous(), "sizes": rows[:, :, 2].contiguous(), "responses": rows[:, :, 3].contiguous(), "descriptors": desc,
                "count": torch.from_numpy(count).to(self.device), "count_host": count}

    def detect(self, image: np.ndarray, max_keypoints: int = 5000, mask: Optional[np.ndarray] = None, cand_capacity: int = 0,
               kp_capacity: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        return self.detect_batch([image], max_keypoints, [mask], cand_capacity, kp_capacity)[0]

    def stage(self, image: np.ndarray, stage: int, mask: Optional[np.ndarray] = None, cand_capacity: int = 0, kp_capacity: int = 0, sync: bool = True):
        """Stage-wise outputs of one image. 0: the pyramid, a float32 device tensor in the layout of include/gtsfm_amd.h; 1: candidates
        (n, 4) int32 numpy, in any order; 2: keypoints, 3: oriented keypoints in the output order -- both as the field dictionaries of
        ``split_keypoints``. A list that was too small raises. ``sync=False`` returns nothing (timing)."""
        torch = self._torch
        if stage not in (0, 1, 2, 3):
            raise ValueError(f"stage must be 0, 1, 2 or 3 (got {stage})")
        gray = self._gray([image])
        _, h, w = (int(s) for s in gray.shape)
        m = self._masks([mask], 1, h, w)
        cand, kp = default_capacities(h, w)
        cand, kp = (int(cand_capacity) or cand), (int(kp_capacity) or kp)
        ws = self._workspace(1, h, w, cand, kp)
        words = {0: max(int(self._lib.gtsfm_sift_pyramid_floats(h, w)), 1), 1: cand * CANDIDATE_WORDS, 2: kp * KEYPOINT_WORDS, 3: kp * ORIENTED_WORDS}[stage]
        out = torch.empty(words, dtype=torch.float32 if stage == 0 else torch.int32, device=self.device)  # read up to the counts only
        counts = torch.zeros(4, dtype=torch.int32, device=self.device)
        rc = self._lib.gtsfm_sift_stage(gray.data_ptr(), self._L.ptr(m), h, w, stage, cand, kp, out.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                        self._L.current_stream_handle())
        self._L.check(rc, "gtsfm_sift_stage")
        if not sync:
            return None
        if stage == 0:
            return out[: int(self._lib.gtsfm_sift_pyramid_floats(h, w))]
        found = counts.cpu().numpy()
        if found[0] > cand or found[1] > kp or found[2] > kp:
            raise RuntimeError(f"SIFT found {found[0]} candidates / {found[1]} keypoints / {found[2]} oriented keypoints, above the capacities {cand} / {kp}")
        if stage == 1:
            return out.view(cand, CANDIDATE_WORDS)[: int(found[0])].cpu().numpy()
        n, per = (int(found[1]), KEYPOINT_WORDS) if stage == 2 else (int(found[2]), ORIENTED_WORDS)
        return split_keypoints(out.view(kp, per)[:n].cpu().numpy())
