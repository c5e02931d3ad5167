"""Host side of the D2-Net detector-descriptor (single scale): the checkpoint parse, the weight packing, the reference's image
normalisation and ``gtsfm_d2net_forward`` (``gtsfm_amd/csrc/d2net_kernels.hip``). PyTorch provides device memory and streams only;
every stage of the model runs in the library, and there is no fallback.

The checkpoint is the file the reference reads, ``d2_tf.pth`` (``torch.load(path)["model"]``, ``thirdparty/d2net/lib/model_test.py:73-77``).
It is never downloaded: a missing file raises ``FileNotFoundError``."""

from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Dict, List, Sequence, Tuple, Union

import numpy as np

from gtsfm_amd.runtime.engine_base import EngineBase

NUM_CONVS = 10
# index of each convolution in ``DenseFeatureExtractionModule.model`` (model_test.py:16-39)
CONV_LAYER_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21)
CONV_SHAPES = ((64, 3), (64, 64), (128, 64), (128, 128), (256, 128), (256, 256), (256, 256), (512, 256), (512, 512), (512, 512))
DESCRIPTOR_DIM = 512
CANDIDATE_WORDS = 6  # int32 channel, i, j; float32 step_i, step_j, score
MIN_EDGE_PX = 8  # below it the stride-1 average pool has no output


def checkpoint_keys() -> List[str]:
    return [f"dense_feature_extraction.model.{i}.{p}" for i in CONV_LAYER_INDEX for p in ("weight", "bias")]


def load_checkpoint(path: Union[str, Path]) -> Dict[str, np.ndarray]:
    """``torch.load(path, map_location="cpu")["model"]`` -> float32 arrays under the checkpoint's own keys."""
    import torch

    path = Path(path)
    if not path.exists():
        raise FileNotFoundError(f"D2-Net checkpoint not found: {path} (gtsfm_amd never downloads weights)")
    blob = torch.load(str(path), map_location="cpu")
    if not isinstance(blob, dict) or "model" not in blob:
        raise KeyError(f"{path}: a D2-Net checkpoint is a dict with a 'model' entry")
    return state_dict_arrays(blob["model"])


def state_dict_arrays(state: Dict[str, object]) -> Dict[str, np.ndarray]:
    """The twenty tensors of the dense feature extractor as contiguous float32 arrays; missing keys and wrong shapes raise."""
    missing = [k for k in checkpoint_keys() if k not in state]
    if missing:
        raise KeyError(f"D2-Net weights are missing {missing}")
    out: Dict[str, np.ndarray] = {}
    for li, (cout, cin) in zip(CONV_LAYER_INDEX, CONV_SHAPES):
        for p, shape in (("weight", (cout, cin, 3, 3)), ("bias", (cout,))):
            k = f"dense_feature_extraction.model.{li}.{p}"
            a = state[k]
            a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
            if a.shape != shape:
                raise ValueError(f"D2-Net weight {k} has shape {a.shape}, expected {shape}")
            out[k] = np.ascontiguousarray(a, dtype=np.float32)
    return out


def normalise(image: np.ndarray) -> np.ndarray:
    """(H, W, 3) array of any dtype -> (3, H, W) float32: the reference's ``preprocess_image(image, "torch")`` followed by the
    ``astype(np.float32)`` of d2net.py:78 (utils.py:23-38: float32 division by 255, float64 mean / std arithmetic)."""
    x = image.astype(np.float32)
    x = np.transpose(x, [2, 0, 1])
    x /= 255.0
    mean = np.array([0.485, 0.456, 0.406])
    std = np.array([0.229, 0.224, 0.225])
    x = (x - mean.reshape([3, 1, 1])) / std.reshape([3, 1, 1])
    return np.ascontiguousarray(x.astype(np.float32))


def preprocessing_table() -> np.ndarray:
    """(3, 256) float32: ``normalise`` of every uint8 value in every channel -- the device looks a uint8 pixel up here."""
    values = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)  # a 256 x 1 x 3 image
    return np.ascontiguousarray(normalise(values)[:, :, 0])


def map_shape(height: int, width: int) -> Tuple[int, int]:
    return height // 2 // 2 - 1, width // 2 // 2 - 1


def pack_weights(weights: Dict[str, object]) -> np.ndarray:
    """Checkpoint-keyed weights (numpy arrays or CPU tensors) -> the packed float32 blob of ``gtsfm_d2net_pack_weights``."""
    from gtsfm_amd.runtime import lib as _lib

    lib = _lib.load()
    arrays = list(state_dict_arrays(weights).values()) + [preprocessing_table()]
    ptrs = (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
    out = np.empty(lib.gtsfm_d2net_packed_weight_floats(), dtype=np.float32)
    _lib.check(lib.gtsfm_d2net_pack_weights(ptrs, out.ctypes.data), "gtsfm_d2net_pack_weights")
    return out


class D2NetEngine(EngineBase):
    """Packed weights resident on one device, a cached workspace; one instance per process / GPU."""

    WS_SLACK = "exact"

    def __init__(self, weights: Dict[str, object], device=None):
        super().__init__(device)
        self._weights = self._torch.from_numpy(pack_weights(weights)).to(self.device)
        self.relaunches = 0  # forward calls repeated because the candidate list was too small

    @classmethod
    def from_checkpoint(cls, path: Union[str, Path], device=None) -> "D2NetEngine":
        return cls(load_checkpoint(path), device)

    def _workspace(self, b: int, h: int, w: int, cap: int):
        need = int(self._lib.gtsfm_d2net_workspace_bytes(b, h, w, cap))
        if need == 0:
            if h < MIN_EDGE_PX or w < MIN_EDGE_PX:
                # the reference raises RuntimeError too (torch's pooling: "Output size is too small")
                raise RuntimeError(f"D2-Net needs images of at least {MIN_EDGE_PX} x {MIN_EDGE_PX} pixels (got a batch of {b} x {h} x {w})")
            why = self._lib.gtsfm_last_error().decode("utf-8", "replace")
            raise ValueError(f"D2-Net cannot take a batch of {b} x {h} x {w} with {cap} candidate records per image: {why}")
        return self._grow(need)

    def _prepare(self, images: Sequence[np.ndarray]):
        """Equal-sized (H, W, 3) or (H, W) arrays -> (device tensor, layout, B, H, W). uint8 goes to the device as it is; any other dtype is
        normalised on the host with the reference's numpy expression and uploaded as float32 CHW (correct, not fast)."""
        torch = self._torch
        images = [np.asarray(im) for im in images]
        if not images:
            raise ValueError("D2-Net needs at least one image")
        first = images[0]
        if any(im.shape != first.shape or im.dtype != first.dtype for im in images):
            raise ValueError("the images of a D2-Net batch must share shape and dtype")
        if not (first.ndim == 2 or (first.ndim == 3 and first.shape[2] == 3)):
            raise ValueError(f"D2-Net takes (H, W, 3) or (H, W) images (got shape {first.shape})")
        h, w = int(first.shape[0]), int(first.shape[1])
        if first.dtype == np.uint8:
            layout = 1 if first.ndim == 3 else 2
            host = np.stack([np.ascontiguousarray(im) for im in images])
        else:
            layout = 0
            host = np.stack([normalise(im if im.ndim == 3 else np.repeat(im[:, :, np.newaxis], 3, -1)) for im in images])
        return torch.from_numpy(host).to(self.device), layout, len(images), h, w

    def _detect_device(self, images: Sequence[np.ndarray], max_keypoints: int, cand_capacity: int = 0):
        """One batch of equal-sized images through ``gtsfm_d2net_forward``, repeated while the candidate list is too small. Returns
        ``(found [B] host counts, k, keypoints [B][k][2], scores [B][k], descriptors [B][k][512])``; image i's first
        ``min(found[i], k)`` rows are valid."""
        torch = self._torch
        if max_keypoints < 1:
            raise ValueError(f"max_keypoints must be positive (got {max_keypoints})")
        dev, layout, b, h, w = self._prepare(images)
        h2, w2 = map_shape(h, w)
        cap = int(cand_capacity) if cand_capacity > 0 else max(2 * h2 * w2, 1)
        k = int(max_keypoints)
        counts = torch.empty(b, dtype=torch.int32, device=self.device)
        kp = torch.empty((b, k, 2), dtype=torch.float32, device=self.device)
        sc = torch.empty((b, k), dtype=torch.float32, device=self.device)
        de = torch.empty((b, k, DESCRIPTOR_DIM), dtype=torch.float32, device=self.device)
        while True:
            ws = self._workspace(b, h, w, cap)
            rc = self._lib.gtsfm_d2net_forward(self._weights.data_ptr(), dev.data_ptr(), layout, b, h, w, k, cap, counts.data_ptr(), kp.data_ptr(),
                                               sc.data_ptr(), de.data_ptr(), ws.data_ptr(), ws.numel(), self._L.current_stream_handle())
            self._L.check(rc, "gtsfm_d2net_forward")
            found = counts.cpu().numpy()
            if int(found.max()) <= cap:
                return found, k, kp, sc, de
            cap = int(found.max())  # the list was too small for at least one image: repeat, never truncate
            self.relaunches += 1

    def detect_batch(self, images: Sequence[np.ndarray], max_keypoints: int = 5000, cand_capacity: int = 0) -> List[Tuple[np.ndarray, np.ndarray, np.ndarray]]:
        """Per image ``(keypoints (N, 2) float32 (x, y), scores (N,) float32, descriptors (N, 512) float32)``, N <= max_keypoints, by
        score descending (equal scores by channel, row, column). ``cand_capacity``: records per image of the candidate list (default
        2 x the map's pixels); when an image has more candidates the call is repeated with the reported count."""
        found, k, kp, sc, de = self._detect_device(images, max_keypoints, cand_capacity)
        out = []
        for i in range(len(found)):
            n = min(int(found[i]), k)
            out.append((kp[i, :n].cpu().numpy(), sc[i, :n].cpu().numpy(), de[i, :n].cpu().numpy()))
        return out

    def detect_table(self, images: Sequence[np.ndarray], max_keypoints: int = 5000, image_batch: int = 8) -> Dict[str, object]:
        """Images of any mix of shapes -> one device-resident feature table with ``cap = max_keypoints`` rows per image: ``xy``
        [n][cap][2], ``responses`` [n][cap], ``descriptors`` [n][cap][512] float32, ``count`` [n] int32. The images are grouped by shape
        (and dtype) and go through ``detect_batch``'s call in groups of at most ``image_batch``; image i's first ``count[i]`` rows are
        byte for byte what ``detect_batch`` returns for it. Rows beyond the count are zero."""
        torch = self._torch
        if image_batch < 1:
            raise ValueError(f"image_batch must be positive (got {image_batch})")
        images = [np.asarray(im) for im in images]
        n, cap = len(images), int(max_keypoints)
        if cap < 1:
            raise ValueError(f"max_keypoints must be positive (got {max_keypoints})")
        xy = torch.zeros((n, cap, 2), dtype=torch.float32, device=self.device)
        resp = torch.zeros((n, cap), dtype=torch.float32, device=self.device)
        desc = torch.zeros((n, cap, DESCRIPTOR_DIM), dtype=torch.float32, device=self.device)
        count = np.zeros(n, dtype=np.int32)
        groups: Dict[Tuple[object, ...], List[int]] = {}
        for i, im in enumerate(images):
            groups.setdefault((tuple(im.shape), im.dtype.str), []).append(i)
        for members in groups.values():
            for g0 in range(0, len(members), image_batch):
                ids = members[g0 : g0 + image_batch]
                found, k, kp, sc, de = self._detect_device([images[i] for i in ids], cap)
                for b, i in enumerate(ids):
                    c = min(int(found[b]), k)
                    count[i] = c
                    xy[i, :c], resp[i, :c], desc[i, :c] = kp[b, :c], sc[b, :c], de[b, :c]
        return {"xy": xy, "responses": resp, "descriptors": desc, "count": torch.from_numpy(count).to(self.device), "count_host": count}

    def detect(self, image: np.ndarray, max_keypoints: int = 5000, cand_capacity: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        return self.detect_batch([image], max_keypoints, cand_capacity)[0]

    def stage(self, images: Sequence[np.ndarray], stage: int, cand_capacity: int = 0):
        """Stage-wise outputs: 0 = relu(conv1_1) [B][H][W][64], 1 = relu(conv3_3) [B][H/4][W/4][256], 2 = the dense map [B][H2][W2][512]
        (device tensors); 3 = ``(counts, records)``: the candidates found per image (numpy int32) and the sorted candidate list as an
        int32 device tensor [B][capacity][6] (columns 3 .. 5 hold float32 bits), untruncated -- the caller compares counts and capacity."""
        torch = self._torch
        dev, layout, b, h, w = self._prepare(images)
        h2, w2 = map_shape(h, w)
        cap = int(cand_capacity) if cand_capacity > 0 else max(2 * h2 * w2, 1)
        shapes = {0: (b, h, w, 64), 1: (b, h // 2 // 2, w // 2 // 2, 256), 2: (b, h2, w2, DESCRIPTOR_DIM), 3: (b, cap, CANDIDATE_WORDS)}
        if stage not in shapes:
            raise ValueError(f"stage must be 0, 1, 2 or 3 (got {stage})")
        ws = self._workspace(b, h, w, cap)
        out = torch.zeros(shapes[stage], dtype=torch.int32 if stage == 3 else torch.float32, device=self.device)
        counts = torch.zeros(b, dtype=torch.int32, device=self.device)
        rc = self._lib.gtsfm_d2net_stage(self._weights.data_ptr(), dev.data_ptr(), layout, b, h, w, stage, cap, out.data_ptr(), counts.data_ptr(),
                                         ws.data_ptr(), ws.numel(), self._L.current_stream_handle())
        self._L.check(rc, "gtsfm_d2net_stage")
        return (counts.cpu().numpy(), out) if stage == 3 else out

    def detect_on_map(self, dense_map, max_keypoints: int = 0, cand_capacity: int = 0):
        """The detection head alone on a [B][H2][W2][512] float32 map (array or tensor). Returns ``(counts, candidates, keypoints,
        scores, descriptors)``: counts as numpy int32 (candidates FOUND, which may exceed the capacity), candidates per image as
        ``(idx (n, 3) int32, val (n, 3) float32)`` sorted, and per image the kept keypoints' arrays (``None`` when max_keypoints is 0)."""
        torch = self._torch
        m = torch.as_tensor(dense_map, dtype=torch.float32).to(self.device).contiguous()
        if m.dim() != 4 or m.shape[3] != DESCRIPTOR_DIM:
            raise ValueError(f"a dense map is [B][H2][W2][512] (got {tuple(m.shape)})")
        b, h2, w2 = int(m.shape[0]), int(m.shape[1]), int(m.shape[2])
        cap = int(cand_capacity) if cand_capacity > 0 else 2 * h2 * w2
        k = int(max_keypoints)
        ws = self._grow(int(self._lib.gtsfm_d2net_detect_workspace_bytes(b, cap)))
        counts = torch.zeros(b, dtype=torch.int32, device=self.device)
        cand = torch.zeros((b, cap, CANDIDATE_WORDS), dtype=torch.int32, device=self.device)
        kp = torch.empty((b, max(k, 1), 2), dtype=torch.float32, device=self.device)
        sc = torch.empty((b, max(k, 1)), dtype=torch.float32, device=self.device)
        de = torch.empty((b, max(k, 1), DESCRIPTOR_DIM), dtype=torch.float32, device=self.device)
        rc = self._lib.gtsfm_d2net_detect(m.data_ptr(), b, h2, w2, k, cap, counts.data_ptr(), cand.data_ptr(), kp.data_ptr(), sc.data_ptr(), de.data_ptr(),
                                          ws.data_ptr(), ws.numel(), self._L.current_stream_handle())
        self._L.check(rc, "gtsfm_d2net_detect")
        found = counts.cpu().numpy()
        cands, kps, scs, des = [], [], [], []
        for i in range(b):
            n = min(int(found[i]), cap)
            cands.append(split_candidates(cand[i, :n]))
            nk = min(n, k)
            kps.append(kp[i, :nk].cpu().numpy() if k else None)
            scs.append(sc[i, :nk].cpu().numpy() if k else None)
            des.append(de[i, :nk].cpu().numpy() if k else None)
        return found, cands, kps, scs, des


def split_candidates(records) -> Tuple[np.ndarray, np.ndarray]:
    """An int32 tensor (n, 6) of candidate records -> ``(channel / i / j (n, 3) int32, step_i / step_j / score (n, 3) float32)``."""
    a = np.ascontiguousarray(records.cpu().numpy())
    return a[:, :3].copy(), a[:, 3:].copy().view(np.float32)
