"""Host side of the two-way (mutual nearest neighbour) matcher: ``gtsfm_twoway_match`` computes every pair's product once on
the device, reduces it to a top-2 per row and per column, and applies the ratio test and the mutual check; the host orders the
kept rows by distance (``gtsfm/frontend/matcher/twoway_matcher.py:117-147``: the one-way matches are sorted by distance, stably,
and the two-way list keeps the 1->2 order). PyTorch provides device memory and streams only.

The contract checks that need no device (``check_inputs``, ``check_ratio_sizes``, ``kept_in_distance_order``) live here too, so
that the plugin can run them before it builds an engine."""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from gtsfm_amd.runtime.engine_base import EngineBase

HAMMING = 1
EUCLIDEAN = 2


def check_inputs(descriptors_i1: np.ndarray, descriptors_i2: np.ndarray, metric: int) -> bool:
    """The dtypes the reference's ``cv.BFMatcher`` accepts for ``metric``; returns whether the descriptors are uint8.
    EUCLIDEAN takes float32 or uint8, HAMMING uint8 only; anything else raises ``TypeError`` (the reference raises ``cv2.error``)."""
    if metric not in (HAMMING, EUCLIDEAN):
        raise TypeError(f"unknown distance metric {metric!r}")
    d1, d2 = np.asarray(descriptors_i1), np.asarray(descriptors_i2)
    if d1.dtype != d2.dtype:
        raise TypeError(f"descriptors of the two images differ in dtype ({d1.dtype} vs {d2.dtype})")
    allowed = (np.dtype(np.uint8),) if metric == HAMMING else (np.dtype(np.float32), np.dtype(np.uint8))
    if d1.dtype not in allowed:
        name = "HAMMING" if metric == HAMMING else "EUCLIDEAN"
        raise TypeError(f"{name} matching takes {' or '.join(str(a) for a in allowed)} descriptors, not {d1.dtype}")
    if d1.ndim != 2 or d2.ndim != 2 or d1.shape[1] != d2.shape[1]:
        raise TypeError(f"descriptors must be (N, D) arrays of the same D (got {d1.shape} and {d2.shape})")
    return d1.dtype == np.uint8


def check_ratio_sizes(n1: int, n2: int, ratio: Optional[float]) -> None:
    """With a ratio test every query needs two neighbours: the reference unpacks a 1-long ``knnMatch`` list and raises
    ``ValueError`` when either side (both are queried) has a single row."""
    if ratio is not None and n1 > 0 and n2 > 0 and min(n1, n2) < 2:
        raise ValueError(f"the ratio test needs at least two descriptors per image (got {n1} and {n2})")


def kept_in_distance_order(matches0: np.ndarray, dist0: np.ndarray) -> np.ndarray:
    """(K, 2) uint32 rows (i, matches0[i]) of the kept rows, sorted by float32 distance with ties in row order; ``np.array([])``
    when nothing is kept (the reference's empty convention)."""
    rows = np.flatnonzero(matches0 >= 0)
    if rows.size == 0:
        return np.array([])
    rows = rows[np.argsort(dist0[rows], kind="stable")]
    return np.stack([rows, matches0[rows]], axis=1).astype(np.uint32)


class TwoWayEngine(EngineBase):
    WS_SLACK = "quarter"

    def match_raw(self, table, dim: int, pairs: Sequence[Tuple[int, int, int, int]], metric: int = EUCLIDEAN, ratio: Optional[float] = None):
        """Device call. ``table``: 2-D device tensor (float32 or uint8), row r = descriptor r (first ``dim`` entries);
        ``pairs``: (first row, n1, first row, n2) per pair, n1, n2 >= 1. Returns device tensors matches0 [sum n1] int32 (partner or
        -1) and dist0 [sum n1] float32, pair p's block after the n1 of the pairs before it."""
        torch = self._torch
        if table.dim() != 2 or table.stride(1) != 1 or table.dtype not in (torch.float32, torch.uint8):
            raise TypeError("match_raw needs a 2-D float32 or uint8 device tensor with contiguous rows")
        is_u8 = int(table.dtype == torch.uint8)
        p4 = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 4))
        need = int(self._lib.gtsfm_twoway_workspace_bytes(is_u8, metric, dim, table.stride(0), len(p4), p4.ctypes.data))
        if need == 0:
            self._L.check(-1, "gtsfm_twoway_workspace_bytes")
        ws = self._grow(need)
        total = int(p4[:, 1].sum())
        matches0 = torch.empty(total, dtype=torch.int32, device=self.device)
        dist0 = torch.empty(total, dtype=torch.float32, device=self.device)
        rc = self._lib.gtsfm_twoway_match(
            table.data_ptr(), is_u8, metric, dim, table.stride(0), len(p4), p4.ctypes.data, int(ratio is not None),
            float(ratio) if ratio is not None else 0.0, ws.data_ptr(), ws.numel(), matches0.data_ptr(), dist0.data_ptr(),
            self._L.current_stream_handle(),
        )
        self._L.check(rc, "gtsfm_twoway_match")
        return matches0, dist0

    def match_pair(self, descriptors_i1: np.ndarray, descriptors_i2: np.ndarray, metric: int = EUCLIDEAN, ratio: Optional[float] = None) -> np.ndarray:
        """Host arrays (validated, NaN-free) in; (K, 2) uint32 out, or ``np.array([])``. Both images go up as one table."""
        is_u8 = check_inputs(descriptors_i1, descriptors_i2, metric)
        n1, n2 = len(descriptors_i1), len(descriptors_i2)
        if n1 == 0 or n2 == 0:
            return np.array([])
        check_ratio_sizes(n1, n2, ratio)
        host = np.ascontiguousarray(np.concatenate([descriptors_i1, descriptors_i2]), dtype=np.uint8 if is_u8 else np.float32)
        table = self._torch.from_numpy(host).to(self.device)
        matches0, dist0 = self.match_raw(table, host.shape[1], [(0, n1, n1, n2)], metric, ratio)
        return kept_in_distance_order(matches0.cpu().numpy(), dist0.cpu().numpy())

    def match_table(self, desc_table, counts: Sequence[int], pairs: Sequence[Tuple[int, int]], metric: int = EUCLIDEAN,
                    ratio: Optional[float] = None, pair_batch: int = 32) -> Dict[Tuple[int, int], np.ndarray]:
        """Device-resident form for a batched generator: ``desc_table`` [images][capacity][D] (device), ``counts`` valid rows per
        image (host), ``pairs`` (i1, i2) edges. The edges go in launches of at most ``pair_batch`` pairs, so the workspace stays
        bounded by the batch, not the graph (results do not depend on the batching); per edge exactly what ``match_pair`` returns
        for the two images' first ``count`` rows."""
        if pair_batch < 1:
            raise ValueError(f"pair_batch must be positive (got {pair_batch})")
        n_img, cap, dim = desc_table.shape
        table = desc_table.reshape(n_img * cap, dim)
        out: Dict[Tuple[int, int], np.ndarray] = {}
        todo: List[Tuple[int, int]] = []
        for i1, i2 in pairs:
            n1, n2 = int(counts[i1]), int(counts[i2])
            if n1 == 0 or n2 == 0:
                out[(i1, i2)] = np.array([])
            else:
                check_ratio_sizes(n1, n2, ratio)
                todo.append((i1, i2))
        for c0 in range(0, len(todo), pair_batch):
            chunk = todo[c0 : c0 + pair_batch]
            spec = [(i1 * cap, int(counts[i1]), i2 * cap, int(counts[i2])) for i1, i2 in chunk]
            matches0, dist0 = self.match_raw(table, dim, spec, metric, ratio)
            m_h, d_h = matches0.cpu().numpy(), dist0.cpu().numpy()
            start = 0
            for (i1, i2), (_, n1, _, _) in zip(chunk, spec):
                out[(i1, i2)] = kept_in_distance_order(m_h[start : start + n1], d_h[start : start + n1])
                start += n1
        return {(int(i1), int(i2)): out[(i1, i2)] for i1, i2 in pairs}

    def order_matches(self, matches0, dist0, blk_off, num_pairs: int, match_idx, match_count) -> None:
        """``gtsfm_twoway_order_matches`` on device tensors: ``blk_off`` int64 [num_pairs + 1] row offsets into ``matches0`` / ``dist0``
        and ``match_idx`` [rows][2] int32; ``match_count`` int32 [num_pairs]. Enqueued on the current stream."""
        torch = self._torch
        if (matches0.dtype != torch.int32 or dist0.dtype != torch.float32 or blk_off.dtype != torch.int64 or match_idx.dtype != torch.int32
                or match_count.dtype != torch.int32 or blk_off.numel() < num_pairs + 1 or match_count.numel() < num_pairs
                or not (matches0.is_contiguous() and dist0.is_contiguous() and blk_off.is_contiguous() and match_idx.is_contiguous() and match_count.is_contiguous())):
            raise TypeError("order_matches needs contiguous int32 matches0 / match_idx / match_count, float32 dist0 and int64 offsets")
        rc = self._lib.gtsfm_twoway_order_matches(matches0.data_ptr(), dist0.data_ptr(), blk_off.data_ptr(), int(num_pairs), match_idx.data_ptr(),
                                                  match_count.data_ptr(), self._L.current_stream_handle())
        self._L.check(rc, "gtsfm_twoway_order_matches")

    def match_table_device(self, desc_table, counts: Sequence[int], pairs: Sequence[Tuple[int, int]], metric: int = EUCLIDEAN,
                           ratio: Optional[float] = None, pair_batch: int = 32) -> Dict[str, object]:
        """``match_table`` with the match lists left on the device, in the contract's order: the edges with two non-empty sides go through
        ``match_raw`` in launches of at most ``pair_batch`` pairs, and ``gtsfm_twoway_order_matches`` writes each launch's kept rows, by
        distance (ties by row), into one scene-wide ``match_idx`` [sum n1][2] int32 in capacity layout (edge p owns rows
        ``match_off[p] .. match_off[p + 1]``, the first ``match_count[p]`` of them are matches) -- what ``VerifierEngine.verify_batch``
        reads. Returns ``pairs`` (the edges matched, in order), ``empty`` (edges with an empty side), ``match_idx``, ``match_off`` (host
        list), ``match_count`` (device). Nothing is copied to the host."""
        torch = self._torch
        if pair_batch < 1:
            raise ValueError(f"pair_batch must be positive (got {pair_batch})")
        n_img, cap, dim = desc_table.shape
        table = desc_table.reshape(n_img * cap, dim)
        todo: List[Tuple[int, int]] = []
        empty: List[Tuple[int, int]] = []
        for i1, i2 in pairs:
            n1, n2 = int(counts[i1]), int(counts[i2])
            if n1 == 0 or n2 == 0:
                empty.append((int(i1), int(i2)))
            else:
                check_ratio_sizes(n1, n2, ratio)
                todo.append((int(i1), int(i2)))
        n1s = np.array([int(counts[i1]) for i1, _ in todo], dtype=np.int64)
        match_off = np.concatenate([[0], np.cumsum(n1s)]).astype(np.int64)
        match_idx = torch.empty((int(match_off[-1]), 2), dtype=torch.int32, device=self.device)
        match_count = torch.zeros(len(todo), dtype=torch.int32, device=self.device)
        # every launch's block offsets (relative to the launch's first row) in one upload: chunk c reads blk[c0 + c : c0 + c + len + 1]
        chunks = [(c0, min(c0 + pair_batch, len(todo))) for c0 in range(0, len(todo), pair_batch)]
        blk_host = np.concatenate([match_off[a : b + 1] - match_off[a] for a, b in chunks]) if chunks else np.zeros(0, dtype=np.int64)
        blk = torch.from_numpy(np.ascontiguousarray(blk_host, dtype=np.int64)).to(self.device)
        for c, (a, b) in enumerate(chunks):
            spec = [(i1 * cap, int(counts[i1]), i2 * cap, int(counts[i2])) for i1, i2 in todo[a:b]]
            matches0, dist0 = self.match_raw(table, dim, spec, metric, ratio)
            self.order_matches(matches0, dist0, blk[a + c : b + c + 1], b - a, match_idx[int(match_off[a]) :], match_count[a:b])
        return {"pairs": todo, "empty": empty, "match_idx": match_idx, "match_off": match_off.tolist(), "match_count": match_count}

    def matches_to_numpy(self, matched: Dict[str, object]) -> Dict[Tuple[int, int], np.ndarray]:
        """``match_table_device``'s result -> per edge what ``match_pair`` returns: (K, 2) uint32, or ``np.array([])`` when nothing is
        kept or a side is empty. Only the first ``match_count`` rows of each edge are copied to the host."""
        torch = self._torch
        out: Dict[Tuple[int, int], np.ndarray] = {p: np.array([]) for p in matched["empty"]}
        pairs = matched["pairs"]
        if pairs:
            off = torch.tensor(matched["match_off"], dtype=torch.int64, device=self.device)
            owner = torch.repeat_interleave(torch.arange(len(pairs), device=self.device), off[1:] - off[:-1])
            within = torch.arange(int(matched["match_off"][-1]), device=self.device) - off[owner]
            kept = matched["match_idx"][within < matched["match_count"].to(torch.int64)[owner]].cpu().numpy()
            count = matched["match_count"].cpu().numpy()
            start = 0
            for p, k in zip(pairs, count):
                out[p] = kept[start : start + int(k)].astype(np.uint32) if k else np.array([])
                start += int(k)
        return out
