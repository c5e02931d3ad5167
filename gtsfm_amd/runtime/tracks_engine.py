"""Host side of the device track builder: ``gtsfm_tracks_from_matches`` merges match rows that lie in HBM into feature tracks (a
union-find over keypoints), replacing ``gtsfm/data_association/dsf_tracks_estimator.py:51-85`` / ``cpp_dsf_tracks_estimator.py:63-84``.
PyTorch provides device memory, concatenation and copies only."""

from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from gtsfm_amd.runtime.engine_base import EngineBase, named

COUNT_FIELDS = ("tracks", "measurements", "discarded", "components", "rounds")


def edge_selection(pairs: Sequence[Tuple[int, int]], edges: Iterable[Tuple[int, int]]) -> np.ndarray:
    """[len(pairs)] uint8: 1 for a pair that ``edges`` lists. The one place a scene's stages look their ``edges=`` argument up."""
    wanted = {(int(a), int(b)) for a, b in edges}
    return np.fromiter((p in wanted for p in pairs), dtype=np.uint8, count=len(pairs))


class TracksEngine(EngineBase):
    def _workspace(self, num_nodes: int, total: int):
        if num_nodes == 0:  # a scene without nodes is no refusal
            return self._grow(int(self._lib.gtsfm_tracks_workspace_bytes(0, total)))
        return self._sized_workspace("gtsfm_tracks_workspace_bytes", num_nodes, total)

    def tracks_from_device(self, match_idx, match_off, pair_images, node_off, match_count=None, mask=None, pair_enable=None, kp_xy=None,
                           num_nodes: Optional[int] = None) -> Dict[str, object]:
        """``match_idx`` [M, 2] int32 (device), ``match_off`` [P + 1] and ``node_off`` [num_images + 1] (host sequences or device int64),
        ``pair_images`` [P, 2]; ``match_count`` [P] int32, ``mask`` [M] uint8, ``pair_enable`` [P] uint8 and ``kp_xy`` [num_nodes, 2]
        float32 are optional device tensors (see include/gtsfm_amd.h). ``num_nodes``: node_off's last entry when the caller knows it,
        otherwise it is read back. Returns device tensors sized to the result: track_off [T + 1] int64, image / kp [S] int32, uv [S, 2]
        float32 (with ``kp_xy``), and ``counts`` as a dict of ints (``COUNT_FIELDS``)."""
        torch = self._torch
        moff = self._dev(match_off, torch.int64)
        noff = self._dev(node_off, torch.int64)
        pimg = self._dev(pair_images, torch.int32).reshape(-1, 2)
        num_pairs, num_images = int(pimg.shape[0]), int(noff.numel()) - 1
        if moff.numel() != num_pairs + 1 or num_images < 0:
            raise ValueError(f"match_off has {moff.numel()} entries for {num_pairs} pairs; node_off has {noff.numel()}")
        total = int(match_idx.numel()) // 2
        if num_nodes is None:
            num_nodes = int(noff[-1].item()) if num_images >= 0 and noff.numel() else 0
        self._check_tensors((("match_idx", match_idx, torch.int32, 2 * total), ("match_count", match_count, torch.int32, num_pairs), ("mask", mask, torch.uint8, total),
                             ("pair_enable", pair_enable, torch.uint8, num_pairs), ("kp_xy", kp_xy, torch.float32, 2 * num_nodes)),
                            optional=("match_idx", "match_count", "mask", "pair_enable", "kp_xy"))
        cap = min(num_nodes, 2 * total)
        track_off = torch.empty(cap + 1, dtype=torch.int64, device=self.device)
        image = torch.empty(cap, dtype=torch.int32, device=self.device)
        kp = torch.empty(cap, dtype=torch.int32, device=self.device)
        uv = torch.empty((cap, 2), dtype=torch.float32, device=self.device) if kp_xy is not None else None
        counts = torch.empty(8, dtype=torch.int32, device=self.device)
        ws = self._workspace(num_nodes, total) if num_pairs and total else None
        ptr = self._ptr
        rc = self._lib.gtsfm_tracks_from_matches(
            ptr(match_idx), moff.data_ptr(), ptr(match_count), ptr(mask), ptr(pair_enable), ptr(pimg), num_pairs, total, noff.data_ptr(), num_images, ptr(kp_xy), ptr(ws),
            0 if ws is None else ws.numel(), track_off.data_ptr(), ptr(image), ptr(kp), ptr(uv), counts.data_ptr(), self._stream())
        self._L.check(rc, "gtsfm_tracks_from_matches")
        c = counts.cpu().numpy()
        t, s = int(c[0]), int(c[1])
        out = {"track_off": track_off[: t + 1], "image": image[:s], "kp": kp[:s], "counts": named(c, COUNT_FIELDS)}
        if uv is not None:
            out["uv"] = uv[:s]
        return out

    def tracks_from_verified(self, launches: List[Dict[str, object]], cap: int, num_images: int, edges: Optional[Iterable[Tuple[int, int]]] = None,
                             extra: Optional[Dict[Tuple[int, int], np.ndarray]] = None, kp_xy=None) -> Dict[str, object]:
        """Tracks of a scene whose verified match lists lie on the device. ``launches``: the ``ver`` dicts that ``FrontEndPipeline.verify``
        and the two-way generator build (match_idx / match_off / match_count / mask / stats / pairs); ``cap``: rows per image of the
        feature table, so node_off[image] = image * cap. A pair is enabled when it has a model (``stats[:, 0] > 0``, computed on the device;
        a pair without one contributes nothing, as its failure tuple has no correspondences) and, with ``edges``, when it is listed there.
        ``extra``: host (K, 2) arrays of edges that were verified through the per-pair fallback; they are uploaded as one more block.
        A second call with another ``edges`` uploads only the edge mask: the blocks are concatenated once and kept."""
        torch = self._torch
        key = (tuple(id(v) for v in launches), id(extra), int(cap), int(num_images))
        st = getattr(self, "_scene", None)
        if st is None or st["key"] != key:
            extra_items = [(p, np.asarray(m).reshape(-1, 2)) for p, m in (extra or {}).items() if np.asarray(m).size]
            for (i1, i2), m in extra_items:
                if m.min() < 0 or m.max() >= cap:
                    raise IndexError(f"edge ({i1}, {i2}): a keypoint index lies outside 0 .. {cap - 1}")
            idx = [v["match_idx"].reshape(-1, 2) for v in launches]
            mask = [v["mask"] for v in launches]
            count = [v["match_count"] for v in launches]
            enable = [(v["stats"][:, 0] > 0).to(torch.uint8) for v in launches]
            pairs: List[Tuple[int, int]] = [tuple(p) for v in launches for p in v["pairs"]]
            off, base = [0], 0
            for v in launches:
                off += [base + int(o) for o in list(v["match_off"])[1:]]
                base = off[-1]
            if extra_items:
                rows = np.concatenate([m for _, m in extra_items]).astype(np.int32)
                idx.append(torch.from_numpy(rows).to(self.device))
                mask.append(torch.ones(len(rows), dtype=torch.uint8, device=self.device))
                count.append(torch.tensor([len(m) for _, m in extra_items], dtype=torch.int32, device=self.device))
                enable.append(torch.ones(len(extra_items), dtype=torch.uint8, device=self.device))
                for p, m in extra_items:
                    pairs.append((int(p[0]), int(p[1])))
                    off.append(off[-1] + len(m))
            empty_i32 = torch.empty((0, 2), dtype=torch.int32, device=self.device)
            st = self._scene = {
                "key": key, "keep": (launches, extra), "pairs": pairs,
                "match_idx": torch.cat(idx).contiguous() if idx else empty_i32,
                "mask": torch.cat(mask).contiguous() if mask else torch.empty(0, dtype=torch.uint8, device=self.device),
                "match_count": torch.cat(count).to(torch.int32).contiguous() if count else torch.empty(0, dtype=torch.int32, device=self.device),
                "enable": torch.cat(enable).contiguous() if enable else torch.empty(0, dtype=torch.uint8, device=self.device),
                "match_off": self._dev(np.asarray(off, dtype=np.int64), torch.int64),
                "pair_images": self._dev(np.asarray(pairs, dtype=np.int32).reshape(-1, 2), torch.int32),
                "node_off": self._dev(np.arange(num_images + 1, dtype=np.int64) * int(cap), torch.int64),
            }
        enable = st["enable"]
        if edges is not None:
            enable = enable & torch.from_numpy(edge_selection(st["pairs"], edges)).to(self.device)
        return self.tracks_from_device(st["match_idx"], st["match_off"], st["pair_images"], st["node_off"], match_count=st["match_count"], mask=st["mask"],
                                       pair_enable=enable, kp_xy=kp_xy, num_nodes=int(num_images) * int(cap))
