"""CPU restatement of the track builder's contract, and the scenes the track tests share.

``tracks_reference`` restates ``gtsfm/data_association/dsf_tracks_estimator.py:51-85`` with a plain union-find: the keypoints (image, k)
are the elements, every match row merges two of them, a set that holds two keypoints of one image is discarded. gtsam's ``DSFMap``
returns the sets in no promised order; the restatement emits the package's contract order: tracks by their smallest (image, keypoint)
member, measurements by image ascending.

``emulate_rounds`` is the device's round scheme in numpy (hook by ``np.minimum.at`` on the roots of the last snapshot, then a full
compress); it returns the labels and the number of rounds, the last one being the round that hooks nothing.
"""

from __future__ import annotations

import json
from pathlib import Path
from typing import Dict, List, Sequence, Tuple

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "tracks_known_answers.json"
Matches = Dict[Tuple[int, int], np.ndarray]


def tracks_reference(matches: Matches, sizes: Sequence[int] = ()) -> Dict[str, object]:
    """CSR tracks (track_off int64, image / kp int32) and the counts of tracks, measurements, discarded sets and all sets, the longest track and the largest set."""
    parent: Dict[Tuple[int, int], Tuple[int, int]] = {}

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for (i1, i2), rows in matches.items():
        rows = np.asarray(rows)
        if rows.size == 0:
            continue
        for k1, k2 in rows.reshape(-1, 2).tolist():
            a, b = (int(i1), int(k1)), (int(i2), int(k2))
            for n in (a, b):
                assert not sizes or 0 <= n[1] < sizes[n[0]], f"keypoint {n} outside its table"
                parent.setdefault(n, n)
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    sets: Dict[Tuple[int, int], List[Tuple[int, int]]] = {}
    for n in parent:
        sets.setdefault(find(n), []).append(n)
    tracks = []
    for members in sets.values():
        members.sort()
        images = [i for i, _ in members]
        if len(set(images)) == len(images):
            tracks.append(members)
    tracks.sort(key=lambda m: m[0])
    flat = [n for t in tracks for n in t]
    return {
        "track_off": np.concatenate([[0], np.cumsum([len(t) for t in tracks], dtype=np.int64)]).astype(np.int64),
        "image": np.array([i for i, _ in flat], dtype=np.int32),
        "kp": np.array([k for _, k in flat], dtype=np.int32),
        "tracks": len(tracks),
        "measurements": len(flat),
        "discarded": len(sets) - len(tracks),
        "components": len(sets),
        "longest": max((len(t) for t in tracks), default=0),
        "largest_component": max((len(m) for m in sets.values()), default=0),
    }


def emulate_rounds(matches: Matches, sizes: Sequence[int]) -> Tuple[np.ndarray, int]:
    """The device scheme on the host: labels [num_nodes] (every touched component's smallest node) and the number of rounds (0 without
    a single match row, as the device call launches nothing then)."""
    node_off = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])
    us, vs = [], []
    for (i1, i2), rows in matches.items():
        rows = np.asarray(rows)
        if rows.size:
            rows = rows.reshape(-1, 2).astype(np.int64)
            us.append(node_off[i1] + rows[:, 0])
            vs.append(node_off[i2] + rows[:, 1])
    parent = np.arange(int(node_off[-1]), dtype=np.int64)
    if not us:
        return parent, 0
    u, v = np.concatenate(us), np.concatenate(vs)
    rounds = 0
    while True:
        rounds += 1
        ru, rv = parent[u], parent[v]  # fully compressed: the parent IS the root
        sel = ru != rv
        if not sel.any():
            return parent, rounds
        np.minimum.at(parent, np.maximum(ru, rv)[sel], np.minimum(ru, rv)[sel])
        while True:
            jumped = parent[parent]
            if np.array_equal(jumped, parent):
                break
            parent = jumped


def known_answers() -> List[dict]:
    """The reference's four known answers (``tests/data_association/test_dsf_tracks_estimator.py``) as data: per case ``sizes``,
    ``matches`` and the expected ``tracks`` / ``discarded`` counts, for the last one also the exact tracks."""
    cases = json.loads(GOLDEN.read_text())["cases"]
    for c in cases:
        c["matches"] = {(m["i1"], m["i2"]): np.array(m["rows"], dtype=np.int64).reshape(-1, 2) for m in c["matches"]}
    return cases


# ---- scenes ----


def scene_rand(num_images: int = 24, num_kp: int = 512, num_points: int = 1500, p_seen: float = 0.25, p_keep: float = 0.7, wrong_per_pair: int = 2,
               seed: int = 0) -> Tuple[List[int], Matches]:
    """Latent points, each seen by an image with ``p_seen`` at a keypoint slot of its own; every pair of images keeps each true match with
    ``p_keep`` and adds ``wrong_per_pair`` random rows; rows shuffled."""
    rng = np.random.default_rng(seed)
    slot = np.full((num_images, num_points), -1, dtype=np.int64)
    for i in range(num_images):
        seen = np.flatnonzero(rng.random(num_points) < p_seen)[:num_kp]
        slot[i, seen] = rng.permutation(num_kp)[: len(seen)]
    matches: Matches = {}
    for i1 in range(num_images):
        for i2 in range(i1 + 1, num_images):
            both = np.flatnonzero((slot[i1] >= 0) & (slot[i2] >= 0))
            both = both[rng.random(len(both)) < p_keep]
            rows = np.concatenate([np.stack([slot[i1, both], slot[i2, both]], 1), rng.integers(0, num_kp, size=(wrong_per_pair, 2))])
            matches[(i1, i2)] = rows[rng.permutation(len(rows))]
    return [num_kp] * num_images, matches


def scene_giant(num_images: int = 12, num_kp: int = 300, wrong_per_pair: int = 40, seed: int = 1) -> Tuple[List[int], Matches]:
    """Only wrong rows: they chain most keypoints into ONE component far above ``num_images`` members."""
    rng = np.random.default_rng(seed)
    matches = {(i1, i2): rng.integers(0, num_kp, size=(wrong_per_pair, 2)) for i1 in range(num_images) for i2 in range(i1 + 1, num_images)}
    return [num_kp] * num_images, matches


def scene_zigzag(num_images: int, num_kp: int, seed: int = 2) -> Tuple[List[int], Matches]:
    """A path through the images in a seeded random order with identity matches: ``num_kp`` tracks of ``num_images`` members whose labels
    alternate along the path."""
    order = np.random.default_rng(seed).permutation(num_images)
    ident = np.stack([np.arange(num_kp), np.arange(num_kp)], 1)
    return [num_kp] * num_images, {(int(a), int(b)): ident.copy() for a, b in zip(order[:-1], order[1:])}


def scene_capacity_layout(sizes: List[int], matches: Matches, seed: int = 3) -> Dict[str, object]:
    """``matches`` re-packed in the generators' capacity layout: every pair owns ``capacity`` rows of which the first ``match_count`` are
    matches and the rest garbage (indices far outside the tables); a mask drops a seeded 30 % of the rows; ``pair_enable`` is off for
    every third pair. ``surviving`` holds the rows that are left: what the restatement has to be run on."""
    rng = np.random.default_rng(seed)
    pairs = list(matches)
    capacity = max(len(m) for m in matches.values()) + 7
    idx = rng.integers(1 << 20, 1 << 30, size=(len(pairs) * capacity, 2)).astype(np.int32)
    idx[::2] *= -1
    mask = (rng.random(len(pairs) * capacity) >= 0.3).astype(np.uint8)
    enable = np.array([p % 3 != 1 for p in range(len(pairs))], dtype=np.uint8)
    count = np.array([len(matches[p]) for p in pairs], dtype=np.int32)
    surviving: Matches = {}
    for p, pair in enumerate(pairs):
        lo = p * capacity
        idx[lo : lo + count[p]] = matches[pair]
        if enable[p]:
            surviving[pair] = np.asarray(matches[pair])[mask[lo : lo + count[p]].astype(bool)]
    return {"match_idx": idx, "match_off": np.arange(len(pairs) + 1, dtype=np.int64) * capacity, "match_count": count, "mask": mask,
            "pair_enable": enable, "pair_images": np.array(pairs, dtype=np.int32), "surviving": surviving, "sizes": sizes}
