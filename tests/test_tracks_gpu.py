"""GPU: ``gtsfm_tracks_from_matches`` against the CPU restatement (tests/tracks_reference.py), exactly: the CSR arrays, the counts and
the number of rounds on every scene; identical bytes across runs, across pair / row orders and with every edge listed twice; the
capacity layout's row and pair filters; the empty cases; and the estimator classes on top. The scenes and why each is there:
tests/test_tracks_host.py checks their properties on the CPU."""

import functools

import numpy as np
import pytest

from tests import tracks_reference as TR
from tests.test_tracks_host import SCENE_FIGURES, build_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(gpu_device):
    from gtsfm_amd.runtime.tracks_engine import TracksEngine

    return TracksEngine(gpu_device)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(sizes, matches, restatement, rounds of the emulation), computed once per scene."""
    sizes, matches = build_scene(name)
    return sizes, matches, TR.tracks_reference(matches, sizes), TR.emulate_rounds(matches, sizes)[1]


def pack(sizes, matches):
    pairs = [p for p, m in matches.items() if np.asarray(m).size]
    rows = [np.asarray(matches[p]).reshape(-1, 2).astype(np.int32) for p in pairs]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows], dtype=np.int64)]).astype(np.int64)
    idx = np.concatenate(rows) if rows else np.zeros((0, 2), np.int32)
    return idx, off, np.array(pairs, dtype=np.int32).reshape(-1, 2), np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]).astype(np.int64)


def run(engine, sizes, matches, kp_xy=None, **extra):
    import torch

    idx, off, pairs, node_off = pack(sizes, matches)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(engine.device) for k, v in extra.items()}
    out = engine.tracks_from_device(torch.from_numpy(idx).to(engine.device), off, pairs, node_off,
                                    kp_xy=None if kp_xy is None else torch.from_numpy(kp_xy).to(engine.device), **dev)
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}


def assert_equals_restatement(out, ref, rounds):
    c = out["counts"]
    print({k: c[k] for k in c}, "restatement:", {k: ref[k] for k in ("tracks", "measurements", "discarded", "components")}, "rounds", rounds)
    assert (c["tracks"], c["measurements"], c["discarded"], c["components"]) == (ref["tracks"], ref["measurements"], ref["discarded"], ref["components"])
    assert c["rounds"] == rounds
    for k in ("track_off", "image", "kp"):
        assert out[k].dtype == ref[k].dtype and np.array_equal(out[k], ref[k]), k


def same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("track_off", "image", "kp")) and a["counts"] == b["counts"]


def test_known_answers_through_the_engine_and_the_estimator(engine):
    from gtsfm_amd.common.keypoints import Keypoints
    from gtsfm_amd.data_association import CppDsfTracksEstimator, DsfTracksEstimator

    for c in TR.known_answers():
        ref = TR.tracks_reference(c["matches"], c["sizes"])
        out = run(engine, c["sizes"], c["matches"])
        assert_equals_restatement(out, ref, TR.emulate_rounds(c["matches"], c["sizes"])[1])
        assert (out["counts"]["tracks"], out["counts"]["discarded"]) == (c["tracks"], c["discarded"])
        coords = c.get("coordinates") or [np.arange(2 * n).reshape(n, 2) for n in c["sizes"]]
        kps = [Keypoints(np.array(x)) for x in coords]
        for cls in (DsfTracksEstimator, CppDsfTracksEstimator):
            tracks = cls().run(c["matches"], kps)
            assert len(tracks) == c["tracks"]
            if "expected_tracks" in c:  # the order the reference's test_track_generation asserts
                assert [[m.i for m in t.measurements] for t in tracks] == [[i for i, _ in t] for t in c["expected_tracks"]]
                for t, exp in zip(tracks, c["expected_tracks"]):
                    assert all(np.array_equal(m.uv, coords[i][k]) for m, (i, k) in zip(t.measurements, exp))


@pytest.mark.parametrize("name", list(SCENE_FIGURES))
def test_scene_equals_the_restatement_whatever_the_order(engine, name):
    sizes, matches, ref, rounds = scene(name)
    assert (ref["tracks"], ref["discarded"], rounds) == (SCENE_FIGURES[name][2], SCENE_FIGURES[name][3], SCENE_FIGURES[name][6])
    rng = np.random.default_rng(11)
    kp_xy = rng.integers(0, 1 << 32, size=(sum(sizes), 2), dtype=np.uint64).astype(np.uint32).view(np.float32)  # any bit pattern, NaNs included
    out = run(engine, sizes, matches, kp_xy=kp_xy)
    assert_equals_restatement(out, ref, rounds)
    node = np.cumsum([0] + sizes)[out["image"]] + out["kp"]
    assert out["uv"].dtype == np.float32 and out["uv"].tobytes() == kp_xy[node].tobytes()
    again = run(engine, sizes, matches, kp_xy=kp_xy)
    assert same_bytes(out, again) and out["uv"].tobytes() == again["uv"].tobytes()
    # the same edges, the pairs in another order and every pair's rows in another order
    pairs = list(matches)
    shuffled = {pairs[p]: np.asarray(matches[pairs[p]])[rng.permutation(len(matches[pairs[p]]))] for p in rng.permutation(len(pairs))}
    assert list(shuffled) != pairs
    assert same_bytes(out, run(engine, sizes, shuffled))
    # every edge twice (rounds included: a duplicate hooks the same roots)
    assert same_bytes(out, run(engine, sizes, {p: np.concatenate([m, m]) for p, m in matches.items()}))


def test_capacity_layout_row_filter_mask_and_pair_enable(engine):
    import torch

    sizes, matches, _, _ = scene("rand24")
    lay = TR.scene_capacity_layout(sizes, matches)
    ref = TR.tracks_reference(lay["surviving"], sizes)
    rounds = TR.emulate_rounds(lay["surviving"], sizes)[1]
    t = {k: torch.from_numpy(lay[k]).to(engine.device) for k in ("match_idx", "match_count", "mask", "pair_enable")}
    node_off = np.cumsum([0] + sizes)
    out = engine.tracks_from_device(t["match_idx"], lay["match_off"], lay["pair_images"], node_off, match_count=t["match_count"], mask=t["mask"],
                                    pair_enable=t["pair_enable"])
    out = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}
    assert_equals_restatement(out, ref, rounds)
    assert same_bytes(out, run(engine, sizes, lay["surviving"]))  # and it equals the compact layout of the surviving rows
    # without the count the garbage rows are active: the call refuses them, it does not follow them out of the tables
    with pytest.raises(RuntimeError, match="outside"):
        engine.tracks_from_device(t["match_idx"], lay["match_off"], lay["pair_images"], node_off)


def test_empty_inputs_give_zero_counts(engine):
    import torch

    empty = {"tracks": 0, "measurements": 0, "discarded": 0, "components": 0, "rounds": 0}
    for sizes, matches in (([5, 5], {}), ([5, 5, 5], {(0, 1): np.array([]), (1, 2): np.zeros((0, 2), np.int64)}), ([7], {}), ([], {})):
        out = run(engine, sizes, matches)
        assert out["counts"] == empty and out["track_off"].tolist() == [0] and len(out["image"]) == 0 and len(out["kp"]) == 0
    # pairs that own zero rows next to one that owns some, and pairs switched off altogether
    idx = torch.tensor([[0, 1], [2, 2]], dtype=torch.int32, device=engine.device)
    out = engine.tracks_from_device(idx, [0, 0, 2, 2], [[0, 1], [1, 2], [0, 2]], [0, 5, 10, 15])
    assert out["counts"]["tracks"] == 2 and out["image"].tolist() == [1, 2, 1, 2] and out["kp"].tolist() == [0, 1, 2, 2]
    off = engine.tracks_from_device(idx, [0, 0, 2, 2], [[0, 1], [1, 2], [0, 2]], [0, 5, 10, 15], pair_enable=torch.zeros(3, dtype=torch.uint8, device=engine.device))
    assert off["counts"] == dict(empty, rounds=1) and off["track_off"].tolist() == [0]
    # a keypoint matched to itself is a set of one: a track with a single measurement
    one = engine.tracks_from_device(torch.tensor([[3, 3]], dtype=torch.int32, device=engine.device), [0, 1], [[1, 1]], [0, 5, 10])
    assert one["counts"]["tracks"] == 1 and one["image"].tolist() == [1] and one["kp"].tolist() == [3] and one["track_off"].tolist() == [0, 1]


def test_the_call_refuses_a_small_workspace_by_name(engine):
    import torch

    from gtsfm_amd.runtime import lib as L

    h = L.load()
    dev = engine.device
    idx = torch.tensor([[0, 1]], dtype=torch.int32, device=dev)
    moff, noff = torch.tensor([0, 1], device=dev), torch.tensor([0, 4, 8], device=dev)
    pimg = torch.tensor([[0, 1]], dtype=torch.int32, device=dev)
    need = h.gtsfm_tracks_workspace_bytes(8, 1)
    ws, out = torch.empty(need, dtype=torch.uint8, device=dev), torch.zeros(64, dtype=torch.int64, device=dev)
    args = [idx.data_ptr(), moff.data_ptr(), None, None, None, pimg.data_ptr(), 1, 1, noff.data_ptr(), 2, None, ws.data_ptr(), need - 1, out.data_ptr(),
            out[8:].data_ptr(), out[16:].data_ptr(), None, out[24:].data_ptr(), None]
    assert h.gtsfm_tracks_from_matches(*args) < 0
    assert b"gtsfm_tracks_from_matches" in h.gtsfm_last_error() and str(need).encode() in h.gtsfm_last_error()
    args[12] = need
    assert h.gtsfm_tracks_from_matches(*args) == 0
    torch.cuda.synchronize()
    assert out[24:29].view(torch.int32)[:5].tolist() == [1, 2, 0, 1, 2]


def test_estimator_on_rand24_returns_the_restatements_tracks_with_the_callers_coordinates():
    from gtsfm_amd.common.keypoints import Keypoints
    from gtsfm_amd.common.sfm_track import SfmMeasurement, SfmTrack2d
    from gtsfm_amd.data_association import DsfTracksEstimator, get_2d_tracks

    sizes, matches, ref, _ = scene("rand24")
    rng = np.random.default_rng(4)
    kps = [Keypoints(rng.random((n, 2)) * 1000.0) for n in sizes]  # float64
    est = DsfTracksEstimator()
    tracks = est.run(matches, kps)
    expected = [SfmTrack2d([SfmMeasurement(int(i), kps[i].coordinates[k]) for i, k in zip(ref["image"][a:b], ref["kp"][a:b])])
                for a, b in zip(ref["track_off"][:-1], ref["track_off"][1:])]
    assert len(tracks) == len(expected) == ref["tracks"] and all(t == e for t, e in zip(tracks, expected))
    assert all(m.uv.dtype == np.float64 and np.array_equal(m.uv, kps[m.i].coordinates[k])
               for t, a in zip(tracks, ref["track_off"][:-1]) for m, k in zip(t.measurements, ref["kp"][a:]))
    arrays = est.run_arrays(matches, kps)
    assert all(np.array_equal(arrays[k], ref[k]) for k in ("track_off", "image", "kp"))
    assert len(get_2d_tracks(matches, kps)) == ref["tracks"]
    kps32 = [Keypoints(k.coordinates.astype(np.float32)) for k in kps]
    assert est.run(matches, kps32)[0].measurement(0).uv.dtype == np.float32
