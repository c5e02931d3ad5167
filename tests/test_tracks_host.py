"""CPU: the host side of the device track builder -- the restatement against the reference's four known answers, the two new entry
points' argument checks, the estimator classes, the stand-in track type -- and the properties of the scenes the GPU tests run, under
the restatement and the round emulation, so that none of those tests is vacuous. None of it needs a GPU."""

import ctypes
import pickle

import numpy as np
import pytest

from tests import tracks_reference as TR

# scene -> (nodes, match rows, tracks, discarded, longest track, largest component, rounds) under tests/tracks_reference.py
SCENE_FIGURES = {
    "rand24": (12288, 18450, 1029, 197, 15, None, 5),
    "giant": (3600, 2640, 205, 30, 6, None, 5),
    "zig96": (768, 760, 8, 0, 96, 96, 6),
    "zig1000": (2000, 1998, 2, 0, 1000, 1000, 8),
    "wide60": (300000, 1534450, 14523, 2345, 35, 218, 5),
}


def build_scene(name):
    return {"rand24": TR.scene_rand, "giant": TR.scene_giant, "zig96": lambda: TR.scene_zigzag(96, 8), "zig1000": lambda: TR.scene_zigzag(1000, 2),
            "wide60": lambda: TR.scene_rand(num_images=60, num_kp=5000, num_points=40000, seed=3)}[name]()


def test_restatement_reproduces_the_four_known_answers():
    cases = TR.known_answers()
    assert [c["name"] for c in cases] == ["no_duplicates", "with_duplicates", "nontransitive", "track_generation"]
    assert (1, 1) in cases[1]["matches"]  # the self-pair
    for c in cases:
        ref = TR.tracks_reference(c["matches"], c["sizes"])
        assert (ref["tracks"], ref["discarded"]) == (c["tracks"], c["discarded"]), c["name"]
        labels, rounds = TR.emulate_rounds(c["matches"], c["sizes"])
        assert 2 <= rounds <= 3
        if "expected_tracks" in c:
            got = [list(map(list, zip(ref["image"][a:b].tolist(), ref["kp"][a:b].tolist()))) for a, b in zip(ref["track_off"][:-1], ref["track_off"][1:])]
            assert got == c["expected_tracks"]
    assert [(c["tracks"], c["discarded"]) for c in cases] == [(4, 0), (4, 1), (0, 1), (3, 0)]


def test_emulation_labels_are_the_restatements_partition():
    """The round scheme and the plain union-find find the same sets: every touched node's label is the smallest node of its set."""
    sizes, matches = TR.scene_rand(num_images=6, num_kp=64, num_points=150, seed=5)
    labels, rounds = TR.emulate_rounds(matches, sizes)
    ref = TR.tracks_reference(matches, sizes)
    node = np.cumsum([0] + sizes)[ref["image"]] + ref["kp"]
    for a, b in zip(ref["track_off"][:-1], ref["track_off"][1:]):
        assert (labels[node[a:b]] == node[a]).all()
    assert rounds >= 2 and (labels <= np.arange(len(labels))).all()


@pytest.mark.parametrize("name", list(SCENE_FIGURES))
def test_gpu_scenes_have_the_stated_properties(name):
    nodes, rows, tracks, discarded, longest, largest, rounds = SCENE_FIGURES[name]
    sizes, matches = build_scene(name)
    ref = TR.tracks_reference(matches, sizes)
    _, r = TR.emulate_rounds(matches, sizes)
    print(name, sum(sizes), sum(len(m) for m in matches.values()), {k: v for k, v in ref.items() if isinstance(v, int)}, r)
    assert (sum(sizes), sum(len(m) for m in matches.values())) == (nodes, rows)
    assert (ref["tracks"], ref["discarded"], ref["longest"], r) == (tracks, discarded, longest, rounds)
    if largest is not None:
        assert ref["largest_component"] == largest
    if name == "rand24":  # valid and duplicate-image sets mixed, more rows than one workgroup reads
        assert ref["tracks"] > 500 and ref["discarded"] > 100 and rows > 64 * 256
    if name == "giant":  # the pigeonhole path: one set far above the image count, and sets that are discarded by the neighbour check too
        assert ref["largest_component"] > 50 * len(sizes)
    if name == "wide60":  # the workload's node count: more than 256 scan blocks of 1024, so the scan of the block sums takes its second trip
        assert nodes > 256 * 1024
    if name.startswith("zig"):  # longer than a wavefront; the labels alternate, so one round cannot finish
        assert ref["longest"] == len(sizes) > 64


def test_capacity_layout_scene_filters_rows_and_pairs():
    sizes, matches = TR.scene_rand()
    lay = TR.scene_capacity_layout(sizes, matches)
    count, off = lay["match_count"], lay["match_off"]
    assert (count < np.diff(off)).all() and lay["pair_enable"].sum() == len(matches) - len(matches) // 3
    beyond = np.concatenate([lay["match_idx"][off[p] + count[p] : off[p + 1]] for p in range(len(count))])
    assert (np.abs(beyond.astype(np.int64)) >= 1 << 20).all()  # garbage rows: out of range on both sides
    kept = sum(len(m) for m in lay["surviving"].values())
    assert 0.4 * count.sum() < kept < 0.55 * count.sum()  # 2/3 of the pairs times 70 % of the rows
    ref, full = TR.tracks_reference(lay["surviving"], sizes), TR.tracks_reference(matches, sizes)
    assert ref["tracks"] > 500 and ref["tracks"] != full["tracks"]


def test_library_exports_the_entry_points_and_they_reject_bad_arguments(built_library):
    from gtsfm_amd.runtime import lib as L

    raw = ctypes.CDLL(str(built_library))
    assert hasattr(raw, "gtsfm_tracks_workspace_bytes") and hasattr(raw, "gtsfm_tracks_from_matches")
    assert "gtsfm_tracks_workspace_bytes" in L.SIGNATURES and "gtsfm_tracks_from_matches" in L.SIGNATURES
    assert len(L.SIGNATURES["gtsfm_tracks_from_matches"][1]) == 19
    h = L.load()
    p = 0x1000  # never dereferenced: every call below is refused before a launch or a copy
    good = [p, p, p, p, p, p, 3, 10, p, 4, p, p, 1 << 20, p, p, p, p, p, None]
    for pos, value, word in ((0, None, b"null"), (1, None, b"null"), (5, None, b"null"), (8, None, b"null"), (11, None, b"null"), (13, None, b"null"),
                             (14, None, b"null"), (15, None, b"null"), (17, None, b"null"), (6, -1, b"negative"), (7, -5, b"negative"), (9, -1, b"negative"),
                             (10, None, b"kp_xy_dev")):
        args = list(good)
        args[pos] = value
        assert h.gtsfm_tracks_from_matches(*args) < 0, pos
        assert b"gtsfm_tracks_from_matches" in h.gtsfm_last_error() and word in h.gtsfm_last_error(), (pos, h.gtsfm_last_error())


def test_workspace_bytes_is_monotone_and_refuses_what_the_call_refuses(built_library):
    from gtsfm_amd.runtime import lib as L

    h = L.load()
    sizes = [h.gtsfm_tracks_workspace_bytes(n, 1000) for n in (1, 2, 1000, 1024, 1025, 230000, 10**7, 2**31 - 1)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0 and sizes[-1] > 40 * (2**31 - 1)
    by_matches = [h.gtsfm_tracks_workspace_bytes(5000, m) for m in (0, 1, 10**6, 10**9)]
    assert all(a <= b for a, b in zip(by_matches, by_matches[1:])) and by_matches[0] > 0
    assert h.gtsfm_tracks_workspace_bytes(2**31, 10) == 0 and h.gtsfm_tracks_workspace_bytes(-1, 10) == 0 and h.gtsfm_tracks_workspace_bytes(10, -1) == 0


def test_estimator_classes_register_pickle_and_check_their_input():
    from gtsfm_amd.common.keypoints import Keypoints
    from gtsfm_amd.data_association import CppDsfTracksEstimator, DsfTracksEstimator, TracksEstimatorBase, get_2d_tracks
    from gtsfm_amd.data_association.dsf_tracks_estimator import pack_matches
    from gtsfm_amd.frontend.registry import GTSFMProcess

    registry = type(GTSFMProcess).get_registry()
    for cls in (DsfTracksEstimator, CppDsfTracksEstimator):
        assert registry[cls.__name__] is cls and issubclass(cls, TracksEstimatorBase)
        est = pickle.loads(pickle.dumps(cls()))
        assert isinstance(est, cls) and est._engine is None
    assert callable(get_2d_tracks)
    flat = [Keypoints(np.zeros(4))]
    with pytest.raises(Exception, match="2D"):
        DsfTracksEstimator().run({}, flat)
    with pytest.raises(ValueError, match=r"i=0: shape=\(4,\)"):
        CppDsfTracksEstimator().run({}, flat)
    kps = [Keypoints(np.zeros((3, 2))), None, Keypoints(np.zeros((5, 2)))]
    idx, off, pairs, node_off = pack_matches({(0, 2): np.array([[0, 4], [2, 1]]), (2, 0): np.array([]), (2, 2): np.array([[1, 3]], dtype=np.uint32)}, kps)
    assert idx.dtype == np.int32 and idx.tolist() == [[0, 4], [2, 1], [1, 3]] and off.tolist() == [0, 2, 3]
    assert pairs.tolist() == [[0, 2], [2, 2]] and node_off.tolist() == [0, 3, 3, 8]
    for bad in ({(0, 2): np.array([[3, 0]])}, {(0, 2): np.array([[0, 5]])}, {(0, 2): np.array([[-1, 0]])}, {(0, 1): np.array([[0, 0]])}, {(0, 3): np.array([[0, 0]])}):
        with pytest.raises(IndexError):
            pack_matches(bad, kps)


def test_standin_track_equality_ignores_the_order_of_measurements():
    from gtsfm_amd.common.sfm_track import SfmMeasurement, SfmTrack2d

    a = SfmTrack2d([SfmMeasurement(0, np.array([1.0, 2.0])), SfmMeasurement(3, np.array([5.0, 6.0]))])
    b = SfmTrack2d([SfmMeasurement(3, np.array([5.0, 6.0])), SfmMeasurement(0, np.array([1.0, 2.0]))])
    c = SfmTrack2d([SfmMeasurement(3, np.array([5.0, 6.5])), SfmMeasurement(0, np.array([1.0, 2.0]))])
    assert a == b and not a != b and a != c and a != SfmTrack2d(a.measurements[:1]) and a != "track"
    assert a.number_measurements() == 2 and a.measurement(1).i == 3 and a.validate_unique_cameras()
    assert not SfmTrack2d([a.measurement(0), a.measurement(0)]).validate_unique_cameras()
    assert a.select_for_cameras({3}).measurements == [a.measurement(1)] and a.select_subset([1, 0]) == a
