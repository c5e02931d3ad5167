"""CPU: the constructed SIFT images (``tests/sift_constructed.py``) reach, in the numpy restatement, the events that the photographs of the
goldens never reach. The census runs the restatement live (under 0.2 s per image) and prints the table of event x image counts; the same
table for the five images of the goldens is in ``profiles/sift_constructed_census.txt`` (``tools/sift_census.py``).

An event that no image of this size reaches is listed in ``UNREACHABLE`` with the argument or the search that failed; where it is a branch
of one of the explicit float32 functions, ``tests/test_sift_math_gpu.py`` hits it on the device through ``gtsfm_sift_math``."""

import numpy as np
import pytest

import sift_constructed as C
import sift_reference as S

F = np.float32

# event -> why no constructed image reaches it (and where the device branch is exercised instead)
UNREACHABLE = {
    "offset_beyond_limit": "an offset beyond 2^31 / 3 needs two pivots near the singular threshold 1.2e-6 that are not below it; 1200 seeded textures, "
                           "edge and sparse images gave none. The branch is the refinement kernel's, not a function's.",
    "peak_bin_at_least_36": "for a peak (h[j] above both neighbours) the parabola's vertex lies within half a bin of j, so j + offset <= 35.5: dead "
                            "code under the peak test. Function-level: test_sift_math_gpu.py::test_peak_angle (bin 37 from a triple that is no peak).",
    "angle_360_set_to_0": "needs a peak at bin 0 whose neighbours are bit-equal (or a vertex within 1.5e-6 bins of 0); the histograms are sums of "
                          "dozens of weighted magnitudes in window order and no image or search gave one. Function-level: test_peak_angle.",
    "o0_at_least_8_wraps": "needs an arc tangent of exactly 360 under an orientation of exactly 0, which itself needs angle_360_set_to_0 or a vertex "
                           "rounding to bin 36; edge_dots_48x48 reaches the arc tangent of 360 inside descriptors, never at orientation 0.",
    "fewer_than_64_samples": "a keypoint lies at least 5 pixels inside its octave and its scale is at least 1.6 * 2^(1/6), so the window holds the "
                             "9 x 9 pixels around it (its inscribed circle has a radius of 13.5 pixels): never fewer than 81 samples.",
    "equal_response_across_layers_or_octaves": "mirrored keypoints tie inside one layer; a tie across layers or octaves needs two unrelated float32 "
                                               "contrasts to be bit-equal, and 1200 searched images gave none. The two photographs of the goldens have "
                                               "17 and 14 such pairs (profiles/sift_constructed_census.txt), so test_sift_gpu.py orders them.",
}
MUST_BE_REACHED = ("radius_clipped_by_diagonal", "equal_response_different_keypoints", "adjacent_candidates_in_a_layer", "singular_solve",
                   "keypoint_in_a_thin_strip", "keypoint_in_a_12_pixel_octave")


@pytest.fixture(scope="module")
def images():
    return C.images()


@pytest.fixture(scope="module")
def counted(images):
    return {name: C.census(image, C.half_mask(image.shape, 1)) for name, image in images.items()}


def test_images_are_small_seeded_uint8(images):
    again = C.images()
    for name, image in images.items():
        h, w = image.shape
        assert image.dtype == np.uint8 and image.flags.c_contiguous, name
        assert (h <= 64 and w <= 64) or (min(h, w) <= 12 and max(h, w) <= 256), (name, image.shape)
        assert np.array_equal(image, again[name]), name


def test_every_event_is_reached_or_listed_with_its_reason(counted):
    counts = {name: ev for name, (ev, _) in counted.items()}
    print()
    print(C.table(counts))
    assert set(counts[next(iter(counts))]) == set(C.EVENTS)
    reached = {e for e in C.EVENTS if any(ev[e] > 0 for ev in counts.values())}
    print("unreachable:", sorted(UNREACHABLE))
    assert set(UNREACHABLE) <= set(C.EVENTS) and all(len(why) > 40 for why in UNREACHABLE.values())
    assert not [e for e in C.EVENTS if e not in reached and e not in UNREACHABLE], "an event is neither reached nor listed"
    assert not [e for e in UNREACHABLE if e in reached], "an event on the unreachable list is reached: take it off the list"
    assert 4 * len(UNREACHABLE) <= len(C.EVENTS)
    assert not set(MUST_BE_REACHED) & set(UNREACHABLE) and set(MUST_BE_REACHED) <= reached


def test_each_image_reaches_the_event_it_is_named_after(counted):
    ev = {name: c for name, (c, _) in counted.items()}
    st = {name: s for name, (_, s) in counted.items()}
    blob = st["blob_24x24"]
    assert len(blob["keypoints"]["octave"]) == 1 and len(blob["oriented_free"]["angle"]) == 4
    assert ev["blob_24x24"]["keypoint_in_a_12_pixel_octave"] == 1 and ev["blob_24x24"]["radius_clipped_by_diagonal"] == 4
    assert ev["mirror_48x48"]["equal_response_different_keypoints"] >= 4 and ev["mirror_48x48"]["adjacent_candidates_in_a_layer"] > 0
    assert len(C.tie_cuts(st["mirror_48x48"]["oriented_free"])) >= 4
    assert ev["bars_40x40"]["singular_solve"] >= 8 and ev["bars_40x40"]["adjacent_candidates_in_a_layer"] >= 13
    for strip in ("strip_12x200", "strip_200x12"):
        assert ev[strip]["keypoint_in_a_thin_strip"] > 0 and ev[strip]["keypoint_in_a_12_pixel_octave"] > 0
    assert ev["odd_45x51"]["odd_octave_is_decimated"] == 2
    assert [o for o in S.octave_shapes(45, 51)][1] == (45, 51)
    assert ev["claim_48x48"]["two_candidates_one_position"] > 0 and ev["claim_48x48"]["rejected_by_edge_ratio"] > 0
    assert ev["edge_dots_48x48"]["element_saturates_at_255"] > 0 and ev["edge_dots_48x48"]["descriptor_atan2_equals_360"] > 0
    assert ev["edge_atan_48x48"]["atan2_equals_360"] > 0
    assert ev["noise_48x48"]["leaves_layer_range"] > 0 and ev["dots_48x48"]["row_exchange_at_pivot_0"] > 0


def test_the_census_leaves_the_restatement_and_its_outputs_unchanged(images, counted):
    before = (S.atan2_deg, S.gaussian_blur, S.solve3, S.refine, S.histogram_peaks, S.describe_one)
    for name in ("mirror_48x48", "blob_24x24", "edge_dots_48x48"):
        mask = C.half_mask(images[name].shape, 1)
        ev, st = C.census(images[name], mask)
        assert ev == counted[name][0]
        xy, sizes, resp, desc, want = S.detect_and_describe(images[name], 1 << 30, stages=True)
        assert st["pyramid"].tobytes() == want["pyramid"].tobytes() and np.array_equal(st["candidates"], want["candidates"])
        for k, v in want["keypoints"].items():
            assert st["keypoints"][k].tobytes() == v.tobytes(), (name, k)
        for k, v in want["oriented"].items():
            assert st["oriented_free"][k].tobytes() == v.tobytes(), (name, k)
        assert np.array_equal(st["descriptors"], desc)
        masked = S.detect_and_describe(images[name], 1 << 30, mask=mask, stages=True)[4]["oriented"]
        assert all(st["oriented"][k].tobytes() == v.tobytes() for k, v in masked.items())
    assert before == (S.atan2_deg, S.gaussian_blur, S.solve3, S.refine, S.histogram_peaks, S.describe_one)


def test_the_lone_keypoint_mask_keeps_exactly_the_keypoint_the_census_names(images, counted):
    image, kp = images["mirror_48x48"], counted["mirror_48x48"][1]["keypoints"]
    mask, t, (x, y) = C.lone_keypoint_mask(image, kp)
    print(f"mirror_48x48: keypoint {t} (octave {kp['octave'][t]}, layer {kp['layer'][t]}, row {kp['row'][t]}, column {kp['column'][t]}) alone rounds to pixel ({x}, {y})")
    assert mask.sum() == 1 and mask[y, x] == 1
    ev, st = C.census(image, mask, describe=False)
    assert ev["dropped_by_mask"] == len(kp["octave"]) - 1
    kept = st["oriented"]
    assert len(kept["angle"]) >= 1 and all((kept[f] == kp[f][t]).all() for f in ("octave", "layer", "row", "column"))


def test_peak_angle_is_the_restatements_interpolation():
    """``peak_angle`` (the twin of the device's ``sift_peak_angle``) on seeded peaks, every bin: ``histogram_peaks`` returns the same bits."""
    rng = np.random.default_rng(9)
    for j in list(range(36)) * 4:
        hl, hr = rng.uniform(0.0, 1.0, 2).astype(F)
        hj = F(max(hl, hr) + F(rng.uniform(0.01, 1.0)))
        hist = np.zeros(36, dtype=F)
        hist[(j + 35) % 36], hist[j], hist[(j + 1) % 36] = hl, hj, hr
        (want,) = S.histogram_peaks(hist)
        assert C.peak_angle(j, hl, hj, hr)[0].tobytes() == F(want).tobytes()
