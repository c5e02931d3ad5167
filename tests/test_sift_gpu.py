"""GPU: the SIFT detector-descriptor (``gtsfm_amd/csrc/sift_kernels.hip``) against the numpy restatement's recorded outputs
(``tests/sift_reference.py``, goldens written by ``tools/make_sift_fixture.py``) and against OpenCV's recorded output. Reads goldens only.

The kernels use the restatement's explicit ``exp`` / ``exp2`` / ``sin`` / ``cos`` and its summation orders, so every comparison with the
restatement is for byte identity: pyramid, candidates (as a set), keypoints (as a set), oriented keypoints, coordinates, sizes, responses
and descriptors. No keypoint is excluded. The figures are printed and kept in ``profiles/sift_gpu_tests.txt``."""

import hashlib

import numpy as np
import pytest

import sift_agreement
import sift_reference as S
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SMALL = ("40x48", "123x157", "240x320")
STORED_KEYPOINTS = 5200  # what the full-size goldens hold (tools/make_sift_fixture.py)
KP_FIELDS = ("octave", "layer", "row", "column", "x", "y", "scl", "response")


@pytest.fixture(scope="module")
def engine(gpu_device):
    from gtsfm_amd.runtime.sift_engine import SiftEngine

    return SiftEngine(gpu_device)


@pytest.fixture(scope="module")
def small():
    return {name: np.load(GOLDEN / f"sift_{name}.npz") for name in SMALL}


@pytest.fixture(scope="module")
def lund():
    return [sift_agreement.load_lund_door(GOLDEN, i) for i in (0, 1)]


@pytest.fixture(scope="module")
def lund_device(engine, lund):
    """The device's output for the two photographs, computed once: the stored tier and the plugin's 5000 are prefixes of it."""
    return [engine.detect(gray, STORED_KEYPOINTS) for gray, _ in lund]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _by_position(kp):
    order = np.lexsort((kp["column"], kp["row"], kp["layer"], kp["octave"]))
    return {k: v[order] for k, v in kp.items()}


@pytest.mark.parametrize("name", SMALL)
def test_stages_equal_the_restatement(engine, small, name):
    g = small[name]
    gray = g["gray"]
    h, w = gray.shape
    pyramid = engine.stage(gray, 0).cpu().numpy()
    at, digests = 0, []
    for images in (6, 5):
        for oh, ow in S.octave_shapes(h, w):
            for _ in range(images):
                digests.append(hashlib.sha256(pyramid[at : at + oh * ow].tobytes()).hexdigest())
                at += oh * ow
    assert at == len(pyramid)
    differing = [i for i, (a, b) in enumerate(zip(digests, g["pyramid_sha256"])) if a != b]
    print(f"{name}: pyramid images differing from the restatement: {differing} of {len(digests)}")
    assert not differing and len(digests) == len(g["pyramid_sha256"])
    if "pyramid" in g.files:
        assert pyramid.tobytes() == g["pyramid"].tobytes()

    cand = engine.stage(gray, 1)
    cand = cand[np.lexsort((cand[:, 3], cand[:, 2], cand[:, 1], cand[:, 0]))]
    print(f"{name}: candidates {len(cand)} (restatement {len(g['candidates'])})")
    assert np.array_equal(cand, g["candidates"])

    kp = _by_position(engine.stage(gray, 2))
    print(f"{name}: keypoints {len(kp['octave'])} (restatement {len(g['kp_octave'])})")
    for k in KP_FIELDS:
        assert _same(kp[k], g["kp_" + k]), (k, np.flatnonzero(kp[k] != g["kp_" + k])[:8] if kp[k].shape == g["kp_" + k].shape else kp[k].shape)

    ori = engine.stage(gray, 3)
    print(f"{name}: oriented keypoints {len(ori['angle'])} (restatement {len(g['ori_angle'])})")
    for k in KP_FIELDS + ("angle",):
        assert _same(ori[k], g["ori_" + k]), k

    xy, sizes, resp, desc = engine.detect(gray, 1 << 20)
    worst = int(np.abs(desc - g["descriptors"].astype(np.float32)).max()) if desc.shape == g["descriptors"].shape else -1
    print(f"{name}: descriptors {desc.shape}, largest element difference from the restatement {worst}, identical rows "
          f"{int((desc == g['descriptors']).all(axis=1).sum()) if worst >= 0 else 0}")
    assert _same(xy, g["coordinates"]) and _same(sizes, g["sizes"]) and _same(resp, g["responses"])
    assert desc.dtype == np.float32 and np.array_equal(desc, g["descriptors"].astype(np.float32))


@pytest.mark.parametrize("index", (0, 1))
def test_full_size_equals_the_restatement_and_meets_the_caps_against_opencv(lund, lund_device, index):
    _, g = lund[index]
    xy, sizes, resp, desc = lund_device[index]
    assert len(xy) == STORED_KEYPOINTS == len(g["coordinates"])
    same_rows = (desc == g["descriptors"].astype(np.float32)).all(axis=1) if desc.shape == g["descriptors"].shape else np.zeros(1, dtype=bool)
    print(f"image {index}: coordinates identical {_same(xy, g['coordinates'])}, sizes {_same(sizes, g['sizes'])}, responses {_same(resp, g['responses'])}, "
          f"identical descriptor rows {int(same_rows.sum())} of {len(same_rows)}")
    twoway = np.load(GOLDEN / "twoway_lund_door_sift.npz")
    fig = sift_agreement.agreement(g["recorded_coordinates"], g["recorded_sizes"], g["recorded_responses"], twoway[f"descriptors_{index}"], xy, sizes, resp, desc)
    print(f"image {index}: device against OpenCV's recorded output: {fig}")
    assert _same(xy, g["coordinates"]) and _same(sizes, g["sizes"]) and _same(resp, g["responses"])
    assert np.array_equal(desc, g["descriptors"].astype(np.float32))
    sift_agreement.check_caps(fig)


def test_two_runs_and_a_batch_of_three_are_byte_identical(engine, small):
    gray = small["123x157"]["gray"]
    images = [gray, np.ascontiguousarray(gray[::-1]), np.ascontiguousarray(gray[:, ::-1])]
    singles = [engine.detect(im, 5000) for im in images]
    again = engine.detect(images[0], 5000)
    batch = engine.detect_batch(images, 5000)
    assert all(_same(a, b) for a, b in zip(singles[0], again))
    for one, many in zip(singles, batch):
        assert len(one[0]) > 100 and all(_same(a, b) for a, b in zip(one, many))
    assert not _same(singles[0][0], singles[1][0])


def test_mask_drops_keypoints_before_the_top_k(engine, small):
    g = small["240x320"]
    gray, mask = g["gray"], g["mask"]
    free = engine.detect(gray, 1 << 20)
    masked = engine.detect(gray, 1 << 20, mask)
    rc = np.rint(masked[0]).astype(int)
    assert len(rc) > 0 and (mask[rc[:, 1], rc[:, 0]] != 0).all()
    rc = np.rint(free[0]).astype(int)
    keep = mask[rc[:, 1], rc[:, 0]] != 0
    assert 0 < keep.sum() < len(keep)
    assert all(_same(m, f[keep]) for m, f in zip(masked, free))
    assert _same(masked[0], g["masked_coordinates"]) and np.array_equal(masked[3], g["masked_descriptors"].astype(np.float32))
    # the mask acts before the top-k: the strongest 50 of the masked image, not the unmasked strongest 50 filtered
    top = engine.detect(gray, 50, mask)
    assert all(_same(t, m[:50]) for t, m in zip(top, masked))


def test_max_keypoints_keeps_the_strongest_in_the_stated_order(engine, small):
    g = small["123x157"]
    full = engine.detect(g["gray"], 1 << 20)
    n = len(full[0])
    assert n == len(g["coordinates"]) and (np.diff(full[2]) <= 0).all()
    for k in (1, 64, n - 1, n, n + 1):
        part = engine.detect(g["gray"], k)
        assert len(part[0]) == min(k, n) and all(_same(p, f[:k]) for p, f in zip(part, full))


def test_images_without_keypoints_return_empty_arrays(engine):
    for image in (np.full((64, 80), 117, dtype=np.uint8), np.zeros((4, 4), dtype=np.uint8), np.full((2, 3), 9, dtype=np.uint8), np.zeros((1, 1), dtype=np.uint8)):
        xy, sizes, resp, desc = engine.detect(image, 100)
        assert xy.shape == (0, 2) and sizes.shape == (0,) and resp.shape == (0,) and desc.shape == (0, 128) and desc.size == 0


def test_a_16x16_image_runs_and_equals_the_restatement(engine, small):
    """16 x 16 doubles to 32 x 32: three octaves of which only the first has an interior beyond the 5-pixel border."""
    for image in (np.ascontiguousarray(small["40x48"]["gray"][:16, :16]), np.zeros((16, 16), dtype=np.uint8)):
        want = S.detect_and_describe(image, 100)
        got = engine.detect(image, 100)
        assert all(_same(a, b) for a, b in zip(got, want))
    assert len(engine.detect(np.zeros((16, 16), dtype=np.uint8), 100)[0]) == 0


def test_colour_images_go_through_the_gray_conversion(engine, small):
    gray = small["40x48"]["gray"]
    want = engine.detect(gray, 100)
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, size=gray.shape + (3,), dtype=np.uint8)
    for image, as_gray in ((np.repeat(gray[:, :, None], 3, axis=2), gray), (np.dstack([np.repeat(gray[:, :, None], 3, axis=2), rgb[:, :, :1]]), gray),
                           (rgb, S.to_gray(rgb))):
        got = engine.detect(np.ascontiguousarray(image), 100)
        ref = want if as_gray is gray else S.detect_and_describe(as_gray, 100)
        assert all(_same(a, b) for a, b in zip(got, ref))
    with pytest.raises(ValueError, match="Input image dimensions are wrong"):
        engine.detect(np.zeros((8, 8, 2), dtype=np.uint8), 100)


def test_a_list_that_is_too_small_is_reported_and_the_call_repeated(engine, small, gpu_device):
    import torch

    g = small["123x157"]
    before = engine.relaunches
    got = engine.detect(g["gray"], 5000, cand_capacity=16, kp_capacity=8)
    assert engine.relaunches > before
    assert _same(got[0], g["coordinates"]) and np.array_equal(got[3], g["descriptors"].astype(np.float32))
    # the C call itself: an error code and the counts in gtsfm_last_error, never a silent truncation
    from gtsfm_amd.runtime import lib as L

    lib = L.load()
    gray = torch.from_numpy(g["gray"]).to(gpu_device)
    h, w = g["gray"].shape
    ws = torch.empty(int(lib.gtsfm_sift_workspace_bytes(1, h, w, 16, 8)), dtype=torch.uint8, device=gpu_device)
    counts = torch.zeros(4, dtype=torch.int32, device=gpu_device)
    kp = torch.empty((8, 4), dtype=torch.float32, device=gpu_device)
    de = torch.empty((8, 128), dtype=torch.float32, device=gpu_device)
    rc = lib.gtsfm_sift_detect_and_describe(gray.data_ptr(), None, 1, h, w, 8, 16, 8, counts.data_ptr(), kp.data_ptr(), de.data_ptr(), ws.data_ptr(), ws.numel(),
                                            L.current_stream_handle())
    assert rc == -3 and f"{len(g['candidates'])} candidates" in lib.gtsfm_last_error().decode()
    assert counts.cpu().numpy().tolist()[:1] == [len(g["candidates"])]
    with pytest.raises(RuntimeError, match="above the capacities"):
        engine.stage(g["gray"], 1, cand_capacity=16)


def test_plugin_and_twoway_matcher_end_to_end(lund, lund_device):
    """SIFTDetectorDescriptor on both photographs, then TwoWayMatcher(ratio 0.8): equal to the same matcher on the restatement's stored
    descriptors on every pair whose four descriptors are identical (here: all of them); the overlap with the recorded OpenCV run's matches
    is reported, not asserted."""
    from gtsfm_amd.common.image import Image
    from gtsfm_amd.frontend.detector_descriptor import SIFTDetectorDescriptor
    from gtsfm_amd.frontend.matcher.twoway_matcher import TwoWayMatcher

    plugin = SIFTDetectorDescriptor()
    out = [plugin.detect_and_describe(Image(np.repeat(gray[:, :, None], 3, axis=2))) for gray, _ in lund]
    for (kps, desc), dev in zip(out, lund_device):
        assert len(kps) == 5000 and desc.shape == (5000, 128) and desc.dtype == np.float32
        assert _same(kps.coordinates, dev[0][:5000]) and _same(kps.scales, dev[1][:5000]) and _same(kps.responses, dev[2][:5000]) and _same(desc, dev[3][:5000])
    matcher = TwoWayMatcher(ratio_test_threshold=0.8)
    shape = lund[0][0].shape + (3,)
    got = matcher.match(out[0][0], out[1][0], out[0][1], out[1][1], shape, shape)
    stored = [g["descriptors"][:5000].astype(np.float32) for _, g in lund]
    want = matcher.match(None, None, stored[0], stored[1], shape, shape)
    same = [(out[i][1] == stored[i]).all(axis=1) for i in (0, 1)]
    print(f"end to end: {len(got)} matches on the device's descriptors, {len(want)} on the restatement's; identical descriptor rows {int(same[0].sum())} / {int(same[1].sum())}")
    assert same[0].all() and same[1].all() and np.array_equal(got, want)
    # how many of the recorded run's matches reappear as coordinate pairs (within 0.01 px at both ends)
    twoway = np.load(GOLDEN / "twoway_lund_door_sift.npz")
    rec = [g["recorded_coordinates"].astype(np.float64) for _, g in lund]
    mine = np.concatenate([out[0][0].coordinates[got[:, 0]], out[1][0].coordinates[got[:, 1]]], axis=1).astype(np.float64)
    theirs = np.concatenate([rec[0][twoway["expected_ratio_0_8"][:, 0]], rec[1][twoway["expected_ratio_0_8"][:, 1]]], axis=1)
    hits = sum(bool((np.abs(mine - t).max(axis=1) <= 0.01).any()) for t in theirs)
    print(f"end to end: {hits} of the recorded run's {len(theirs)} matches reappear among the device pipeline's {len(got)}")
    assert len(got) > 1000
