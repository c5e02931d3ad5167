"""GPU: D2-Net on libgtsfm_amd.so against the goldens of tests/d2net_reference.py (the reference's model, bit for bit on the CPU): stage
by stage; the detection head on a known map, bit for bit; end to end; top-k truncation; batch / run-to-run identity; gray and float
inputs; candidate-list overflow; the plugin through the cacher and the two-way matcher; accuracy against float64.

Tolerances. Both sides are float32 and differ in summation order only, so every bound derives from the float32 restatement's own
distance to a float64 evaluation of the same path, which tools/make_d2net_fixture.py records in each golden (``*_err64``), times 4,
plus a floor of about one float32 unit in the last place of the quantity's largest value:
  * stages, relative to the stage's largest magnitude: recorded 2.2 - 2.5e-7 (relu(conv1_1)), 4.4 - 6.1e-7 (relu(conv3_3)) and
    3.9 - 4.8e-7 (dense map) over the four goldens -> bounds of about 1.1e-6, 2.5e-6 and 2.0e-6; floor 1.2e-7 = 2^-23;
  * keypoint coordinates: recorded 0.05 - 4.7e-5 px; floor = the spacing of float32 at the image's largest coordinate (3e-5 px at 320);
  * scores, relative to the largest score: recorded 2.0 - 3.4e-7; floor 2^-23;
  * descriptor entries (unit rows, |entry| < 1): recorded 0.8 - 4.6e-7; floor 2^-23.
The head on a known map is compared bit for bit, except the descriptors: their norm sums 512 squares in another order than torch.
Both orders are tree-like (torch: vectorised partial sums; here: 8 terms per lane, then a 6-level butterfly), so the norm's relative
error is at most about (9 + 14) / 2 units of 2^-24 = 7e-7 on either side, and an entry below 1 differs by less than DESC_HEAD_ATOL = 1e-6."""

from __future__ import annotations

import pickle
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import d2net_reference as dr

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
CASES = ["d2net_64x80", "d2net_123x157", "d2net_240x320", "d2net_16x16"]
ULP = 2.0**-23
DESC_HEAD_ATOL = 1e-6
MAX_UNMATCHED = 0.01


@pytest.fixture(scope="module")
def weights():
    return dr.seeded_weights(0)


@pytest.fixture(scope="module")
def engine(weights):
    from gtsfm_amd.runtime.d2net_engine import D2NetEngine

    return D2NetEngine(weights)


@pytest.fixture(scope="module")
def goldens():
    out = {}
    for name in CASES:
        g = np.load(GOLDEN / f"{name}.npz")
        out[name] = (g, dr.seeded_image(int(g["seed"]), int(g["height"]), int(g["width"])))
    return out


@pytest.fixture(scope="module")
def full_240(engine, goldens):
    """The device's untruncated result at 240 x 320, computed once."""
    return engine.detect(goldens["d2net_240x320"][1], 5000)


def _candidates(engine, image, cap=0):
    from gtsfm_amd.runtime.d2net_engine import split_candidates

    counts, records = engine.stage([image], 3, cap)
    return int(counts[0]), split_candidates(records[0, : min(int(counts[0]), records.shape[1])])


def _match(ca, cb):
    index = {tuple(r): k for k, r in enumerate(np.asarray(cb).tolist())}
    pairs = [(k, index[tuple(r)]) for k, r in enumerate(np.asarray(ca).tolist()) if tuple(r) in index]
    return np.array([p[0] for p in pairs], dtype=np.int64), np.array([p[1] for p in pairs], dtype=np.int64)


@pytest.mark.parametrize("batch,h,w,cin,cout,relu", [(2, 13, 21, 64, 64, 1), (1, 3, 3, 128, 68, 0), (1, 17, 33, 256, 128, 1), (1, 1, 1, 64, 4, 0)])
def test_dilated_convolution_matches_aten(batch, h, w, cin, cout, relu):
    """gtsfm_conv3x3_dil2_f32 against F.conv2d(padding=2, dilation=2): ragged tiles, maps smaller than the dilation halo, several input
    chunks, an output written at a channel offset of a wider tensor. Bound: 4 x torch's own float32 distance to float64, plus one unit
    in the last place of the largest output."""
    import torch.nn.functional as F

    from gtsfm_amd.runtime import lib as L

    lib = L.load()
    gen = torch.Generator().manual_seed(1000 * h + w + cin)
    x = torch.randn((batch, cin, h, w), generator=gen)
    wt = torch.randn((cout, cin, 3, 3), generator=gen) * float(np.sqrt(2.0 / (9 * cin)))
    bias = torch.randn((cout,), generator=gen) * 0.1
    act = (lambda t: F.relu(t)) if relu else (lambda t: t)
    ref = act(F.conv2d(x, wt, bias, padding=2, dilation=2))
    ref64 = act(F.conv2d(x.double(), wt.double(), bias.double(), padding=2, dilation=2))
    packed = np.empty(lib.gtsfm_packed_conv3x3_floats(cin, cout), dtype=np.float32)
    L.check(lib.gtsfm_pack_conv3x3(wt.numpy().ctypes.data, cin, cout, packed.ctypes.data), "gtsfm_pack_conv3x3")
    bpad = torch.zeros((cout + 63) // 64 * 64)
    bpad[:cout] = bias
    xd = x.permute(0, 2, 3, 1).contiguous().cuda()
    out = torch.full((batch, h, w, cout + 8), 7.0, device="cuda")
    wd, bd = torch.from_numpy(packed).cuda(), bpad.cuda()  # named: a temporary's memory may be handed out again before the kernel reads it
    L.check(lib.gtsfm_conv3x3_dil2_f32(xd.data_ptr(), cin, 0, out.data_ptr(), cout + 8, 8, wd.data_ptr(), bd.data_ptr(), batch, h, w, cin, cout, relu,
                                       L.current_stream_handle()), "gtsfm_conv3x3_dil2_f32")
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.all(got[..., :8] == 7.0), "wrote outside its channels"
    got = got[..., 8:].permute(0, 3, 1, 2).double()
    scale = float(ref64.abs().max())
    err, err_ref = float((got - ref64).abs().max()) / scale, float((ref.double() - ref64).abs().max()) / scale
    print(f"dilated conv {cin}->{cout} {h}x{w}: GPU {err:.3e}, torch fp32 {err_ref:.3e} of the maximum")
    assert err <= 4 * err_ref + ULP


@pytest.mark.parametrize("name", CASES)
def test_stages_match_goldens(engine, goldens, name):
    g, image = goldens[name]
    for stage, key in ((0, "conv1"), (1, "conv3"), (2, "dense")):
        out = engine.stage([image], stage)
        if stage:
            assert tuple(out.shape) == tuple(int(v) for v in g[f"{key}_shape"][[0, 2, 3, 1]])
        got, want = out.cpu().reshape(-1).numpy()[g[f"{key}_idx"]], g[f"{key}_val"]
        scale = float(g["dense_max"]) if stage == 2 else float(np.abs(want).max())
        err, bound = float(np.abs(got - want).max()) / scale, 4 * float(g[f"{key}_err64"]) + ULP
        print(f"{name} stage {stage}: {err:.3e} of the maximum (bound {bound:.3e})")
        assert err <= bound, f"stage {stage}: {err} > {bound}"


@pytest.mark.parametrize("name", CASES)
def test_head_on_the_device_map_is_the_restatement_bit_for_bit(engine, goldens, name):
    _, image = goldens[name]
    dense = engine.stage([image], 2)
    found, cands, kps, scs, des = engine.detect_on_map(dense, max_keypoints=5000)
    want = dr.head(dense[0].permute(2, 0, 1).contiguous().cpu())
    idx, val = cands[0]
    assert int(found[0]) == len(want["cand"]) > 0
    assert np.array_equal(idx, want["cand"]) and np.array_equal(val[:, :2], want["steps"]) and np.array_equal(val[:, 2], want["cand_scores"])
    assert np.array_equal(kps[0], want["keypoints"]) and np.array_equal(scs[0], want["scores"])
    assert des[0].shape == want["descriptors"].shape and np.abs(des[0] - want["descriptors"]).max() <= DESC_HEAD_ATOL
    assert np.abs(np.linalg.norm(des[0].astype(np.float64), axis=1) - 1).max() < 1e-6


def handmade_map() -> np.ndarray:
    """A 10 x 12 x 512 map with one case per branch of the head (see the test below)."""
    m = np.zeros((10, 12, 512), np.float32)

    def bump(c, i, j, x, up, down, left, right, tl=0.0, tr=0.0, bl=0.0, br=0.0):
        for (di, dj), v in {(0, 0): x, (-1, 0): up, (1, 0): down, (0, -1): left, (0, 1): right, (-1, -1): tl, (-1, 1): tr, (1, -1): bl, (1, 1): br}.items():
            if 0 <= i + di < m.shape[0] and 0 <= j + dj < m.shape[1]:
                m[i + di, j + dj, c] = v

    bump(5, 0, 2, 4.0, 0.0, 2.5, 2.0, 2.0)             # on the border row: the step points into the map -> kept
    bump(6, 4, 0, 4.0, 2.0, 2.0, 0.0, 2.5)             # on the border column -> kept
    bump(7, 3, 4, 4.0, 3.9, 3.9, 1.0, 1.0, 3.9, 0.0, 0.0, 3.9)  # det <= 0
    bump(8, 3, 8, 4.0, 3.9, 3.9, 0.0, 0.0)             # a ridge: tr^2 / det = 42 > 7.2
    bump(9, 6, 3, 4.0, 0.0, 4.0, 2.0, 2.0, 0.0, 0.0, 2.0, 2.0)  # a plateau of two: step_i = 0.5 exactly at (6, 3) ...
    bump(9, 7, 3, 4.0, 4.0, 0.0, 2.0, 2.0, 2.0, 2.0, 0.0, 0.0)  # ... and -0.5 at (7, 3): |step| < 0.5 fails for both
    bump(12, 0, 7, 4.0, 0.0, -1.0, 2.0, 2.0)           # on the border row with the step pointing out: floor(i) = -1, corner test
    for c in (10, 11):                                 # two channels tie for the pixel's maximum: both are kept, channel 10 first
        bump(c, 7, 8, 4.0, 2.0, 2.4, 1.8, 2.2, 1.0, 0.6, 0.7, 1.3)
    return m


def test_head_on_a_handmade_map(engine):
    m = handmade_map()
    want = dr.head(torch.from_numpy(m).permute(2, 0, 1).contiguous())
    assert sorted(map(tuple, want["cand"].tolist())) == [(5, 0, 2), (6, 4, 0), (10, 7, 8), (11, 7, 8)]
    found, cands, kps, scs, des = engine.detect_on_map(m[None], max_keypoints=8)
    idx, val = cands[0]
    assert int(found[0]) == 4 and np.array_equal(idx, want["cand"])
    assert np.array_equal(val[:, :2], want["steps"]) and np.array_equal(val[:, 2], want["cand_scores"])
    assert np.array_equal(kps[0], want["keypoints"]) and np.array_equal(scs[0], want["scores"])
    assert np.abs(des[0] - want["descriptors"]).max() <= DESC_HEAD_ATOL
    # the tie: same score, same step, channel 10 before channel 11
    tie = [k for k, r in enumerate(idx.tolist()) if r[0] in (10, 11)]
    assert tie[1] == tie[0] + 1 and idx[tie[0], 0] == 10 and val[tie[0], 2] == val[tie[1], 2]
    # a batch of two maps (the second mirrored left to right) equals the maps one at a time
    m2 = np.ascontiguousarray(m[:, ::-1])
    fb, cb, *_ = engine.detect_on_map(np.stack([m, m2]))
    f2, c2, *_ = engine.detect_on_map(m2[None])
    assert np.array_equal(cb[0][0], idx) and np.array_equal(cb[0][1], val) and np.array_equal(cb[1][0], c2[0][0]) and np.array_equal(cb[1][1], c2[0][1])
    assert fb.tolist() == [4, int(f2[0])]


@pytest.mark.parametrize("name", CASES)
def test_end_to_end_against_goldens(engine, goldens, name):
    g, image = goldens[name]
    xy, sc, de = engine.detect(image, 5000)
    n_found, (idx, _) = _candidates(engine, image)
    assert len(xy) == len(sc) == len(de) == n_found == len(idx) and xy.dtype == sc.dtype == de.dtype == np.float32 and de.shape[1] == 512
    ia, ib = _match(idx, g["cand"])
    unmatched = max(len(idx) - len(ia), len(g["cand"]) - len(ib))
    print(f"{name}: {len(idx)} keypoints, golden {len(g['cand'])}, unmatched {unmatched}")
    assert unmatched <= MAX_UNMATCHED * len(g["cand"])
    smax = float(np.abs(g["scores"]).max())
    e_xy = float(np.abs(xy[ia] - g["keypoints"][ib]).max())
    e_sc = float(np.abs(sc[ia] - g["scores"][ib]).max()) / smax
    e_de = float(np.abs(de[ia][:, g["desc_cols"]] - g["descriptors"][ib]).max())
    b_xy = 4 * float(g["kp_err64"]) + float(np.spacing(np.float32(max(image.shape[:2]))))
    b_sc, b_de = 4 * float(g["score_err64"]) + ULP, 4 * float(g["desc_err64"]) + ULP
    print(f"{name}: coordinates {e_xy:.3e} px (bound {b_xy:.3e}), scores {e_sc:.3e} (bound {b_sc:.3e}), descriptors {e_de:.3e} (bound {b_de:.3e})")
    assert e_xy <= b_xy and e_sc <= b_sc and e_de <= b_de


@pytest.mark.parametrize("k", [10, 100])
def test_max_keypoints_truncation(engine, goldens, full_240, k):
    g, image = goldens["d2net_240x320"]
    xy_full, sc_full, de_full = full_240
    xy, sc, de = engine.detect(image, k)
    assert len(xy) == k < len(xy_full)
    # exactly the head of the device's own sorted list
    assert np.array_equal(xy, xy_full[:k]) and np.array_equal(sc, sc_full[:k]) and np.array_equal(de, de_full[:k])
    # the order: scores non-increasing, equal scores by (channel, i, j)
    _, (idx, val) = _candidates(engine, image)
    assert np.array_equal(val[:k, 2], sc) and np.all(np.diff(val[:, 2]) <= 0)
    lin = (idx[:, 0].astype(np.int64) * 10**4 + idx[:, 1]) * 10**4 + idx[:, 2]
    assert np.all((np.diff(val[:, 2]) < 0) | (np.diff(lin) > 0))
    # against the golden's first k: a keypoint may differ only if its score lies within the score tolerance of the k-th score
    tol = (4 * float(g["score_err64"]) + ULP) * float(np.abs(g["scores"]).max())
    ours, theirs = set(map(tuple, idx[:k].tolist())), set(map(tuple, g["cand"][:k].tolist()))
    kth = float(g["scores"][k - 1])
    score_of = {tuple(r): float(s) for r, s in zip(idx.tolist(), val[:, 2])}
    score_of_golden = {tuple(r): float(s) for r, s in zip(g["cand"].tolist(), g["scores"])}
    for r in ours - theirs:
        assert abs(score_of[r] - kth) <= tol, (r, score_of[r], kth)
    for r in theirs - ours:
        assert abs(score_of_golden[r] - kth) <= tol, (r, score_of_golden[r], kth)


def test_batch_equals_single_and_repeatable(engine, goldens):
    _, image = goldens["d2net_123x157"]
    images = [image, dr.seeded_image(41, 123, 157), np.ascontiguousarray(image[::-1])]
    batch = engine.detect_batch(images, 5000)
    again = engine.detect_batch(images, 5000)
    assert len(batch) == 3
    for i, im in enumerate(images):
        single = engine.detect(im, 5000)
        assert len(batch[i][0]) > 0
        for a, b, c in zip(batch[i], single, again[i]):
            assert np.array_equal(a, b), f"image {i}: batched != alone"
            assert np.array_equal(a, c), f"image {i}: two runs differ"
    dense = engine.stage(images, 2)
    assert torch.equal(dense[1:2], engine.stage(images[1:2], 2))
    top = engine.detect_batch(images, 7)
    assert all(np.array_equal(t[2], b[2][:7]) for t, b in zip(top, batch))


def test_gray_and_float_inputs(engine, goldens):
    _, image = goldens["d2net_64x80"]
    gray = np.ascontiguousarray(image[:, :, 1])
    stacked = np.repeat(gray[:, :, None], 3, -1)
    assert torch.equal(engine.stage([gray], 0), engine.stage([stacked], 0))
    for a, b in zip(engine.detect(gray, 5000), engine.detect(stacked, 5000)):
        assert np.array_equal(a, b) and len(a) > 0
    for dtype in (np.float32, np.float64, np.int32):
        assert torch.equal(engine.stage([image.astype(dtype)], 0), engine.stage([image], 0)), dtype
        for a, b in zip(engine.detect(image.astype(dtype), 5000), engine.detect(image, 5000)):
            assert np.array_equal(a, b)
    for a, b in zip(engine.detect(gray.astype(np.float32), 5000), engine.detect(gray, 5000)):
        assert np.array_equal(a, b)


def test_candidate_list_overflow_is_reported_and_recovered(engine, goldens):
    from gtsfm_amd.runtime import lib as L

    g, image = goldens["d2net_64x80"]
    want = engine.detect(image, 5000)
    n = len(want[0])
    assert n == len(g["cand"]) > 5
    # the ABI with a deliberately small capacity: the count it reports is the capacity the call needs
    found, partial = _candidates(engine, image, cap=5)
    assert found == n and len(partial[0]) == 5
    full_found, (idx, val) = _candidates(engine, image, cap=found)
    assert full_found == n and np.array_equal(val[:, 2], want[1])
    dev = torch.from_numpy(image[None]).cuda()
    counts = torch.zeros(1, dtype=torch.int32, device="cuda")
    kp, sc, de = (torch.zeros(s, device="cuda") for s in ((1, 8, 2), (1, 8), (1, 8, 512)))
    ws = torch.empty(int(L.load().gtsfm_d2net_workspace_bytes(1, 64, 80, 5)), dtype=torch.uint8, device="cuda")
    rc = L.load().gtsfm_d2net_forward(engine._weights.data_ptr(), dev.data_ptr(), 1, 1, 64, 80, 8, 5, counts.data_ptr(), kp.data_ptr(), sc.data_ptr(),
                                      de.data_ptr(), ws.data_ptr(), ws.numel(), L.current_stream_handle())
    assert rc == 0 and int(counts.item()) == n
    # the engine recovers: one repeated launch, the same result
    before = engine.relaunches
    got = engine.detect(image, 5000, cand_capacity=5)
    assert engine.relaunches == before + 1
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    # a too small workspace and an invalid shape are refused before any launch
    assert L.load().gtsfm_d2net_forward(engine._weights.data_ptr(), dev.data_ptr(), 1, 1, 64, 80, 8, 5, counts.data_ptr(), kp.data_ptr(), sc.data_ptr(),
                                        de.data_ptr(), ws.data_ptr(), 1024, L.current_stream_handle()) != 0
    with pytest.raises(RuntimeError, match="8 x 8"):
        engine.detect(np.zeros((7, 40, 3), np.uint8))


def test_plugin_through_cacher_and_twoway_matcher(tmp_path, weights):
    from gtsfm_amd.common.image import Image
    from gtsfm_amd.frontend.cacher.detector_descriptor_cacher import DetectorDescriptorCacher
    from gtsfm_amd.frontend.detector_descriptor import D2NetDetDesc
    from gtsfm_amd.frontend.matcher.twoway_matcher import TwoWayMatcher

    checkpoint = tmp_path / "d2_tf.pth"
    torch.save({"model": weights}, str(checkpoint))
    plugin = pickle.loads(pickle.dumps(D2NetDetDesc(max_keypoints=200, model_path=checkpoint)))
    cacher = DetectorDescriptorCacher(plugin, cache_root=tmp_path / "cache")
    scene = dr.seeded_image(31, 128, 200)
    views = [np.ascontiguousarray(scene[:, :160]), np.ascontiguousarray(scene[:, 40:])]  # a shift of 40 px = 10 map pixels
    feats = [cacher.detect_and_describe(Image(value_array=v)) for v in views]
    for (kps, desc), view in zip(feats, views):
        want = dr.forward(weights, view, max_keypoints=200)
        assert kps.coordinates.dtype == np.float32 and kps.coordinates.shape == (len(kps), 2) and desc.shape == (len(kps), 512) and desc.dtype == np.float32
        assert 0 < len(kps) <= 200 and kps.responses.shape == (len(kps),) and np.all(np.diff(kps.responses) <= 0)
        assert abs(len(kps) - len(want["keypoints"])) <= 2
    assert len(list((tmp_path / "cache" / "detector_descriptor").glob("D2NetDetDesc_*.pbz2"))) == 2
    again = cacher.detect_and_describe(Image(value_array=views[0]))  # a cache hit returns what was stored
    assert np.array_equal(again[0].coordinates, feats[0][0].coordinates) and np.array_equal(again[1], feats[0][1])
    matcher = TwoWayMatcher(ratio_test_threshold=0.8)
    (k0, d0), (k1, d1) = feats
    m01 = matcher.match(k0, k1, d0, d1, views[0].shape, views[1].shape)
    m10 = matcher.match(k1, k0, d1, d0, views[1].shape, views[0].shape)
    assert len(m01) > 0 and m01.shape[1] == 2
    assert sorted(map(tuple, m01.tolist())) == sorted((b, a) for a, b in m10.tolist()), "the two-way matches are not symmetric"
    # matched keypoints of the overlap lie 40 px apart
    shift = k0.coordinates[m01[:, 0]] - k1.coordinates[m01[:, 1]]
    assert np.median(np.abs(shift - np.array([40.0, 0.0])).max(axis=1)) < 1.0


def test_accuracy_against_float64(engine, weights, goldens):
    """max |GPU - float64| <= 4 x max |fp32 restatement - float64| (+ a floor) for the dense map, the coordinates, the scores and the descriptors."""
    g, image = goldens["d2net_123x157"]
    s64: dict = {}
    f64 = dr.forward(weights, image, dtype=torch.float64, stages=s64)
    dense64 = s64["dense"][0].permute(1, 2, 0).numpy()
    gpu_dense = engine.stage([image], 2)[0].cpu().numpy().astype(np.float64)
    err_map = float(np.abs(gpu_dense - dense64).max() / np.abs(dense64).max())
    print(f"dense map: GPU {err_map:.3e}, fp32 restatement {float(g['dense_err64']):.3e} of the maximum")
    assert err_map <= 4 * float(g["dense_err64"]) + ULP
    xy, sc, de = engine.detect(image, 5000)
    _, (idx, _) = _candidates(engine, image)
    ia, ib = _match(idx, f64["cand"])
    assert max(len(idx) - len(ia), len(f64["cand"]) - len(ib)) <= MAX_UNMATCHED * len(f64["cand"])
    smax = float(np.abs(f64["scores"]).max())
    e_xy = float(np.abs(xy[ia] - f64["keypoints"][ib]).max())
    e_sc = float(np.abs(sc[ia] - f64["scores"][ib]).max()) / smax
    e_de = float(np.abs(de[ia] - f64["descriptors"][ib]).max())
    print(f"GPU against float64: coordinates {e_xy:.3e} px (fp32 restatement {float(g['kp_err64']):.3e}), scores {e_sc:.3e} ({float(g['score_err64']):.3e}), "
          f"descriptors {e_de:.3e} ({float(g['desc_err64']):.3e})")
    assert e_xy <= 4 * float(g["kp_err64"]) + float(np.spacing(np.float32(157.0)))
    assert e_sc <= 4 * float(g["score_err64"]) + ULP and e_de <= 4 * float(g["desc_err64"]) + ULP
