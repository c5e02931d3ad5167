"""GPU: TwoWayMatcher (mutual nearest neighbour + ratio test, ``gtsfm_twoway_match``) against the reference's known answers, the
recorded Lund-door SIFT expectations and the restatement in tests/twoway_reference.py: bit-exact on integer data (order included),
decision-exact beyond a 1e-5 relative margin on real-valued data; independent of the batch a pair is launched in and of the run."""

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.test_twoway_host import DESC_1, DESC_2, EXPECTED_NO_RATIO, EXPECTED_RATIO_0_8
from tests.twoway_reference import EUCLIDEAN, HAMMING, twoway_match, twoway_valid

pytestmark = pytest.mark.gpu

SHAPE = (480, 640, 3)


@pytest.fixture(scope="module")
def engine(gpu_device):
    from gtsfm_amd.runtime.twoway_engine import TwoWayEngine

    return TwoWayEngine(gpu_device)


def _plugin(ratio=None, hamming=False):
    from gtsfm_amd.frontend.matcher.twoway_matcher import MatchingDistanceType, TwoWayMatcher

    return TwoWayMatcher(MatchingDistanceType.HAMMING if hamming else MatchingDistanceType.EUCLIDEAN, ratio)


def _match(matcher, d1, d2):
    return matcher.match(None, None, d1, d2, SHAPE, SHAPE)


@pytest.mark.parametrize("ratio,expected", [(0.8, EXPECTED_RATIO_0_8), (None, EXPECTED_NO_RATIO)])
def test_reference_known_answers(gpu_device, ratio, expected):
    got = _match(_plugin(ratio), DESC_1, DESC_2)
    assert got.dtype == np.uint32
    assert np.array_equal(got, np.array(expected)), got.tolist()


@pytest.fixture(scope="module")
def lund():
    return np.load(GOLDEN / "twoway_lund_door_sift.npz")


@pytest.mark.parametrize("as_u8", [False, True], ids=["float32", "uint8"])
@pytest.mark.parametrize("ratio,key", [(0.8, "expected_ratio_0_8"), (None, "expected_no_ratio")])
def test_lund_door_sift_bit_exact(gpu_device, lund, as_u8, ratio, key):
    d0, d1 = lund["descriptors_0"], lund["descriptors_1"]
    if not as_u8:
        d0, d1 = d0.astype(np.float32), d1.astype(np.float32)
    got = _match(_plugin(ratio), d0, d1)
    assert got.dtype == np.uint32 and np.array_equal(got, lund[key]), f"{len(got)} vs {len(lund[key])} matches"


def test_lund_door_distances_are_the_correctly_rounded_sqrtf(engine, lund):
    import torch

    d0, d1 = lund["descriptors_0"], lund["descriptors_1"]
    table = torch.from_numpy(np.concatenate([d0, d1])).to(engine.device)
    m0, dist0 = engine.match_raw(table, 128, [(0, 5000, 5000, 5000)], EUCLIDEAN, None)
    m0, dist0 = m0.cpu().numpy(), dist0.cpu().numpy()
    ok = m0 >= 0  # kept rows: m0 is the nearest neighbour
    e = ((d0[ok].astype(np.int64) - d1[m0[ok]].astype(np.int64)) ** 2).sum(1)
    want = np.sqrt(e.astype(np.float32))
    assert np.array_equal(dist0[ok].view(np.int32), want.view(np.int32))
    assert ok.sum() == len(lund["expected_no_ratio"])


def _integer_data(rng, n1, n2, d, hi):
    a = rng.integers(0, hi, size=(n1, d)).astype(np.float32)
    b = rng.integers(0, hi, size=(n2, d)).astype(np.float32)
    k = min(n1, n2) // 3
    b[:k] = a[rng.permutation(n1)[:k]]  # zero-distance partners
    if n2 > 4:
        b[n2 // 2] = b[n2 // 2 + 1]  # exact duplicates on the B side
    return a, b


@pytest.mark.parametrize("n1,n2", [(1, 1), (2, 2), (31, 129), (129, 31), (300, 257), (5000, 2)])
@pytest.mark.parametrize("d", [1, 3, 32, 64, 128, 256, 512])
def test_integer_data_bit_exact_with_ties(gpu_device, n1, n2, d):
    rng = np.random.default_rng(n1 * 1000 + n2 * 10 + d)
    a, b = _integer_data(rng, n1, n2, d, 3 if d > 8 else 6)
    for ratio in (None, 0.8, 1.0):
        if ratio is not None and min(n1, n2) < 2:
            with pytest.raises(ValueError):
                _match(_plugin(ratio), a, b)
            continue
        want = twoway_match(a, b, ratio=ratio)
        got = _match(_plugin(ratio), a, b)
        assert got.dtype == want.dtype and np.array_equal(got, want), (n1, n2, d, ratio)


def test_inclusive_zero_ratio_case(gpu_device):
    a = np.array([[0, 0], [5, 5]], np.float32)
    b = np.array([[20, 20], [0, 0], [0, 0]], np.float32)
    assert np.array_equal(_match(_plugin(0.8), a, b), np.array([[0, 1]]))
    assert np.array_equal(_match(_plugin(0.8), a.astype(np.uint8), b.astype(np.uint8)), np.array([[0, 1]]))


def test_sift_sized_integer_data_5000(gpu_device, lund):
    rng = np.random.default_rng(11)
    a = lund["descriptors_0"].astype(np.float32)
    b = np.concatenate([lund["descriptors_1"][:4000].astype(np.float32), a[rng.permutation(5000)[:1000]]])  # 1000 exact duplicates
    for ratio in (None, 0.8):
        assert np.array_equal(_match(_plugin(ratio), a, b), twoway_match(a, b, ratio=ratio))


@pytest.mark.parametrize("nbytes", [32, 64])
@pytest.mark.parametrize("ratio", [None, 0.8])
def test_hamming_bit_exact(gpu_device, nbytes, ratio):
    rng = np.random.default_rng(nbytes)
    a = rng.integers(0, 256, size=(700, nbytes), dtype=np.uint8)
    b = rng.integers(0, 256, size=(650, nbytes), dtype=np.uint8)
    b[:100] = a[:100]
    b[200:260] ^= (rng.random((60, nbytes)) < 0.05).astype(np.uint8)  # near-duplicates: many equal distances
    want = twoway_match(a, b, HAMMING, ratio)
    got = _match(_plugin(ratio, hamming=True), a, b)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n1,n2,d", [(3000, 2500, 256), (1500, 1700, 64), (1000, 900, 512), (5000, 4800, 256)])
@pytest.mark.parametrize("ratio", [None, 0.8])
def test_real_valued_decisions_beyond_margin(gpu_device, n1, n2, d, ratio):
    rng = np.random.default_rng(n1 + d)
    a = rng.standard_normal((n1, d)).astype(np.float32)
    b = np.concatenate([a[:n2 // 2] + 0.05 * rng.standard_normal((n2 // 2, d)).astype(np.float32),
                        rng.standard_normal((n2 - n2 // 2, d)).astype(np.float32)])
    if d == 256:  # SuperPoint-like: unit norm
        a /= np.linalg.norm(a, axis=1, keepdims=True)
        b /= np.linalg.norm(b, axis=1, keepdims=True)
    want, margin = twoway_valid(a, b, EUCLIDEAN, ratio, with_margins=True)
    got = _match(_plugin(ratio), a, b)
    got_map = dict(zip(got[:, 0].tolist(), got[:, 1].tolist())) if got.size else {}
    want_map = dict(zip(want[:, 0].tolist(), want[:, 1].tolist()))
    confident = margin > 1e-5
    disagree = [i for i in np.flatnonzero(confident) if got_map.get(int(i)) != want_map.get(int(i))]
    print(f"{n1}x{n2}x{d} ratio={ratio}: {len(want)} reference matches, {len(got)} GPU matches, "
          f"{int((~confident).sum())} rows within the margin, {len(disagree)} disagreements beyond it")
    assert len(disagree) == 0
    assert len(want) > 0


def test_nan_rows_and_empty_sides(gpu_device):
    rng = np.random.default_rng(4)
    a, b = _integer_data(rng, 200, 150, 16, 4)
    a[[0, 7, 199]] = np.nan
    b[[3, 149]] = np.nan
    for ratio in (None, 0.8):
        assert np.array_equal(_match(_plugin(ratio), a, b), twoway_match(a, b, ratio=ratio))
    for d1, d2 in [(np.array([]), b), (a, np.zeros((0, 16), np.float32)), (np.full((3, 16), np.nan, np.float32), b)]:
        out = _match(_plugin(), d1, d2)
        assert out.shape == (0,) and out.dtype == np.float64


def test_batch_composition_and_run_to_run_bit_identical(engine):
    import torch

    rng = np.random.default_rng(8)
    sizes = [int(x) for x in rng.integers(1, 700, size=64)]
    sizes[10], sizes[11] = 2000, 1900
    rows = [rng.standard_normal((n, 128)).astype(np.float32) for n in sizes]
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    table = torch.from_numpy(np.concatenate(rows)).to(engine.device)
    pairs = [(int(offsets[2 * p]), sizes[2 * p], int(offsets[2 * p + 1]), sizes[2 * p + 1]) for p in range(32)]
    pairs = [p for p in pairs if min(p[1], p[3]) >= 2]
    for ratio in (None, 0.8):
        m_all, d_all = (t.cpu().numpy() for t in engine.match_raw(table, 128, pairs, EUCLIDEAN, ratio))
        m_again, d_again = (t.cpu().numpy() for t in engine.match_raw(table, 128, pairs, EUCLIDEAN, ratio))
        assert np.array_equal(m_all, m_again) and np.array_equal(d_all.view(np.int32), d_again.view(np.int32))
        start = 0
        for p in pairs:
            m1, d1 = (t.cpu().numpy() for t in engine.match_raw(table, 128, [p], EUCLIDEAN, ratio))
            assert np.array_equal(m1, m_all[start : start + p[1]]) and np.array_equal(d1.view(np.int32), d_all[start : start + p[1]].view(np.int32))
            start += p[1]


def test_batched_generator_matches_the_per_pair_plugin(gpu_device, tmp_path):
    """BatchedDetDescCorrespondenceGenerator with a TwoWayMatcher (all edges from the resident descriptor table in one launch) vs
    per-image / per-pair plugin calls, edge by edge: same arrays, dtype and empty convention."""
    import torch

    from gtsfm_amd.common.image import Image
    from gtsfm_amd.frontend.correspondence_generator.batched_det_desc_correspondence_generator import BatchedDetDescCorrespondenceGenerator
    from gtsfm_amd.frontend.detector_descriptor.superpoint import SuperPointDetectorDescriptor
    from gtsfm_amd.utils import synthetic

    torch.save(synthetic.synthetic_superpoint_state_dict(), str(tmp_path / "sp.pth"))
    images = [Image(value_array=synthetic.synthetic_gray_image(160, 200, s)) for s in (81, 82, 83)]
    images.append(Image(value_array=synthetic.synthetic_gray_image(120, 176, 84)))
    graph = [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3), (0, 3)]
    det = SuperPointDetectorDescriptor(max_keypoints=300, weights_path=tmp_path / "sp.pth")
    host = []
    for im in images:
        kp, d = det.detect_and_describe(im)
        order = np.lexsort((kp.coordinates[:, 0], kp.coordinates[:, 1]))  # the plugin's top-k order is argpartition's
        host.append((kp.extract_indices(order), d[order]))
    for ratio in (None, 0.8):
        matcher = _plugin(ratio)
        kps, corr = BatchedDetDescCorrespondenceGenerator(matcher, det).generate_correspondences(None, images, graph)
        assert sorted(corr) == sorted(graph)
        for i in range(4):
            assert len(kps[i]) > 10 and kps[i] == host[i][0]
        for i, j in graph:
            ref = _plugin(ratio).match(host[i][0], host[j][0], host[i][1], host[j][1], SHAPE, SHAPE)
            assert corr[(i, j)].dtype == ref.dtype and np.array_equal(corr[(i, j)], ref), (i, j, ratio)
        assert any(len(corr[p]) > 0 for p in graph)


def test_batch_with_partials_beyond_2_31_entries(engine):
    """10 800 pairs of 5000 x 5000 in ONE call: their column partials (40 row blocks x 5000 columns per pair) number 2.16e9 > 2^31,
    so the offsets of the last pairs only fit in 64 bits. Every pair's block equals that pair matched alone."""
    import torch

    rng = np.random.default_rng(21)
    n, d, n_img = 5000, 8, 4
    host = rng.integers(0, 6, size=(n_img * n, d)).astype(np.float32)
    table = torch.from_numpy(host).to(engine.device)
    combos = [(i, j) for i in range(n_img) for j in range(n_img) if i != j]
    alone = {}
    for i, j in combos:
        m, dist = engine.match_raw(table, d, [(i * n, n, j * n, n)], EUCLIDEAN, 0.8)
        alone[(i, j)] = (m.cpu().numpy(), dist.cpu().numpy())
    npairs = 10800
    assert npairs * 40 * n > 2**31
    spec = [(combos[p % len(combos)][0] * n, n, combos[p % len(combos)][1] * n, n) for p in range(npairs)]
    m_all, d_all = engine.match_raw(table, d, spec, EUCLIDEAN, 0.8)
    m_all = m_all.view(npairs, n)
    d_all = d_all.view(npairs, n)
    for k, (i, j) in enumerate(combos):
        m1 = torch.from_numpy(alone[(i, j)][0]).to(engine.device)
        d1 = torch.from_numpy(alone[(i, j)][1]).to(engine.device)
        rows = torch.arange(k, npairs, len(combos), device=engine.device)
        assert torch.equal(m_all[rows], m1.expand(len(rows), n)), (i, j)
        assert torch.equal(d_all[rows].view(torch.int32), d1.view(torch.int32).expand(len(rows), n)), (i, j)
    assert int((m_all[-1] >= 0).sum()) > 0
    engine._ws = None  # give the large workspace back
    del m_all, d_all
    torch.cuda.empty_cache()


def test_batched_generator_pair_batch_does_not_change_results(gpu_device):
    """match_table in launches of pair_batch edges: the same arrays for any batch size."""
    import torch

    from gtsfm_amd.runtime.twoway_engine import TwoWayEngine

    rng = np.random.default_rng(5)
    counts = [700, 650, 0, 512, 3, 690]
    base = rng.standard_normal((700, 256)).astype(np.float32)
    views = base[None] + 0.05 * rng.standard_normal((6, 700, 256)).astype(np.float32)  # overlapping views: real matches
    table = torch.from_numpy(np.ascontiguousarray(views[:, rng.permutation(700)])).to(gpu_device)
    graph = [(i, j) for i in range(6) for j in range(i + 1, 6)]
    eng = TwoWayEngine(gpu_device)
    want = eng.match_table(table, counts, graph, ratio=0.9, pair_batch=len(graph))
    for batch in (1, 4):
        got = eng.match_table(table, counts, graph, ratio=0.9, pair_batch=batch)
        assert list(got) == list(want)
        for p in graph:
            assert got[p].dtype == want[p].dtype and np.array_equal(got[p], want[p]), (batch, p)
    assert want[(0, 2)].shape == (0,) and any(len(want[p]) > 0 for p in graph)
