"""GPU: the explicit float32 functions behind SIFT's byte-identity contract (``sift_exp2``, ``sift_exp``, ``sift_atan2_deg``,
``sift_sincos_deg``, ``sift_solve3``, ``sift_reflect101``, ``sift_peak_angle`` of ``gtsfm_amd/csrc/sift_kernels.hip``), applied element-wise
through ``gtsfm_sift_math`` and compared bit for bit with their numpy twins in ``tests/sift_reference.py`` on dense and edge inputs. This is
where the branches that no image reaches are executed on the device: an arc tangent of exactly 360, an interpolated bin of 36 or more, an
angle of 360 set to 0 (``tests/test_sift_census_host.py``: ``UNREACHABLE``)."""

import numpy as np
import pytest

import sift_constructed as C
import sift_reference as S

pytestmark = pytest.mark.gpu

F = np.float32
EXP2, EXP, ATAN2, SINCOS, SOLVE3, REFLECT101, PEAK = range(7)


@pytest.fixture(scope="module")
def apply(gpu_device):
    import torch

    from gtsfm_amd.runtime import lib as L

    lib = L.load()

    def run(fn, inp, out_words, out_dtype=np.float32):
        inp = np.ascontiguousarray(inp)
        assert inp.dtype.itemsize == 4
        n = len(inp)
        src = torch.from_numpy(inp.view(np.int32).reshape(-1)).to(gpu_device)
        dst = torch.full((n * out_words,), -7, dtype=torch.int32, device=gpu_device)
        L.check(lib.gtsfm_sift_math(fn, src.data_ptr(), dst.data_ptr(), n, L.current_stream_handle()), "gtsfm_sift_math")
        out = dst.cpu().numpy().view(out_dtype)
        return out.reshape(n, out_words) if out_words > 1 else out

    return run


def _differing(got, want):
    """Indices where two float32 arrays differ in their bits, NaNs of any payload counting as equal."""
    got, want = np.asarray(got, dtype=F), np.asarray(want, dtype=F)
    assert got.shape == want.shape
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    return np.argwhere(~same)


def test_exp2_and_exp(apply):
    halves = np.arange(-300, 5, dtype=np.float64) / 2.0  # the rint ties, -150 .. +2
    t = np.concatenate([halves, np.nextafter(halves.astype(F), F(np.inf)), np.nextafter(halves.astype(F), F(-np.inf)), np.linspace(-150.0, 2.0, 20001),
                        [0.0, -0.0]]).astype(F)
    with np.errstate(all="ignore"):
        want2, want = S.exp2_f32(t), S.exp_f32(t)
    bad2, bad = _differing(apply(EXP2, t, 1), want2), _differing(apply(EXP, t, 1), want)
    print(f"exp2: {len(t)} inputs, {len(bad2)} differ; exp: {len(bad)} differ")
    assert len(bad2) == 0, (t[bad2[:4, 0]], want2[bad2[:4, 0]])
    assert len(bad) == 0, (t[bad[:4, 0]], want[bad[:4, 0]])


def test_atan2_deg(apply):
    rng = np.random.default_rng(21)
    tiny = np.float32(1e-5)
    edge = [(0, 1), (1, 0), (0, -1), (-1, 0), (-tiny, 200), (-tiny, 28), (-tiny, -200), (tiny, 200), (-1e-30, 1), (1, 1), (-1, 1), (1, -1), (-1, -1),
            (3.5, 3.5), (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (-0.0, 1.0), (1.0, -0.0), (255, 255), (1e-38, 1e-38)]
    ang = np.radians(np.arange(0, 1440) / 4.0)
    yx = np.concatenate([np.array(edge, dtype=F), np.stack([np.sin(ang), np.cos(ang)], 1).astype(F) * F(37.0),
                         (rng.standard_normal((4096, 2)) * rng.choice([1e-4, 1.0, 200.0], size=(4096, 1))).astype(F)])
    want = S.atan2_deg(yx[:, 0].copy(), yx[:, 1].copy())
    got = apply(ATAN2, yx, 1)
    bad = _differing(got, want)
    print(f"atan2: {len(yx)} inputs, {len(bad)} differ, {int((want == 360).sum())} are exactly 360")
    assert (want == F(360.0)).sum() >= 2  # the branch no orientation window of a photograph reaches
    assert len(bad) == 0, (yx[bad[:4, 0]], got[bad[:4, 0]], want[bad[:4, 0]])


def test_sincos_deg(apply):
    a = (np.arange(0, 1441) / 4.0).astype(F)  # every multiple of 0.25 degrees in [0, 360]
    want = np.array([S.sincos_deg(v) for v in a], dtype=F)
    got = apply(SINCOS, a, 2)
    bad = _differing(got, want)
    print(f"sincos: {len(a)} angles, {len(bad)} values differ")
    assert len(bad) == 0, (a[bad[:4, 0]], got[bad[:4, 0]], want[bad[:4, 0]])


def test_solve3(apply):
    rng = np.random.default_rng(5)  # the systems of test_solve3_pivots_and_reports_singular_systems_as_zero
    a = rng.standard_normal((64, 3, 3)).astype(F)
    a[0] = [[0, 1, 2], [3, 0, 1], [1, 1, 0]]
    a[1] = 0
    b = rng.standard_normal((64, 3)).astype(F)
    rng = np.random.default_rng(6)
    more_a, more_b = rng.standard_normal((4096, 3, 3)).astype(F), rng.standard_normal((4096, 3)).astype(F)
    # near-singular: a pivot just below and just above 10 FLT_EPSILON at each elimination step, and rank-deficient matrices
    near_a, near_b = rng.standard_normal((96, 3, 3)).astype(F), rng.standard_normal((96, 3)).astype(F)
    for i, scale in enumerate((1.1e-6, 1.3e-6)):
        near_a[i * 16 : i * 16 + 16, :, 0] *= F(scale)  # the first column: pivot 0
        near_a[32 + i * 16 : 48 + i * 16, 1:, 1:] *= F(scale)
        near_a[32 + i * 16 : 48 + i * 16, 1:, 0] = 0  # pivot 1
    near_a[64:80, 2] = near_a[64:80, 0] + near_a[64:80, 1]  # rank 2: the last pivot is rounding noise
    near_a[80:96, 1] = near_a[80:96, 0] * F(2.0)  # two proportional rows: pivot 1 is exactly 0 after the exchange
    a, b = np.concatenate([a, near_a, more_a]), np.concatenate([b, near_b, more_b])
    want, singular, exchanged = C.trace_solve3(a, b)
    got = apply(SOLVE3, np.concatenate([a.reshape(-1, 9), b], axis=1), 3)
    bad = _differing(got, want)
    print(f"solve3: {len(a)} systems, {int(singular.sum())} singular, row exchanges at pivot 0 / 1: {int(exchanged[:, 0].sum())} / {int(exchanged[:, 1].sum())}, "
          f"{len(np.unique(bad[:, 0]))} systems differ")
    assert singular[1] and singular.sum() >= 16 and exchanged[0, 0] and exchanged[:, 1].sum() > 100
    assert np.array_equal(want[1], np.zeros(3, dtype=F))
    assert len(bad) == 0, (a[bad[:2, 0]], got[bad[:2, 0]], want[bad[:2, 0]])


def test_reflect101(apply):
    table = np.stack([np.arange(-7, 9), np.full(16, 3)], axis=1).astype(np.int32)
    got = apply(REFLECT101, table, 1, np.int32)
    assert np.array_equal(got, [1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0])  # the table asserted on the host
    rows = [(p, n) for n in (1, 2, 3, 5, 6, 12, 13, 200) for p in range(-3 * n - 15, 4 * n + 16)]
    pn = np.array(rows, dtype=np.int32)
    want = np.concatenate([S.reflect101(pn[pn[:, 1] == n, 0].astype(np.int64), int(n)) for n in (1, 2, 3, 5, 6, 12, 13, 200)])
    got = apply(REFLECT101, pn, 1, np.int32)
    print(f"reflect101: {len(pn)} index / length pairs, {int((got != want).sum())} differ")
    assert np.array_equal(got, want)
    assert np.array_equal(apply(REFLECT101, np.array([(0, 0), (1, -4), (1 << 25, 8)], dtype=np.int32), 1, np.int32), [-1, -1, -1])


def test_peak_angle(apply):
    rng = np.random.default_rng(9)
    hand = [(0, 1.0, 2.0, 0.5),  # bin < 0: wraps to 36 + bin
            (0, 1.0, 2.0, 0.99999994),  # bin a hair below 0: 36 + bin rounds to 36, the angle is 0
            (35, 3.0, 1.75, 1.0),  # no peak, but the only way to a bin >= 36: 35 + 2 wraps to 1
            (35, 0.5, 2.0, 1.0),  # a true peak at the last bin stays below 36
            (0, 1.0, 2.0, 1.0),  # bin exactly 0: 360 is set to 0
            (0, 1.0, 2.0, 1.0000001),  # bin 3e-8: 360 - 10 bin rounds to 360 and is set to 0
            (18, 0.25, 0.75, 0.5), (1, 0.0, 1.0, 0.0), (7, 1.0, 1.0, 1.0)]  # the last: 0 / 0
    j = np.concatenate([[h[0] for h in hand], rng.integers(0, 36, 4096)]).astype(np.int32)
    tri = rng.uniform(0.0, 1.0, (4096, 3)).astype(F)
    tri[:2048, 1] = np.maximum(tri[:2048, 0], tri[:2048, 2]) + rng.uniform(1e-4, 1.0, 2048).astype(F)  # half of them true peaks
    tri = np.concatenate([np.array([h[1:] for h in hand], dtype=F), tri])
    packed = np.empty((len(j), 4), dtype=np.int32)
    packed[:, 0], packed[:, 1:] = j, tri.view(np.int32)
    twin = [C.peak_angle(int(jj), *t) for jj, t in zip(j, tri)]
    want = np.array([t[0] for t in twin], dtype=F)
    raw, before = np.array([t[1] for t in twin], dtype=F), np.array([t[2] for t in twin], dtype=F)
    got = apply(PEAK, packed, 1)
    bad = _differing(got, want)
    below, above, zeroed = int((raw < 0).sum()), int((raw >= 36).sum()), int((np.abs(before - F(360.0)) < S.FLT_EPSILON).sum())
    print(f"peak angle: {len(j)} triples, bin < 0: {below}, bin >= 36: {above}, 360 set to 0: {zeroed}, {len(bad)} differ")
    assert raw[0] < 0 and raw[2] >= 36 and want[2] == F(350.0) and raw[4] == 0 and want[4] == 0 and before[4] == 360 and want[5] == 0 and want[1] == 0
    assert below > 20 and above > 0 and zeroed >= 2  # the inputs do reach every branch
    assert len(bad) == 0, (j[bad[:4, 0]], tri[bad[:4, 0]], got[bad[:4, 0]], want[bad[:4, 0]])
