"""Verifier kernels == ``oracle/verifier_oracle.py`` on the scene catalogue of ``tests/verifier_scenes.py``: different and
anisotropic cameras, the match counts the kernels are built around, degenerate geometry, non-finite keypoints, seeds with the
top bit set -- every exit of the RANSAC loop (``tests/test_verifier_scenes_host.py`` proves that the catalogue reaches them).
Same criteria as ``tests/test_verifier_gpu.py``: hypothesis count, winner, inlier mask and cheirality counts identical, E / R /
t (and F) within 1e-9. Device time is microseconds per pair; the wall time is the oracle on the host, computed once per entry."""

import numpy as np
import pytest
import torch

from tests import verifier_scenes as vs
from tests.test_verifier_gpu import _compare

pytestmark = pytest.mark.gpu

FILLERS = ("count_0", "count_5")  # fail before the threshold is read, so they may sit in a batch of any threshold
POSE_KEYS = {"E": ("E", "R", "t", "stats"), "F": ("E", "R", "t", "F", "stats")}


def _groups(mode):
    """The catalogue's entries of a mode as batches: ``threshold_px`` is one argument per ``verify_batch`` call, so entries are
    grouped by it (catalogue order kept: degenerate pairs sit between healthy ones), and every batch gets the empty pair and
    the five-match pair interleaved."""
    by_thr = {}
    for name, m in vs.cases():
        if m == mode and name not in FILLERS:
            by_thr.setdefault(vs.scene(name)["threshold_px"], []).append(name)
    for thr, names in by_thr.items():
        names.insert(1, FILLERS[0])
        names.insert(min(3, len(names)), FILLERS[1])
        yield thr, names


def _pack(names, device, pads=None, rng=None):
    """One keypoint table, offsets per pair, ragged match lists (``tests/test_verifier_gpu.py::_batch`` with a K per camera).
    ``pads``: rows of capacity behind each pair's matches, filled with in-range garbage indices."""
    tables, off1, off2, idx, moff, intr, seeds, counts = [], [], [], [], [0], [], [], []
    row = 0
    for p, name in enumerate(names):
        s = vs.scene(name)
        off1.append(row)
        row += s["coordinates_i1"].shape[0]
        off2.append(row)
        row += s["coordinates_i2"].shape[0]
        tables += [s["coordinates_i1"], s["coordinates_i2"]]
        mi = s["match_indices"]
        if pads is not None:
            garbage = np.stack([rng.integers(0, s["coordinates_i1"].shape[0], pads[p]), rng.integers(0, s["coordinates_i2"].shape[0], pads[p])], 1)
            mi = np.concatenate([mi, garbage.astype(np.int32)], 0)
        idx.append(mi)
        counts.append(s["match_indices"].shape[0])
        moff.append(moff[-1] + mi.shape[0])
        intr.append(list(s["intrinsics_i1"]) + list(s["intrinsics_i2"]))
        seeds.append(s["seed"])
    kp = torch.from_numpy(np.concatenate(tables, 0)).to(device)
    mi = torch.from_numpy(np.ascontiguousarray(np.concatenate(idx, 0), dtype=np.int32)).to(device)
    return kp, off1, off2, mi, moff, np.asarray(intr), seeds, counts


def _bits(t):
    """Bit patterns, so that NaN == NaN."""
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def _compare_failure(out, p, lo, hi, ref, mode):
    stats = out["stats"][p].cpu().numpy()
    assert stats[0] == 0 and stats[1] == ref["hypotheses"]
    assert not out["mask"][lo:hi].any()
    if ref["no_model"]:
        assert tuple(stats[2:4]) == (-1, -1)
        for key in POSE_KEYS[mode][:-1]:
            assert torch.isnan(out[key][p]).all(), key


def _compare_with_oracle(out, p, lo, hi, ref, mode):
    if ref["R"] is None:
        _compare_failure(out, p, lo, hi, ref, mode)
        return
    _compare(out, p, lo, hi, ref)
    if mode == "F":
        np.testing.assert_allclose(out["F"][p].cpu().numpy(), ref["F"], rtol=0, atol=1e-9 * np.abs(ref["F"]).max())


@pytest.fixture(scope="module")
def engine(gpu_device):
    from gtsfm_amd.runtime.verifier_engine import VerifierEngine

    return VerifierEngine(gpu_device)


@pytest.fixture(scope="module")
def tight(engine, gpu_device):
    """{mode: [(threshold, names, match_off, output of the tight-layout batch)]}, computed once per mode."""
    cache = {}

    def get(mode):
        if mode not in cache:
            cache[mode] = []
            for thr, names in _groups(mode):
                kp, off1, off2, mi, moff, intr, seeds, _ = _pack(names, gpu_device)
                out = engine.verify_batch(kp, off1, off2, mi, moff, intr, thr, seeds, use_intrinsics=mode == "E")
                cache[mode].append((thr, names, moff, out))
        return cache[mode]

    return get


@pytest.mark.parametrize("mode", ["E", "F"])
def test_whole_catalogue_in_batches_equals_oracle_and_single_calls(engine, gpu_device, tight, mode):
    seen = set()
    for thr, names, moff, out in tight(mode):
        assert len(names) >= 3 and vs.scene(names[1])["match_indices"].shape[0] == 0  # an empty pair between two others
        for p, name in enumerate(names):
            try:
                _compare_with_oracle(out, p, moff[p], moff[p + 1], vs.oracle(name, mode), mode)
                kp, off1, off2, mi, soff, intr, seeds, _ = _pack([name], gpu_device)
                single = engine.verify_batch(kp, off1, off2, mi, soff, intr, thr, seeds, use_intrinsics=mode == "E")
                for key in POSE_KEYS[mode]:
                    assert torch.equal(_bits(single[key][0]), _bits(out[key][p])), key  # batched == single, bit for bit
                assert torch.equal(single["mask"], out["mask"][moff[p] : moff[p + 1]])
            except AssertionError as err:
                raise AssertionError(f"entry {name!r}, mode {mode}, threshold {thr}: {err}") from err
            seen.add(name)
    assert seen == {name for name, m in vs.cases() if m == mode}


@pytest.mark.parametrize("mode", ["E", "F"])
def test_capacity_layout_equals_the_tight_layout(engine, gpu_device, tight, mode):
    """Each pair's slice padded to a larger capacity (``compact_matches``' layout), ``match_count`` given: results identical
    to the tight layout, the mask behind each count zero. The pads cross the 256-row stride of the clearing loop."""
    rng = np.random.default_rng(8)
    for thr, names, moff, ref in tight(mode):
        pads = [(0, 1, 7, 255, 256, 300)[p % 6] for p in range(len(names))]
        kp, off1, off2, mi, coff, intr, seeds, counts = _pack(names, gpu_device, pads, rng)
        count = torch.tensor(counts, dtype=torch.int32, device=gpu_device)
        out = engine.verify_batch(kp, off1, off2, mi, coff, intr, thr, seeds, match_count=count, use_intrinsics=mode == "E")
        for key in POSE_KEYS[mode]:
            assert torch.equal(_bits(out[key]), _bits(ref[key])), (key, thr)
        for p, name in enumerate(names):
            m = counts[p]
            assert torch.equal(out["mask"][coff[p] : coff[p] + m], ref["mask"][moff[p] : moff[p + 1]]), name
            assert not out["mask"][coff[p] + m : coff[p + 1]].any(), name


def _cam(k, cls=None):
    from gtsfm_amd.common.calibration import PinholeIntrinsics

    return (cls or PinholeIntrinsics)(k[0], k[2], k[3], fy=k[1])


def _compare_plugin(got, ref, match_indices):
    rot, direction, verified, ratio = got
    if ref["R"] is None:
        assert rot is None and direction is None and verified.size == 0 and verified.dtype == np.uint64 and ratio == 0.0
        return
    np.testing.assert_array_equal(verified, ref["v_corr_idxs"])
    assert verified.dtype == match_indices.dtype and ratio == ref["inlier_ratio"]
    np.testing.assert_allclose(np.asarray(getattr(rot, "matrix", lambda: rot)()), ref["R"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(np.asarray(getattr(direction, "point3", lambda: direction)()), ref["t"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("name", ["anisotropic", "same_point_pair", "identity_motion", "non_finite", "vanishing_threshold", "seed_all_ones"])
def test_per_pair_plugin_equals_oracle(gpu_device, name):
    from gtsfm_amd.common.keypoints import Keypoints
    from gtsfm_amd.frontend.verifier.ransac import Ransac

    s = vs.scene(name)
    for mode in s["modes"]:
        got = Ransac(mode == "E", s["threshold_px"], seed=s["seed"]).verify(
            Keypoints(s["coordinates_i1"]), Keypoints(s["coordinates_i2"]), s["match_indices"], _cam(s["intrinsics_i1"]), _cam(s["intrinsics_i2"]))
        _compare_plugin(got, vs.oracle(name, mode), s["match_indices"])


def test_per_pair_plugin_with_a_skewed_calibration_equals_oracle_on_the_calibrated_coordinates(gpu_device):
    """A calibration with skew takes the plugin's host path: its own ``calibrate``, the float32 table, unit intrinsics and the
    threshold in normalised units. The oracle gets exactly that input."""
    from gtsfm_amd.common.calibration import PinholeIntrinsics
    from gtsfm_amd.common.keypoints import Keypoints
    from gtsfm_amd.frontend.verifier.ransac import Ransac

    skew = 0.5

    class Skewed(PinholeIntrinsics):
        def K(self):  # noqa: N802
            k = super().K()
            k[0, 1] = skew
            return k

        def calibrate(self, uv):
            uv = np.asarray(uv, dtype=np.float64).reshape(2)
            y = (uv[1] - self.v0) / self.fy
            return np.array([(uv[0] - self.u0 - skew * y) / self.fx, y])

    s = vs.scene("anisotropic")
    (fx1, fy1, cx1, cy1), (fx2, fy2, cx2, cy2) = s["intrinsics_i1"], s["intrinsics_i2"]
    c1, c2 = s["coordinates_i1"].astype(np.float64), s["coordinates_i2"].astype(np.float64)
    y1 = (c1[:, 1] - cy1) / fy1
    n1 = np.stack([(c1[:, 0] - cx1 - skew * y1) / fx1, y1], 1).astype(np.float32)
    n2 = np.stack([(c2[:, 0] - cx2) / fx2, (c2[:, 1] - cy2) / fy2], 1).astype(np.float32)
    unit = (1.0, 1.0, 0.0, 0.0)
    ref = vs.run_oracle(s, "E", coordinates_i1=n1, coordinates_i2=n2, intrinsics_i1=unit, intrinsics_i2=unit, threshold_px=s["threshold_px"] / max(fx1, fx2))
    assert ref["R"] is not None and ref["mask"].sum() >= 0.9 * s["is_inlier"].sum()
    got = Ransac(True, s["threshold_px"], seed=s["seed"]).verify(
        Keypoints(s["coordinates_i1"]), Keypoints(s["coordinates_i2"]), s["match_indices"], _cam(s["intrinsics_i1"], Skewed), _cam(s["intrinsics_i2"]))
    _compare_plugin(got, ref, s["match_indices"])


def test_compaction_at_the_ballot_widths(engine, gpu_device):
    """``verify_compact_matches_kernel`` orders 256 rows per step by a ballot prefix: blocks of 255 / 256 / 257 / 512 / 513 rows,
    one block all valid, one all unmatched, against the plugins' numpy expression (superglue_matcher.py:100-102)."""
    rng = np.random.default_rng(5)
    n0 = [255, 256, 257, 512, 513, 300, 257, 256, 1]
    n1 = [10, 0, 257, 3, 513, 300, 4, 256, 1]
    blocks, rows, row = [], [], 0
    for p, (a, b) in enumerate(zip(n0, n1)):
        m0 = np.where(rng.random(a) < 0.4, rng.integers(0, max(b, 1), a), -1).astype(np.int32)
        if p in (5, 7):
            m0 = rng.integers(0, b, a).astype(np.int32)  # all valid
        if p == 6:
            m0[:] = -1  # all unmatched
        blocks += [m0, rng.integers(-1, max(a, 1), b).astype(np.int32)]
        rows.append(row)
        row += a + b
    matches = torch.from_numpy(np.concatenate(blocks)).to(gpu_device)
    idx, off, count = engine.compact_matches(matches, rows, n0)
    idx, count = idx.cpu().numpy(), count.cpu().numpy()
    assert count[5] == 300 and count[7] == 256 and count[6] == 0
    for p, a in enumerate(n0):
        m0 = blocks[2 * p]
        valid = m0 > -1
        expect = np.stack([np.flatnonzero(valid), m0[valid]], -1)
        assert count[p] == valid.sum() and off[p + 1] - off[p] == a
        np.testing.assert_array_equal(idx[off[p] : off[p] + count[p]], expect)
