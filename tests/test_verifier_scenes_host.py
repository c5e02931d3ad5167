"""CPU: the scene catalogue of ``tests/verifier_scenes.py`` reaches every exit of the verifier's RANSAC loop. These are
conditions on the INPUTS of ``tests/test_verifier_scenes_gpu.py`` (device == oracle on the same catalogue), checked on the oracle:
if a recipe stops reaching its branch, the recipe is changed, never the condition."""

import numpy as np
import pytest

from tests import verifier_scenes as vs


@pytest.fixture(scope="module")
def results():
    """{(entry, mode): oracle result}, each computed once (shared with every other test of the process)."""
    return {case: vs.oracle(*case) for case in vs.cases()}


def _models(results, mode=None):
    return {c: r for c, r in results.items() if r["R"] is not None and mode in (None, c[1])}


def test_every_entry_is_well_formed():
    for name in vs.CATALOGUE:
        s = vs.scene(name)
        assert s["coordinates_i1"].dtype == np.float32 and s["coordinates_i2"].dtype == np.float32 and s["match_indices"].dtype == np.int32
        idx = s["match_indices"]
        assert idx.ndim == 2 and idx.shape[1] == 2 and set(s["modes"]) <= {"E", "F"} and s["modes"]
        if idx.size:  # an out-of-range index would be an out-of-bounds read on the device
            assert idx.min() >= 0 and idx[:, 0].max() < s["coordinates_i1"].shape[0] and idx[:, 1].max() < s["coordinates_i2"].shape[0]
    assert len(vs.cases()) == len(set(vs.cases()))


def test_hypothesis_counts_cover_every_number_of_rounds(results):
    assert {0, 512, 768, 1024, 1280} <= {r["hypotheses"] for r in results.values()}


def test_four_rounds_end_both_without_a_model_and_with_the_local_optimisation_skipped(results):
    assert any(r["R"] is None and r["no_model"] and r["hypotheses"] == 1024 for r in results.values())
    skipped = [c for c, r in _models(results).items() if r["hypotheses"] == 1024]
    assert skipped
    for name, mode in skipped:  # four rounds and no fifth: the winner has fewer inliers than a minimal sample plus one
        assert results[(name, mode)]["winner"][0] < 1024 and results[(name, mode)]["mask"].sum() < vs.MIN_MATCHES[mode]


def test_a_model_without_a_single_inlier_occurs(results):
    assert any(r["R"] is None and not r["no_model"] and r["hypotheses"] == 1024 for r in results.values())


def test_the_polish_is_both_kept_and_rejected_in_essential_mode(results):
    assert {r["polished"] for r in _models(results, "E").values()} == {True, False}


def test_winners_come_from_the_first_round_a_later_round_and_the_local_optimisation(results):
    winners = [r["winner"][0] for r in _models(results).values()]
    assert any(w < 256 for w in winners) and any(256 <= w < 1024 for w in winners) and any(w >= 1024 for w in winners)
    assert any(r["winner"][1] >= 3 for r in _models(results).values())


def test_every_cheirality_candidate_is_picked_and_ties_and_all_zero_counts_occur(results):
    picks, ties, zeros = set(), 0, 0
    for r in _models(results).values():
        good = list(r["cheirality"])
        picks.add(good.index(max(good)))  # recoverPose: the first candidate whose count is >= all others
        ties += good.count(max(good)) > 1 and max(good) > 0
        zeros += max(good) == 0
    assert picks == {0, 1, 2, 3} and ties >= 1 and zeros >= 1


@pytest.mark.parametrize("mode", ["E", "F"])
def test_failure_at_or_above_the_minimum_count_occurs_in_each_mode(results, mode):
    assert any(r["R"] is None and r["num_matches"] >= vs.MIN_MATCHES[mode] for (_, m), r in results.items() if m == mode)
    assert any(r["R"] is None and r["num_matches"] < vs.MIN_MATCHES[mode] and r["hypotheses"] == 0 for (_, m), r in results.items() if m == mode)


@pytest.mark.parametrize("mode", ["E", "F"])
def test_match_counts_sit_on_the_kernels_edges(results, mode):
    counts = {r["num_matches"] for (_, m), r in results.items() if m == mode}
    assert {0, 5, 6, 7, 8, 9, 255, 256, 257, 513} <= counts
    need = vs.MIN_MATCHES[mode]
    assert results[(f"count_{need - 1}", mode)]["R"] is None and results[(f"count_{need}", mode)]["R"] is not None


def test_count_edge_outcomes(results):
    assert results[("count_6", "E")]["hypotheses"] == 512 and not results[("count_6", "E")]["polished"]
    assert results[("count_8", "F")]["mask"].sum() == 8 and results[("count_8", "F")]["hypotheses"] == 512  # one round + the LO round


@pytest.mark.parametrize("mode", ["E", "F"])
def test_non_finite_keypoints_are_outliers_and_nothing_else_is_lost(results, mode):
    s, r = vs.scene("non_finite"), results[("non_finite", mode)]
    c1, c2, idx = s["coordinates_i1"], s["coordinates_i2"], s["match_indices"]
    touched = ~(np.isfinite(c1[idx[:, 0]]).all(1) & np.isfinite(c2[idx[:, 1]]).all(1))
    np.testing.assert_array_equal(np.flatnonzero(touched), s["nonfinite_rows"])
    assert touched.sum() == 3 and not r["mask"][touched].any()
    assert r["mask"].sum() >= 40 and vs.rotation_angle_deg(r["R"], s["i2Ri1"]) < 2.0  # the rest of the scene is still solved


@pytest.mark.parametrize("mode", ["E", "F"])
def test_anisotropic_cameras_recover_the_planted_rotation(results, mode):
    s, r = vs.scene("anisotropic"), results[("anisotropic", mode)]
    assert s["intrinsics_i1"] != s["intrinsics_i2"]
    for fx, fy, cx, cy in (s["intrinsics_i1"], s["intrinsics_i2"]):
        assert fx != fy and cx != cy
    assert s["intrinsics_i1"][0] < s["intrinsics_i2"][0]  # max(fx1, fx2) is the SECOND camera's: the threshold cannot come from K1 alone
    assert vs.rotation_angle_deg(r["R"], s["i2Ri1"]) < 2.0 and abs(np.linalg.det(r["R"]) - 1.0) < 1e-9
    assert (r["mask"] & s["is_inlier"]).sum() >= 0.9 * s["is_inlier"].sum()


def test_big_seeds_draw_other_samples_than_their_low_bits(results):
    assert vs.scene("seed_top_bit")["seed"] == 2**63 and vs.scene("seed_all_ones")["seed"] == 2**64 - 1
    winners = {results[(n, "E")]["winner"] for n in ("seed_all_ones", "seed_top_bit", "seed_high_word")}
    low = vs.run_oracle(vs.scene("seed_high_word"), "E", seed=3)  # (7 << 32) | 3 without its high word
    assert len(winners) == 3 and low["winner"] not in winners
