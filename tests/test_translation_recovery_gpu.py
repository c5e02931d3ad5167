"""GPU: ``gtsfm_translation_recovery_f64`` on every scene of tests/translation_recovery_scenes.py against the restatement
(tests/translation_recovery_reference.py). The stage is float64 + - * / sqrt in one stated order, so the device's positions, mask, counters
and costs are ASSERTED to be the restatement's bytes on every scene: that is the contract the documents state. Equal bytes run to run,
alone against batched (P = 4), and under a permutation of the rows with the anchor given; inputs untouched; invalid input refused with
nothing written; a short workspace is GTSFM_ERR_WORKSPACE; the drop-in entry points agree with the engine. ``-s`` prints the lines of
profiles/translation_recovery_gpu_tests.txt."""

import numpy as np
import pytest

from tests import translation_recovery_reference as ref
from tests import translation_recovery_scenes as scenes

pytestmark = pytest.mark.gpu

KEYS = ("translation", "node_valid", "counters", "costs")


@pytest.fixture(scope="module")
def engine(gpu_device):
    from gtsfm_amd.runtime.translation_recovery_engine import TranslationRecoveryEngine

    return TranslationRecoveryEngine(gpu_device)


def run_device(engine, sc, **override):
    opts = dict(sc["options"], **override)
    anchor = opts.pop("anchor", sc["anchor"])
    dev = engine.upload(*scenes.arrays_of(sc))
    keep = [None if t is None else t.clone() for t in dev]
    out = engine.recover(*dev, num_images=sc["num_images"], anchor=anchor, **opts)
    for before, after in zip(keep, dev):
        assert before is None or before.cpu().numpy().tobytes() == after.cpu().numpy().tobytes(), "an input was changed"
    return {"translation": out["translation"].cpu().numpy()[0], "node_valid": out["node_valid"].cpu().numpy()[0], "counters": out["counters"][0], "costs": out["costs"][0]}


def same_bytes(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in KEYS)


def restated(want):
    return {"translation": want["translation"], "node_valid": want["node_valid"], "counters": np.array([want["counters"][k] for k in ref.COUNTER_FIELDS], np.int32),
            "costs": np.array([want["costs"][k] for k in ref.COST_FIELDS], np.float64)}


@pytest.mark.parametrize("name", scenes.SCENE_NAMES)
def test_device_bytes_are_the_restatements(engine, name):
    sc, want = scenes.get(name), scenes.expected(name)
    assert sc["check"](want), "the scene does not contain what it is named for"
    got = run_device(engine, sc)
    c = dict(zip(ref.COUNTER_FIELDS, (int(x) for x in got["counters"])))
    w = restated(want)
    equal = {k: np.asarray(got[k]).tobytes() == np.asarray(w[k]).tobytes() for k in KEYS}
    with np.errstate(invalid="ignore"):
        far = float(np.nanmax(np.abs(got["translation"] - want["translation"]), initial=0.0))
    print(f"\ntranslation_recovery {name}: status {ref.STATUS_NAMES[c['status']]} n {c['component_size']} rows {c['valid_rows']} outer {c['outer_iterations']} accepted {c['accepted_steps']} "
          f"hessian {c['hessian_applications']} init {c['init_cg_steps']} cost {got['costs'][0]:.6e} -> {got['costs'][1]:.6e} |g|_inf {got['costs'][2]:.3e} | "
          f"device-restatement {far:.3e}, bytes equal {equal}")
    assert all(equal.values()), equal
    assert same_bytes(got, run_device(engine, sc)), "two runs differ"
    if c["status"] in (ref.CONVERGED, ref.MAX_ITERATIONS):
        assert not got["translation"][c["anchor"]].any(), "the gauge"
    else:
        assert np.isnan(got["translation"]).all() and not got["node_valid"].any()


def test_batch_equals_alone(engine):
    """P = 4 over ranges of the same arrays: every problem gives the bytes it gives alone, and the restatement's."""
    arrays, off, n, parts = scenes.batch()
    dev = engine.upload(*arrays)
    out = engine.recover(*dev, num_images=n, problem_row_off=off)
    tr, valid = out["translation"].cpu().numpy(), out["node_valid"].cpu().numpy()
    for p, sc in enumerate(parts):
        alone = run_device(engine, dict(sc, num_images=n, options={}, anchor=-1))
        m = len(alone["translation"])
        inside = {"translation": tr[p][:m], "node_valid": valid[p][:m], "counters": out["counters"][p], "costs": out["costs"][p]}
        assert same_bytes(alone, inside), f"problem {p}"
        assert not valid[p][m:].any() and np.isnan(tr[p][m:]).all()
        assert same_bytes(alone, restated(ref.solve(*ref.problem_arrays(*arrays, off, p), num_images=n))), f"problem {p} against the restatement"


@pytest.mark.parametrize("name", ["planted_noise", "gaps", "masked_rows", "tracks_only", "two_components_anchor"])
def test_row_permutation(engine, name):
    """With the anchor given, the order of the pair rows and of each track's measurements changes no byte; the first row, which carries the scale
    row, stays (for masked_rows it is not valid: there the scale row moves with the permutation, so that scene permutes the measurements only)."""
    sc = scenes.get(name)
    anchor = scenes.expected(name)["counters"]["anchor"]
    moved = scenes.permuted(sc)
    if name == "masked_rows":
        moved = dict(moved, pair_images=sc["pair_images"], world_pair=sc["world_pair"], pair_enable=sc["pair_enable"])
    assert same_bytes(run_device(engine, sc, anchor=anchor), run_device(engine, moved, anchor=anchor))


def raw_call(engine, arrays, num_images, row_off, ws_bytes=None, anchor=-1, **override):
    """The C call with outputs filled with 7: (rc, outputs untouched)."""
    import torch

    from gtsfm_amd.runtime import lib as L

    dev = engine.upload(*arrays)
    e, t, s = len(arrays[0]), len(arrays[3]) - 1, len(arrays[4])
    off = np.asarray(row_off, np.int64).reshape(-1, 2)
    p = len(off) - 1
    t_max = override.pop("max_tracks", min(max(int(np.diff(off[:, 1]).max()), 0), t))
    off_dev = torch.from_numpy(off).to(engine.device)
    lib = L.load()
    need = int(lib.gtsfm_translation_recovery_workspace_bytes(e, s, num_images, t, t_max, p))
    ws = torch.zeros((need if ws_bytes is None else ws_bytes) + 256, dtype=torch.uint8, device=engine.device)
    m = num_images + t_max
    tr = torch.full((p, m, 3), 7.0, dtype=torch.float64, device=engine.device)
    valid = torch.full((p, m), 7, dtype=torch.uint8, device=engine.device)
    counters = torch.full((p, 8), 7, dtype=torch.int32, device=engine.device)
    costs = torch.full((p, 4), 7.0, dtype=torch.float64, device=engine.device)
    o = dict(ref.DEFAULTS, **override)
    rc = lib.gtsfm_translation_recovery_f64(dev[0].data_ptr(), dev[1].data_ptr(), None, e, dev[3].data_ptr(), dev[4].data_ptr(), dev[5].data_ptr(), None, t, s, num_images,
                                            off_dev.data_ptr(), p, t_max, anchor, o["scale_factor"], o["sigma"], o["huber_k"], o["init_tol"], o["init_max_iterations"], o["delta0"],
                                            o["kappa_cg"], o["gradient_tol"], o["rel_tol"], o["abs_tol"], o["max_outer"], o["max_inner"], ws.data_ptr(),
                                            need if ws_bytes is None else ws_bytes, tr.data_ptr(), valid.data_ptr(), counters.data_ptr(), costs.data_ptr(),
                                            torch.cuda.current_stream(engine.device).cuda_stream)
    torch.cuda.synchronize()
    untouched = bool((tr == 7.0).all() and (valid == 7).all() and (counters == 7).all() and (costs == 7.0).all())
    return rc, untouched, lib.gtsfm_last_error()


@pytest.mark.parametrize("case", ["unordered_pair", "self_pair", "out_of_range", "negative", "camera", "track_offsets", "track_total", "problem_offsets", "problem_tracks", "anchor", "sigma"])
def test_invalid_input_is_refused_with_nothing_written(engine, case):
    pairs = {"unordered_pair": [(1, 0), (1, 2)], "self_pair": [(0, 1), (2, 2)], "out_of_range": [(0, 1), (1, 5)], "negative": [(-1, 1), (1, 2)]}.get(case, [(0, 1), (1, 2)])
    track_off = {"track_offsets": [0, 2, 1, 3], "track_total": [0, 1, 2, 2], "problem_tracks": [0, 1, 2, 3, 3]}.get(case, [0, 1, 2, 3])
    image = [0, 7, 2] if case == "camera" else [0, 1, 2]
    row_off = {"problem_offsets": [[0, 0], [3, 3]], "problem_tracks": [[0, 0], [1, 1], [2, 2], [2, 4]]}.get(case, [[0, 0], [2, 3]])
    arrays = (np.asarray(pairs, np.int32), np.tile([0.0, 0.0, 1.0], (2, 1)), None, np.asarray(track_off, np.int64), np.asarray(image, np.int32), np.tile([0.0, 1.0, 0.0], (3, 1)), None)
    extra = {"sigma": {"sigma": 0.0}, "problem_tracks": {"max_tracks": 1}}.get(case, {})
    rc, untouched, err = raw_call(engine, arrays, 3, row_off, anchor=9 if case == "anchor" else -1, **extra)
    assert rc == -1 and err
    assert untouched, "an output was written"


def test_short_workspace(engine):
    from gtsfm_amd.runtime import lib as L

    sc = scenes.get("pairs_only")
    arrays = scenes.arrays_of(sc)
    whole = [[0, 0], [len(sc["pair_images"]), 0]]
    need = int(L.load().gtsfm_translation_recovery_workspace_bytes(len(sc["pair_images"]), 0, sc["num_images"], 0, 0, 1))
    rc, untouched, err = raw_call(engine, arrays, sc["num_images"], whole, ws_bytes=need - 1)
    assert rc == -3 and untouched and b"workspace" in err
    rc, untouched, _ = raw_call(engine, arrays, sc["num_images"], whole, ws_bytes=need)
    assert rc == 0 and not untouched


def test_drop_in_agrees_with_the_engine(engine, gpu_device):
    """``recover_arrays`` and ``device_translation_recovery`` (dicts in, a list of wti or None out) give the engine's bytes."""
    from gtsfm_amd.averaging.translation import TranslationAveraging1DSFM
    from gtsfm_amd.averaging.translation.averaging_1dsfm import device_translation_recovery

    sc = scenes.get("two_components")
    got = run_device(engine, sc)
    obj = TranslationAveraging1DSFM(translation_recovery="device", device=gpu_device)
    res = obj.recover_arrays(sc["pair_images"], sc["world_pair"], num_images=sc["num_images"])
    assert res["translation"].tobytes() == got["translation"].tobytes() and res["node_valid"].tobytes() == got["node_valid"].tobytes()
    pairs = {(int(a), int(b)): z for (a, b), z in zip(sc["pair_images"], sc["world_pair"])}
    wRi = [np.eye(3)] * 16 + [None]
    wti = device_translation_recovery(sc["num_images"], pairs, {}, wRi, {}, [], 1.0, True)
    assert [t is None for t in wti] == [True] * 10 + [False] * 6 + [True]
    assert np.stack(wti[10:16]).tobytes() == got["translation"][10:16].tobytes()
    with pytest.raises(NotImplementedError):
        device_translation_recovery(sc["num_images"], pairs, {}, wRi, {(0, 1): object()}, [], 1.0, True)
    # with tracks: the dict's (track, camera) keys become the CSR in track order
    sc = scenes.get("leaves")
    got = run_device(engine, sc)
    track = np.repeat(np.arange(len(sc["track_off"]) - 1), np.diff(sc["track_off"]))
    on = sc["meas_enable"] != 0
    pairs = {(int(a), int(b)): z for (a, b), z in zip(sc["pair_images"], sc["world_pair"])}
    meas = {(int(j), int(i)): z for j, i, z in zip(track[on], sc["image"][on], sc["world_meas"][on])}
    wti = device_translation_recovery(sc["num_images"], pairs, meas, [np.eye(3)] * 10, {}, [], 1.0, True)
    assert np.stack(wti).tobytes() == got["translation"][:10].tobytes()
    assert obj._translation_recovery is device_translation_recovery
