"""GPU: the SIFT kernels (``gtsfm_amd/csrc/sift_kernels.hip``) on the constructed images of ``tests/sift_constructed.py``, which reach what the
photographs of the goldens never reach (``tests/test_sift_census_host.py``): a descriptor radius clipped by the octave's diagonal, response
ties between different keypoints, plateau candidates, singular solves, an arc tangent of exactly 360, a descriptor element saturating at
255, thin strips and a 12-pixel octave. Everything is byte identity with the numpy restatement run live; there is no tolerance and nothing
is excluded. The figures are printed and kept in ``profiles/sift_gpu_tests.txt``."""

import numpy as np
import pytest

import sift_constructed as C
import sift_reference as S
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

KP_FIELDS = ("octave", "layer", "row", "column", "x", "y", "scl", "response")
NAMES = tuple(C.IMAGES)


@pytest.fixture(scope="module")
def engine(gpu_device):
    from gtsfm_amd.runtime.sift_engine import SiftEngine

    return SiftEngine(gpu_device)


@pytest.fixture(scope="module")
def images():
    return C.images()


@pytest.fixture(scope="module")
def counted(images):
    """The restatement's stages and the census of every image, with the seeded half mask, computed once."""
    return {name: C.census(image, C.half_mask(image.shape, 1)) for name, image in images.items()}


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _by_position(kp):
    order = np.lexsort((kp["column"], kp["row"], kp["layer"], kp["octave"]))
    return {k: v[order] for k, v in kp.items()}


def _final(st, count=None):
    """The restatement's (coordinates, sizes, responses, descriptors) of the first ``count`` oriented keypoints of the unmasked image."""
    free = st["oriented_free"]
    n = len(free["angle"]) if count is None else min(count, len(free["angle"]))
    xy, sizes, resp = S.final_outputs(free, n)
    return xy, sizes, resp, st["descriptors"][:n]


@pytest.mark.parametrize("name", NAMES)
def test_every_stage_equals_the_restatement(engine, images, counted, name):
    image, (ev, st) = images[name], counted[name]
    pyramid = engine.stage(image, 0).cpu().numpy()
    assert pyramid.dtype == np.float32 and pyramid.tobytes() == st["pyramid"].tobytes()

    cand = engine.stage(image, 1)
    cand = cand[np.lexsort((cand[:, 3], cand[:, 2], cand[:, 1], cand[:, 0]))]
    assert np.array_equal(cand, st["candidates"])

    kp = _by_position(engine.stage(image, 2))
    for k in KP_FIELDS:
        assert _same(kp[k], st["keypoints"][k]), k

    ori = engine.stage(image, 3)
    for k in KP_FIELDS + ("angle",):
        assert _same(ori[k], st["oriented_free"][k]), k

    got, want = engine.detect(image, 1 << 20), _final(st)
    rows = int((got[3] == want[3]).all(axis=1).sum()) if got[3].shape == want[3].shape else -1
    print(f"{name} {image.shape}: pyramid {len(pyramid)} floats identical, candidates {len(cand)}, keypoints {len(kp['octave'])}, oriented {len(ori['angle'])}, "
          f"identical descriptor rows {rows} of {len(want[3])}; reached: "
          + ", ".join(f"{e} {ev[e]}" for e in ("radius_clipped_by_diagonal", "equal_response_different_keypoints", "adjacent_candidates_in_a_layer", "singular_solve",
                                               "two_candidates_one_position", "atan2_equals_360", "descriptor_atan2_equals_360", "element_saturates_at_255",
                                               "keypoint_in_a_12_pixel_octave") if ev[e]))
    assert all(_same(a, b) for a, b in zip(got, want))


def test_the_blob_in_the_12_pixel_octave_has_four_descriptors_clipped_by_the_diagonal(engine, images, counted):
    ev, st = counted["blob_24x24"]
    assert ev["keypoint_in_a_12_pixel_octave"] == 1 and ev["radius_clipped_by_diagonal"] == 4
    got = engine.detect(images["blob_24x24"], 100)
    assert len(got[0]) == 4 and got[3].any(axis=1).all()
    assert all(_same(a, b) for a, b in zip(got, _final(st)))


def test_strips_and_odd_octaves(engine, images, counted):
    """12 x 200, its transpose, and 45 x 51 whose second octave is odd in both axes (the decimation drops a row and a column)."""
    assert S.octave_shapes(45, 51)[1:3] == [(45, 51), (22, 25)]
    for name in ("strip_12x200", "strip_200x12", "odd_45x51"):
        got, want = engine.detect(images[name], 1 << 20), _final(counted[name][1])
        assert len(want[0]) >= 40 and all(_same(a, b) for a, b in zip(got, want)), name
    assert _same(engine.stage(images["strip_200x12"], 0).cpu().numpy(), counted["strip_200x12"][1]["pyramid"])


def test_top_k_cuts_inside_groups_of_equal_response(engine, images, counted):
    """Every k from 1 to N on the mirrored image: the first k rows of the restatement's output, also where k cuts between two different
    keypoints of equal response, which only the (octave, layer, row, column) half of the order decides."""
    image, st = images["mirror_48x48"], counted["mirror_48x48"][1]
    n = len(st["oriented_free"]["angle"])
    cuts = C.tie_cuts(st["oriented_free"])
    print(f"mirror_48x48: {n} oriented keypoints, cuts between different keypoints of equal response at k = {cuts}")
    assert len(cuts) >= 1 and n >= 16
    for k in range(1, n + 1):
        got, want = engine.detect(image, k), _final(st, k)
        assert len(got[0]) == k and all(_same(a, b) for a, b in zip(got, want)), (k, k in cuts)


def test_masks_on_stage_three_in_a_batch_and_on_one_pixel(engine, images, counted):
    names = ("mirror_48x48", "noise_48x48", "dots_48x48")
    for name in NAMES:  # stage 3 under the seeded half mask
        ev, st = counted[name]
        ori = engine.stage(images[name], 3, C.half_mask(images[name].shape, 1))
        for k in KP_FIELDS + ("angle",):
            assert _same(ori[k], st["oriented"][k]), (name, k)
    kp = counted["mirror_48x48"][1]["keypoints"]
    mask_a, t, (x, y) = C.lone_keypoint_mask(images["mirror_48x48"], kp)
    mask_b = C.half_mask((48, 48), 2)
    masks = [mask_a, None, mask_b]
    batch = engine.detect_batch([images[n] for n in names], 5000, masks)
    for name, mask, many in zip(names, masks, batch):
        one = engine.detect(images[name], 5000, mask)
        want = S.detect_and_describe(images[name], 5000, mask=mask)
        assert all(_same(a, b) for a, b in zip(one, many)) and all(_same(a, b) for a, b in zip(one, want)), name
    lone = batch[0]
    print(f"mirror_48x48: the one-pixel mask at ({x}, {y}) keeps keypoint {t} with {len(lone[0])} orientation(s) of {len(kp['octave'])} keypoints; "
          f"batch of three with masks [one pixel, none, half]: {[len(b[0]) for b in batch]} rows")
    assert 1 <= len(lone[0]) <= 4 and (np.rint(lone[0]) == (x, y)).all()
    assert 0 < len(batch[2][0]) < len(engine.detect(images["dots_48x48"], 5000)[0])


def test_capacities_at_the_boundary(engine, gpu_device):
    """sift_40x48 has 48 candidates, 41 keypoints and 53 oriented keypoints: lists of exactly that size pass, one record fewer is reported."""
    import torch

    from gtsfm_amd.runtime import lib as L

    g = np.load(GOLDEN / "sift_40x48.npz")
    assert (len(g["candidates"]), len(g["kp_octave"]), len(g["ori_angle"])) == (48, 41, 53)
    lib = L.load()
    h, w = g["gray"].shape
    gray = torch.from_numpy(g["gray"]).to(gpu_device)

    def call(cand_cap, kp_cap):
        ws = torch.empty(int(lib.gtsfm_sift_workspace_bytes(1, h, w, cand_cap, kp_cap)), dtype=torch.uint8, device=gpu_device)
        counts = torch.zeros(4, dtype=torch.int32, device=gpu_device)
        kp = torch.zeros((kp_cap, 4), dtype=torch.float32, device=gpu_device)
        de = torch.zeros((kp_cap, 128), dtype=torch.float32, device=gpu_device)
        rc = lib.gtsfm_sift_detect_and_describe(gray.data_ptr(), None, 1, h, w, kp_cap, cand_cap, kp_cap, counts.data_ptr(), kp.data_ptr(), de.data_ptr(),
                                                ws.data_ptr(), ws.numel(), L.current_stream_handle())
        return rc, lib.gtsfm_last_error().decode(), counts.cpu().numpy().tolist(), kp.cpu().numpy(), de.cpu().numpy()

    rc, _, counts, kp, de = call(48, 53)
    assert rc == 0 and counts[:3] == [48, 41, 53]
    assert _same(np.ascontiguousarray(kp[:, :2]), g["coordinates"]) and _same(np.ascontiguousarray(kp[:, 2]), g["sizes"])
    assert _same(np.ascontiguousarray(kp[:, 3]), g["responses"]) and np.array_equal(de, g["descriptors"].astype(np.float32))
    rc, why, counts, _, _ = call(47, 53)
    print(f"47 / 53: rc {rc}, {why}")
    assert rc == -3 and "48 candidates" in why and counts[0] == 48
    rc, why, counts, _, _ = call(48, 52)
    print(f"48 / 52: rc {rc}, {why}")
    assert rc == -3 and "48 candidates / 41 keypoints / 53 oriented keypoints" in why and counts[:3] == [48, 41, 53]
    # from 1 / 1 the engine learns the candidates, then the keypoints, then the oriented keypoints: three repeats
    before = engine.relaunches
    got = engine.detect(g["gray"], 5000, cand_capacity=1, kp_capacity=1)
    print(f"1 / 1: {engine.relaunches - before} relaunches")
    assert engine.relaunches - before == 3
    assert _same(got[0], g["coordinates"]) and _same(got[1], g["sizes"]) and _same(got[2], g["responses"])
    assert np.array_equal(got[3], g["descriptors"].astype(np.float32))
