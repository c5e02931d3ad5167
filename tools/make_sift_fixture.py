"""Writes the SIFT goldens (``tests/golden/sift_*.npz``) from a GTSfM checkout's Lund-door data.

    python tools/make_sift_fixture.py <gtsfm checkout>

Reads ``tests/data/set1_lund_door/images/DSC_000{1,2}.JPG`` (PIL) and ``features/keypoints_{0,1}.pkl`` (OpenCV's recorded SIFT output,
5000 keypoints per image), runs the numpy restatement ``tests/sift_reference.py`` and writes

* ``sift_lund_door_{0,1}.npz``: the recorded keypoints, the restatement's first ``STORED_KEYPOINTS`` keypoints and descriptors, and the
  agreement figures of the two (also written to ``profiles/sift_reference_agreement.txt``); the recorded descriptors are read from the
  existing ``twoway_lund_door_sift.npz``. The restatement keeps 200 keypoints more than the recording holds because the two cut their
  top-k at slightly different responses;
* ``sift_lund_door_{0,1}_gray{0,1,..}.npz``: the gray uint8 image in row strips, each file below 1 MB;
* ``sift_40x48.npz``, ``sift_123x157.npz``, ``sift_240x320.npz``: crops of image 0 with the restatement's output at every stage (a
  SHA-256 per pyramid image; the 40 x 48 golden holds the whole pyramid as well); the last one also carries a mask and the masked output."""

from __future__ import annotations

import hashlib
import pickle
import sys
import types
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tests"))
import sift_agreement  # noqa: E402
import sift_reference as S  # noqa: E402

GOLDEN = REPO / "tests" / "golden"
STORED_KEYPOINTS = 5200
STRIP_BYTES = 900_000
CROPS = {"40x48": (600, 640, 400, 448), "123x157": (500, 623, 700, 857), "240x320": (900, 1140, 500, 820)}  # row0, row1, col0, col1


def load_recorded(path: Path):
    """The pickled ``gtsfm.common.keypoints.Keypoints`` without importing GTSfM (its module imports cv2): a stub class takes its place."""

    class Keypoints:
        pass

    stubs = {}
    for name in ("gtsfm", "gtsfm.common", "gtsfm.common.keypoints"):
        stubs[name] = sys.modules.get(name)
        sys.modules[name] = types.ModuleType(name)
    sys.modules["gtsfm.common.keypoints"].Keypoints = Keypoints
    try:
        with open(path, "rb") as f:
            kp = pickle.load(f)
    finally:
        for name, old in stubs.items():
            if old is None:
                del sys.modules[name]
            else:
                sys.modules[name] = old
    return np.asarray(kp.coordinates), np.asarray(kp.scales), np.asarray(kp.responses)


def pyramid_digests(height: int, width: int, flat: np.ndarray) -> np.ndarray:
    """One SHA-256 per pyramid image in the device layout's order (6 Gaussian images per octave, then 5 DoG images per octave)."""
    out, at = [], 0
    for images in (6, 5):
        for h, w in S.octave_shapes(height, width):
            for _ in range(images):
                out.append(hashlib.sha256(np.ascontiguousarray(flat[at : at + h * w]).tobytes()).hexdigest())
                at += h * w
    assert at == len(flat)
    return np.array(out)


def stage_arrays(stages: dict) -> dict:
    out = {"candidates": stages["candidates"]}
    for k, v in stages["keypoints"].items():
        out["kp_" + k] = v
    for k, v in stages["oriented"].items():
        out["ori_" + k] = v
    return out


def write_crop(name: str, gray: np.ndarray, mask=None) -> None:
    xy, sizes, resp, desc, st = S.detect_and_describe(gray, 1 << 30, stages=True)
    data = {"gray": gray, "coordinates": xy, "sizes": sizes, "responses": resp, "descriptors": desc.astype(np.uint8),
            "pyramid_sha256": pyramid_digests(*gray.shape, st["pyramid"]), **stage_arrays(st)}
    if name == "40x48":
        data["pyramid"] = st["pyramid"]
    if mask is not None:
        mxy, msz, mre, mde = S.detect_and_describe(gray, 1 << 30, mask=mask)
        data.update(mask=mask, masked_coordinates=mxy, masked_sizes=msz, masked_responses=mre, masked_descriptors=mde.astype(np.uint8))
    path = GOLDEN / f"sift_{name}.npz"
    np.savez_compressed(path, **data)
    print(f"{path.name}: {len(st['candidates'])} candidates, {len(st['keypoints']['octave'])} keypoints, {len(xy)} oriented, {path.stat().st_size} bytes")
    assert path.stat().st_size < (1 << 20), path


def write_full(index: int, gray: np.ndarray, recorded, rec_desc: np.ndarray, report: list) -> dict:
    rec_xy, rec_size, rec_resp = recorded
    xy, sizes, resp, desc, st = S.detect_and_describe(gray, STORED_KEYPOINTS, stages=True)
    fig = sift_agreement.agreement(rec_xy, rec_size, rec_resp, rec_desc, xy, sizes, resp, desc)
    ori = {k: v[: len(xy)] for k, v in st["oriented"].items()}
    f32 = lambda a: a.astype(np.float32) if np.array_equal(a.astype(np.float32).astype(np.float64), a) else a  # noqa: E731
    data = {"recorded_coordinates": f32(rec_xy), "recorded_sizes": f32(rec_size), "recorded_responses": f32(rec_resp),
            "coordinates": xy, "sizes": sizes, "responses": resp, "descriptors": desc.astype(np.uint8),
            "octave": ori["octave"].astype(np.int8), "layer": ori["layer"].astype(np.int8), "angle": ori["angle"],
            "counts": np.array([len(st["candidates"]), len(st["keypoints"]["octave"]), len(st["oriented"]["angle"])], dtype=np.int64),
            "agreement_names": np.array(sorted(fig)), "agreement_values": np.array([fig[k] for k in sorted(fig)], dtype=np.float64)}
    path = GOLDEN / f"sift_lund_door_{index}.npz"
    np.savez_compressed(path, **data)
    assert path.stat().st_size < (1 << 20), (path, path.stat().st_size)
    strips, row = 0, 0
    rows_per = max(1, STRIP_BYTES // gray.shape[1])  # uncompressed bound: a strip never exceeds STRIP_BYTES
    while row < gray.shape[0]:
        p = GOLDEN / f"sift_lund_door_{index}_gray{strips}.npz"
        np.savez_compressed(p, rows=gray[row : row + rows_per], first_row=np.int64(row), height=np.int64(gray.shape[0]))
        assert p.stat().st_size < (1 << 20), p
        row += rows_per
        strips += 1
    line = f"image {index}: {data['counts'].tolist()} candidates / keypoints / oriented; " + ", ".join(f"{k} {fig[k]:.6g}" for k in sorted(fig))
    print(line)
    report.append(line)
    return fig


def main() -> None:
    from PIL import Image

    if len(sys.argv) != 2:
        sys.exit(__doc__)
    data = Path(sys.argv[1]) / "tests" / "data" / "set1_lund_door"
    rec_desc = np.load(GOLDEN / "twoway_lund_door_sift.npz")
    report = ["tools/make_sift_fixture.py: tests/sift_reference.py against OpenCV's recorded SIFT output (set1_lund_door, 5000 keypoints per image);",
              f"the restatement's first {STORED_KEYPOINTS} keypoints are compared. Caps: {sift_agreement.CAPS}"]
    grays = []
    for index, name in enumerate(("DSC_0001.JPG", "DSC_0002.JPG")):
        grays.append(S.to_gray(np.asarray(Image.open(data / "images" / name))))
    for name, (r0, r1, c0, c1) in CROPS.items():
        crop = np.ascontiguousarray(grays[0][r0:r1, c0:c1])
        mask = None
        if name == "240x320":
            mask = np.ones(crop.shape, dtype=np.uint8)
            mask[:, :100] = 0
            mask[60:120, 150:260] = 0
        write_crop(name, crop, mask)
    figures = []
    for index, gray in enumerate(grays):
        figures.append(write_full(index, gray, load_recorded(data / "features" / f"keypoints_{index}.pkl"), rec_desc[f"descriptors_{index}"], report))
    (REPO / "profiles" / "sift_reference_agreement.txt").write_text("\n".join(report) + "\n")
    for fig in figures:  # after everything is written, so that a miss can be looked at
        sift_agreement.check_caps(fig)


if __name__ == "__main__":
    main()
