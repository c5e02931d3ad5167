"""Record what the library's layout functions return, so that a refactor of the layouts can be held to it.

    GTSFM_LIB=/path/to/libgtsfm_amd.so python tools/record_layout_sizes.py          # writes tests/golden/layout_sizes.json
    python tools/record_layout_sizes.py --check                                     # compares the loaded library with the file

The file holds, per size function, a list of ``[arguments, bytes or floats]`` (a list among the arguments is an int32 array, passed
by pointer) and the SHA-256 of two packed weight blobs. Everything runs on the host: no GPU is needed. The matcher sizes are those of
the default environment (no ``GTSFM_*`` switch set) and of a 256-CU device, which is also what a machine without a GPU reports.
``tests/test_layout_sizes.py`` asserts the same comparison as ``--check``."""

from __future__ import annotations

import argparse
import hashlib
import json
import sys
from pathlib import Path
from typing import Dict, List

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

GOLDEN = REPO / "tests" / "golden" / "layout_sizes.json"
BENCH_HW = (760, 1013)  # tools/bench_netvlad.py, bench_d2net.py, bench_classical_scene.py
D2_BENCH_CAP = 2 * 189 * 252  # D2NetEngine's default capacity at 760 x 1013: twice the dense map's pixels
SIFT_BENCH_CAPS = (4 * 760 * 1013 // 8, 4 * 760 * 1013 // 32)  # sift_engine.default_capacities(760, 1013)


def cases() -> Dict[str, List[list]]:
    """Argument tuples per function: the refused sizes, 1, both sides of each 256-byte / 64-float rounding, ragged shapes, every
    conditional piece on and off, and the shapes the benchmarks run."""
    h, w = BENCH_HW
    c: Dict[str, List[list]] = {}
    c["gtsfm_netvlad_packed_weight_floats"] = [[0], [1]]
    c["gtsfm_netvlad_workspace_bytes"] = [[0, 16, 16], [-1, 16, 16], [1, 15, 16], [1, 16, 15], [1, 0, 0], [1, 16, 16], [1, 17, 31], [1, 32, 32], [3, 33, 47],
                                          [2, 123, 157], [1, 157, 123], [4, h, w], [32, h, w]]
    c["gtsfm_retrieval_workspace_bytes"] = [[0, 4096, 0], [1, 0, 0], [-1, 8, 1]] + [
        [n, d, s] for n in (1, 8, 9, 64, 65, 1000, 1024, 1025, 10000) for d in (1, 33, 64, 4096) for s in (0, 1)]
    c["gtsfm_d2net_packed_weight_floats"] = [[]]
    c["gtsfm_d2net_workspace_bytes"] = [[0, 8, 8, 1], [-1, 8, 8, 1], [1, 7, 8, 1], [1, 8, 7, 1], [1, 8, 8, 0], [1, 8, 8, -1], [2, 8, 8, 1 << 28],
                                        [1, 8, 8, 1], [1, 8, 8, 10], [1, 8, 8, 11], [1, 9, 13, 32], [1, 9, 13, 33], [64, 8, 8, 5], [65, 8, 8, 5],
                                        [1, 61, 47, 2 * 14 * 10], [2, 123, 157, 2 * 29 * 38], [1, h, w, D2_BENCH_CAP], [8, h, w, D2_BENCH_CAP]]
    c["gtsfm_d2net_detect_workspace_bytes"] = [[0, 1], [1, 0], [-1, 5], [2, 1 << 28], [1, 1], [1, 10], [1, 11], [64, 10], [65, 10], [3, 2204],
                                               [1, D2_BENCH_CAP], [8, D2_BENCH_CAP]]
    c["gtsfm_megaloc_packed_weight_floats"] = [[0, 64], [65, 64], [12, 0], [12, 100], [1, 64], [2, 128], [12, 8448]]
    # 64 patches or fewer are refused; the score matrices leave LDS above 612 patches (252 x 476 = 612, 308 x 392 = 616, 14 x 8582 = 613)
    c["gtsfm_megaloc_workspace_bytes"] = [[0, 322, 322, 8448], [-1, 322, 322, 8448], [1, 0, 0, 8448], [1, 14, 14, 8448], [1, 112, 112, 8448], [1, 323, 322, 8448],
                                          [1, 322, 322, 100], [1, 126, 112, 64], [3, 308, 322, 512], [1, 252, 476, 8448], [2, 14, 8568, 8448], [2, 14, 8582, 8448],
                                          [1, 308, 392, 8448], [1, 322, 322, 8448], [16, 322, 322, 8448], [64, 322, 322, 8448], [100, 322, 322, 8448]]
    c["gtsfm_sift_workspace_bytes"] = [[0, 16, 16, 1, 1], [-1, 16, 16, 1, 1], [1, 0, 16, 1, 1], [1, 16, 0, 1, 1], [1, 16, 16, 0, 1], [1, 16, 16, 1, 0],
                                       [1, 16384, 16, 1, 1], [1, 16, 16, (1 << 26) + 1, 1], [1, 16, 16, 1, (1 << 24) + 1],
                                       [1, 1, 1, 1, 1], [1, 1, 1, 16, 1], [1, 1, 1, 17, 1], [1, 2, 3, 4096, 2048], [1, 8, 8, 4096, 2048], [1, 123, 157, 4096, 2048],
                                       [2, 157, 123, 9655, 2413], [1, 16383, 16, 4096, 2048], [1, h, w, *SIFT_BENCH_CAPS], [16, h, w, *SIFT_BENCH_CAPS]]
    c["gtsfm_sp_packed_weight_floats"] = [[]]
    c["gtsfm_sp_workspace_bytes"] = [[0, 64, 64], [1, 0, 64], [1, 64, -1], [1, 1, 1], [1, 7, 7], [1, 8, 8], [1, 8, 16], [1, 9, 17], [3, 8, 8], [1, 16, 24], [2, 123, 157],
                                     [1, 160, 200], [1, 1024, 1024], [8, 1024, 1024], [1, h, w]]
    c["gtsfm_sp_nms_scratch_bytes"] = [[0, 8, 8], [1, 1, 1], [1, 8, 8], [1, 8, 32], [1, 1, 257], [1, 5, 13], [2, 123, 157], [1, 1024, 1024], [8, 1024, 1024]]
    c["gtsfm_twoway_workspace_bytes"] = [[u8, metric, dim, stride, len(p) // 4, p] for (u8, metric, dim, stride) in ((0, 2, 128, 128), (1, 1, 32, 32), (1, 2, 128, 128), (0, 2, 512, 512), (0, 2, 7, 9))
                                         for p in ([0, 1, 1, 1], [0, 2, 2, 3], [0, 63, 63, 65], [0, 64, 64, 64], [0, 123, 123, 157, 123, 157, 280, 5], [0, 5000, 5000, 5000],
                                                   [0, 5000, 5000, 5000] * 8)]
    c["gtsfm_twoway_workspace_bytes"] += [[0, 3, 128, 128, 1, [0, 1, 1, 1]], [0, 1, 128, 128, 1, [0, 1, 1, 1]], [0, 2, 0, 128, 1, [0, 1, 1, 1]], [0, 2, 128, 64, 1, [0, 1, 1, 1]],
                                          [0, 2, 128, 128, 0, []], [0, 2, 128, 128, 1, [0, 0, 1, 1]], [0, 2, 128, 128, 1, [-1, 1, 1, 1]]]
    pairs = [([1], [1]), ([2], [3]), ([63], [65]), ([64], [64]), ([123], [157]), ([123, 1, 300], [157, 640, 2]), ([1024], [1024]), ([1025], [1025]), ([2048] * 32, [2048] * 32),
             ([5000], [5000]), ([5000] * 8, [5000] * 8)]
    for name in ("gtsfm_sg_workspace_bytes", "gtsfm_lg_workspace_bytes", "gtsfm_sinkhorn_workspace_bytes", "gtsfm_lg_assignment_workspace_bytes"):
        c[name] = [[0, [], []], [-1, [1], [1]]] + [[len(a), a, b] for a, b in pairs]
    c["gtsfm_score_matrices_workspace_bytes"] = [[0], [-1], [1], [2], [3], [7], [8], [9], [16], [32], [1000]]
    # (rows, images, problems): refused, no rows, no images, both sides of the 256-byte roundings (64 ints, 256 validity bytes), batches
    c["gtsfm_rotation_averaging_workspace_bytes"] = [[-1, 4, 1], [4, 4, 0], [0, 0, 1], [0, 5, 1], [7, 0, 1], [1, 2, 1], [32, 62, 1], [33, 63, 1], [256, 64, 1], [257, 65, 3],
                                                     [1035, 46, 1], [1035, 46, 64], [48725, 1000, 1]]
    # (pairs, measurements, images, tracks, the most tracks of a problem, problems); more tracks per problem than tracks is refused
    c["gtsfm_translation_recovery_workspace_bytes"] = [[-1, 0, 4, 0, 0, 1], [4, 4, 4, 2, 3, 1], [0, 0, 0, 0, 0, 1], [0, 0, 5, 0, 0, 1], [3, 0, 0, 0, 0, 1], [0, 6, 4, 2, 2, 1],
                                                       [1, 0, 2, 0, 0, 1], [20, 12, 40, 22, 22, 1], [20, 13, 40, 23, 23, 1], [200, 57, 30, 35, 9, 4], [256, 0, 64, 0, 0, 3],
                                                       [1035, 552, 46, 184, 184, 1], [1035, 552, 46, 184, 3, 64], [48725, 12000, 1000, 4000, 4000, 1]]
    return c


def call(lib, name: str, args: list) -> int:
    keep = [np.ascontiguousarray(a, dtype=np.int32) if isinstance(a, list) else a for a in args]
    return int(getattr(lib, name)(*[(a.ctypes.data if a.size else None) if isinstance(a, np.ndarray) else a for a in keep]))


def blob_hashes() -> Dict[str, str]:
    """SHA-256 of the packed blobs of the seeded test weights (NetVLAD without the 512 MiB whitening matrix)."""
    from gtsfm_amd.runtime import d2net_engine, netvlad_engine
    from tests import d2net_reference, netvlad_reference

    return {"netvlad_seeded_weights_0_plain": hashlib.sha256(netvlad_engine.pack_weights(netvlad_reference.seeded_weights(0, whiten=False), whiten=False).tobytes()).hexdigest(),
            "d2net_seeded_weights_0": hashlib.sha256(d2net_engine.pack_weights(d2net_reference.seeded_weights(0)).tobytes()).hexdigest()}


def record() -> dict:
    from gtsfm_amd.runtime import lib as _lib

    lib = _lib.load()
    return {"sizes": {name: [[args, call(lib, name, args)] for args in tuples] for name, tuples in cases().items()}, "blobs": blob_hashes()}


def differences(golden: dict) -> List[str]:
    """What the loaded library answers differently from ``golden`` (empty: nothing)."""
    from gtsfm_amd.runtime import lib as _lib

    lib = _lib.load()
    out = [f"{name}{tuple(args)}: recorded {want}, got {call(lib, name, args)}" for name, rows in golden["sizes"].items() for args, want in rows
           if call(lib, name, args) != want]
    return out + [f"blob {k}: recorded {golden['blobs'][k]}, got {v}" for k, v in blob_hashes().items() if golden["blobs"][k] != v]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="compare with the recorded file and write nothing")
    args = ap.parse_args()
    if args.check:
        diff = differences(json.loads(GOLDEN.read_text()))
        print("\n".join(diff) if diff else f"{GOLDEN.name}: the library agrees on every entry")
        return 1 if diff else 0
    data = record()
    compact = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
    sizes = ",\n".join(f"{compact(name)}:{compact(rows)}" for name, rows in data["sizes"].items())  # one function per line
    GOLDEN.write_text(f'{{"sizes":{{\n{sizes}}},\n"blobs":{compact(data["blobs"])}}}\n')
    print(f"wrote {GOLDEN} ({sum(len(v) for v in data['sizes'].values())} tuples)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
