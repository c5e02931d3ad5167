"""CPU: the compiled gfx950 code of the SIFT kernels (``gtsfm_amd/csrc/sift_kernels.hip``): every kernel is there and none spills
(``private_segment_fixed_size == 0``). Compiles the file to assembly (hipcc cross-compiles without a GPU) and reads the kernel descriptors."""

import re
import subprocess

import pytest

from conftest import REPO

CSRC = REPO / "gtsfm_amd" / "csrc"
KERNELS = ("sift_upsample_kernel", "sift_blur_row_kernel", "sift_blur_col_kernel", "sift_decimate_kernel", "sift_dog_kernel", "sift_extrema_kernel",
           "sift_refine_kernel", "sift_orient_kernel", "sift_rank_kernel", "sift_describe_kernel", "sift_math_kernel")


@pytest.fixture(scope="module")
def descriptors(tmp_path_factory):
    from gtsfm_amd.csrc import build

    out = tmp_path_factory.mktemp("isa") / "sift_kernels.s"
    flags = [f for f in build.FLAGS if f not in ("-Wall",)]
    cmd = [build.HIPCC, *flags, "-I", str(REPO / "include"), "-S", "--cuda-device-only", str(CSRC / "sift_kernels.hip"), "-o", str(out)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        field = lambda key: int(re.search(key + r"\s+(\d+)", m.group(2)).group(1))  # noqa: E731,B023
        found[m.group(1)] = {"scratch": field(r"\.amdhsa_private_segment_fixed_size"), "lds": field(r"\.amdhsa_group_segment_fixed_size"),
                             "vgprs": field(r"\.amdhsa_next_free_vgpr")}
    return found


def test_every_kernel_is_compiled(descriptors):
    for kernel in KERNELS:
        assert sum(kernel in name for name in descriptors) == 1, (kernel, sorted(descriptors))
    assert len(descriptors) == len(KERNELS), sorted(descriptors)


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_has_no_scratch(descriptors, kernel):
    (name,) = [n for n in descriptors if kernel in n]
    print(name, descriptors[name])
    assert descriptors[name]["scratch"] == 0, f"private_segment_fixed_size = {descriptors[name]['scratch']}"
