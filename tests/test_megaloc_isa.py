"""CPU: the compiled gfx950 code of the MegaLoc kernels (``gtsfm_amd/csrc/megaloc_kernels.hip``, ``splitk_linear.h``): nothing spills, the LDS
allocations are what DESIGN.md states, and the patch embedding multiplies on the fp32 MFMA. Compiles the file to assembly (hipcc
cross-compiles without a GPU) and reads every kernel descriptor."""

import re
import subprocess

import pytest

from conftest import REPO

CSRC = REPO / "gtsfm_amd" / "csrc"
KERNELS = ("ml_patch_embed_kernel", "ml_layernorm_kernel", "ml_gelu_kernel", "ml_problems_kernel", "ml_salad_kernelILb1", "ml_salad_kernelILb0",
           "sk_linear_kernelILi5", "sk_finish_kernel")
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    from gtsfm_amd.csrc import build

    out = tmp_path_factory.mktemp("isa") / "megaloc_kernels.s"
    flags = [f for f in build.FLAGS if f not in ("-Wall",)]
    cmd = [build.HIPCC, *flags, "-I", str(REPO / "include"), "-S", "--cuda-device-only", str(CSRC / "megaloc_kernels.hip"), "-o", str(out)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    return out.read_text()


def _kernels(assembly: str) -> dict:
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", assembly, re.S):
        field = lambda key: int(re.search(key + r"\s+(\d+)", m.group(2)).group(1))  # noqa: E731
        body = assembly[assembly.index(f"\n{m.group(1)}:") : m.start()]
        out[m.group(1)] = {"vgprs": field(r"\.amdhsa_next_free_vgpr"), "scratch": field(r"\.amdhsa_private_segment_fixed_size"),
                           "lds": field(r"\.amdhsa_group_segment_fixed_size"), "body": body}
    return out


def _find(kernels: dict, key: str) -> dict:
    hits = [v for k, v in kernels.items() if key in k]
    assert len(hits) == 1, (key, sorted(kernels))
    return hits[0]


def test_every_kernel_is_there_and_none_spills(assembly):
    kernels = _kernels(assembly)
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for key in KERNELS:
        d = _find(kernels, key)
        assert d["scratch"] == 0, f"{key}: private_segment_fixed_size = {d['scratch']}"
        assert d["vgprs"] <= 256, (key, d["vgprs"])
    assert _find(kernels, "ml_salad_kernelILb1")["vgprs"] <= 128  # 1024 threads = 4 waves per SIMD: at most 128 registers each


def test_lds_allocations_are_what_design_states(assembly):
    kernels = _kernels(assembly)
    # patch embedding: the patch and the weight chunk, [64][99] floats each, static
    assert _find(kernels, "ml_patch_embed_kernel")["lds"] == 2 * 64 * 99 * 4 == 50688
    # SALAD: all of it dynamic, (512 + ceil64(n) + 65 n) floats: 141,892 bytes at 322 x 322 (n = 529), inside the CU's 160 KiB up to n = 612
    for key in ("ml_salad_kernelILb1", "ml_salad_kernelILb0"):
        assert _find(kernels, key)["lds"] == 0
    salad_bytes = lambda n: (512 + (n + 63) // 64 * 64 + 65 * n) * 4  # noqa: E731
    assert salad_bytes(529) == 141892 and salad_bytes(612) <= LDS_PER_CU < salad_bytes(613)
    assert _find(kernels, "sk_finish_kernel")["lds"] == 64 and _find(kernels, "sk_linear_kernelILi5")["lds"] == 0


def test_matrix_instructions_are_where_they_should_be(assembly):
    kernels = _kernels(assembly)
    mfma = lambda key: re.findall(r"^\s*(v_mfma_\w+)", _find(kernels, key)["body"], re.M)  # noqa: E731
    patch = mfma("ml_patch_embed_kernel")
    assert patch and set(patch) == {"v_mfma_f32_32x32x2_f32"}, set(patch)
    for key in KERNELS[1:]:
        assert not mfma(key), key  # the other products of the forward are launch_gemm / launch_attention (tests/test_gemm_isa.py)
    # the Sinkhorn runs in the kernel, out of LDS: exponentials, logarithms and LDS reads are all there
    salad = _find(kernels, "ml_salad_kernelILb1")["body"]
    assert "v_exp_f32" in salad and "v_log_f32" in salad and "ds_read" in salad
