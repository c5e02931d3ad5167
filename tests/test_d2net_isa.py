"""CPU: the compiled gfx950 code of D2-Net's dilated convolution (``conv3x3_dil2_mfma_kernel``, ``gtsfm_amd/csrc/dense_kernels.hip``): it
multiplies on the fp32 32 x 32 x 2 MFMA inside its loop and nothing spills. Compiles the file to assembly (hipcc cross-compiles without a
GPU) and reads the kernel's descriptor and body."""

import re
import subprocess

import pytest

from conftest import REPO

CSRC = REPO / "gtsfm_amd" / "csrc"
KERNEL = "conv3x3_dil2_mfma_kernel"


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    from gtsfm_amd.csrc import build

    out = tmp_path_factory.mktemp("isa") / "dense_kernels.s"
    flags = [f for f in build.FLAGS if f not in ("-Wall",)]
    cmd = [build.HIPCC, *flags, "-I", str(REPO / "include"), "-S", "--cuda-device-only", str(CSRC / "dense_kernels.hip"), "-o", str(out)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    return out.read_text()


def _kernel(assembly: str) -> dict:
    hits = [m for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", assembly, re.S) if KERNEL in m.group(1)]
    assert len(hits) == 1, [m.group(1) for m in hits]
    m = hits[0]
    field = lambda key: int(re.search(key + r"\s+(\d+)", m.group(2)).group(1))  # noqa: E731
    start = assembly.index(f"\n{m.group(1)}:")
    body = assembly[start : assembly.index("s_endpgm", start)]
    return {"vgprs": field(r"\.amdhsa_next_free_vgpr"), "scratch": field(r"\.amdhsa_private_segment_fixed_size"),
            "lds": field(r"\.amdhsa_group_segment_fixed_size"), "body": body}


def test_dilated_kernel_has_no_scratch(assembly):
    k = _kernel(assembly)
    assert k["scratch"] == 0, f"private_segment_fixed_size = {k['scratch']}"


def test_dilated_kernel_multiplies_on_the_fp32_mfma_in_its_loop(assembly):
    body = _kernel(assembly)["body"]
    mfma = re.findall(r"^\s*(v_mfma_\w+)", body, re.M)
    assert mfma and set(mfma) == {"v_mfma_f32_32x32x2_f32"}, set(mfma)
    # inside a loop: a backward branch follows MFMAs, and the loop body reads its A fragments from LDS as 16-byte reads
    lines = body.splitlines()
    labels = {ln.split(":")[0].strip(): i for i, ln in enumerate(lines) if re.match(r"^\.?\w+:\s*(;.*)?$", ln.strip())}
    loops = []
    for i, ln in enumerate(lines):
        m = re.match(r"\s*s_cbranch_\w+\s+(\S+)", ln) or re.match(r"\s*s_branch\s+(\S+)", ln)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append((labels[m.group(1)], i))
    assert loops, "no backward branch in the kernel"
    inner = [(a, b) for a, b in loops if any("v_mfma_f32_32x32x2_f32" in ln for ln in lines[a:b])]
    assert inner, "no loop holds an MFMA"
    a, b = min(inner, key=lambda ab: ab[1] - ab[0])
    loop_text = "\n".join(lines[a:b])
    assert loop_text.count("v_mfma_f32_32x32x2_f32") >= 64 and "ds_read_b128" in loop_text  # at least one tap: 8 k-steps x 8 MFMAs
