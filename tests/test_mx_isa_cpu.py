"""CPU suite: the register form of the matrix-core top-2 search (bf_mx.hip), on the built library's gfx950 code object.
The kernel is bound by vector issue, so its MFMA accumulators and their C operand must live in VGPRs (the Makefile builds
bf_mx.hip with -amdgpu-mfma-vgpr-form): a toolchain that drops the option brings back 32 v_accvgpr_* per 16-row group, and
one that needs more than 128 registers drops the kernel to three waves per SIMD.  Both are caught here, at build time."""
import os
import re
import shutil
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
OBJDUMP = os.path.join(LLVM, "llvm-objdump")
READELF = os.path.join(LLVM, "llvm-readelf")


@pytest.fixture(scope="module")
def mx_kernel(built, tmp_path_factory):
    """(disassembly of bf_top2_mx_kernel, its metadata note) from the library the package loads."""
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm-objdump / llvm-readelf of the ROCm toolchain not found")
    from slamhip import _lib

    tmp = str(tmp_path_factory.mktemp("mx_isa"))
    local = os.path.join(tmp, "lib.so")
    shutil.copy(_lib.LIB_PATH, local)
    subprocess.run([OBJDUMP, "--offloading", local], cwd=tmp, check=True, capture_output=True)
    for f in sorted(os.listdir(tmp)):                               # one gfx950 code object per source file
        if "gfx950" not in f:
            continue
        obj = os.path.join(tmp, f)
        text = subprocess.run([OBJDUMP, "-d", obj], check=True, capture_output=True, text=True).stdout
        m = re.search(r"^[0-9a-f]+ <(_Z\d+bf_top2_mx_kernel\w*)>:$", text, re.M)
        if not m:
            continue
        body = text[m.end():].split("\n\n", 1)[0]
        notes = subprocess.run([READELF, "--notes", obj], check=True, capture_output=True, text=True).stdout
        meta = next(b for b in re.split(r"\n\s+- \.agpr_count", notes) if re.search(r"\.name:\s+" + m.group(1) + r"\n", b))
        return body, "\n    - .agpr_count" + meta
    pytest.fail("bf_top2_mx_kernel is not in the library")


def field(meta, key):
    m = re.search(rf"\.{key}:\s+(\d+)", meta)
    assert m, f"no .{key} in the kernel's metadata"
    return int(m.group(1))


def test_accumulators_stay_in_vgprs(mx_kernel):
    body, meta = mx_kernel
    hits = [ln.strip() for ln in body.splitlines() if "v_accvgpr_" in ln]
    assert not hits, f"{len(hits)} v_accvgpr_* in bf_top2_mx_kernel (was -amdgpu-mfma-vgpr-form dropped?): {hits[:2]}"
    assert field(meta, "agpr_count") == 0
    # the eight MFMAs of a group read C from and write D to VGPRs
    mfma = [ln for ln in body.splitlines() if "v_mfma" in ln]
    assert len(mfma) >= 8 and not any(re.search(r"\ba\[?\d", ln.split("v_mfma", 1)[1]) for ln in mfma), mfma[:2]


def test_four_waves_per_simd(mx_kernel):
    _, meta = mx_kernel
    # gfx950: 512 registers per SIMD lane, VGPRs and AGPRs of a wave allocated together in blocks of 8
    vgpr, agpr = field(meta, "vgpr_count"), field(meta, "agpr_count")
    assert vgpr + agpr <= 128, (vgpr, agpr)


def test_no_spills_and_no_scratch(mx_kernel):
    body, meta = mx_kernel
    assert "scratch_" not in body, "the MX kernel touches scratch"
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        assert field(meta, key) == 0, key


def test_fold_is_integer_and_branches_are_uniform(mx_kernel):
    body, _ = mx_kernel
    # the group fold: eight signed integer maxima on the bit patterns, no float maximum (and so no NaN canonicalisation)
    assert len([ln for ln in body.splitlines() if "v_max3_i32" in ln]) >= 7
    assert not [ln for ln in body.splitlines() if re.search(r"v_max3?_f32", ln)]
