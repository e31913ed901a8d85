"""The descriptors of the frame converter's five kernels (scenelib2_amd/csrc/sl2_convert.hip, sl2_convert_remap.hip): each unit
is cross-compiled to assembly ONCE for the whole file, with the Makefile's code generation flags, and every kernel's registers,
spills, scratch and LDS are held to the budget its comment states.  (What the kernels compute: tests/test_gpu_frame_*.py; which
of them a sequence goes to and the dynamic LDS of a launch: tests/test_convert_plan_host.py.)"""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "scenelib2_amd", "csrc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")


def _assembly(tmp, unit):
    out = os.path.join(tmp, unit + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-Wno-unused-value",
                    "-Wno-unused-result", "--cuda-device-only", "-S", os.path.join(CSRC, unit + ".hip"), "-o", out],
                   check=True, capture_output=True, timeout=900)
    return open(out).read()


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    """The device assembly of both units, by unit name."""
    tmp = str(tmp_path_factory.mktemp("frame_convert_kernels"))
    return {unit: _assembly(tmp, unit) for unit in ("sl2_convert", "sl2_convert_remap")}


def test_kernel_leaves_room_for_two_workgroups_per_cu_and_does_not_spill(assembly):
    """k_convert_frames' descriptor: its static LDS (the staged grey rows and the slot lists) fits a CU's 160 KB eight times, the width cap fits a pass of two output rows, and nothing spills."""
    text = assembly["sl2_convert"]
    m = re.search(r"\.name:\s+\S*k_convert_frames\S*\n", text)
    assert m
    block = text[text.rfind("- .agpr_count", 0, m.start()):]
    lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
    assert lds <= 160 * 1024 // 8, lds          # eight workgroups a CU (the issue asks for two at least)
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0
    assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", block).group(1)) <= 8          # scalars parked in vector lanes, no memory
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)) <= 64           # eight wavefronts per SIMD: eight workgroups of four a CU
    hdr = open(os.path.join(CSRC, "sl2_convert_dev.hpp")).read()
    cap = int(re.search(r"constexpr int kConvertMaxWidth = (\d+);", hdr).group(1))
    assert cap >= 4096 and int(re.search(r"constexpr int kConvertMaxHeight = (\d+);", hdr).group(1)) == 16384
    assert lds >= 4 * (cap + 16)          # four staged rows at the cap: a pass of two output rows


def test_area_kernel_does_not_spill_and_its_lds_leaves_the_stated_workgroups_per_cu(assembly):
    """k_convert_area's descriptor, by the budget its comment states: no scratch, no spilled vector register, at most 80 registers
    (six workgroups a CU by registers), and static LDS that with colsum - a word per source column of the widest listed source -
    fits a CU's 160 KB six times up to 2400 columns and four times at the width cap."""
    text = assembly["sl2_convert"]
    m = re.search(r"\.name:\s+\S*k_convert_area\S*\n", text)
    assert m
    block = text[text.rfind("- .agpr_count", 0, m.start()):]
    lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
    assert 6 * (lds + 4 * 2400) <= 160 * 1024, lds
    assert 4 * (lds + 4 * 4096) <= 160 * 1024, lds
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)) <= 80


def test_raw_kernels_do_not_spill_and_their_lds_leaves_the_stated_workgroups_per_cu(assembly):
    """k_raw_linear's and k_raw_area's descriptors: no scratch, no spilled vector register, at most 80 registers (six workgroups a
    CU by registers), and static LDS that, with the dynamic part DESIGN.md section 8f states - the raw stage, 16448 bytes at
    most, and for the area kernel a word per source column, 16384 bytes at the cap - still fits a CU's 160 KB three times at the
    width cap and four times with a 1280-column Bayer source."""
    text = assembly["sl2_convert"]
    src = open(os.path.join(CSRC, "sl2_convert_plan.hpp")).read()
    stage_cap = 4 * (4096 + 16)
    assert re.search(r"constexpr int kRawLdsBytes = 4 \* \(kConvertMaxWidth \+ 16\);", src)
    stage_1280 = min(18 * ((1280 + 30) & ~15), stage_cap)
    for name, dyn_cap, dyn_1280 in (("k_raw_linear", stage_cap, stage_1280), ("k_raw_area", stage_cap + 4 * 4096, stage_1280 + 4 * 1280)):
        assert "k_convert_frames" not in name and "k_convert_area" not in name
        m = re.search(r"\.name:\s+\S*%s\S*\n" % name, text)
        assert m, name
        block = text[text.rfind("- .agpr_count", 0, m.start()):]
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
        assert lds >= 4 * (4096 + 16)                      # four staged grey rows at the width cap: a pass of two output rows
        assert 3 * (lds + dyn_cap) <= 160 * 1024, (name, lds)
        assert 4 * (lds + dyn_1280) <= 160 * 1024, (name, lds)
        assert 6 * lds <= 160 * 1024, (name, lds)          # no Bayer source, deep grey under LINEAR: six workgroups a CU
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)) <= 80


def test_remap_kernel_does_not_spill_and_uses_no_scratch_and_no_lds(assembly):
    """k_convert_remap's descriptor: no scratch, no spilled register, no LDS (a gather: nothing is staged, and no per-lane array
    may have been moved there), at most 80 registers - six waves a SIMD, the launch bound of its siblings (at 64 registers the
    sixteen Bayer bytes of each of a lane's four pixels spilled)."""
    text = assembly["sl2_convert_remap"]
    m = re.search(r"\.name:\s+\S*k_convert_remap\S*\n", text)
    assert m
    block = text[text.rfind("- .agpr_count", 0, m.start()):]
    block = block[:block.find("- .agpr_count", 10)] if block.find("- .agpr_count", 10) > 0 else block
    assert "k_convert_remap" in block
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0
    assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", block).group(1)) == 0
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0
    assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1)) == 0
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)) <= 80
