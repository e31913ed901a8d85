"""Register budgets of the hot kernels, checked at build time (hipcc cross-compiles without a GPU).

Occupancy on gfx950 is decided by the unified register file: 512 / registers wavefronts per SIMD (in steps of 8
registers).  A change that pushes a kernel over its budget - or makes the compiler spill - does not fail any parity test,
it only shows up as a slower launch on the GPU box (round 2: a loop-carried index in k_chol_left cost six spilled
registers and 3 % of the launch).  This test reads the kernel descriptors of the device assembly."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scenelib2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel name fragment -> (file, extra flags, max total registers (arch + accumulator), wavefronts per SIMD that buys,
#                         scalar registers the compiler may park in vector lanes)
BUDGET = {
    "k_syrkEPKd": ("sl2_update_syrk.hip", ["-ffp-contract=fast"], 128, 4, 0),
    "k_fwdsub_ldsILi7E": ("sl2_update_fwdsub.hip", ["-ffp-contract=fast"], 168, 3, 0),
    "k_chol_left": ("sl2_update_chol.hip", ["-ffp-contract=fast"], 128, 4, 0),
    "k_build_ASILi1ELi4E": ("sl2_update_build.hip", ["-ffp-contract=fast"], 80, 6, 0),
    # (scalar spills: eleven in the workgroups that own positions - the records of two positions in flight - and nineteen more
    # on the path of the trailing workgroups that work off the large windows' units, which the others never enter; 39 in all
    # with the near-units exact walk on that path; round 5: 41 with the row coordinates of the ellipse test as floats)
    "k_search_mfma": ("sl2_search.hip", ["-ffp-contract=off"], 128, 4, 42),
    # the mapping step's per-job kernels (round 4): a job has a CU to itself, sixteen wavefronts = four per SIMD
    "k_map_me_search": ("sl2_mapping.hip", ["-ffp-contract=off"], 128, 4, 0),
    "k_map_find": ("sl2_mapping.hip", ["-ffp-contract=off"], 128, 4, 0),      # (region + detector: the detector's 1024 threads)
    "k_map_compact_slots": ("sl2_mapping.hip", ["-ffp-contract=off"], 168, 3, 8),
    # the fused small-map step's second kernel: three workgroups per CU at large batches, so three wavefronts per SIMD must fit
    # (149 registers and fourteen parked scalars)
    "k_small_back": ("sl2_small.hip", ["-ffp-contract=off"], 168, 3, 14),
}


def _assembly(src, flags, tmp_path):
    out = os.path.join(str(tmp_path), src + ".s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-Wno-unused-value", "-Wno-unused-result",
           "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", out] + flags
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    return open(out).read()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_hot_kernels_stay_inside_their_register_budgets(tmp_path):
    texts = {}
    for frag, (src, flags, max_regs, waves, max_sspill) in BUDGET.items():
        if src not in texts:
            texts[src] = _assembly(src, flags, tmp_path)
        t = texts[src]
        m = re.search(r"\.name:\s+(\S*%s\S*)\n(.*?)\.wavefront_size" % re.escape(frag), t, re.S)
        assert m, "kernel %s not found in %s" % (frag, src)
        meta = m.group(2)
        # the fields of one kernel descriptor follow its .name in any order up to the next kernel: take the enclosing block
        start = t.rfind("- .agpr_count", 0, m.start())
        end = t.find("- .agpr_count", m.end())
        block = t[start:end if end > 0 else len(t)]
        vg = int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1))
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        sspills = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", block).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        assert spills == 0 and scratch == 0, "%s spills (%d vector registers, %d bytes of scratch)" % (frag, spills, scratch)
        assert sspills <= max_sspill, "%s spills %d scalar registers (allowed %d)" % (frag, sspills, max_sspill)
        assert vg <= max_regs, "%s uses %d registers, budget %d (= %d wavefronts per SIMD)" % (frag, vg, max_regs, waves)
        assert 512 // ((vg + 7) // 8 * 8) >= waves


def _descriptor(text, frag):
    m = re.search(r"\.name:\s+(\S*%s\S*)\n" % re.escape(frag), text)
    assert m, "kernel %s not found" % frag
    start = text.rfind("- .agpr_count", 0, m.start())
    end = text.find("- .agpr_count", m.end())
    return text[start:end if end > 0 else len(text)]


def _constexpr(src, name):
    m = re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, src)).read())
    assert m, "%s not found in %s" % (name, src)
    return int(m.group(1))


LDS_PER_CU = 160 * 1024          # gfx950


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_small_back_leaves_room_for_three_workgroups_per_cu(tmp_path):
    """k_small_back's LDS: its static arrays (the update's sH, sR, sPos, sS, sLinv, sCol and the bookkeeping bodies' own) plus the
    largest dynamic region launch_small_back asks for - the [32][kSmallW] panel of doubles, or the bookkeeping phases' scratch at
    the largest capacity sl2_create accepts (ld <= 2048) if that were bigger - must fit a third of the CU's LDS: three workgroups
    per CU at large batches (sl2_small.hip).  A static array added to the kernel fails no parity test; it fails this one."""
    block = _descriptor(_assembly("sl2_small.hip", ["-ffp-contract=off"], tmp_path), "k_small_back")
    static = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
    panel = 8 * _constexpr("sl2_step_plan.hpp", "kSmallM") * _constexpr("sl2_step_plan.hpp", "kSmallW")
    n_max = (2048 - 13 - 6 - 1) // 3                       # ld = roundup(13 + 3 N + 6 kpart + 1, 64) <= 2048, kpart >= 1
    scratch = 4 * (2 * n_max + 10) + 8 * (16 + 169 + 169 + 16 * _constexpr("sl2_seq_arrays.hpp", "kWorkDoubles"))
    dyn = max(panel, scratch)
    assert static + dyn <= LDS_PER_CU // 3, "k_small_back: %d B static + %d B dynamic > %d B (a third of the CU's LDS)" % (
        static, dyn, LDS_PER_CU // 3)
