"""Resource budget of k_build_AS_ahead (sl2_update_build.hip), checked at build time like tests/test_kernel_resources.py.

The form exists to keep more bytes in flight per CU than k_build_AS, so what it may spend is fixed: at most 96 registers
(five wavefronts per SIMD; the kernel as measured uses 80, six per SIMD), nothing spilled, and at most 40 KB of LDS per workgroup - four workgroups of the headline shape
(ld = 320: five wavefronts each) share a CU's 160 KB, twenty wavefronts per CU.  Its LDS is dynamic: 2 * BATCH rows of At of ld
doubles and the measurement table, kAheadEntry doubles for each of the engine's number_of_features_to_select.
make_update_plan (sl2_update_plan.hpp, where the two constants live) takes BATCH = 4 where that fits kAheadLdsMax, else 2, else
k_build_AS; the rule is restated here."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scenelib2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = "sl2_update_build.hip"
PLAN_HDR = "sl2_update_plan.hpp"
MAX_REGS, MAX_LDS = 96, 40 * 1024

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("build_ahead")), SRC + ".s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-Wno-unused-value", "-Wno-unused-result",
           "--cuda-device-only", "-S", os.path.join(CSRC, SRC), "-o", out, "-ffp-contract=fast"]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    return open(out).read()


def descriptor(text, frag):
    m = re.search(r"\.name:\s+(\S*%s\S*)\n" % re.escape(frag), text)
    assert m, "kernel %s not found" % frag
    start = text.rfind("- .agpr_count", 0, m.start())
    end = text.find("- .agpr_count", m.end())
    return text[start:end if end > 0 else len(text)]


def field(block, name):
    return int(re.search(r"\.%s:\s+(\d+)" % name, block).group(1))


def constexpr(name):
    m = re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, PLAN_HDR)).read())
    assert m, "%s not found in %s" % (name, PLAN_HDR)
    return int(m.group(1))


def launch_choice(ld, nsel):
    """(BATCH, dynamic LDS bytes) of make_update_plan for one workgroup per sequence, or (0, 0): k_build_AS."""
    entry, cap = constexpr("kAheadEntry"), constexpr("kAheadLdsMax")
    if ld > 1024:
        return 0, 0
    for batch in (4, 2):
        shm = 8 * (2 * batch * ld + entry * nsel)
        if shm <= cap:
            return batch, shm
    return 0, 0


@pytest.mark.parametrize("batch", [4, 2])
def test_registers_and_no_spills(assembly, batch):
    block = descriptor(assembly, "k_build_AS_aheadILi%dE" % batch)
    vg = field(block, "vgpr_count")
    assert field(block, "vgpr_spill_count") == 0 and field(block, "private_segment_fixed_size") == 0, "k_build_AS_ahead<%d> spills" % batch
    assert field(block, "sgpr_spill_count") == 0
    assert vg <= MAX_REGS, "k_build_AS_ahead<%d> uses %d registers, budget %d (five wavefronts per SIMD)" % (batch, vg, MAX_REGS)
    assert 512 // ((vg + 7) // 8 * 8) >= 5


# (ld, number_of_features_to_select): the headline shape (1024 x 100 features, all selected) and the largest ld the form takes,
# with the 24 selected features of tests/ekf_update_cases.py: f_build_ld1024
@pytest.mark.parametrize("ld,nsel,want_batch", [(320, 100, 4), (1024, 24, 2)])
def test_lds_leaves_room_for_four_workgroups_per_cu(assembly, ld, nsel, want_batch):
    assert constexpr("kAheadLdsMax") <= MAX_LDS
    batch, dyn = launch_choice(ld, nsel)
    assert batch == want_batch, "ld = %d, %d selected: the launch takes BATCH = %d" % (ld, nsel, batch)
    static = field(descriptor(assembly, "k_build_AS_aheadILi%dE" % batch), "group_segment_fixed_size")
    assert static + dyn <= MAX_LDS, "k_build_AS_ahead<%d> at ld = %d: %d B static + %d B dynamic > %d B" % (batch, ld, static, dyn, MAX_LDS)


def test_old_fragment_matches_the_old_kernel_only(assembly):
    """tests/test_kernel_resources.py finds k_build_AS<1,4> by the fragment k_build_ASILi1ELi4E: the new kernel's name must not
    contain it."""
    names = re.findall(r"\.name:\s+(\S*k_build_ASILi1ELi4E\S*)\n", assembly)
    assert len(names) == 1 and "ahead" not in names[0], names
