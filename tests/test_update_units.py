"""The dense EKF update is a translation unit per phase (sl2_update_build / _chol / _fwdsub / _syrk.hip), the plan's walk
(sl2_ekf_update.hip) and one TEST-only unit with the superseded kernels and the micro-benchmarks (sl2_update_testing.hip).

Every __global__ kernel, template instantiations included, must be defined in exactly one of them: two code objects that
register one kernel symbol leave it to the runtime which is launched.  And the phase units are compiled once for both
libraries, so no superseded kernel may sit in one.  Checked at build time on the device assembly (hipcc cross-compiles without
a GPU), the way tests/test_kernel_resources.py reads its descriptors."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scenelib2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

PRODUCT_UNITS = ["sl2_ekf_update.hip", "sl2_update_build.hip", "sl2_update_chol.hip", "sl2_update_fwdsub.hip", "sl2_update_syrk.hip"]
TEST_UNIT = "sl2_update_testing.hip"

# the product kernels of the update, as sl2_ekf_update.hip held them before it was split (demangled, without arguments)
PRODUCT_KERNELS = sorted(
    ["sl2::k_build_AS<1, 4>", "sl2::k_build_AS<2, 2>", "sl2::k_build_AS_ahead<4>", "sl2::k_build_AS_ahead<2>",
     "sl2::k_chol_left", "sl2::k_chol_syrk", "sl2::k_fwdsub_ksplit", "sl2::k_fwd_gemm", "sl2::k_syrk"] +
    ["sl2::k_fwdsub_lds<%d>" % nb for nb in range(1, 14)])
SUPERSEDED = ["sl2::k_build_A", "sl2::k_build_S", "sl2::k_chol_diag", "sl2::k_chol_panel", "sl2::k_chol_trail", "sl2::k_fwdsub",
              "sl2::k_gemm_kt"]

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")


def _kernel_symbols(src, out_dir):
    out = os.path.join(out_dir, src + ".s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-Wno-unused-value", "-Wno-unused-result",
           "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", out, "-ffp-contract=fast"]
    if src == TEST_UNIT:
        cmd += ["-DSL2_TESTING", "-Wno-pass-failed"]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    return re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(out).read(), re.M)


def _demangled(symbols):
    """'sl2::k_fwdsub_lds<7>' for the symbol of 'void sl2::k_fwdsub_lds<7>(double const*, ...)'."""
    names = []
    for s in symbols:      # _ZN3sl2 <length> <name> [I (Li <int> E)+ E] E <arguments>: the update's kernels take integer parameters only
        m = re.match(r"_ZN3sl2(\d+)", s)
        assert m, "not a kernel of namespace sl2: %s" % s
        end = m.end() + int(m.group(1))
        name, rest = s[m.end():end], s[end:]
        t = re.match(r"I((?:Li\d+E)+)E", rest)
        if t:
            name += "<%s>" % ", ".join(re.findall(r"Li(\d+)E", t.group(1)))
            rest = rest[t.end():]
        assert rest.startswith("E"), "unexpected template arguments in %s" % s
        names.append("sl2::" + name)
    return names


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """unit -> the kernels it defines"""
    out_dir = str(tmp_path_factory.mktemp("update_units"))
    units = PRODUCT_UNITS + [TEST_UNIT]
    with ThreadPoolExecutor(len(units)) as pool:
        symbols = list(pool.map(lambda u: _kernel_symbols(u, out_dir), units))
    return {u: _demangled(s) for u, s in zip(units, symbols)}


def test_every_kernel_is_defined_in_one_unit(kernels):
    seen = {}
    for unit, names in kernels.items():
        for n in names:
            assert n not in seen, "%s is defined in %s and in %s" % (n, seen[n], unit)
            seen[n] = unit


def test_product_units_hold_exactly_the_product_kernels(kernels):
    product = sorted(n for u in PRODUCT_UNITS for n in kernels[u])
    assert product == PRODUCT_KERNELS
    assert kernels["sl2_ekf_update.hip"] == [], "the plan's walk holds no kernel"


def test_superseded_kernels_are_in_the_test_unit_alone(kernels):
    test_only = kernels[TEST_UNIT]
    ubench = [n for n in test_only if n.startswith("sl2::k_ubench_")]
    assert len(ubench) >= 8, ubench      # k_ubench_mfma<1 | 4 | 8>, copy, write, read, fma64, mix
    for n in SUPERSEDED:
        assert n in test_only, "%s is not in %s" % (n, TEST_UNIT)
    for u in PRODUCT_UNITS:
        bad = [n for n in kernels[u] if n in SUPERSEDED or n.startswith("sl2::k_ubench_")]
        assert not bad, "%s holds %s" % (u, bad)
