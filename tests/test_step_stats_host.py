"""sl2_get_step_stats on a machine without a GPU: the record's layout as the header declares it, the same layout in the ctypes
and NumPy mirrors, the exported symbol, and the wrappers of every layer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "scenelib2_amd.h")
# name, offset, bytes - the layout of the 96-byte record
LAYOUT = [("stepped", 0, 4), ("status_flags", 4, 4), ("sequence_steps", 8, 4), ("n_features", 12, 4), ("n_partial", 16, 4),
          ("n_visible", 20, 4), ("n_selected", 24, 4), ("n_matched", 28, 4), ("dof", 32, 4), ("worst_label", 36, 4),
          ("nis", 40, 8), ("log_det_S", 48, 8), ("min_pivot", 56, 8), ("max_pivot", 64, 8), ("worst_feature_d2", 72, 8),
          ("position_var", 80, 8), ("reserved", 88, 8)]


def test_the_header_lays_the_record_out_in_96_bytes():
    """The C compiler's view of include/scenelib2_amd.h: sizeof, alignment and every offsetof."""
    bdir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(bdir, exist_ok=True)
    src = os.path.join(bdir, "step_stats_layout.c")
    exe = os.path.join(bdir, "step_stats_layout")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n' % HEADER)
        f.write('  printf("sizeof %zu %zu\\n", sizeof(sl2_step_stats), _Alignof(sl2_step_stats));\n')
        for name, _, _ in LAYOUT:
            f.write('  printf("%s %%zu %%zu\\n", offsetof(sl2_step_stats, %s), sizeof(((sl2_step_stats*)0)->%s));\n' % (name, name, name))
        f.write("  return 0;\n}\n")
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-o", exe, src])
    lines = subprocess.check_output([exe], text=True).split("\n")
    assert lines[0] == "sizeof 96 8"
    assert [tuple(l.split()) for l in lines[1:] if l] == [(n, str(o), str(s)) for n, o, s in LAYOUT]


def test_ctypes_and_numpy_mirror_the_record():
    from scenelib2_amd import _lib
    assert C.sizeof(_lib.sl2_step_stats) == 96 and C.alignment(_lib.sl2_step_stats) == 8
    assert [(n, getattr(_lib.sl2_step_stats, n).offset, getattr(_lib.sl2_step_stats, n).size) for n, _, _ in LAYOUT] == LAYOUT
    dt = _lib.STEP_STATS_DTYPE
    assert dt.itemsize == 96 and list(dt.names) == [n for n, _, _ in LAYOUT]
    assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == LAYOUT
    assert all(dt.fields[n][0].base == (np.int32 if s == 4 or n == "reserved" else np.float64) for n, _, s in LAYOUT)


def test_the_symbol_is_declared_exported_and_bound():
    from scenelib2_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+sl2_get_step_stats\s*\(\s*sl2_engine\s*\*\s*e\s*,\s*int\s+seq0\s*,\s*int\s+nseq\s*,\s*sl2_step_stats\s*\*\s*out\s*,"
                     r"\s*int\s+out_on_device\s*\)\s*;", text)
    assert re.search(r"#define\s+SL2_API_VERSION\s+5\b", text)          # an addition within version 5
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        assert re.search(r"\bT sl2_get_step_stats$", out, flags=re.M), path
    assert "sl2_get_step_stats" in _lib.EXPORTED_SYMBOLS
    L = _lib.load()
    assert L.sl2_get_step_stats.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    # a null engine is refused before anything touches a device
    assert L.sl2_get_step_stats(None, 0, 1, None, 0) == _lib.SL2_ERR_INVALID


def test_every_layer_has_its_wrapper():
    from scenelib2_amd import Engine, MonoSLAM
    assert callable(Engine.step_stats) and callable(Engine.step_stats_device)
    assert isinstance(MonoSLAM.step_stats_, property)
    hpp = open(os.path.join(ROOT, "include", "scenelib2_amd_monoslam.hpp")).read()
    assert re.search(r"sl2_step_stats\s+StepStats\s*\(\s*\)", hpp) and "sl2_get_step_stats(eng_, 0, 1" in hpp
    mk = open(os.path.join(ROOT, "examples", "Makefile")).read()
    assert "watchdog_monoslam" in mk and os.path.exists(os.path.join(ROOT, "examples", "watchdog_monoslam.cpp"))


def test_the_documents_say_what_the_record_means():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "8c" in design and "sl2_get_step_stats" in design and "step_mark" in design and "chi-square" in design
    assert "sl2_get_step_stats" in open(os.path.join(ROOT, "README.md")).read()
    assert "sl2_get_step_stats" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
