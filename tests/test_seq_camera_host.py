"""Host side of the per-sequence camera calibration: the two entry points are declared in the header, exported by both libraries,
listed in _lib.EXPORTED_SYMBOLS and wrapped in Python; the adapters have SetCameraParameters; the record is one 64-byte line per
sequence; no step kernel keeps a camera in its launch arguments.  (What they do on the device: tests/test_gpu_seq_camera.py.)"""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

NEW = ["sl2_set_cameras", "sl2_get_cameras"]
CSRC = os.path.join(ROOT, "scenelib2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _header():
    return open(os.path.join(ROOT, "include", "scenelib2_amd.h")).read()


def _comment_before(h, name):
    at = re.search(r"\n[a-z_ ]*\b%s\s*\(" % name, h).start()
    return h[h.rfind("/*", 0, at):at]


def test_new_symbols_are_declared_exported_and_bound():
    from scenelib2_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), "%s is not declared" % name
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(L, name), "%s is not exported" % name
        assert getattr(L, name).argtypes, "%s has no ctypes signature" % name
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        for name in NEW:
            assert re.search(r"\b%s$" % name, out, flags=re.M), (path, name)
    assert "#define SL2_API_VERSION 5" in _header()          # additions within version 5
    history = _header()[:_header().find("#define SL2_API_VERSION")]
    assert all(name in history for name in NEW)              # ... noted in the version history
    assert "#define SL2_BLOB_LAYOUT_VERSION 1" in _header()  # the blob records the sequence's camera in the field it always had


def test_signatures_are_the_issue_s():
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S))
    assert "int sl2_set_cameras(sl2_engine* e, int seq0, int nseq, const sl2_camera* cams);" in flat
    assert "int sl2_get_cameras(sl2_engine* e, int seq0, int nseq, sl2_camera* cams);" in flat


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_the_record_is_one_cache_line_and_the_camera_struct_is_unchanged():
    """tests/seq_cam_host.cpp: sl2_common.hpp compiled for the host (its static_asserts hold the record to 8 doubles = 64 bytes,
    the six intrinsics in places 0 .. 5)."""
    from scenelib2_amd import _lib
    bdir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(bdir, exist_ok=True)
    so = os.path.join(bdir, "libseq_cam_host.so")
    src = os.path.join(ROOT, "tests", "seq_cam_host.cpp")
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "include")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-result", "-D__HIP_PLATFORM_AMD__", "-I" + inc,
                           "-shared", "-o", so, src])
    L = C.CDLL(so)
    assert L.sc_record_bytes() == 64
    assert L.sc_camera_bytes() == 56 == C.sizeof(_lib.sl2_camera)          # sizeof(sl2_camera) as before this feature
    assert L.sc_blob_header_bytes() == 256
    table = open(os.path.join(CSRC, "sl2_seq_arrays.hpp")).read()      # the extents of the table's rows are declared with it
    m = re.search(r"constexpr int kSeqCamDoubles = (\d+)", table)
    assert m and int(m.group(1)) * 8 == 64
    assert table.find("kSeqCamDoubles") > table.find("kSeqTimeDoubles") > 0         # declared beside the time record's


def test_the_chunk_of_the_host_form_fits_the_kernel_argument_segment():
    eng = open(os.path.join(CSRC, "sl2_engine.hip")).read()
    chunk = int(re.search(r"constexpr int kCamChunk = (\d+);", eng).group(1))
    assert chunk == 64                                        # what tests/test_gpu_seq_camera.py sizes its batch by
    assert chunk * 6 * 8 + 8 + 4 <= 4096
    assert "struct CamChunk { double v[kCamChunk][6]; };" in eng


def test_python_wrappers_and_adapters():
    from scenelib2_amd import Engine, MonoSLAM
    p = inspect.signature(Engine.set_cameras).parameters
    assert list(p) == ["self", "cams", "seq0"] and p["seq0"].default == 0
    p = inspect.signature(Engine.get_cameras).parameters
    assert list(p) == ["self", "seq0", "nseq"] and p["seq0"].default == 0 and p["nseq"].default is None
    src = inspect.getsource(MonoSLAM.SetCameraParameters)
    assert "camera_" in src and "set_cameras" in src
    assert list(inspect.signature(MonoSLAM.SetCameraParameters).parameters) == ["self", "width", "height", "fku", "fkv", "u0", "v0", "kd1", "sd"]
    hpp = open(os.path.join(ROOT, "include", "scenelib2_amd_monoslam.hpp")).read()
    body = hpp[hpp.find("void SetCameraParameters("):]
    body = body[:body.find("\n  }")]
    assert "sl2_set_cameras" in body and "camera_->fku_ =" in body and "camera_->centre_ =" in body
    ref = open(os.path.join(ROOT, "examples", "ref_binding", "monoslam_amd.h")).read()
    assert "void SetCameraParameters(const int camera_width, const int camera_height" in ref and "impl_.SetCameraParameters(" in ref


def test_header_documents_the_contract():
    h = _header()
    flat = re.sub(r"[\s*]+", " ", _comment_before(h, "sl2_set_cameras")).lower()      # whatever the comment's line breaks
    for phrase in ("consumed before the call returns", "engine's stream", "never waits", "drops no captured step",
                   "mask is not consulted", "nothing changed", "width / height", "not finite", "sd < 0", "destination sequence's"):
        assert phrase in flat, phrase
    c = _comment_before(h, "sl2_get_cameras")
    assert "does NOT synchronise" in c and "width / height" in c
    assert "sl2_set_cameras" in _comment_before(h, "sl2_load_sequences")


def test_no_step_kernel_keeps_a_camera_launch_argument():
    """The calibration is data the kernels read (a replayed graph must see a new one): among the __global__ functions only the
    synthetic renderer, which is no step kernel, takes a CameraParams by value."""
    found = []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith(".hip"):
            continue
        src = open(os.path.join(CSRC, name)).read()
        for m in re.finditer(r"__global__[^{;]*?\b(k_\w+)\s*\(([^{;]*?)\)\s*\{", src, flags=re.S):
            if "CameraParams" in m.group(2):
                found.append(m.group(1))
    assert found == ["k_synth_render"], found
    for name in ("sl2_frontend.hip", "sl2_small.hip", "sl2_mapping.hip"):
        src = open(os.path.join(CSRC, name)).read()
        assert "e->cam," not in src and "load_cam(" in src, name
        assert not re.search(r"e->cam\.(fku|fkv|u0|v0|kd1|sd)\b", src), name
    # the shared models are as they were: they take the struct by reference
    math = open(os.path.join(CSRC, "sl2_math.hpp")).read() + open(os.path.join(CSRC, "sl2_mapmath.hpp")).read()
    for fn in ("measurement_model", "visibility_test", "part_create_model", "part_measurement_model"):
        assert re.search(r"\b%s\(const CameraParams& cam," % fn, math), fn


def test_the_record_is_a_row_of_the_table_and_only_the_setter_writes_it():
    """Allocation, a group's view (+ kSeqCamDoubles * first) and release are the table's (tests/test_seq_arrays_host.py checks
    their extents and offsets for every row); nothing in the engine does them by hand."""
    assert "X(double, seq_cam, kSeqCamDoubles)" in open(os.path.join(CSRC, "sl2_seq_arrays.hpp")).read()
    eng = open(os.path.join(CSRC, "sl2_engine.hip")).read()
    assert "g->seq_cam" not in eng and "dmalloc(&e->seq_cam" not in eng and "hipFree(e->seq_cam)" not in eng
    assert "hipMemcpy(e->seq_cam, rec.data()" in eng          # sl2_create fills it with the engine's calibration
    setter = eng[eng.find("int sl2_set_cameras("):eng.find("int sl2_get_cameras(")]
    getter = eng[eng.find("int sl2_get_cameras("):eng.find("// ---", eng.find("int sl2_get_cameras("))]
    for body in (setter, getter):
        assert "drop_step_graphs" not in body and "sync_all" not in body and "Synchronize" not in body and "hipMemcpy" not in body
    ck = open(os.path.join(CSRC, "sl2_checkpoint.hip")).read()
    assert ck.count("seq_cam") == 2 and "const double* rec = S.seq_cam +" in ck      # the pack kernel reads it (and a comment names it) ...
    unpack = ck[ck.find("void __launch_bounds__(kCkptThreads) k_seq_unpack"):ck.find("static CkptParams ckpt_params(")]      # (the whole kernel)
    assert "k_seq_unpack(const SeqArrays S" in unpack and "S.n_slots[b] = ns" in unpack and "seq_cam" not in unpack      # ... the unpack kernel does not touch it
    assert "cams_host[dst_seq]" in ck and '"camera"' in ck


def test_example_design_and_readme_know_the_feature():
    mk = open(os.path.join(ROOT, "examples", "Makefile")).read()
    assert re.search(r"^all:.*\bmixed_camera_monoslam\b", mk, flags=re.M) and "mixed_camera_monoslam.cpp" in mk
    ex = open(os.path.join(ROOT, "examples", "mixed_camera_monoslam.cpp")).read()
    for call in ("sl2_synth_render_host", "sl2_set_cameras", "sl2_get_cameras", "sl2_go_one_step"):
        assert call in ex, call
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^#+ *8e\b", design, flags=re.M) and "seq_cam" in design and "sl2_set_cameras" in design
    sec = design[re.search(r"^#+ *8e\b", design, flags=re.M).start():]
    assert "seq_cam_ab.json" in sec and "image size" in sec and "sharding" in sec
    assert "sl2_set_cameras" in open(os.path.join(ROOT, "README.md")).read()
    assert "sl2_set_cameras" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "seq_cam_ab.json"))
