"""Host side of the per-sequence time step: the three entry points are declared in the header, exported by both libraries, listed
in _lib.EXPORTED_SYMBOLS and wrapped in Python; the adapters have SetDeltaT; no kernel keeps a `dt` launch argument.  (What they do
on the device: tests/test_gpu_seq_dt.py.)"""
import inspect
import os
import re
import subprocess

from conftest import ROOT

NEW = ["sl2_set_delta_t", "sl2_get_delta_t", "sl2_set_pause_catch_up"]
CSRC = os.path.join(ROOT, "scenelib2_amd", "csrc")


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
    assert "sl2_set_delta_t" in _header()[:_header().find("#define SL2_API_VERSION")]      # ... noted in the version history


def test_signatures_are_the_issue_s():
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S))
    assert "int sl2_set_delta_t(sl2_engine* e, int seq0, int nseq, const double* dt, int on_device);" in flat
    assert "int sl2_get_delta_t(sl2_engine* e, int seq0, int nseq, double* dt, double* owed, double* last_used);" in flat
    assert "int sl2_set_pause_catch_up(sl2_engine* e, int enabled);" in flat


def test_python_wrappers_and_adapters():
    from scenelib2_amd import Engine, MonoSLAM
    p = inspect.signature(Engine.set_delta_t).parameters
    assert list(p)[:4] == ["self", "dt", "seq0", "on_device"] and p["seq0"].default == 0 and p["on_device"].default is False
    p = inspect.signature(Engine.get_delta_t).parameters
    assert list(p) == ["self", "seq0", "nseq"] and p["seq0"].default == 0 and p["nseq"].default is None
    assert list(inspect.signature(Engine.set_pause_catch_up).parameters) == ["self", "enabled"]
    assert "kDeltaT_" in inspect.getsource(MonoSLAM.SetDeltaT) and "set_delta_t" in inspect.getsource(MonoSLAM.SetDeltaT)
    hpp = open(os.path.join(ROOT, "include", "scenelib2_amd_monoslam.hpp")).read()
    body = hpp[hpp.find("void SetDeltaT(double"):]
    body = body[:body.find("\n  }")]
    assert "sl2_set_delta_t" in body and "kDeltaT_ =" in body


def test_header_documents_the_contract():
    h = _header()
    c = _comment_before(h, "sl2_set_delta_t")
    flat = re.sub(r"[\s*]+", " ", c).lower()            # whatever the comment's line breaks
    for phrase in ("consumed before the call returns", "engine's stream", "never waits", "drops no captured step", "skips"):
        assert phrase in flat, phrase
    assert "Synchronises" in _comment_before(h, "sl2_get_delta_t") and "may be NULL" in _comment_before(h, "sl2_get_delta_t")
    c = _comment_before(h, "sl2_set_pause_catch_up")
    assert "cleared" in c and "drops no captured step" in c
    c = _comment_before(h, "sl2_set_active_sequences")
    assert "predicts over one delta_t" not in c and "sl2_set_pause_catch_up" in c and "nominal" in c
    assert re.search(r"double delta_t;\s*/\*[^\n]*initial", h)


def test_no_kernel_keeps_a_dt_launch_argument():
    """The time step is data the kernels read (a replayed graph must see a new one): params.delta_t is used on the host, to fill
    the record at sl2_create, and nowhere in a launch."""
    for name in ("sl2_frontend.hip", "sl2_small.hip", "sl2_mapping.hip", "sl2_frontend_dev.hpp"):
        src = open(os.path.join(CSRC, name)).read()
        assert "prm.delta_t" not in src and "double dt," not in src and "double dt)" not in src and "mp.dt" not in src, name
    dev = open(os.path.join(CSRC, "sl2_frontend_dev.hpp")).read()
    assert re.search(r"predict_body\([^)]*double\* __restrict__ seq_time\)", dev, flags=re.S)


def test_the_record_is_a_row_of_the_table_outside_the_blob():
    """Allocation, a group's view (+ kSeqTimeDoubles * first) and release are the table's (tests/test_seq_arrays_host.py checks
    their extents and offsets for every row); nothing in the engine does them by hand, and no blob carries the record."""
    arrays = open(os.path.join(CSRC, "sl2_seq_arrays.hpp")).read()
    assert "X(double, seq_time, kSeqTimeDoubles)" in arrays
    assert "seq_time" not in open(os.path.join(CSRC, "sl2_checkpoint.hip")).read()
    eng = open(os.path.join(CSRC, "sl2_engine.hip")).read()
    assert "g->seq_time" not in eng and "dmalloc(&e->seq_time" not in eng and "hipFree(e->seq_time)" not in eng
    assert "hipMemcpy(e->seq_time, rec.data()" in eng         # sl2_create fills it with params.delta_t
    setter = eng[eng.find("int sl2_set_delta_t("):eng.find("int sl2_get_delta_t(")]
    catch_up = eng[eng.find("int sl2_set_pause_catch_up("):eng.find("// ---", eng.find("int sl2_set_pause_catch_up("))]
    for body in (setter, catch_up):
        assert "drop_step_graphs" not in body and "sync_all" not in body and "Synchronize" not in body


def test_example_design_and_readme_know_the_feature():
    mk = open(os.path.join(ROOT, "examples", "Makefile")).read()
    assert re.search(r"^all:.*\bmixed_rate_monoslam\b", mk, flags=re.M) and "mixed_rate_monoslam.cpp" in mk
    ex = open(os.path.join(ROOT, "examples", "mixed_rate_monoslam.cpp")).read()
    for call in ("sl2_synth_render_host", "sl2_set_delta_t", "sl2_set_active_sequences", "sl2_go_one_step"):
        assert call in ex, call
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^#+ *8d\b", design, flags=re.M) and "seq_time" in design and "sl2_set_pause_catch_up" in design
    assert "`delta_t` is the engine's, not the sequence's" not in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "sl2_set_delta_t" in readme
