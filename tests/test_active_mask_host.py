"""Host side of the per-sequence active mask and of the ragged ingest: the four entry points are declared in the header, exported
by both libraries, listed in _lib.EXPORTED_SYMBOLS and wrapped in Python, and the header says what each of them does.  (What they
do on the device: tests/test_gpu_active_mask.py.)"""
import inspect
import os
import re

from conftest import ROOT

NEW = ["sl2_set_active_sequences", "sl2_get_active_sequences", "sl2_ingest_frame_counts", "sl2_ingest_next_ragged"]


def _header():
    return open(os.path.join(ROOT, "include", "scenelib2_amd.h")).read()


def test_new_symbols_are_declared_exported_and_bound():
    from scenelib2_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), "%s is not declared" % name
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(L, name), "%s is not exported" % name
        assert getattr(L, name).argtypes, "%s has no ctypes signature" % name
    import subprocess
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        for name in NEW:
            assert re.search(r"\b%s$" % name, out, flags=re.M), (path, name)
    assert "#define SL2_API_VERSION 5" in _header()          # additions within version 5


def test_signatures_are_the_issue_s():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    flat = re.sub(r"\s+", " ", text)
    assert "int sl2_set_active_sequences(sl2_engine* e, int seq0, int nseq, const uint8_t* active, int on_device);" in flat
    assert "int sl2_get_active_sequences(sl2_engine* e, int seq0, int nseq, uint8_t* active);" in flat
    assert "int sl2_ingest_frame_counts(const sl2_ingest* g, int32_t* counts, int capacity);" in flat
    assert "int sl2_ingest_next_ragged(sl2_ingest* g, void* stream, const uint8_t** d_frames, size_t* seq_stride, uint8_t* have);" in flat


def test_python_wrappers_exist():
    from scenelib2_amd import Engine
    from scenelib2_amd.ingest import FrameIngest
    assert list(inspect.signature(Engine.set_active).parameters)[:3] == ["self", "mask", "seq0"]
    assert inspect.signature(Engine.set_active).parameters["seq0"].default == 0
    assert callable(Engine.active) and callable(FrameIngest.next_ragged)
    assert "frame_counts" in inspect.getsource(FrameIngest.__init__)


def test_header_documents_each_new_call():
    """The comment in front of each declaration says what the issue fixes about it."""
    h = _header()

    def comment_before(name):
        at = re.search(r"\n[a-z_ ]*\b%s\s*\(" % name, h).start()
        start = h.rfind("/*", 0, at)
        # several declarations may share one comment block: go back to the block that closes last before the declaration
        return h[start:at]

    c = comment_before("sl2_set_active_sequences")
    for phrase in ("consumed before the call returns", "engine's stream", "never waits", "bit for bit", "position log",
                   "sequence_steps", "not part of a sequence blob", "sl2_add_known_features", "sl2_delete_features",
                   "sl2_initialise_feature", "undefined"):
        assert phrase in c, phrase
    assert "Synchronises" in comment_before("sl2_get_active_sequences")
    c = comment_before("sl2_ingest_frame_counts")
    for phrase in ("sl2_ingest_next_ragged", "have[s]", "LONGEST", "unspecified", "SL2_ERR_CAPACITY", "SL2_ERR_INVALID", "zero-copy"):
        assert phrase in c, phrase
    assert "paused" in h[h.find("Algorithmic work of the last completed step"):h.find("#define SL2_STEP_WORK_COUNT")]


def test_design_and_readme_know_the_feature():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "sl2_set_active_sequences" in design and "m_gate" in design and "sel_gate" in design
    assert "cannot be paused" not in design
    assert re.search(r"\|\s*`?active`?[^|]*\|[^\n]*engine-global", design)
    assert "sl2_set_active_sequences" in open(os.path.join(ROOT, "README.md")).read()
    assert "next_ragged" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
