"""Save / restore / copy / reset of sequences, the part that needs no GPU: the five entry points are exported and declared, the
blob layout arithmetic of the library equals its restatement here, and the two kernels neither spill nor use scratch."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "scenelib2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ENTRY_POINTS = ["sl2_sequence_blob_capacity", "sl2_save_sequences", "sl2_load_sequences", "sl2_copy_sequences", "sl2_reset_sequences"]


def test_entry_points_are_exported_and_declared():
    from scenelib2_amd import _lib
    text = open(os.path.join(ROOT, "include", "scenelib2_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        exported = set(re.findall(r"\b(sl2_[a-z0-9_]+)$", out, flags=re.M))
        for name in ENTRY_POINTS:
            assert name in exported, "%s lacks %s" % (os.path.basename(path), name)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, text), "%s is not declared in scenelib2_amd.h" % name
        assert name in _lib.EXPORTED_SYMBOLS
    assert re.search(r"#define SL2_API_VERSION 5\b", text)          # additions within version 5


# bytes per slot of the per-slot arrays, in blob order (include/scenelib2_amd.h)
SLOT_BYTES = [288, 8, 64, 4, 4, 4, 4, 4, 4, 16, 112, 48, 8, 32, 8, 16, 16, 4, 4, 8, 4, 4]


def up64(v):
    return (v + 63) // 64 * 64


def layout(n_slots, n_partial, n_particles):
    """The documented layout, restated: every section on a 64-byte boundary."""
    n = 13 + 3 * n_slots + 6 * n_partial
    pitch = (n + 7) // 8 * 8
    offs = [256]                                  # x
    offs.append(offs[-1] + up64(pitch * 8))       # P
    off = offs[-1] + n * pitch * 8
    assert off % 64 == 0
    offs.append(off)                              # the per-slot arrays
    for b in SLOT_BYTES:
        offs.append(off)
        off += up64(n_slots * b)
    offs.append(off)                              # per-sequence values
    off += 448
    offs.append(off)                              # particles
    off += up64(n_partial * n_particles * 12 * 8)
    offs.append(off)                              # trajectory_store_
    off += up64(1000 * 24)
    offs.append(off)                              # position log
    off += up64(1000 * 24)
    return off, offs, pitch, n


@pytest.mark.parametrize("shape", [(0, 0, 0), (12, 0, 0), (12, 1, 100), (7, 2, 37), (100, 1, 128), (500, 1, 100), (676, 4, 1024),
                                   (1, 4, 1), (33, 3, 64)])
def test_blob_layout_arithmetic(shape):
    from scenelib2_amd import _lib
    L = _lib.load()
    assert len(SLOT_BYTES) == _lib.SL2_BLOB_SLOT_ARRAYS
    got = (C.c_uint64 * _lib.SL2_BLOB_LAYOUT_OFFSETS)()
    total = L.sl2_sequence_blob_layout(shape[0], shape[1], shape[2], got, len(got))
    want_total, want, pitch, n = layout(*shape)
    assert total == want_total and list(got) == want
    assert total % 64 == 0 and all(o % 64 == 0 for o in want)
    assert pitch % 8 == 0 and pitch >= n
    # the capacity argument is respected, and nonsense is refused
    few = (C.c_uint64 * 3)(7, 7, 7)
    assert L.sl2_sequence_blob_layout(shape[0], shape[1], shape[2], few, 2) == want_total and list(few) == want[:2] + [7]
    assert L.sl2_sequence_blob_layout(-1, 0, 0, got, len(got)) == 0 and L.sl2_sequence_blob_layout(677, 0, 0, got, len(got)) == 0
    assert L.sl2_sequence_blob_layout(1, 5, 0, got, len(got)) == 0 and L.sl2_sequence_blob_layout(1, 1, 1025, got, len(got)) == 0


def test_header_structs_are_256_bytes():
    from scenelib2_amd import _lib
    assert C.sizeof(_lib.sl2_sequence_blob_header) == 256 and C.sizeof(_lib.sl2_snapshot_header) == 256
    assert _lib.sl2_sequence_blob_header.camera.offset == 96 and _lib.sl2_sequence_blob_header.params.offset == 152
    assert _lib.sl2_snapshot_header.sequence_steps.offset == _lib.sl2_snapshot_header.steps_done.offset + 4


def test_adapters_have_save_and_load_state():
    from scenelib2_amd import Engine, MonoSLAM
    for name in ("save_sequences", "load_sequences", "copy_sequences", "reset_sequences", "sequence_blob_capacity"):
        assert callable(getattr(Engine, name))
    assert callable(MonoSLAM.SaveState) and callable(MonoSLAM.LoadState)
    hpp = open(os.path.join(ROOT, "include", "scenelib2_amd_monoslam.hpp")).read()
    assert "SaveState" in hpp and "LoadState" in hpp


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_checkpoint_kernels_neither_spill_nor_use_scratch(tmp_path):
    out = os.path.join(str(tmp_path), "sl2_checkpoint.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-Wno-unused-value",
           "-Wno-unused-result", "--cuda-device-only", "-S", os.path.join(CSRC, "sl2_checkpoint.hip"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    text = open(out).read()
    for frag in ("k_seq_pack", "k_seq_unpack"):
        m = re.search(r"\.name:\s+(\S*%s\S*)\n" % re.escape(frag), text)
        assert m, "kernel %s not found" % frag
        start = text.rfind("- .agpr_count", 0, m.start())
        end = text.find("- .agpr_count", m.end())
        block = text[start:end if end > 0 else len(text)]
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
        vg = int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1))
        assert spills == 0 and scratch == 0, "%s spills (%d vector registers, %d bytes of scratch)" % (frag, spills, scratch)
        assert vg <= 128, "%s uses %d registers: a copy kernel wants at least four wavefronts per SIMD" % (frag, vg)
