"""sl2_snapshot_batch / sl2_snapshot_bound (include/scenelib2_amd.h), the parts that need no device: the bound is
sl2_snapshot_capacity's arithmetic section by section, the header keeps its 256 bytes with omitted_sections where reserved[0]
was, both libraries export the symbols and the Python mirror knows them.  (What the call packs is tests/test_gpu_snapshot_batch.py.)"""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from scenelib2_amd import _lib

FI = 8 * 4 + 8 * (3 + 2 + 2 + 2 + 1 + 4 + 14 + 6 + 7) + 2 * 4 + 8 * 3      # sizeof(sl2_feature_info), tests/test_capi_symbols.py
BITS = dict(FEATURES=1, COV=2, SELECTION=4, TRAJ=8, PARTIAL=16, PATCHES=32)
ALL = 63


def capacity_restated(N, kpart, pcap):
    """sl2_snapshot_capacity as the parent wrote it: header, xv_, Pxx_, N feature records, N full + kpart partial covariance
    records, the selection rounded up to 8 bytes, 1000 trajectory entries, kpart partial records with pcap particles of 12
    doubles, N templates of 128 bytes; rounded up to 16."""
    b = 256 + 13 * 8 + 169 * 8 + N * FI + (N * (13 * 3 + 9) + kpart * (13 * 6 + 36)) * 8 + ((N * 4 + 7) & ~7) + 1000 * 24 + \
        kpart * (32 + pcap * 12 * 8) + N * 128
    return (b + 15) & ~15


@pytest.mark.parametrize("shape", [(16, 1, 128), (100, 4, 128), (676, 4, 1024)])
def test_bound_with_all_sections_is_the_capacity(shape):
    L = _lib.load()
    assert C.sizeof(_lib.sl2_feature_info) == FI
    assert L.sl2_snapshot_bound(*shape, ALL) == capacity_restated(*shape)
    assert L.sl2_snapshot_bound(*shape, ALL) % 16 == 0


@pytest.mark.parametrize("shape", [(16, 1, 128), (100, 4, 128), (676, 4, 1024)])
def test_bound_is_monotone_in_the_sections(shape):
    L = _lib.load()
    pose = L.sl2_snapshot_bound(*shape, 0)
    assert pose == 256 + 13 * 8 + 169 * 8 == 107 * 16      # header, xv_, Pxx_: always present
    for s in range(ALL + 1):
        b = L.sl2_snapshot_bound(*shape, s)
        assert b % 16 == 0 and pose <= b <= L.sl2_snapshot_bound(*shape, ALL)
        for bit in BITS.values():
            if not s & bit:
                assert L.sl2_snapshot_bound(*shape, s | bit) > b, (s, bit)


def test_bound_refuses_bad_arguments():
    L = _lib.load()
    assert L.sl2_snapshot_bound(16, 1, 128, ALL) > 0
    for bad in ((-1, 1, 128, ALL), (16, -1, 128, ALL), (16, 1, -64, ALL), (16, 1, 128, 64), (16, 1, 128, ALL | 128), (16, 1, 128, -1)):
        assert L.sl2_snapshot_bound(*bad) == 0, bad


def test_header_keeps_its_size_and_omitted_sections_sits_where_reserved_began():
    H = _lib.sl2_snapshot_header
    assert C.sizeof(H) == 256
    assert H.sequence_steps.offset == 132 and H.omitted_sections.offset == 136 and H.omitted_sections.size == 4
    assert H.reserved.offset == 140 and H.reserved.size == 4 * 29
    text = open(os.path.join(ROOT, "include", "scenelib2_amd.h")).read()
    body = text[text.index("typedef struct sl2_snapshot_header {"):text.index("} sl2_snapshot_header;")]
    names = re.findall(r"\b([a-z_A-Z]+)(?:\[\d+\])?[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names[-3:] == ["sequence_steps", "omitted_sections", "reserved"] and "int32_t reserved[29];" in body
    for k, v in BITS.items():
        assert re.search(r"\bSL2_SNAP_%s = %d\b" % (k, v), text), k
        assert getattr(_lib, "SL2_SNAP_" + k) == v
    assert re.search(r"\bSL2_SNAP_ALL = 63\b", text) and _lib.SL2_SNAP_ALL == 63


def test_symbols_are_exported_bound_and_refuse_a_null_engine():
    for name in ("sl2_snapshot_bound", "sl2_snapshot_batch"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name) and hasattr(_lib.load_testing(), name)
    L = _lib.load()
    out = (C.c_uint8 * 64)()
    offs = (C.c_uint64 * 2)()
    for on_device in (0, 1):
        assert L.sl2_snapshot_batch(None, 0, 1, ALL, None, C.cast(out, _lib.vp), 64, C.cast(offs, _lib.vp), on_device) == _lib.SL2_ERR_INVALID
    assert bytes(out) == bytes(64) and list(offs) == [0, 0]


def test_python_mirror_and_documents_know_the_call():
    from scenelib2_amd import Engine, decode_snapshot
    for name in ("snapshot_batch", "snapshot_batch_raw", "snapshot_batch_device", "snapshot_bound"):
        assert callable(getattr(Engine, name))
    assert callable(decode_snapshot)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^#+ *8g\b", design, flags=re.M)
    sec = design[re.search(r"^#+ *8g\b", design, flags=re.M).start():]
    for word in ("k_snapshot_sizes", "k_snapshot_scan", "k_snapshot_batch", "snapshot_batch_bench.json"):
        assert word in sec, word
    assert "sl2_snapshot_batch" in open(os.path.join(ROOT, "README.md")).read()
    assert "sl2_snapshot_batch" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    mk = open(os.path.join(ROOT, "examples", "Makefile")).read()
    assert re.search(r"^all:.*\bpublish_monoslam\b", mk, flags=re.M) and "publish_monoslam.cpp" in mk
