"""The table of per-sequence device arrays (scenelib2_amd/csrc/sl2_seq_arrays.hpp), compiled for the host: the engine's members,
their allocation, a sequence group's view of them and their release are all expansions of this one list, so what is checked
here - the extents, the view offsets, the split of a batch into groups - holds for all four."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

HDR = os.path.join(ROOT, "scenelib2_amd", "csrc", "sl2_seq_arrays.hpp")
SRC = os.path.join(ROOT, "tests", "seq_arrays_host.cpp")

# (N, ld, mld, nblk_max, kpart, pcap): max_features 16, one partial slot, 10 selected; max_features 100, four partial slots
DIMS = [(16, 128, 32, 1, 1, 128), (100, 384, 256, 8, 4, 128)]
# the per-sequence arrays struct sl2_engine held by hand before the table (counted in its allocation, view and release lists):
# 57 rows, then the step record, the time record and the camera calibration
N_ARRAYS = 60


@pytest.fixture(scope="module")
def sa():
    bdir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(bdir, exist_ok=True)
    so = os.path.join(bdir, "libseq_arrays_host.so")
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-Wall", "-shared", "-o", so, SRC])
    L = C.CDLL(so)
    L.sa_name.restype = C.c_char_p
    L.sa_elem_size.restype = C.c_size_t
    L.sa_elems.restype = C.c_size_t
    L.sa_elems.argtypes = [C.c_int] + [C.c_size_t] * 6
    L.sa_view_offset.restype = C.c_size_t
    L.sa_view_offset.argtypes = [C.c_int] + [C.c_size_t] * 7
    L.sa_group_range.argtypes = [C.c_int] * 3 + [C.POINTER(C.c_int)] * 2
    return L


def group_range(L, B, G, k):
    first, count = C.c_int(-1), C.c_int(-1)
    L.sa_group_range(B, G, k, C.byref(first), C.byref(count))
    return first.value, count.value


def test_header_needs_no_hip():
    text = open(HDR).read()
    assert "hip_runtime" not in text and "#include \"" not in text


def test_rows_are_the_members_and_their_count(sa):
    names = [sa.sa_name(i).decode() for i in range(sa.sa_count())]
    assert len(names) == N_ARRAYS
    assert len(set(names)) == len(names)
    assert sa.sa_struct_pointers() == N_ARRAYS                  # SeqArrays holds one pointer per row and nothing else
    assert sa.sa_name(N_ARRAYS) is None and sa.sa_name(-1) is None
    assert names[:2] == ["x", "P"]                              # the allocation order starts and ends as sl2_create's did
    assert names[-4:] == ["me_desc", "step_mark", "seq_time", "seq_cam"]
    order = [names.index(n) for n in ("P", "At", "Vt", "St")]   # the large matrices, in the order their placement compares
    assert order == sorted(order)


@pytest.mark.parametrize("B,G", [(5, 3), (4, 4), (3, 1), (1024, 3)])
def test_group_range_splits_the_batch(sa, B, G):
    ranges = [group_range(sa, B, G, k) for k in range(G)]
    assert ranges[0][0] == 0
    for (f0, c0), (f1, _) in zip(ranges, ranges[1:]):
        assert f0 + c0 == f1
    counts = [c for _, c in ranges]
    assert sum(counts) == B and ranges[-1][0] + ranges[-1][1] == B
    assert max(counts) - min(counts) <= 1 and min(counts) >= 1
    assert counts == sorted(counts, reverse=True)               # the first B % G groups are the longer ones
    if (B, G) == (5, 3):
        assert ranges == [(0, 2), (2, 2), (4, 1)]


@pytest.mark.parametrize("dims", DIMS)
def test_views_abut_and_cover_the_allocation(sa, dims):
    B, G = 5, 3
    ranges = [group_range(sa, B, G, k) for k in range(G)]
    for i in range(sa.sa_count()):
        size, elems = sa.sa_elem_size(i), sa.sa_elems(i, *dims)
        assert size in (1, 4, 8) and elems >= 1
        offs = [sa.sa_view_offset(i, *dims, first) for first, _ in ranges]
        for k, (first, count) in enumerate(ranges):
            assert offs[k] == first * elems * size
            end = offs[k] + count * elems * size
            assert end == (offs[k + 1] if k + 1 < G else B * elems * size), sa.sa_name(i)


@pytest.mark.parametrize("dims", DIMS)
def test_extents_restated(sa, dims):
    N, ld, mld, nblk_max, kpart, pcap = dims
    want = {"x": ld, "P": ld * ld, "At": mld * ld, "Vt": mld * ld, "St": mld * mld, "LinvT": nblk_max * 1024, "patch": N * 288,
            "srch_sel": N * 16, "f_Hx": N * 14, "particles": kpart * pcap * 12, "me_desc": kpart * pcap * 8, "ps_i": kpart * 8,
            "traj": 3000, "pos_log": 3000, "active": 1, "step_mark": 1, "seq_time": 4, "seq_cam": 8}
    rows = {sa.sa_name(i).decode(): i for i in range(sa.sa_count())}
    for name, elems in want.items():
        assert sa.sa_elems(rows[name], *dims) == elems, name
    assert sa.sa_elem_size(rows["active"]) == 1 and sa.sa_elem_size(rows["patch"]) == 1
    assert sa.sa_elem_size(rows["srch_sel"]) == 4 and sa.sa_elem_size(rows["P"]) == 8 and sa.sa_elem_size(rows["rand48"]) == 8
    # every other row is [N][w] or [w] with a small w
    for name, i in rows.items():
        if name not in want:
            e = sa.sa_elems(i, *dims)
            assert e in (1, 3, 4, 5, 16) or (e % N == 0 and e // N in (1, 2, 4, 6, 8)), name
