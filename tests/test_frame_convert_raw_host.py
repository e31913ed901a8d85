"""Machine-vision frames, host side: both host forms for the deep grey and the Bayer formats against a NumPy restatement of the
definition (frame_convert_raw_cases.py, written from the header's text; it calls nothing of the library), the exact anchors, the
phase check that needs no restatement, the refusals, the Python surface and the stand-alone bounds program under AddressSanitizer.
(The kernels: tests/test_gpu_frame_convert_raw.py; their descriptors: tests/test_frame_convert_kernels.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import frame_convert_cases as fc
import frame_convert_raw_cases as rc
from frame_convert_raw_cases import AREA, LINEAR

from scenelib2_amd import _lib, convert

FILTER_NAME = {LINEAR: "linear", AREA: "area"}


def test_case_table_covers_every_format_filter_offset_and_pad():
    assert {(c[2], c[3]) for c in rc.CASES} == {(f, flt) for f in rc.FORMATS for flt in (LINEAR, AREA)}
    for f in rc.FORMATS:
        for flt in (LINEAR, AREA):
            mine = [c for c in rc.CASES if c[2] == f and c[3] == flt]
            assert {(c[4], c[5]) for c in mine} == {(p, o) for p in rc.PITCH_PADS[f] for o in rc.OFFSETS[f]}, (f, flt)
    widths = {c[1][0] for c in rc.CASES}
    heights = {c[1][1] for c in rc.CASES}
    assert {2, 3, 15, 16, 17, 31, 33, 47, 1001, 4096} <= widths and {2, 3, 9, 17} <= heights
    assert (4096, 6) in {c[1] for c in rc.CASES}
    outs = {c[0] for c in rc.CASES}
    assert {(1, 1), (7, 5), (33, 17)} <= outs and {8, 9} <= {o[1] for o in outs}
    ratios = {(c[1][0] / c[0][0], c[1][1] / c[0][1]) for c in rc.CASES}
    assert {(1.0, 1.0), (2.0, 2.0), (3.0, 3.0)} <= ratios                                     # identity, 2 x, 3 x
    assert any(1 < rx < 2 and ry != int(ry) for rx, ry in ratios)                             # a non-integer reduction
    assert any(c[3] == LINEAR and c[1][0] < c[0][0] and c[1][1] < c[0][1] for c in rc.CASES)  # an enlargement
    assert all(c[1][0] >= c[0][0] and c[1][1] >= c[0][1] for c in rc.CASES if c[3] == AREA)


def test_host_forms_equal_the_definition():
    for (ow, oh), (sw, sh), fmt, flt, pad, off, seed in rc.CASES:
        s = rc.source(sw, sh, fmt, pad, off)
        raw = rc.random_raw(s, seed)
        got = convert.convert_frame_host(s, raw, ow, oh, filter=FILTER_NAME[flt])
        want = rc.reference(s, raw, ow, oh, flt)
        assert got.shape == (oh, ow) and np.array_equal(got, want), (ow, oh, s, flt, int(np.abs(got.astype(int) - want).max()))


def test_linear_filter_through_the_filtered_entry_point_gives_the_same_bytes():
    L = _lib.load()
    s = rc.source(47, 17, rc.BAYER_GBRG8, 13, 7)
    raw = rc.random_raw(s, 5)
    out = np.zeros((17, 33), np.uint8)
    src = convert.make_source(s)
    _lib.check(L.sl2_convert_frame_host_filtered(C.byref(src), LINEAR, raw.ctypes.data_as(_lib.vp), raw.size, 33, 17, _lib.u8p(out)), L)
    assert np.array_equal(out, convert.convert_frame_host(s, raw, 33, 17))


@pytest.mark.parametrize("flt", (LINEAR, AREA))
@pytest.mark.parametrize("fmt", rc.FORMATS)
def test_identity_size_reproduces_the_grey_plane(fmt, flt):
    pads, offs = rc.PITCH_PADS[fmt], rc.OFFSETS[fmt]
    for (w, h), pad, off in (((320, 240), pads[2], offs[2]), ((2, 2), pads[1], offs[1]), ((33, 17), pads[0], offs[0])):
        s = rc.source(w, h, fmt, pad, off)
        raw = rc.random_raw(s, 7 + fmt)
        assert np.array_equal(convert.convert_frame_host(s, raw, w, h, filter=FILTER_NAME[flt]), rc.grey_plane(s, raw).astype(np.uint8))


@pytest.mark.parametrize("flt", (LINEAR, AREA))
@pytest.mark.parametrize("fmt", rc.FORMATS)
def test_a_constant_image_stays_constant(fmt, flt):
    for value in (0, 1, 127, 254, 255):
        for (sw, sh), (ow, oh) in (((64, 48), (32, 24)), ((31, 17), (33, 17)), ((16, 12), (32, 24)), ((961, 3), (7, 3))):
            if flt == AREA and (sw < ow or sh < oh):
                continue
            if fmt in rc.BAYER:
                s, raw = rc.pack_mosaic(np.full((sh, sw), value, np.uint8), fmt, pad=1, offset=1, seed=value)
                want = value
            else:       # the value in the top byte of the N significant bits, random bits below it and above N
                n = rc.DEEP[fmt]
                rng = np.random.default_rng(value)
                low = rng.integers(0, 1 << (n - 8), (sh, sw)) if n > 8 else 0
                high = rng.integers(0, 1 << (16 - n), (sh, sw)) << n if n < 16 else 0
                s, raw = rc.pack_words(((value << (n - 8)) | low | high).astype(np.uint16), fmt, pad=2, offset=2, seed=value)
                want = value
            out = convert.convert_frame_host(s, raw, ow, oh, filter=FILTER_NAME[flt])
            assert (out == want).all(), (fmt, value, sw, sh, ow, oh)


@pytest.mark.parametrize("fmt", sorted(rc.BAYER))
def test_a_flat_colour_mosaic_gives_the_rgb_grey_everywhere(fmt):
    for rgb in ((255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255), (201, 37, 118), (1, 2, 3)):
        want = (4899 * rgb[0] + 9617 * rgb[1] + 1868 * rgb[2] + 8192) >> 14
        rgb24 = convert.convert_frame_host(fc.source(1, 1, fc.RGB24), np.array(rgb, np.uint8), 1, 1)
        assert rgb24[0, 0] == want
        for w, h in ((2, 2), (3, 2), (2, 3), (17, 9), (16, 8)):
            s, raw = rc.pack_mosaic(rc.flat_colour_mosaic(fmt, w, h, rgb), fmt, pad=13, offset=15)
            assert (convert.convert_frame_host(s, raw, w, h) == want).all(), (fmt, rgb, w, h)
            assert (convert.convert_frame_host(s, raw, w, h, filter="area") == want).all(), (fmt, rgb, w, h)


def test_a_region_of_interest_is_the_matching_sibling_pattern():
    """The phase check, independent of the restatement: the source that starts one column into an RGGB mosaic, declared GRBG,
    sees the same colours at the same sensor sites, so its grey plane is the RGGB one in every column but its own first (whose
    left neighbour is now a reflection); likewise one row down (GBRG), and both (BGGR)."""
    w, h, pitch = 37, 23, 41
    full = rc.source(w, h, rc.BAYER_RGGB8, pitch - w, 5)
    raw = rc.random_raw(full, 11)
    whole = convert.convert_frame_host(full, raw, w, h)
    for fmt, dx, dy in ((rc.BAYER_GRBG8, 1, 0), (rc.BAYER_GBRG8, 0, 1), (rc.BAYER_BGGR8, 1, 1)):
        roi = dict(width=w - dx, height=h - dy, pitch=pitch, format=fmt, offset=5 + dy * pitch + dx)
        part = convert.convert_frame_host(roi, raw, w - dx, h - dy)
        assert np.array_equal(part[dy:, dx:], whole[2 * dy:, 2 * dx:]), fmt
        assert np.array_equal(convert.convert_frame_host(roi, raw, w - dx, h - dy, filter="area"), part)
    # and a wrong sibling does not: the check can fail
    wrong = dict(width=w - 1, height=h, pitch=pitch, format=rc.BAYER_RGGB8, offset=6)
    assert not np.array_equal(convert.convert_frame_host(wrong, raw, w - 1, h)[:, 1:], whole[:, 2:])


@pytest.mark.parametrize("fmt", (rc.GRAY10, rc.GRAY12))
def test_bits_above_n_do_not_change_the_output(fmt):
    n = rc.DEEP[fmt]
    rng = np.random.default_rng(fmt)
    words = rng.integers(0, 1 << n, (17, 33)).astype(np.uint16)
    s, clean = rc.pack_words(words, fmt, pad=2, offset=14, seed=1)
    _, dirty = rc.pack_words(words | (rng.integers(1, 1 << (16 - n), (17, 33)) << n).astype(np.uint16), fmt, pad=2, offset=14, seed=1)
    assert not np.array_equal(clean, dirty)
    for (ow, oh), flt in (((33, 17), "linear"), ((16, 8), "linear"), ((16, 8), "area")):
        assert np.array_equal(convert.convert_frame_host(s, clean, ow, oh, filter=flt), convert.convert_frame_host(s, dirty, ow, oh, filter=flt))
    assert np.array_equal(convert.convert_frame_host(s, clean, 33, 17), (words >> (n - 8)).astype(np.uint8))


def test_gray16_is_the_high_byte_like_uyvy_over_the_same_bytes():
    for w, h, pad, off in ((64, 3, 0, 0), (16, 9, 2, 14), (2, 2, 14, 2)):
        s16 = rc.source(w, h, rc.GRAY16, pad, off)
        raw = rc.random_raw(s16, w)
        s422 = dict(s16, format=fc.UYVY)
        for (ow, oh), flt in (((w, h), "linear"), ((7, 5), "linear"), ((w // 2, h // 2), "area")):
            assert np.array_equal(convert.convert_frame_host(s16, raw, ow, oh, filter=flt), convert.convert_frame_host(s422, raw, ow, oh, filter=flt))


def _rc(s, raw_bytes, ow=2, oh=2, nbuf=None, flt=LINEAR):
    L = _lib.load()
    buf = np.zeros(nbuf if nbuf is not None else max(int(raw_bytes), 1), np.uint8)
    out = np.zeros(ow * oh, np.uint8)
    src = _lib.sl2_frame_source(s["width"], s["height"], s["pitch"], s["format"], s["offset"])
    return L.sl2_convert_frame_host_filtered(C.byref(src), flt, buf.ctypes.data_as(_lib.vp), int(raw_bytes), ow, oh, _lib.u8p(out))


def test_refusals():
    L = _lib.load()
    for fmt in rc.FORMATS:          # one byte short of its reach, per format; the exact size passes
        good = rc.source(16, 9, fmt, rc.PITCH_PADS[fmt][2], rc.OFFSETS[fmt][1])
        need = rc.source_bytes(good)
        assert need == convert.source_bytes(good)
        for flt in (LINEAR, AREA):
            assert _rc(good, need, flt=flt) == _lib.SL2_OK
            assert _rc(good, need - 1, nbuf=need, flt=flt) == _lib.SL2_ERR_INVALID
            assert "sequence 0" in L.sl2_last_error().decode() and "past the raw buffer" in L.sl2_last_error().decode()
        assert _rc(good, need, ow=17, oh=9, flt=AREA) == _lib.SL2_ERR_INVALID          # AREA only reduces
        assert "only reduces" in L.sl2_last_error().decode()
        assert _rc(good, need, ow=17, oh=9, flt=LINEAR) == _lib.SL2_OK
    for fmt in rc.BAYER:
        assert _rc(rc.source(1, 8, fmt), 1 << 10, nbuf=64) == _lib.SL2_ERR_INVALID
        assert "Bayer source under 2 pixels" in L.sl2_last_error().decode() and "sequence 0" in L.sl2_last_error().decode()
        assert _rc(rc.source(8, 1, fmt), 1 << 10, nbuf=64) == _lib.SL2_ERR_INVALID
        assert _rc(rc.source(2, 2, fmt), 4) == _lib.SL2_OK
        assert _rc(rc.source(3, 3, fmt, 1, 1), 1 + 2 * 4 + 3) == _lib.SL2_OK           # odd sizes, offset and pitch are fine
    for fmt in rc.DEEP:
        assert _rc(rc.source(8, 4, fmt, pad=1), 1 << 10, nbuf=256) == _lib.SL2_ERR_INVALID
        assert "odd offset or pitch" in L.sl2_last_error().decode()
        assert _rc(rc.source(8, 4, fmt, offset=1), 1 << 10, nbuf=256) == _lib.SL2_ERR_INVALID
        assert _rc(rc.source(1, 1, fmt), 2, ow=1, oh=1) == _lib.SL2_OK
    for fmt in list(range(5, 16)) + list(range(19, 24)) + [28, 255, 256 + 16, 512 + 24]:
        assert _rc(dict(rc.source(8, 4, rc.GRAY16), format=fmt), 1 << 10, nbuf=256) == _lib.SL2_ERR_INVALID, fmt
        assert "unknown pixel format" in L.sl2_last_error().decode()
    assert _rc(rc.source(4096, 2, rc.BAYER_BGGR8), 2 * 4096) == _lib.SL2_OK                   # the caps themselves pass
    assert _rc(rc.source(4097, 2, rc.BAYER_BGGR8), 2 * 4097) == _lib.SL2_ERR_INVALID


def test_python_surface():
    names = {"gray10": 16, "gray12": 17, "gray16": 18, "bayer_rggb8": 24, "bayer_grbg8": 25, "bayer_gbrg8": 26, "bayer_bggr8": 27}
    for name, fmt in names.items():
        assert convert.FORMATS[name] == fmt
        assert getattr(_lib, "SL2_PIX_" + name.upper()) == fmt and getattr(convert, "SL2_PIX_" + name.upper()) == fmt
        assert convert.BYTES_PER_PIXEL[fmt] == rc.BPP[fmt]
        s = convert.make_source(dict(width=10, height=4, format=name))
        assert (s.format, s.pitch) == (fmt, 10 * rc.BPP[fmt])
        assert convert.source_bytes(dict(width=10, height=4, format=name, pitch=32, offset=6)) == 6 + 3 * 32 + 10 * rc.BPP[fmt]
    assert len(convert.FORMATS) == 12 and C.sizeof(_lib.sl2_frame_source) == 24
    raw = np.arange(64, dtype=np.uint8)
    assert np.array_equal(convert.convert_frame_host(dict(width=8, height=4, format="GRAY16"), raw, 8, 4), raw.reshape(4, 16)[:, 1::2])
    header = open(os.path.join(ROOT, "include", "scenelib2_amd.h")).read()
    for name, fmt in names.items():
        assert re.search(r"SL2_PIX_%s = %d\b" % (name.upper(), fmt), header)


def test_host_bodies_stay_inside_exactly_sized_blocks_under_asan(tmp_path):
    """tests/frame_convert_raw_host.cpp: a program of its own (nothing loaded into Python), built with the address and
    undefined-behaviour sanitizers, over the edge shapes with exactly sized heap blocks."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = os.path.join(str(tmp_path), "frame_convert_raw_host")
    src = os.path.join(ROOT, "tests", "frame_convert_raw_host.cpp")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.startswith("ok ")

