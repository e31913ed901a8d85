"""SL2_RESIZE_AREA, host side: sl2_convert_frame_host_filtered against a NumPy restatement of the definition
(frame_convert_area_cases.py, written from the header's text; it calls nothing of the library) byte for byte, the np.kron
cross-check of that restatement, the accumulator's width, the aliasing anchor, an NV12 frame, the refusals, the Python surface
and the stand-alone host program under AddressSanitizer.  (The kernel: tests/test_gpu_frame_convert_area.py.)"""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import frame_convert_cases as fc
import frame_convert_area_cases as fa

from scenelib2_amd import _lib, convert

CASES = list(fa.cases())


def test_case_list_covers_every_shape_format_pitch_and_offset():
    assert {(c[0], c[1]) for c in CASES} == set(fa.SHAPES) and len(fa.SHAPES) == 14
    even = sum(1 for (sw, _), _ in fa.SHAPES if sw % 2 == 0)
    assert even == 8 and len(CASES) == 5 * even + 3 * (14 - even) + 2          # every format the width allows; a ninth case for UYVY and YUYV
    assert {(c[2], c[3], c[4]) for c in CASES} == {(f, p, o) for f in fc.FORMATS for p in fc.PITCH_PADS for o in fc.OFFSETS}


def test_host_form_equals_the_definition_byte_for_byte():
    for (sw, sh), (ow, oh), fmt, pad, off, seed in CASES:
        s = fa.source(sw, sh, fmt, pad, off)
        raw = fa.random_raw(s, seed)
        got = convert.convert_frame_host(s, raw, ow, oh, filter="area")
        want = fa.reference(s, raw, ow, oh)
        assert got.shape == (oh, ow) and np.array_equal(got, want), (ow, oh, s, int(np.abs(got.astype(int) - want).max()))
        if (sw, sh) == (ow, oh):
            assert np.array_equal(got, fa.grey_plane(s, raw).astype(np.uint8)), s          # the identity


def test_the_definition_equals_block_sums_of_the_kron_refinement():
    ran = 0
    for (sw, sh), (ow, oh) in fa.SHAPES:
        if sw * sh * ow * oh >= 5e7:
            continue
        g = np.random.default_rng(sw * 31 + sh).integers(0, 256, (sh, sw), dtype=np.uint8)
        assert np.array_equal(fa.accumulate(g, ow, oh), fa.kron_accumulate(g, ow, oh)), (sw, sh, ow, oh)
        ran += 1
    assert ran == 7          # all but the HD sources and the two large near-identities


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_a_constant_image_maps_to_itself(fmt):
    for value in (1, 127, 255):
        for (sw, sh), (ow, oh) in (((640, 480), (320, 240)), ((31, 17), (7, 5)), ((322, 242), (320, 240)), ((962, 18), (33, 17))):
            if not fc.allowed(fmt, sw):
                continue
            s, raw = fa.pack_grey(np.full((sh, sw), value, np.uint8), fmt, pad=1, offset=1, seed=value)
            out = convert.convert_frame_host(s, raw, ow, oh, filter="area")
            assert (out == value).all(), (fmt, value, sw, sh, ow, oh)


def test_accumulator_beyond_32_bits():
    """4096 x 4200: 255 Sx Sy = 4.39e9 > 2^32."""
    sw, sh = 4096, 4200
    assert 255 * sw * sh > 1 << 32
    s = fa.source(sw, sh, fc.GRAY8)
    white = np.full(sw * sh, 255, np.uint8)
    for ow, oh in ((7, 5), (320, 240)):
        assert (convert.convert_frame_host(s, white, ow, oh, filter="area") == 255).all(), (ow, oh)
    del white
    raw = fa.random_raw(s, 77)
    for ow, oh in ((7, 5), (320, 240)):
        assert np.array_equal(convert.convert_frame_host(s, raw, ow, oh, filter="area"), fa.reference(s, raw, ow, oh)), (ow, oh)


def test_aliasing_anchor_area_averages_what_linear_skips():
    s = fa.source(1280, 960, fc.GRAY8)
    p4 = fa.stripes(1280, 960, (0, 255, 255, 0))
    assert (convert.convert_frame_host(s, p4, 320, 240, filter="area") == 128).all()          # the mean, 127.5, rounded up
    assert (convert.convert_frame_host(s, p4, 320, 240, filter="linear") == 255).all()        # both taps land on the bright pair
    assert (convert.convert_frame_host(s, p4, 320, 240) == 255).all()
    p5 = fa.stripes(1280, 960, (0, 0, 255, 255, 255))
    area = convert.convert_frame_host(s, p5, 320, 240, filter="area")
    lin = convert.convert_frame_host(s, p5, 320, 240, filter="linear")
    print("period 5: area %d .. %d, linear %d .. %d" % (area.min(), area.max(), lin.min(), lin.max()))
    assert area.min() >= 128 and area.max() <= 191
    assert (int(lin.min()), int(lin.max())) == (0, 255)


def test_nv12_luma_plane_is_a_gray8_source():
    w, h = 642, 482
    rng = np.random.default_rng(9)
    luma = rng.integers(0, 256, (h, w), dtype=np.uint8)
    chroma = rng.integers(0, 256, (h // 2, w), dtype=np.uint8)          # interleaved U V, half the rows
    nv12 = np.concatenate([luma.reshape(-1), chroma.reshape(-1)])
    s = fa.source(w, h, fc.GRAY8)
    for flt in ("area", "linear"):
        alone = convert.convert_frame_host(s, luma, 320, 240, filter=flt)
        assert np.array_equal(convert.convert_frame_host(s, nv12, 320, 240, filter=flt), alone)
        assert np.array_equal(convert.convert_frame_host(s, nv12, 320, 240, raw_bytes=w * h, filter=flt), alone)
    assert np.array_equal(convert.convert_frame_host(s, luma, 320, 240, filter="area"), fa.reference(s, luma.reshape(-1), 320, 240))


def test_linear_filter_is_the_unfiltered_host_form():
    for (sw, sh), (ow, oh), fmt in (((640, 480), (320, 240), fc.UYVY), ((31, 17), (33, 17), fc.RGB24), ((961, 3), (7, 5), fc.BGR24)):
        s = fa.source(sw, sh, fmt, 13, 7)
        raw = fa.random_raw(s, 5)
        plain = convert.convert_frame_host(s, raw, ow, oh)
        assert np.array_equal(convert.convert_frame_host(s, raw, ow, oh, filter="linear"), plain)
        assert np.array_equal(convert.convert_frame_host(s, raw, ow, oh, filter=_lib.SL2_RESIZE_LINEAR), plain)
        out = np.zeros((oh, ow), np.uint8)
        src = convert.make_source(s)
        L = _lib.load()
        assert L.sl2_convert_frame_host_filtered(C.byref(src), 0, raw.ctypes.data_as(_lib.vp), raw.size, ow, oh, _lib.u8p(out)) == _lib.SL2_OK
        assert np.array_equal(out, plain)


def _rc(s, flt, ow, oh, raw_bytes=None):
    L = _lib.load()
    need = fc.source_bytes(dict(s, format=s["format"] if s["format"] in fc.BPP else fc.GRAY8))
    buf = np.zeros(need, np.uint8)
    out = np.zeros(ow * oh, np.uint8)
    src = _lib.sl2_frame_source(s["width"], s["height"], s["pitch"], s["format"], s["offset"])
    return L.sl2_convert_frame_host_filtered(C.byref(src), flt, buf.ctypes.data_as(_lib.vp), need if raw_bytes is None else raw_bytes,
                                             ow, oh, _lib.u8p(out))


def test_refusals():
    L = _lib.load()
    good = fa.source(33, 17, fc.GRAY8)
    assert _rc(good, fa.AREA, 33, 17) == _lib.SL2_OK and _rc(good, fa.LINEAR, 33, 17) == _lib.SL2_OK
    for flt in (2, -1):
        assert _rc(good, flt, 33, 17) == _lib.SL2_ERR_INVALID
        assert "filter" in L.sl2_last_error().decode()
    for sw, sh in ((31, 17), (33, 16)):          # narrower, lower: area only reduces
        small = fa.source(sw, sh, fc.GRAY8)
        assert _rc(small, fa.AREA, 33, 17) == _lib.SL2_ERR_INVALID
        assert "smaller than the output" in L.sl2_last_error().decode()
        assert _rc(small, fa.LINEAR, 33, 17) == _lib.SL2_OK          # linear enlarges as before
        with pytest.raises(_lib.Sl2Error):
            convert.convert_frame_host(small, np.zeros(fc.source_bytes(small), np.uint8), 33, 17, filter="area")
    # the refusals of sl2_convert_frame_host hold under either filter
    for flt in (fa.LINEAR, fa.AREA):
        assert _rc(good, flt, 33, 17, raw_bytes=fc.source_bytes(good) - 1) == _lib.SL2_ERR_INVALID
        assert _rc(dict(good, format=5), flt, 33, 17) == _lib.SL2_ERR_INVALID
        assert _rc(dict(good, pitch=32), flt, 33, 17) == _lib.SL2_ERR_INVALID
        assert _rc(good, flt, 0, 17) == _lib.SL2_ERR_INVALID


def test_python_surface():
    import scenelib2_amd
    assert convert.FILTERS == {"linear": 0, "area": 1} and (_lib.SL2_RESIZE_LINEAR, _lib.SL2_RESIZE_AREA) == (0, 1)
    sig = inspect.signature(convert.convert_frame_host)
    assert list(sig.parameters) == ["src", "raw", "out_width", "out_height", "raw_bytes", "filter"] and sig.parameters["filter"].default == "linear"
    assert list(inspect.signature(scenelib2_amd.MonoSLAM.SetFrameFilter).parameters) == ["self", "filter"]
    assert list(inspect.signature(scenelib2_amd.MonoSLAM.SetFrameSource).parameters) == ["self", "width", "height", "pitch", "format"]
    assert list(inspect.signature(convert.FrameConverter.set_filters).parameters) == ["self", "filters", "seq0"]
    assert list(inspect.signature(convert.FrameConverter.get_filters).parameters) == ["self", "seq0", "nseq"]
    for name in ("sl2_converter_set_filters", "sl2_converter_get_filters", "sl2_convert_frame_host_filtered"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)
    assert C.sizeof(_lib.sl2_frame_source) == 24
    hpp = open(os.path.join(ROOT, "include", "scenelib2_amd_monoslam.hpp")).read()
    assert "void SetFrameFilter(int filter)" in hpp and "sl2_converter_set_filters" in hpp
    hdr = open(os.path.join(ROOT, "include", "scenelib2_amd.h")).read()
    assert "enum { SL2_RESIZE_LINEAR = 0, SL2_RESIZE_AREA = 1 };" in hdr


def test_area_host_body_stays_inside_exactly_sized_blocks_under_asan(tmp_path):
    """tests/frame_convert_area_host.cpp: a program of its own (nothing loaded into Python), built with the address and
    undefined-behaviour sanitizers, over the small shapes and the wide-accumulator case with exactly sized heap blocks."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = os.path.join(str(tmp_path), "frame_convert_area_host")
    src = os.path.join(ROOT, "tests", "frame_convert_area_host.cpp")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.startswith("ok ")
