"""The lens remap, host side: sl2_remap_frame_host against a NumPy restatement of the pixel rule (frame_remap_cases.py, written from
the header's text; it calls nothing of the library) over the case table, the properties that need no restatement,
sl2_lens_map_host against a restatement of "maps from calibrations", its anchors, sl2_lens_pinhole_camera, the refusals, the
Python surface and the stand-alone bounds program under AddressSanitizer.
(The kernel: tests/test_gpu_frame_remap.py; its descriptor: tests/test_frame_convert_kernels.py.)"""
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
import frame_remap_cases as rm

from scenelib2_amd import _lib, convert


def test_case_table_covers_every_format_size_pitch_offset_and_kind_of_map():
    assert len(rm.FORMATS) == 12 and {c[2] for c in rm.CASES} == set(rm.FORMATS)
    assert {c[0] for c in rm.CASES} == {(1, 1), (7, 5), (33, 17), (64, 8), (65, 9)}
    assert {(2, 2), (3, 3), (47, 17), (4096, 6)} <= {c[1] for c in rm.CASES}
    for fmt in rm.FORMATS:
        mine = [c for c in rm.CASES if c[2] == fmt]
        pads, offs = rm.pads_offsets(fmt)
        assert {(c[4], c[5]) for c in mine} == {(p, o) for p in pads for o in offs}, fmt
        assert {c[0] for c in mine} == set(rm.OUT_SIZES) and {c[3] for c in mine} == set(rm.KINDS), fmt
        want = {(2, 2), (4096, 6)} | ({(4, 3), (48, 17)} if fmt in (fc.UYVY, fc.YUYV) else {(3, 3), (47, 17)})
        assert want <= {c[1] for c in mine}, fmt
    assert rm.pads_offsets(fc.RGB24) == (fc.PITCH_PADS, fc.OFFSETS) and rm.pads_offsets(rc.GRAY12) == (rc.PITCH_PADS[rc.GRAY12], rc.OFFSETS[rc.GRAY12])
    # the maps themselves hold what their names say
    seen = set()
    for case in rm.CASES:
        (ow, oh), (W, H), fmt, kind, _, _, _ = case
        if (kind, ow, W) in seen:
            continue
        seen.add((kind, ow, W))
        xy = rm.case_inputs(case)[2].astype(np.int64)
        X, Y = xy[..., 0], xy[..., 1]
        fx, ix = X & 31, (X - (X & 31)) // 32
        if kind == "identity":
            assert (X == 32 * np.arange(ow)[None, :]).all() and (Y == 32 * np.arange(oh)[:, None]).all()
        elif kind == "shift":
            assert (fx == 0).all() and ((Y & 31) == 0).all() and len(set((ix - np.arange(ow)[None, :]).reshape(-1))) == 1
        elif kind == "left_edge":
            assert (ix == -1).all() and (fx != 0).all() and ((Y[0] < 0) & (Y[0] > -32)).all()
        elif kind == "last_column":
            assert (ix == W - 1).all() and (fx == 0).all() and (Y[:, 0] == 32 * (H - 1)).all()
        elif kind == "border":
            assert (X == rm.BORDER).all()
    rnd = np.concatenate([rm.case_inputs(c)[2].reshape(-1, 2).astype(np.int64) for c in rm.CASES if c[3] == "random" and c[0] == (33, 17) and c[1] == (47, 17)])
    assert (rnd[:, 0] < -32).any() and (rnd[:, 1] < -32).any() and (rnd[:, 0] >= 32 * 47).any() and (rnd[:, 1] >= 32 * 17).any()
    assert (rnd[:, 1] == rm.BORDER).any() and not (rnd[:, 0] == rm.BORDER).any()          # INT32_MIN in Y alone is a position, not the border
    # one source size needs the two-word device form, every other the one-word form (sl2_convert_dev.hpp, remap_packed_xbits)
    bits = lambda S: (32 * (S + 1) - 1).bit_length()
    assert bits(rm.WIDE_SIZE[0]) + bits(rm.WIDE_SIZE[1]) > 32 and all(bits(w) + bits(h) < 32 for w, h in rm.SRC_SIZES)
    assert {c[2] for c in rm.CASES if c[1] == rm.WIDE_SIZE} == set(rm.WIDE_FORMATS)


def test_host_form_equals_the_definition():
    for case in rm.CASES:
        s, raw, xy = rm.case_inputs(case)
        got = convert.remap_frame_host(s, xy, raw)
        want = rm.reference(s, raw, xy)
        assert got.shape == want.shape and np.array_equal(got, want), (case, int(np.abs(got.astype(int) - want).max()))


@pytest.mark.parametrize("fmt", rm.FORMATS)
def test_identity_map_reproduces_the_grey_plane(fmt):
    pads, offs = rm.pads_offsets(fmt)
    for (w, h), pad, off in (((320, 240), pads[2], offs[2]), ((2, 2), pads[1], offs[1]), ((34, 17), pads[0], offs[0])):
        s = rm.source(w, h, fmt, pad, off)
        raw = rm.random_raw(s, 11 + fmt)
        got = convert.remap_frame_host(s, rm.make_map("identity", w, h, w, h, 0), raw)
        assert np.array_equal(got, rm.grey_plane(s, raw).astype(np.uint8))
        assert np.array_equal(got, convert.convert_frame_host(s, raw, w, h))          # ... which the identity resize gives too


@pytest.mark.parametrize("fmt", (fc.GRAY8, fc.RGB24, fc.YUYV, rc.GRAY12, rc.BAYER_RGGB8, rc.BAYER_BGGR8))
def test_a_constant_source_stays_constant_wherever_all_four_taps_lie_inside(fmt):
    W, H, ow, oh = 40, 30, 33, 17
    rng = np.random.default_rng(fmt)
    xy = np.stack([rng.integers(-40, 32 * W + 40, (oh, ow)), rng.integers(-40, 32 * H + 40, (oh, ow))], axis=-1).astype(np.int32)
    inside = (xy[..., 0] >= 0) & (xy[..., 0] <= 32 * (W - 1)) & (xy[..., 1] >= 0) & (xy[..., 1] <= 32 * (H - 1))
    assert inside.sum() > 100 and (~inside).sum() > 10
    for value in (0, 1, 127, 254, 255):
        if fmt in rc.BAYER:
            s, raw = rc.pack_mosaic(np.full((H, W), value, np.uint8), fmt, pad=1, offset=1, seed=value)
        elif fmt in rc.DEEP:
            s, raw = rc.pack_words(np.full((H, W), value << (rc.DEEP[fmt] - 8), np.uint16), fmt, pad=2, offset=2, seed=value)
        else:
            s, raw = fc.pack_grey(np.full((H, W), value, np.uint8), fmt, pad=1, offset=1, seed=value)
        out = convert.remap_frame_host(s, xy, raw)
        assert (out[inside] == value).all() and (out <= value).all(), (fmt, value)


def test_a_half_pixel_shift_of_a_two_valued_image_gives_the_rounded_mean():
    W, H = 16, 8
    for lo, hi in ((0, 255), (10, 13), (254, 255), (7, 7)):
        cols = np.where(np.arange(W) % 2 == 0, lo, hi)
        s, raw = fc.pack_grey(np.broadcast_to(cols, (H, W)).astype(np.uint8), fc.GRAY8)
        y, x = np.mgrid[0:H, 0:W - 1]
        out = convert.remap_frame_host(s, np.stack([32 * x + 16, 32 * y], axis=-1).astype(np.int32), raw)
        assert (out == (lo + hi + 1) // 2).all()                                   # (16 * 32 (lo + hi) + 512) >> 10: halves rounded up
        s, raw = fc.pack_grey(np.broadcast_to(cols[:H, None], (H, W)).astype(np.uint8), fc.GRAY8)
        y, x = np.mgrid[0:H - 1, 0:W]
        out = convert.remap_frame_host(s, np.stack([32 * x, 32 * y + 16], axis=-1).astype(np.int32), raw)
        assert (out == (lo + hi + 1) // 2).all()
        out = convert.remap_frame_host(s, np.stack([32 * x + 16, 32 * y + 16], axis=-1).astype(np.int32)[:, :-1], raw)
        assert (out == (lo + hi + 1) // 2).all()                                   # four taps: 256 (2 lo + 2 hi)


@pytest.mark.parametrize("name", [n for n in rm.LENS_CASES if not n.startswith("fisheye")])
def test_radial1_and_brown_maps_equal_the_definition_exactly(name):
    ln, target = rm.LENS_CASES[name]
    got = convert.lens_map(ln, target)
    want = rm.lens_reference(ln, target)
    assert got.shape == (target["height"], target["width"], 2) and got.dtype == np.int32
    assert np.array_equal(got, want), int((got != want).any(axis=-1).sum())
    live = want[..., 0] != rm.BORDER
    assert live.sum() > 100
    if name in ("radial1_to_radial", "brown_to_radial", "brown_zero_denominator", "radial1_negative"):
        assert (~live).any(), name           # f <= 0, q <= 0 or den == 0 somewhere: border entries are part of the comparison
    if name == "brown_zero_denominator":
        assert not live[8, 20] and not live[12, 16] and live[8, 19]          # (dx, dy) = (4, 0), (0, 4): r2 == 1, den == 0


FISHEYE_WINDOW = 1e-9


@pytest.mark.parametrize("name", [n for n in rm.LENS_CASES if n.startswith("fisheye")])
def test_fisheye_maps_equal_the_definition_but_for_atan_at_a_rounding_edge(name):
    """atan may differ in its last place between NumPy's and the C library's, so an entry may differ by one unit - only where the
    restatement's unrounded 32 us + 0.5 lies within 1e-9 of an integer.  With the coefficients of frame_remap_cases.LENS_CASES the
    restatement alone puts 0 of the 2 x 153600 coordinates in that window (asserted below: the comparison is exact for these
    calibrations, and the test fails loudly if an edit of the table moves an entry into the window unnoticed); the nearest lies
    1.3e-6 from an integer."""
    ln, target = rm.LENS_CASES[name]
    got = convert.lens_map(ln, target).astype(np.int64)
    valid, tx, ty = rm.lens_positions(ln, target)
    want = rm.lens_reference(ln, target).astype(np.int64)
    assert np.array_equal(got[..., 0] == rm.BORDER, ~valid)
    near = np.stack([np.abs(tx - np.rint(tx)) < FISHEYE_WINDOW, np.abs(ty - np.rint(ty)) < FISHEYE_WINDOW], axis=-1) & valid[..., None]
    print("%s: %d coordinates within %g of an integer" % (name, int(near.sum()), FISHEYE_WINDOW))
    assert int(near.sum()) == 0
    diff = np.abs(got - want)
    assert (diff[~near] == 0).all() and (diff[near] <= 1).all()
    assert valid.all() and (want[..., 0].min() < 32 * 320) and (want[..., 0].max() > 32 * 960)      # half the width of the source and more
    if name == "fisheye_to_radial":
        assert tuple(got[120, 160]) == (int(np.floor(639.4 * 32 + 0.5)), int(np.floor(481.2 * 32 + 0.5)))      # r == 0 gives (cx, cy)


def test_brown_without_distortion_and_lens_equal_to_target_is_the_identity_map_exactly():
    for w, h, f, cx, cy in ((320, 240, 195.0, 162.0, 125.0), (33, 17, 20.0, 16.0, 8.0), (64, 48, 64.0, 0.0, 47.0)):
        xy = convert.lens_map(rm.lens(rm.BROWN, w, h, f, f, cx, cy), rm.camera(w, h, f, f, cx, cy))
        assert np.array_equal(xy, rm.make_map("identity", w, h, w, h, 0))


def test_radial1_with_lens_equal_to_target_is_the_identity_to_within_one_unit():
    for w, h, fx, fy, cx, cy, kd1 in ((320, 240, 195.0, 193.0, 162.3, 125.1, 6e-6), (97, 53, 60.0, 61.0, 47.3, 25.9, 4e-5)):
        xy = convert.lens_map(rm.lens(rm.RADIAL1, w, h, fx, fy, cx, cy, [kd1]), rm.camera(w, h, fx, fy, cx, cy, kd1)).astype(np.int64)
        assert (xy[..., 0] != rm.BORDER).all()
        assert np.abs(xy - rm.make_map("identity", w, h, w, h, 0)).max() <= 1


def test_pinhole_camera_of_a_lens_without_distortion_gives_the_plain_resize():
    """Exact where the scale is a power of two (every intermediate is a binary fraction); elsewhere the entry is the rounding of
    (x + 0.5) W / out_w - 0.5 up to the few ulps of the detour through the image plane: |X - 32 us| <= 0.5 + 1e-6."""
    for (W, H), (ow, oh) in (((640, 480), (320, 240)), ((64, 48), (128, 96)), ((1280, 960), (320, 240)), ((640, 480), (33, 17)), ((47, 17), (65, 9))):
        ln = rm.lens(rm.BROWN, W, H, 400.0, 300.0, W / 2 - 0.5, H / 2 - 0.5)
        cam = convert.pinhole_camera(ln, ow, oh, sd=2)
        assert cam == dict(width=ow, height=oh, fku=400.0 * ow / W, fkv=300.0 * oh / H, u0=(W / 2) * ow / W - 0.5, v0=(H / 2) * oh / H - 0.5, kd1=0.0, sd=2)
        xy = convert.lens_map(ln, cam).astype(np.float64)
        us = (np.arange(ow) + 0.5) * W / ow - 0.5
        vs = (np.arange(oh) + 0.5) * H / oh - 0.5
        if (W / ow, H / oh) in ((2.0, 2.0), (0.5, 0.5), (4.0, 4.0)):
            assert np.array_equal(xy[..., 0], np.broadcast_to(np.floor(32 * us + 0.5)[None, :], (oh, ow)))
            assert np.array_equal(xy[..., 1], np.broadcast_to(np.floor(32 * vs + 0.5)[:, None], (oh, ow)))
        assert np.abs(xy[..., 0] - 32 * us[None, :]).max() <= 0.5 + 1e-6 and np.abs(xy[..., 1] - 32 * vs[:, None]).max() <= 0.5 + 1e-6
    # with a resize of equal scale it is sl2_scale_camera's calibration of the same lens
    ln = rm.lens(rm.RADIAL1, 640, 480, 400.0, 300.0, 317.0, 245.0, [0.0])
    assert convert.pinhole_camera(ln, 320, 240, sd=1) == convert.scale_camera(rm.camera(640, 480, 400.0, 300.0, 317.0, 245.0), 320, 240)


def test_a_remapped_frame_of_a_distorted_camera_matches_the_target_cameras_view():
    """End to end on the host, no restatement: a smooth scene sampled under a RADIAL1 lens, remapped into a pinhole target, equals
    the scene sampled under the target, up to interpolation (the scene varies by less than 2 grey levels a source pixel)."""
    ln = rm.lens(rm.RADIAL1, 320, 240, 200.0, 200.0, 159.5, 119.5, [4e-6])
    target = rm.camera(160, 120, 100.0, 100.0, 79.5, 59.5)

    def scene(a, b):            # grey of the ray with image-plane coordinates (a, b)
        return 128 + 60 * np.sin(3 * a) * np.cos(2 * b) + 40 * np.cos(5 * b + a)

    v, u = np.mgrid[0:240, 0:320].astype(np.float64)
    cx, cy = u - 159.5, v - 119.5
    s = np.sqrt(1 - 2 * 4e-6 * (cx * cx + cy * cy))                                # Unproject: source pixel -> image plane
    src_img = np.rint(scene(cx / s / 200.0, cy / s / 200.0)).astype(np.uint8)
    y, x = np.mgrid[0:120, 0:160].astype(np.float64)
    want = scene((x - 79.5) / 100.0, (y - 59.5) / 100.0)
    s8, raw = fc.pack_grey(src_img, fc.GRAY8)
    xy = convert.lens_map(ln, target)
    got = convert.remap_frame_host(s8, xy, raw).astype(np.float64)
    live = xy[..., 0] != rm.BORDER
    assert live.all() and np.abs(got - want).max() <= 2.0
    # a mirrored or turned map would miss by far more
    assert np.abs(got[:, ::-1] - want).max() > 20 and np.abs(got[::-1] - want).max() > 20


def _host_rc(s, raw_bytes, xy_ok=True, ow=2, oh=2, nbuf=None):
    L = _lib.load()
    buf = np.zeros(nbuf if nbuf is not None else max(int(raw_bytes), 1), np.uint8)
    out = np.zeros(ow * oh, np.uint8)
    xy = np.zeros((oh, ow, 2), np.int32)
    src = _lib.sl2_frame_source(s["width"], s["height"], s["pitch"], s["format"], s["offset"])
    return L.sl2_remap_frame_host(C.byref(src), _lib.ip(xy) if xy_ok else None, buf.ctypes.data_as(_lib.vp), int(raw_bytes), ow, oh, _lib.u8p(out))


def test_host_refusals_name_the_sequence():
    L = _lib.load()
    err = lambda: L.sl2_last_error().decode()
    for fmt in rm.FORMATS:          # one byte short of its reach, per format; the exact size passes
        pads, offs = rm.pads_offsets(fmt)
        good = rm.source(16, 9, fmt, pads[2], offs[1])
        need = rm.source_bytes(good)
        assert _host_rc(good, need) == _lib.SL2_OK
        assert _host_rc(good, need - 1, nbuf=need) == _lib.SL2_ERR_INVALID
        assert "sl2_remap_frame_host" in err() and "sequence 0" in err() and "past the raw buffer" in err()
    assert _host_rc(rm.source(16, 9, fc.GRAY8), 144, xy_ok=False) == _lib.SL2_ERR_INVALID and "bad arguments" in err()
    src = _lib.sl2_frame_source(16, 9, 16, 0, 0)
    one = np.zeros(8, np.int32)
    buf = np.zeros(144, np.uint8)
    for ow, oh in ((0, 2), (2, 0), (4097, 1), (1, 4097)):
        assert L.sl2_remap_frame_host(C.byref(src), _lib.ip(one), buf.ctypes.data_as(_lib.vp), 144, ow, oh, _lib.u8p(buf)) == _lib.SL2_ERR_INVALID
    for bad, text in ((dict(rm.source(16, 9, fc.GRAY8), format=5), "unknown pixel format"), (rm.source(15, 9, fc.UYVY), "odd width"),
                      (rm.source(1, 9, rc.BAYER_RGGB8), "Bayer source under 2 pixels"), (rm.source(16, 9, rc.GRAY12, pad=1), "odd offset or pitch"),
                      (rm.source(4097, 2, fc.GRAY8), "width over 4096"), (rm.source(2, 16385, fc.GRAY8), "height over 16384"),
                      (dict(rm.source(16, 9, fc.RGB24), pitch=47), "pitch below"), (rm.source(0, 9, fc.GRAY8), "below 1")):
        assert _host_rc(bad, 1 << 20, nbuf=64) == _lib.SL2_ERR_INVALID, bad
        assert text in err() and "sequence 0" in err(), (bad, err())
    # the map builder and the pinhole target
    good_lens, good_cam = _lib.sl2_lens(1, 64, 48, 40.0, 40.0, 32.0, 24.0), _lib.make_camera(rm.camera(8, 4, 5.0, 5.0, 4.0, 2.0))
    xy = np.zeros((4, 8, 2), np.int32)
    out = _lib.sl2_camera()
    assert L.sl2_lens_map_host(C.byref(good_lens), C.byref(good_cam), _lib.ip(xy)) == _lib.SL2_OK
    assert L.sl2_lens_map_host(None, C.byref(good_cam), _lib.ip(xy)) == _lib.SL2_ERR_INVALID
    assert L.sl2_lens_map_host(C.byref(good_lens), None, _lib.ip(xy)) == _lib.SL2_ERR_INVALID
    assert L.sl2_lens_map_host(C.byref(good_lens), C.byref(good_cam), None) == _lib.SL2_ERR_INVALID
    for model in (-1, 3, 99):
        bad = _lib.sl2_lens(model, 64, 48, 40.0, 40.0, 32.0, 24.0)
        assert L.sl2_lens_map_host(C.byref(bad), C.byref(good_cam), _lib.ip(xy)) == _lib.SL2_ERR_INVALID and "unknown lens model" in err()
        assert L.sl2_lens_pinhole_camera(C.byref(bad), 8, 4, 1, C.byref(out)) == _lib.SL2_ERR_INVALID and "unknown lens model" in err()
    for w, h in ((0, 48), (64, 0), (4097, 48), (64, 16385)):
        bad = _lib.sl2_lens(1, w, h, 40.0, 40.0, 32.0, 24.0)
        assert L.sl2_lens_map_host(C.byref(bad), C.byref(good_cam), _lib.ip(xy)) == _lib.SL2_ERR_INVALID and "lens image" in err()
        assert L.sl2_lens_pinhole_camera(C.byref(bad), 8, 4, 1, C.byref(out)) == _lib.SL2_ERR_INVALID
    for w, h in ((0, 4), (8, 0), (4097, 4), (8, 4097)):
        bad = _lib.make_camera(rm.camera(w, h, 5.0, 5.0, 4.0, 2.0))
        assert L.sl2_lens_map_host(C.byref(good_lens), C.byref(bad), _lib.ip(xy)) == _lib.SL2_ERR_INVALID and "target size" in err()
        assert L.sl2_lens_pinhole_camera(C.byref(good_lens), w, h, 1, C.byref(out)) == _lib.SL2_ERR_INVALID and "output size" in err()
    assert L.sl2_lens_pinhole_camera(C.byref(good_lens), 8, 4, 1, None) == _lib.SL2_ERR_INVALID


def test_python_surface_and_header():
    assert convert.LENS_MODELS == {"radial1": 0, "brown": 1, "fisheye": 2} and convert.SL2_REMAP_BORDER == -2 ** 31 == rm.BORDER
    assert C.sizeof(_lib.sl2_lens) == 112
    ln = convert.make_lens(dict(model="Fisheye", width=10, height=8, fx=1, fy=2, cx=3, cy=4, k=[5, 6]))
    assert (ln.model, ln.width, ln.height, ln.fx, ln.fy, ln.cx, ln.cy, list(ln.k)) == (2, 10, 8, 1.0, 2.0, 3.0, 4.0, [5.0, 6.0, 0, 0, 0, 0, 0, 0])
    assert convert.make_lens(ln) is ln
    header = open(os.path.join(ROOT, "include", "scenelib2_amd.h")).read()
    assert re.search(r"#define SL2_REMAP_BORDER INT32_MIN\b", header)
    assert re.search(r"SL2_LENS_RADIAL1 = 0, SL2_LENS_BROWN = 1, SL2_LENS_FISHEYE = 2", header)
    for sym in ("sl2_converter_set_map", "sl2_converter_set_remaps", "sl2_converter_get_remaps", "sl2_remap_frame_host", "sl2_lens_map_host",
                "sl2_lens_pinhole_camera"):
        assert sym in _lib.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % sym, header) and hasattr(_lib.load(), sym)
    assert re.search(r"#define SL2_API_VERSION 5\b", header)
    for m in ("set_map", "set_remaps", "get_remaps"):
        assert callable(getattr(convert.FrameConverter, m))


def test_host_body_stays_inside_exactly_sized_blocks_under_asan(tmp_path):
    """tests/frame_remap_host.cpp: a program of its own (nothing loaded into Python), built with the address and
    undefined-behaviour sanitizers: maps that point at and around every edge of a tightly allocated source, every format."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = os.path.join(str(tmp_path), "frame_remap_host")
    src = os.path.join(ROOT, "tests", "frame_remap_host.cpp")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.startswith("ok ")


def test_adapters_have_set_lens_and_the_cpp_one_compiles(tmp_path):
    import inspect
    import scenelib2_amd
    assert list(inspect.signature(scenelib2_amd.MonoSLAM.SetLens).parameters) == ["self", "lens", "target"]
    hpp = open(os.path.join(ROOT, "include", "scenelib2_amd_monoslam.hpp")).read()
    assert "void SetLens(const sl2_lens& lens, const sl2_camera& target)" in hpp
    for call in ("sl2_lens_map_host", "sl2_converter_set_map", "sl2_converter_set_remaps"):
        assert call in hpp
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(str(tmp_path), "set_lens.cpp")
    with open(src, "w") as f:
        f.write('#include <scenelib2_amd_monoslam.hpp>\n'
                'void use(SceneLib2Amd::MonoSLAM& m, const sl2_lens& lens) {\n'
                '  sl2_camera target;\n'
                '  if (sl2_lens_pinhole_camera(&lens, 320, 240, 1, &target) == SL2_OK) m.SetLens(lens, target);\n'
                '  m.SetFrameSource(lens.width, lens.height, lens.width, SL2_PIX_GRAY8);\n'
                '}\n')
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src])
