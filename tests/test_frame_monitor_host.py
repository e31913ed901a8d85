"""The frame monitor, host side: sl2_frame_stats_host and sl2_frame_verdict_host against a NumPy restatement of the definitions
(frame_monitor_cases.py, written from the header's text; it calls nothing of the library) over the case table, the digest's
properties, accumulators beyond 32 bits, the verdict's truth table, the Python surface, the stand-alone bounds program under
AddressSanitizer and the adapters.  (The kernels: tests/test_gpu_frame_monitor.py, which also holds the refusals of the setters
of a live monitor - a monitor needs a device.)"""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import frame_monitor_cases as fm

from scenelib2_amd import _lib, frame_monitor as M


def test_case_table_covers_the_shapes_the_band_edges_and_the_contents():
    assert {(1, 1), (2, 2), (3, 3), (8, 1), (1, 9), (7, 5), (16, 3), (17, 4), (33, 9), (64, 64), (321, 7), (320, 240)} <= set(fm.SHAPES)
    assert fm.BAND == 32 and fm.BAND % 16 == 0
    for k in (1, 2):
        for d in (-1, 0, 1):          # a band that ends one row before, at and one row after the last row
            assert {w for w, h in fm.SHAPES if h == k * fm.BAND + d} >= {5, 16, 23}
    assert set(fm.CONTENTS) == {"random", "zeros", "white", "checker", "corners", "band_edges"}
    assert fm.STRIDE_PADS == (0, 1, 3, 16) and fm.OFFSETS == (0, 1, 8)
    f = fm.frame((23, 65), "band_edges")
    assert f[31, 0] == f[32, 0] == f[63, 0] == f[64, 0] == 240 and f[31, 22] == f[64, 22] == 241 and f[30, 0] == 16
    f = fm.frame((7, 5), "corners")
    assert f[0, 0] == f[0, 6] == f[4, 0] == f[4, 6] == 250 and (f == 250).sum() == 4
    src = open(os.path.join(ROOT, "scenelib2_amd", "csrc", "sl2_frame_monitor_dev.hpp")).read()
    assert re.search(r"constexpr int kFrameBandRows = %d;" % fm.BAND, src)


def test_host_form_equals_the_definition_on_the_whole_table():
    for shape, content in fm.CASES:
        f = fm.frame(shape, content)
        got, want = fm.as_dict(M.frame_stats_host(f)), fm.reference(f)
        assert got == want, (shape, content, {k: (got[k], want[k]) for k in got if got[k] != want[k]})


def test_digest_notices_a_changed_byte_a_swap_and_swapped_rows():
    f = fm.frame((33, 9), "random")
    d0 = int(M.frame_stats_host(f)["digest"])
    for y, x in ((0, 0), (0, 7), (0, 8), (4, 16), (8, 32)):
        g = f.copy(); g[y, x] ^= 1
        assert int(M.frame_stats_host(g)["digest"]) != d0
    for a, b in (((0, 0), (0, 1)), ((0, 7), (0, 8)), ((0, 0), (8, 32)), ((3, 3), (3, 19))):          # inside a word, across words, far apart
        assert f[a] != f[b]
        g = f.copy(); g[a], g[b] = f[b], f[a]
        s = M.frame_stats_host(g)
        assert int(s["digest"]) != d0 and int(s["sum"]) == int(f.sum()) and list(s["hist"]) == list(M.frame_stats_host(f)["hist"])
    g = f.copy(); g[[2, 5]] = f[[5, 2]]
    assert int(M.frame_stats_host(g)["digest"]) != d0
    # a frame of equal words still depends on where they are: the word index is mixed in
    z = np.zeros((4, 8), np.uint8); z[0, 0] = 1
    z2 = np.zeros((4, 8), np.uint8); z2[1, 0] = 1
    assert int(M.frame_stats_host(z)["digest"]) != int(M.frame_stats_host(z2)["digest"])


def test_digest_and_record_are_the_same_under_every_stride_and_pointer_offset():
    for shape in ((7, 5), (17, 4), (33, 9), (16, 33)):
        f = fm.frame(shape, "random")
        want = M.frame_stats_host(f).tobytes()
        n = f.size
        for pad in fm.STRIDE_PADS:
            for off in fm.OFFSETS:
                buf = np.full(off + 2 * (n + pad) + 64, 0xEE, np.uint8)
                for b in range(2):          # the second frame of a batch with this stride
                    buf[off + b * (n + pad): off + b * (n + pad) + n] = f.reshape(-1)
                    view = buf[off + b * (n + pad):]
                    assert M.frame_stats_host(view, shape[0], shape[1]).tobytes() == want, (shape, pad, off, b)


def test_accumulators_beyond_32_bits():
    w, h = 4096, 4200
    s = M.frame_stats_host(np.full((h, w), 255, np.uint8))
    assert int(s["sum_sq"]) == 255 ** 2 * 17203200 > 2 ** 32 and int(s["sum"]) == 255 * 17203200
    assert int(s["hist"][15]) == w * h and int(s["gradient_energy"]) == 0 and (int(s["min"]), int(s["max"])) == (255, 255)
    y, x = np.mgrid[0:h, 0:w]
    s = M.frame_stats_host((((x + y) & 1) * 255).astype(np.uint8))          # a checkerboard: both differences vanish (x +- 1 share a colour)
    assert int(s["gradient_energy"]) == 0
    s = M.frame_stats_host((((x >> 1) & 1) * 255).astype(np.uint8))         # columns in pairs: |dx| = 255 everywhere inside
    assert int(s["gradient_energy"]) == 255 ** 2 * (w - 2) * (h - 2) > 2 ** 32


def _rec(**kw):
    r = dict(sum=0, sum_sq=0, gradient_energy=0, digest=0, min=0, max=0, hist=[0] * 16)
    r.update(kw)
    return r


def _both(rec, gate, have=False, prev=0):
    arr = np.zeros(1, _lib.FRAME_STATS_DTYPE)
    for k, v in rec.items():
        arr[0][k] = v
    got = M.frame_verdict_host(arr[0], gate, have, prev)
    assert got == fm.verdict(rec, gate, have, prev), (rec, gate, have, prev)
    return got


def test_verdict_truth_table_at_and_around_every_threshold():
    # FLAT: max - min < min_range
    for rng, want in ((9, 0), (10, 0), (11, fm.FLAT)):
        assert _both(_rec(min=20, max=30), dict(min_range=rng)) == want
    assert _both(_rec(min=7, max=7), dict(min_range=0)) == 0 and _both(_rec(min=7, max=7), dict(min_range=1)) == fm.FLAT
    # DARK / BRIGHT: more pixels than the threshold in the end bins
    hist = list(range(1, 17))          # bin b holds b + 1 pixels
    for bins in (1, 2, 15, 16):
        dark, bright = sum(hist[:bins]), sum(hist[16 - bins:])
        for d, want in ((-1, fm.DARK), (0, 0), (1, 0)):
            assert _both(_rec(hist=hist), dict(dark_bins=bins, max_dark_pixels=dark + d)) == want
        for d, want in ((-1, fm.BRIGHT), (0, 0), (1, 0)):
            assert _both(_rec(hist=hist), dict(bright_bins=bins, max_bright_pixels=bright + d)) == want
    assert _both(_rec(hist=hist), dict(dark_bins=0, max_dark_pixels=0, bright_bins=0, max_bright_pixels=0)) == 0          # 0 bins: off
    assert _both(_rec(hist=[2 ** 32 - 1] * 16), dict(dark_bins=16, max_dark_pixels=2 ** 32 - 1)) == fm.DARK               # the sum is wider than a word
    # BLURRED: gradient_energy < min_gradient_energy, 64-bit
    for e in (5, 2 ** 40):
        for d, want in ((-1, 0), (0, 0), (1, fm.BLURRED)):
            assert _both(_rec(gradient_energy=e), dict(min_gradient_energy=e + d)) == want
    assert _both(_rec(gradient_energy=0), dict(min_gradient_energy=0)) == 0
    # REPEATED: only with the rule on, a previous digest, and that digest
    for on, have, prev, want in ((1, True, 99, fm.REPEATED), (1, False, 99, 0), (1, True, 98, 0), (0, True, 99, 0), (7, True, 99, fm.REPEATED)):
        assert _both(_rec(digest=99), dict(reject_repeated=on), have, prev) == want
    assert _both(_rec(digest=2 ** 64 - 1), dict(reject_repeated=1), True, 2 ** 64 - 1) == fm.REPEATED
    # several rules together OR their bits
    g = dict(min_range=5, dark_bins=1, max_dark_pixels=3, bright_bins=1, max_bright_pixels=3, reject_repeated=1, min_gradient_energy=50)
    r = _rec(min=3, max=4, hist=[4] + [0] * 14 + [4], gradient_energy=49, digest=5)
    assert _both(r, g, True, 5) == fm.FLAT | fm.DARK | fm.BRIGHT | fm.BLURRED | fm.REPEATED == 31
    assert _both(r, dict(g, dark_bins=0, min_gradient_energy=0), True, 6) == fm.FLAT | fm.BRIGHT
    assert _both(r, {}, True, 5) == 0          # every rule is off by default


def test_host_refusals():
    L = _lib.load()
    s = _lib.sl2_frame_stats()
    f = np.zeros(16, np.uint8)
    ptr = f.ctypes.data_as(_lib.vp)
    assert L.sl2_frame_stats_host(ptr, 4, 4, C.byref(s)) == _lib.SL2_OK
    for w, h in ((0, 4), (4, 0), (-1, 4), (65536, 32768)):
        assert L.sl2_frame_stats_host(ptr, w, h, C.byref(s)) == _lib.SL2_ERR_INVALID and "sl2_frame_stats_host" in L.sl2_last_error().decode()
    assert L.sl2_frame_stats_host(None, 4, 4, C.byref(s)) == _lib.SL2_ERR_INVALID and L.sl2_frame_stats_host(ptr, 4, 4, None) == _lib.SL2_ERR_INVALID
    g = _lib.sl2_frame_gate()
    assert L.sl2_frame_verdict_host(C.byref(s), C.byref(g), 0, 0) == 0
    assert L.sl2_frame_verdict_host(None, C.byref(g), 0, 0) == 0xFFFFFFFF and L.sl2_frame_verdict_host(C.byref(s), None, 0, 0) == 0xFFFFFFFF
    for bad in (dict(dark_bins=17), dict(bright_bins=17), dict(dark_bins=2 ** 32 - 1)):
        with pytest.raises(_lib.Sl2Error) as ei:
            M.frame_verdict_host(s, bad)
        assert ei.value.code == _lib.SL2_ERR_INVALID and "bins over 16" in str(ei.value)
    assert M.frame_verdict_host(_lib.sl2_frame_stats(), dict(dark_bins=16, bright_bins=16)) == 0          # 16 bins pass the validator; an empty record has no pixel
    assert M.frame_verdict_host(s, dict(dark_bins=16, bright_bins=16, max_dark_pixels=15, max_bright_pixels=16)) == fm.DARK          # s: 16 black pixels
    if _lib.device_count() < 1:          # a monitor needs a device: loudly, no host-only stand-in
        h = _lib.vp()
        assert L.sl2_frame_monitor_create(0, 1, 4, 4, C.byref(h)) == _lib.SL2_ERR_NO_DEVICE and not h.value


def test_python_surface_and_header():
    assert C.sizeof(_lib.sl2_frame_stats) == 104 == _lib.FRAME_STATS_DTYPE.itemsize and C.sizeof(_lib.sl2_frame_gate) == 32
    assert [n for n, _ in _lib.sl2_frame_gate._fields_] == list(fm.GATE_FIELDS) == list(M.GATE_FIELDS)
    assert [n for n, _ in _lib.sl2_frame_stats._fields_] == list(_lib.FRAME_STATS_DTYPE.names)
    assert M.VERDICT_BITS == dict(flat=1, dark=2, bright=4, blurred=8, repeated=16, skipped=32)
    assert (fm.FLAT, fm.DARK, fm.BRIGHT, fm.BLURRED, fm.REPEATED, fm.SKIPPED) == (1, 2, 4, 8, 16, 32)
    assert M.verdict_names(18) == ["dark", "repeated"]
    header = open(os.path.join(ROOT, "include", "scenelib2_amd.h")).read()
    assert re.search(r"SL2_FRAME_FLAT = 1, SL2_FRAME_DARK = 2, SL2_FRAME_BRIGHT = 4, SL2_FRAME_BLURRED = 8, SL2_FRAME_REPEATED = 16, SL2_FRAME_SKIPPED = 32", header)
    assert re.search(r"typedef struct sl2_frame_stats \{\s+/\* 104 bytes \*/", header)
    body = re.search(r"typedef struct sl2_frame_gate \{(.*?)\} sl2_frame_gate;", header, flags=re.S).group(1)
    assert re.findall(r"uint(?:32|64)_t (\w+);", body) == list(fm.GATE_FIELDS)
    body = re.search(r"typedef struct sl2_frame_stats \{(.*?)\} sl2_frame_stats;", header, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[16\])?[;,]", re.sub(r"/\*.*?\*/", "", body)) == ["sum", "sum_sq", "gradient_energy", "digest", "min", "max", "hist"]
    for sym in ("sl2_frame_monitor_create", "sl2_frame_monitor_set_gates", "sl2_frame_monitor_get_gates", "sl2_frame_monitor_reset",
                "sl2_examine_frames", "sl2_frame_monitor_read", "sl2_frame_stats_host"):
        assert sym in _lib.EXPORTED_SYMBOLS and re.search(r"\bint %s\(" % sym, header) and hasattr(_lib.load(), sym)
    assert "sl2_frame_monitor_destroy" in _lib.EXPORTED_SYMBOLS and re.search(r"\bvoid sl2_frame_monitor_destroy\(", header)
    assert "sl2_frame_verdict_host" in _lib.EXPORTED_SYMBOLS and re.search(r"\buint32_t sl2_frame_verdict_host\(", header)
    assert re.search(r"#define SL2_API_VERSION 5\b", header) and "sl2_examine_frames, sl2_frame_monitor_read" in header.split("#define SL2_API_VERSION")[0]
    for m in ("examine", "read", "set_gates", "get_gates", "reset"):
        assert callable(getattr(M.FrameMonitor, m))
    g = M.make_gate(dict(min_range=3), reject_repeated=1, min_gradient_energy=2 ** 40)
    assert M.gate_dict(g) == dict(min_range=3, dark_bins=0, max_dark_pixels=0, bright_bins=0, max_bright_pixels=0, reject_repeated=1,
                                  min_gradient_energy=2 ** 40) and M.make_gate(g) is g
    with pytest.raises(ValueError):
        M.make_gate(dict(min_rnge=3))


def test_host_body_stays_inside_exactly_sized_blocks_under_asan(tmp_path):
    """tests/frame_monitor_host.cpp: a program of its own (nothing loaded into Python), built with the address and
    undefined-behaviour sanitizers: the host body over a heap block of exactly width * height bytes for every shape of the table."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = os.path.join(str(tmp_path), "frame_monitor_host")
    src = os.path.join(ROOT, "tests", "frame_monitor_host.cpp")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src])
    shapes = [str(v) for s in fm.SHAPES for v in s]
    res = subprocess.run([exe] + shapes, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.startswith("ok %d runs" % (5 * len(fm.SHAPES)))


def test_adapters_have_set_frame_gate_and_the_cpp_one_compiles(tmp_path):
    import scenelib2_amd
    assert list(inspect.signature(scenelib2_amd.MonoSLAM.SetFrameGate).parameters) == ["self", "gate", "catch_up"]
    assert inspect.signature(scenelib2_amd.MonoSLAM.SetFrameGate).parameters["catch_up"].default is False
    assert callable(scenelib2_amd.MonoSLAM.LastFrameVerdict)
    hpp = open(os.path.join(ROOT, "include", "scenelib2_amd_monoslam.hpp")).read()
    assert "void SetFrameGate(const sl2_frame_gate& gate, bool catch_up = false)" in hpp and "uint32_t LastFrameVerdict() const" in hpp
    for call in ("sl2_frame_monitor_create", "sl2_examine_frames", "sl2_set_active_sequences", "sl2_frame_stats_host", "sl2_frame_verdict_host",
                 "sl2_set_pause_catch_up", "sl2_frame_monitor_destroy"):
        assert call in hpp
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(str(tmp_path), "set_frame_gate.cpp")
    with open(src, "w") as f:
        f.write('#include <scenelib2_amd_monoslam.hpp>\n'
                'unsigned use(SceneLib2Amd::MonoSLAM& m) {\n'
                '  sl2_frame_gate gate = sl2_frame_gate();\n'
                '  gate.reject_repeated = 1; gate.dark_bins = 1; gate.max_dark_pixels = 320 * 240 / 2;\n'
                '  m.SetFrameGate(gate);\n'
                '  m.SetFrameGate(gate, true);\n'
                '  return m.LastFrameVerdict() & SL2_FRAME_REPEATED;\n'
                '}\n')
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src])
