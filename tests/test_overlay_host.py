"""Annotated frames, host side: sl2_draw_items_host byte for byte against a NumPy restatement of the header's pixel rules
(overlay_cases.py; it calls nothing of the library), the refusals, the particle counter and its bound, the symbols, and the
stand-alone program over the same cases under the address and undefined-behaviour sanitizers.  (The kernels:
tests/test_gpu_overlay.py.)"""
import ctypes as C
import inspect
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import overlay_cases as oc

from scenelib2_amd import _lib, overlay

NEW = ["sl2_overlay_item_bound", "sl2_overlay_items", "sl2_draw_items_batch", "sl2_draw_overlays", "sl2_draw_items_host"]


def _header():
    return open(os.path.join(ROOT, "include", "scenelib2_amd.h")).read()


def test_item_is_64_bytes_and_the_python_dtype_is_the_cases_dtype():
    assert oc.ITEM.itemsize == 64 and overlay.ITEM_DTYPE == oc.ITEM
    assert [oc.ITEM.fields[n][1] for n in ("kind", "label", "a", "patch", "rgb", "pad", "q")] == [0, 4, 8, 24, 28, 31, 32]
    h = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = h[h.index("typedef struct sl2_overlay_item {"):h.index("} sl2_overlay_item;")]
    assert re.findall(r"\b(\w+)(?:\[\d\])?;", body) == ["kind", "label", "a", "patch", "rgb", "pad", "q"]
    assert "SL2_ITEM_RING = 1, SL2_ITEM_PATCH = 2, SL2_ITEM_RECT = 3" in h
    assert "SL2_OVERLAY_SEARCH_REGIONS = 1, SL2_OVERLAY_DESCRIPTORS = 2, SL2_OVERLAY_INITIALISATION = 4" in h
    assert (overlay.SL2_ITEM_RING, overlay.SL2_ITEM_PATCH, overlay.SL2_ITEM_RECT) == (oc.RING, oc.PATCH, oc.RECT) == (1, 2, 3)


def test_case_list_holds_what_the_contract_names():
    names = [c[0] for c in oc.CASES]
    assert len(names) == len(set(names))
    for w, h in oc.SIZES:
        for stem in ("empty", "ring_interior", "ring_clipped_left", "ring_clipped_right", "ring_clipped_top", "ring_clipped_bottom",
                     "ring_centre_off_image", "ring_larger_than_image", "ring_one_pixel", "ring_eccentric_30", "ring_invalid_forms",
                     "ring_across_tile_edges", "patch_corners", "patch_half_off", "rect_forms", "painter_order_0", "painter_order_5",
                     "bad_kind", "bad_patch_index", "many_items"):
            assert "%s_%dx%d" % (stem, w, h) in names
    assert (70 * 3) % 4 != 0 and 70 % 64 and 37 % 16 and (64, 16) in oc.SIZES
    assert max(len(c[2]) for c in oc.CASES) > 2 * 256          # more than two rounds of the kernel's staging


@pytest.mark.parametrize("case", oc.CASES, ids=[c[0] for c in oc.CASES])
def test_host_form_equals_the_restated_rules(case):
    name, (w, h), items, patches = case
    frame = oc.frame_of(w, h, seed=len(name))
    want = oc.reference(frame, items, patches)
    got = overlay.draw_items_host(frame, oc.items_array(items), patches)
    assert got.shape == (h, w, 3)
    assert np.array_equal(got, want), (name, np.argwhere((got != want).any(axis=2))[:5].tolist())


def test_cases_draw_what_their_names_say():
    """The restated rules themselves, on anchors small enough to check by eye."""
    by = {c[0]: c for c in oc.CASES}
    grey = lambda f: np.repeat(f[:, :, None], 3, axis=2)
    for w, h in oc.SIZES:
        sfx = "_%dx%d" % (w, h)
        for name in ("empty", "ring_invalid_forms", "bad_kind", "patch_without_array"):
            _, _, items, patches = by[name + sfx]
            f = oc.frame_of(w, h, 1)
            out = oc.reference(f, items, patches)
            changed = (out != grey(f)).any(axis=2)
            if name == "bad_kind":          # only its one good rectangle shows
                assert changed.sum() > 0 and not changed[5:, :].any() and not changed[:, 5:].any()
            elif name == "patch_without_array":          # the ring shows, the patch does not
                assert 0 < changed.sum() < 40
            else:
                assert not changed.any(), name
        f = np.zeros((h, w), np.uint8)
        one = oc.reference(f, by["ring_one_pixel" + sfx][2])
        assert (one.any(axis=2)).sum() == 3 and tuple(one[h // 2, w // 2]) == oc.GREEN and tuple(one[0, 0]) == oc.RED
        # a circle of radius 3: 16 rim pixels, none at the centre, symmetric
        c = oc.reference(f, [oc.circle(w // 2, h // 2, 3, oc.RED)]).any(axis=2)
        assert c.sum() == 16 and not c[h // 2 - 1:h // 2 + 2, w // 2 - 1:w // 2 + 2].any()
        assert c[h // 2 - 2:h // 2 + 3, w // 2 - 2:w // 2 + 3].sum() == 16
        # the painter's rule: each order of the three overlapping items gives another image, and the last item is whole
        imgs = [oc.reference(f, by["painter_order_%d%s" % (n, sfx)][2], by["painter_order_%d%s" % (n, sfx)][3]) for n in range(6)]
        assert len({im.tobytes() for im in imgs}) == 6
        for n in range(6):
            _, _, items, patches = by["painter_order_%d%s" % (n, sfx)]
            mask, colour = oc.covers(items[-1], w, h, patches)
            assert mask.any() and np.array_equal(imgs[n][mask], colour[mask])
    # a patch: 11 x 11 grey inside a one-pixel frame of its colour
    P = oc.patches_of(1)
    out = oc.reference(np.zeros((30, 30), np.uint8), [oc.patch(15, 14, 0, oc.BLUE)], P)
    assert np.array_equal(out[9:20, 10:21, 0], P[0].reshape(11, 11)) and np.array_equal(out[9:20, 10:21, 2], P[0].reshape(11, 11))
    assert (out[8, 9:22] == oc.BLUE).all() and (out[20, 9:22] == oc.BLUE).all() and (out[8:21, 9] == oc.BLUE).all() and (out[8:21, 21] == oc.BLUE).all()
    assert not out[7].any() and not out[:, 22].any()


def test_particle_counter_and_bound():
    for n in (1, 9, 10, 11, 19, 20, 25, 100):
        assert oc.particles_drawn(n) == oc.particles_drawn_reference(n), n
    assert oc.particles_drawn(1) == [0] and len(oc.particles_drawn(19)) == 19 and len(oc.particles_drawn(20)) == 10
    assert oc.particles_drawn(25) == list(range(1, 25, 2)) and oc.particles_drawn(100) == list(range(9, 100, 10))
    assert max(len(oc.particles_drawn(n)) for n in range(0, 1025)) == 19
    L = _lib.load()
    for N, k in ((16, 1), (100, 4), (676, 4), (0, 0)):
        assert L.sl2_overlay_item_bound(N, k) == 2 * N + 19 * k + 2 == overlay.item_bound(N, k)
    assert L.sl2_overlay_item_bound(-1, 1) == 0 and L.sl2_overlay_item_bound(4, -1) == 0


def _host_rc(frame, w, h, items, count, patches, stride, npatches, out):
    p = lambda a: None if a is None else a.ctypes.data_as(_lib.vp)
    return _lib.load().sl2_draw_items_host(p(frame), w, h, p(items), count, p(patches), stride, npatches, p(out))


def test_host_form_refusals():
    f, out = np.zeros((8, 8), np.uint8), np.full((8, 8, 3), 7, np.uint8)
    it = oc.items_array([oc.circle(4, 4, 2)])
    P = oc.patches_of(2)
    assert _host_rc(f, 8, 8, it, 1, P, 121, 2, out) == _lib.SL2_OK
    out[:] = 7
    for args in ((None, 8, 8, it, 1, P, 121, 2, out), (f, 8, 8, it, 1, P, 121, 2, None), (f, 8, 8, None, 1, P, 121, 2, out),
                 (f, 8, 8, it, -1, P, 121, 2, out), (f, 0, 8, it, 1, P, 121, 2, out), (f, 8, 0, it, 1, P, 121, 2, out),
                 (f, 32769, 1, it, 1, P, 121, 2, out), (f, 8, 8, it, 1, P, 120, 2, out), (f, 8, 8, it, 1, None, 121, 2, out),
                 (f, 8, 8, it, 1, P, 121, -1, out)):
        assert _host_rc(*args) == _lib.SL2_ERR_INVALID, args[1:3]
    assert (out == 7).all()
    assert _host_rc(f, 8, 8, None, 0, None, 0, 0, out) == _lib.SL2_OK and (out == 0).all()          # an empty list: the grey frame


def _batch_rc(frames, n, w, h, seq_stride, items, item_stride, counts, patches, pstride, npatches, out, out_stride, frames_dev=0, items_dev=0, out_dev=0):
    p = lambda a: None if a is None else a.ctypes.data_as(_lib.vp)
    return _lib.load().sl2_draw_items_batch(0, None, p(frames), frames_dev, n, w, h, seq_stride, p(items), item_stride, p(counts), items_dev, p(patches),
                                            pstride, npatches, p(out), out_stride, out_dev)


def test_batch_refusals_happen_on_the_host_and_name_the_image():
    """Every refusal comes before the device is touched, so it is the same with and without a GPU."""
    L = _lib.load()
    w, h, n = 8, 8, 3
    f, out = np.zeros((n, h, w), np.uint8), np.full((n, h, w, 3), 7, np.uint8)
    items = np.zeros((n, 4), oc.ITEM)
    items[:, 0] = oc.circle(4, 4, 2)
    items[:, 1] = oc.patch(4, 4, 1)
    counts = np.full(n, 2, np.int32)
    P = oc.patches_of(2)
    good = dict(frames=f, n=n, w=w, h=h, seq_stride=w * h, items=items, item_stride=4, counts=counts, patches=P, pstride=121, npatches=2, out=out,
                out_stride=3 * w * h)
    def rc(**kw):
        a = dict(good)
        a.update(kw)
        return _batch_rc(**a), L.sl2_last_error().decode()
    for kw in (dict(frames=None), dict(items=None), dict(counts=None), dict(out=None), dict(n=0), dict(w=0), dict(h=32769), dict(item_stride=-1),
               dict(seq_stride=w * h - 1), dict(out_stride=3 * w * h - 1), dict(pstride=120), dict(patches=None), dict(npatches=-1)):
        code, msg = rc(**kw)
        assert code == _lib.SL2_ERR_INVALID and "sl2_draw_items_batch" in msg, kw
    assert "seq_stride" in rc(seq_stride=1)[1] and "out_stride" in rc(out_stride=1)[1]
    c2 = counts.copy(); c2[1] = 5
    code, msg = rc(counts=c2)
    assert code == _lib.SL2_ERR_INVALID and "image 1" in msg and "item_stride" in msg
    c2[1] = -1
    assert rc(counts=c2)[0] == _lib.SL2_ERR_INVALID
    i2 = items.copy(); i2[2, 1]["kind"] = 9
    code, msg = rc(items=i2)
    assert code == _lib.SL2_ERR_INVALID and "image 2" in msg and "kind" in msg
    i2 = items.copy(); i2[0, 1]["patch"] = 2
    code, msg = rc(items=i2)
    assert code == _lib.SL2_ERR_INVALID and "image 0" in msg and "patch" in msg
    assert (out == 7).all()                          # nothing was drawn by any refused call
    i2 = items.copy(); i2[1, 3]["kind"] = 9          # behind the count: not part of the list
    assert rc(items=i2)[0] == (_lib.SL2_OK if _lib.device_count() > 0 else _lib.SL2_ERR_NO_DEVICE)


def test_engine_calls_refuse_a_null_engine():
    L = _lib.load()
    buf = np.zeros(64 * 40, np.uint8)
    cnt = np.zeros(1, np.int32)
    for on_device in (0, 1):
        assert L.sl2_overlay_items(None, 0, 1, 7, None, buf.ctypes.data_as(_lib.vp), 40, cnt.ctypes.data_as(_lib.vp), on_device) == _lib.SL2_ERR_INVALID
        assert L.sl2_draw_overlays(None, 0, 1, buf.ctypes.data_as(_lib.vp), 16, 0, 7, None, buf.ctypes.data_as(_lib.vp), 48, on_device) == _lib.SL2_ERR_INVALID
    assert not buf.any() and cnt[0] == 0


def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, text), "%s is not declared" % name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name) and hasattr(_lib.load_testing(), name)
        assert getattr(L, name).argtypes, "%s has no ctypes signature" % name
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        for name in NEW:
            assert re.search(r"\b%s$" % name, out, flags=re.M), (path, name)
    assert "#define SL2_API_VERSION 5" in _header()          # additions within version 5 ...
    history = _header()[:_header().find("#define SL2_API_VERSION")]
    assert all(name in history for name in NEW)              # ... noted in the version history


def test_signatures_are_the_issue_s():
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S))
    for sig in ("size_t sl2_overlay_item_bound(int max_features, int partial_slots);",
                "int sl2_overlay_items(sl2_engine* e, int seq0, int nseq, int layers, const int32_t* marked , sl2_overlay_item* items, "
                "int item_stride, int32_t* counts, int on_device);",
                "int sl2_draw_items_batch(int device, void* stream, const uint8_t* frames, int frames_on_device, int nimages, int width, "
                "int height, size_t seq_stride, const sl2_overlay_item* items, int item_stride, const int32_t* counts, int items_on_device, "
                "const uint8_t* patches, size_t patch_stride, int npatches, uint8_t* out, size_t out_stride, int out_on_device);",
                "int sl2_draw_overlays(sl2_engine* e, int seq0, int nseq, const uint8_t* frames, size_t seq_stride, int frames_on_device, "
                "int layers, const int32_t* marked, uint8_t* out, size_t out_stride, int out_on_device);",
                "int sl2_draw_items_host(const uint8_t* frame, int width, int height, const sl2_overlay_item* items, int count, "
                "const uint8_t* patches, size_t patch_stride, int npatches, uint8_t* out);"):
        assert sig in flat, sig


def test_kernels_python_layer_and_build():
    src = open(os.path.join(ROOT, "scenelib2_amd", "csrc", "sl2_overlay.hip")).read()
    for m in re.finditer(r"__global__[^{;]*?\b(k_\w+)\s*\(([^{;]*?)\)\s*\{", src, flags=re.S):
        assert "CameraParams" not in m.group(2), m.group(1)
    assert "k_overlay_list(const SeqArrays S" in src and "load_cam(" in src and "measurement_model(" in src
    assert "k_overlay_draw" in src and "overlay_hit(" in src and "overlay_prepare(" in src
    dev = open(os.path.join(ROOT, "scenelib2_amd", "csrc", "sl2_overlay_dev.hpp")).read()
    assert "overlay_draw_host_body" in dev and "overlay_draw_host_body(" in src          # one source for both forms
    mk = open(os.path.join(ROOT, "scenelib2_amd", "csrc", "Makefile")).read()
    assert mk.count("sl2_overlay.hip") == 1 and "sl2_overlay_dev.hpp" in mk
    assert not re.search(r"^sl2_overlay\.o:", mk, flags=re.M)          # the default flags: -ffp-contract=off
    from scenelib2_amd import Engine
    for name in ("overlay_items", "draw_overlays", "draw_overlays_device", "overlay_item_bound"):
        assert callable(getattr(Engine, name))
    p = inspect.signature(Engine.overlay_items).parameters
    assert list(p) == ["self", "seq0", "nseq", "layers", "marked"] and p["layers"].default == 7 and p["marked"].default is None
    assert callable(overlay.draw_items) and callable(overlay.draw_items_host)


def test_adapters_example_and_documents_know_the_feature():
    from scenelib2_amd import MonoSLAM
    assert list(inspect.signature(MonoSLAM.DrawRawAR).parameters) == ["self", "frame", "out_rgb", "chk_display_2d_descriptors",
                                                                      "chk_display_2d_search_regions", "chk_display_initialisation"]
    hpp = open(os.path.join(ROOT, "include", "scenelib2_amd_monoslam.hpp")).read()
    body = hpp[hpp.find("void DrawRawAR("):]
    body = body[:body.find("\n  }")]
    assert "sl2_draw_overlays" in body and "marked_feature_label_" in body and "chk_display_2d_search_regions" in body
    ref = open(os.path.join(ROOT, "examples", "ref_binding", "monoslam_amd.h")).read()
    assert "void DrawRawAR(cv::Mat frame, cv::Mat& out_rgb, const bool& chk_display_2d_descriptors" in ref and "impl_.DrawRawAR(" in ref
    mk = open(os.path.join(ROOT, "examples", "Makefile")).read()
    assert re.search(r"^all:.*\boverlay_monoslam\b", mk, flags=re.M) and "overlay_monoslam.cpp" in mk
    ex = open(os.path.join(ROOT, "examples", "overlay_monoslam.cpp")).read()
    for call in ("sl2_draw_overlays", "sl2_overlay_items", "sl2_overlay_item_bound", "sl2_go_one_step"):
        assert call in ex, call
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^#+ *8h\b", design, flags=re.M)
    sec = design[re.search(r"^#+ *8h\b", design, flags=re.M).start():]
    for word in ("k_overlay_list", "k_overlay_draw", "overlay_bench.json", "overlay_ab.json", "DrawRectifiedAR", "anti-aliasing", "scratch"):
        assert word in sec, word
    assert "OpenGL drawing and the 3-D view" in design
    assert "sl2_draw_overlays" in open(os.path.join(ROOT, "README.md")).read()
    assert "sl2_draw_overlays" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("overlay_bench.json", "overlay_ab.json"):
        assert os.path.exists(os.path.join(ROOT, "profiles", name)), name


def test_cxx_adapter_draw_raw_ar_compiles_with_the_reference_s_argument_order(tmp_path):
    """include/scenelib2_amd_monoslam.hpp: DrawRawAR(frame, out_rgb, descriptors, search regions, initialisation) type-checks, and
    its body maps each check box to its own layer bit.  (What it draws is the engine call's: tests/test_gpu_overlay.py.)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(str(tmp_path), "use_adapter.cpp")
    with open(src, "w") as f:
        f.write("#include <scenelib2_amd_monoslam.hpp>\n"
                "void use(SceneLib2Amd::MonoSLAM& m, const SceneLib2Amd::Frame& fr, uint8_t* rgb) {\n"
                "  void (SceneLib2Amd::MonoSLAM::*p)(const SceneLib2Amd::Frame&, uint8_t*, bool, bool, bool) = &SceneLib2Amd::MonoSLAM::DrawRawAR;\n"
                "  (m.*p)(fr, rgb, true, false, true);\n}\n")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src])
    hpp = open(os.path.join(ROOT, "include", "scenelib2_amd_monoslam.hpp")).read()
    body = hpp[hpp.find("void DrawRawAR("):]
    body = re.sub(r"\s+", " ", body[:body.find("\n  }")])
    assert "bool chk_display_2d_descriptors, bool chk_display_2d_search_regions, bool chk_display_initialisation" in body
    for box, bit in (("chk_display_2d_search_regions", "SL2_OVERLAY_SEARCH_REGIONS"), ("chk_display_2d_descriptors", "SL2_OVERLAY_DESCRIPTORS"),
                     ("chk_display_initialisation", "SL2_OVERLAY_INITIALISATION")):
        assert "(%s ? %s : 0)" % (box, bit) in body, box


def test_host_body_matches_and_stays_inside_exactly_sized_blocks_under_asan(tmp_path):
    """tests/overlay_host.cpp: a program of its own (nothing loaded into Python), built with the address and undefined-behaviour
    sanitizers, over the same cases with exactly sized heap blocks; it compares with what the restated rules expect."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = os.path.join(str(tmp_path), "overlay_host")
    casefile = os.path.join(str(tmp_path), "cases.bin")
    with open(casefile, "wb") as f:
        f.write(struct.pack("<i", len(oc.CASES)))
        for name, (w, h), items, patches in oc.CASES:
            frame = oc.frame_of(w, h, seed=len(name))
            n, stride = (0, 0) if patches is None else patches.shape
            f.write(struct.pack("<5i", w, h, len(items), n, stride))
            f.write(frame.tobytes())
            f.write(oc.items_array(items).tobytes())
            if n:
                f.write(patches.tobytes()[:(n - 1) * stride + 121])
            f.write(oc.reference(frame, items, patches).tobytes())
    src = os.path.join(ROOT, "tests", "overlay_host.cpp")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src])
    res = subprocess.run([exe, casefile], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.startswith("ok %d cases" % len(oc.CASES))
