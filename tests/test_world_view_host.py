"""The world view and picking, the part that needs no GPU (include/scenelib2_amd.h, "the world view and picking").

The arithmetic of the list (world_view_cases.py, a NumPy restatement of the header's text) against a stand-alone program over
scenelib2_amd/csrc/sl2_world_view_dev.hpp, bit for bit and under sanitizers; sl2_view_look_at against plain linear algebra; the
view-frame covariance against the 3-sigma ellipsoid sampled in the world; the pick rule against a coverage found by drawing
each item alone; the test scenes as the CPU oracle runs them, through the fixed test views, with no rounded coordinate near a
half-integer; the header, the symbols, the Python names, the adapters and the documents."""
import inspect
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import overlay_cases as oc
import rectified_cases as rc
import world_view_cases as wc
from conftest import ROOT
from scenelib2_amd import _lib, overlay, world_view

NEW = ["sl2_view_look_at", "sl2_world_item_bound", "sl2_world_items", "sl2_draw_world", "sl2_pick_items_batch", "sl2_pick_items_host"]
VIEWS = wc.fixed_views()


def _header():
    return open(os.path.join(ROOT, "include", "scenelib2_amd.h")).read()


# ------------------------------------------------------------------------------------------------- header, symbols, Python
def test_symbols_signatures_struct_and_python_names():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    flat = re.sub(r"\s+", " ", text)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, text), "%s is not declared" % name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name) and hasattr(_lib.load_testing(), name)
        assert getattr(L, name).argtypes, "%s has no ctypes signature" % name
    for sig in ("int sl2_view_look_at(const double eye[3], const double target[3], const double up[3], double fku, double fkv, double u0, double v0, "
                "sl2_view* out);",
                "size_t sl2_world_item_bound(int max_features, int partial_slots);",
                "int sl2_world_items(sl2_engine* e, int seq0, int nseq, const sl2_view* views, int nviews, int layers, const int32_t* marked, "
                "sl2_overlay_item* items, int item_stride, int32_t* counts, double* extents , int on_device);",
                "int sl2_draw_world(sl2_engine* e, int seq0, int nseq, const sl2_view* views, int nviews, int width, int height, int background, "
                "int layers, const int32_t* marked, uint8_t* out, size_t out_stride, int out_on_device);",
                "int sl2_pick_items_batch(int device, void* stream, int nimages, int width, int height, const sl2_overlay_item* items, int item_stride, "
                "const int32_t* counts, int npatches, const int32_t* clicks , int32_t* picked , int on_device);",
                "int sl2_pick_items_host(int width, int height, const sl2_overlay_item* items, int count, int npatches, int x, int y, int32_t picked[2]);",
                "typedef struct sl2_view { double r[3]; double q[4]; double fku, fkv, u0, v0; } sl2_view;"):
        assert sig in flat, sig
    assert "#define SL2_API_VERSION 5" in _header()          # additions within version 5 ...
    history = _header()[:_header().find("#define SL2_API_VERSION")]
    assert all(name in history for name in NEW + ["sl2_view", "SL2_WORLD_"])          # ... noted in the version history
    import ctypes as C
    assert C.sizeof(_lib.sl2_view) == 88 == _lib.VIEW_DTYPE.itemsize == wc.VIEW.itemsize
    assert ("SL2_WORLD_TRAJECTORY = 1, SL2_WORLD_FEATURES = 2, SL2_WORLD_UNCERTAINTIES = 4, SL2_WORLD_CAMERA = 8, SL2_WORLD_AXES = 16, "
            "SL2_WORLD_ALL = 31") in flat
    assert (_lib.SL2_WORLD_TRAJECTORY, _lib.SL2_WORLD_FEATURES, _lib.SL2_WORLD_UNCERTAINTIES, _lib.SL2_WORLD_CAMERA, _lib.SL2_WORLD_AXES,
            _lib.SL2_WORLD_ALL) == (1, 2, 4, 8, 16, 31) == (wc.TRAJECTORY, wc.FEATURES, wc.UNCERTAINTIES, wc.CAMERA, wc.AXES, wc.ALL)
    assert "SL2_ITEM_RING = 1, SL2_ITEM_PATCH = 2, SL2_ITEM_RECT = 3, SL2_ITEM_SEGMENT = 5" in text          # no new item kind
    from scenelib2_amd import Engine
    import scenelib2_amd
    for name in ("world_items", "draw_world", "draw_world_device", "world_item_bound"):
        assert callable(getattr(Engine, name))
    p = inspect.signature(Engine.world_items).parameters
    assert list(p) == ["self", "views", "seq0", "nseq", "layers", "marked"] and p["layers"].default == 31 and p["marked"].default is None
    assert list(inspect.signature(Engine.draw_world).parameters)[:4] == ["self", "views", "width", "height"]
    for name in ("look_at", "view", "pick_items", "pick_items_host"):
        assert callable(getattr(world_view, name))
    assert scenelib2_amd.world_view is world_view and scenelib2_amd.look_at is world_view.look_at


def test_bound_and_null_engine_refusals():
    L = _lib.load()
    for N, k in ((16, 1), (100, 4), (676, 4), (0, 0)):
        assert L.sl2_world_item_bound(N, k) == 3 * N + k + 999 + 19 == wc.world_item_bound(N, k) == world_view.item_bound(N, k)
        assert L.sl2_world_item_bound(N, k) == L.sl2_scene_item_bound(N, k) + 19
    assert L.sl2_world_item_bound(-1, 1) == 0 and L.sl2_world_item_bound(4, -1) == 0 and L.sl2_world_item_bound(-3, -3) == 0
    buf = np.zeros(64 * 40, np.uint8)
    cnt = np.zeros(1, np.int32)
    ext = np.zeros(6)
    v = np.ascontiguousarray(VIEWS["reference"]).reshape(1)
    vp = _lib.vp
    for on_device in (0, 1):
        assert L.sl2_world_items(None, 0, 1, v.ctypes.data_as(vp), 1, 31, None, buf.ctypes.data_as(vp), 2000, cnt.ctypes.data_as(vp), ext.ctypes.data_as(vp),
                                 on_device) == _lib.SL2_ERR_INVALID
        assert "sl2_world_items" in L.sl2_last_error().decode() and "null engine" in L.sl2_last_error().decode()
        assert L.sl2_draw_world(None, 0, 1, v.ctypes.data_as(vp), 1, 4, 4, 0, 31, None, buf.ctypes.data_as(vp), 48, on_device) == _lib.SL2_ERR_INVALID
        assert "sl2_draw_world" in L.sl2_last_error().decode()
    assert not buf.any() and cnt[0] == 0 and not ext.any()


def test_pick_host_refusals():
    L = _lib.load()
    vp = _lib.vp
    items = oc.items_array([wc._lab(oc.rect(1, 1, 5, 5), 3)])
    out = np.full(2, 9, np.int32)
    ip, op = items.ctypes.data_as(vp), out.ctypes.data_as(vp)
    for args in ((0, 10, ip, 1, 0, 1, 1, op), (10, 32769, ip, 1, 0, 1, 1, op), (10, 10, ip, -1, 0, 1, 1, op), (10, 10, None, 1, 0, 1, 1, op),
                 (10, 10, ip, 1, -1, 1, 1, op), (10, 10, ip, 1, 0, 1, 1, None)):
        assert L.sl2_pick_items_host(*args) == _lib.SL2_ERR_INVALID and "sl2_pick_items_host" in L.sl2_last_error().decode()
    assert (out == 9).all()
    assert L.sl2_pick_items_host(10, 10, None, 0, 0, 1, 1, op) == _lib.SL2_OK and out.tolist() == [-1, -1]          # an empty list needs no pointer
    assert L.sl2_pick_items_host(10, 10, ip, 1, 0, 1, 1, op) == _lib.SL2_OK and out.tolist() == [3, 0]
    cnt, clk = np.ones(1, np.int32), np.ones(2, np.int32)
    cp, kp = cnt.ctypes.data_as(vp), clk.ctypes.data_as(vp)
    out[:] = 9
    # the checks of sl2_pick_items_batch come before any device is looked for
    for args, word in (((0, None, 0, 10, 10, ip, 1, cp, 0, kp, op, 0), "no images"), ((0, None, 1, 10, 10, None, 1, cp, 0, kp, op, 0), "null"),
                       ((0, None, 1, 10, 10, ip, 1, None, 0, kp, op, 0), "null"), ((0, None, 1, 10, 10, ip, 1, cp, 0, None, op, 0), "null"),
                       ((0, None, 1, 10, 10, ip, 1, cp, 0, kp, None, 0), "null"), ((0, None, 1, 10, 10, ip, -1, cp, 0, kp, op, 0), "item_stride"),
                       ((0, None, 1, 10, 10, ip, 1, cp, -1, kp, op, 0), "npatches"), ((0, None, 1, 0, 10, ip, 1, cp, 0, kp, op, 0), "width"),
                       ((0, None, 1, 10, 40000, ip, 1, cp, 0, kp, op, 0), "height"), ((0, None, 1, 10, 10, vp(items.ctypes.data + 4), 1, cp, 0, kp, op, 1), "aligned"),
                       ((0, None, 1, 10, 10, ip, 0, cp, 0, kp, op, 0), "image 0: count")):
        assert L.sl2_pick_items_batch(*args) == _lib.SL2_ERR_INVALID, word
        msg = L.sl2_last_error().decode()
        assert "sl2_pick_items_batch" in msg and word in msg, (word, msg)
    bad = items.copy()
    bad["kind"] = 4
    assert L.sl2_pick_items_batch(0, None, 1, 10, 10, bad.ctypes.data_as(vp), 1, cp, 0, kp, op, 0) == _lib.SL2_ERR_INVALID
    assert "image 0: unknown item kind" in L.sl2_last_error().decode()
    assert (out == 9).all()


# ------------------------------------------------------------------------------------------------- sl2_view_look_at
def _project(view, Y):
    """A world point through the view, by the header's two sentences, in NumPy."""
    q = np.array(view["q"], np.float64)
    R = np.array(rc._quat_to_rot(rc._quat_inverse([float(v) for v in q]))).reshape(3, 3)
    X = R @ (np.asarray(Y, np.float64) - np.array(view["r"]))
    return np.array([view["u0"] - view["fku"] * X[0] / X[2], view["v0"] - view["fkv"] * X[1] / X[2]]), X


def test_look_at_places_target_up_and_right():
    """Coordinates within 10 m and focal lengths up to 1000: FP64 rounding there is about 1e-12 pixel, so the bound of 1e-9 is
    three decades of slack and not a measurement."""
    rng = np.random.default_rng(41)
    anchor = world_view.look_at(wc.REFERENCE_EYE, wc.REFERENCE_TARGET, wc.REFERENCE_UP, 195.0, 195.0, 162.0, 125.0)
    assert np.array_equal(anchor["r"], wc.REFERENCE_EYE) and anchor["q"][0] > 0.99 and anchor["q"][2] == 0.0 and anchor["q"][3] == 0.0
    # (the test helper takes a small component from the square root of a cancelling sum: 1e-16 / 0.018 of relative error there)
    assert np.abs(np.array(anchor["q"]) - np.array(VIEWS["reference"]["q"])).max() < 1e-13
    worst = 0.0
    for k in range(300):
        eye, target = rng.uniform(-10, 10, 3), rng.uniform(-10, 10, 3)
        up = rng.normal(size=3) if k % 3 else np.array([0.0, 1.0, 0.0])
        z = (target - eye) / np.linalg.norm(target - eye)
        if np.linalg.norm(np.cross(up, z)) < 0.05 * np.linalg.norm(up):
            continue
        fku, fkv, u0, v0 = rng.uniform(50, 1000), rng.uniform(50, 1000), rng.uniform(0, 640), rng.uniform(0, 480)
        v = world_view.look_at(eye, target, up, fku, fkv, u0, v0)
        assert abs(np.linalg.norm(v["q"]) - 1.0) <= 1e-15 and v["q"][0] >= 0.0 and not np.signbit(v["q"][0])
        assert np.array_equal(v["r"], eye) and (v["fku"], v["fkv"], v["u0"], v["v0"]) == (fku, fkv, u0, v0)
        p, X = _project(v, target)
        worst = max(worst, np.abs(p - (u0, v0)).max())
        assert X[2] > 0
        for t in (0.1, 0.5, 3.0):          # the optical axis stays at the principal point
            worst = max(worst, np.abs(_project(v, eye + t * (target - eye))[0] - (u0, v0)).max())
        upn = up - (up @ z) * z          # `up` as the view sees it
        upn /= np.linalg.norm(upn)
        right = np.cross(z, upn)          # x = up x z is image LEFT: the viewer's right is its opposite
        d = 0.1 * np.linalg.norm(target - eye)
        pu, pr = _project(v, target + d * upn)[0], _project(v, target + d * right)[0]
        assert pu[1] < v0 - 1.0 and pr[0] > u0 + 1.0
        worst = max(worst, abs(pu[0] - u0), abs(pr[1] - v0))          # and neither leaves its axis
        lib_up = _project(v, target + d * up / np.linalg.norm(up))[0]
        assert lib_up[1] < v0          # a point displaced along `up` itself lands at a smaller v
    assert worst <= 1e-9, worst
    print("look_at: worst deviation %.3e pixel" % worst)


def test_look_at_refusals():
    L = _lib.load()
    out = np.zeros(1, _lib.VIEW_DTYPE)
    def call(eye=(0.0, 0.0, 0.0), target=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), fku=100.0, null=None):
        a = [np.array(v, np.float64) for v in (eye, target, up)]
        ptrs = [None if null == k else _lib.dp(a[k]) for k in range(3)]
        return L.sl2_view_look_at(ptrs[0], ptrs[1], ptrs[2], fku, 100.0, 10.0, 10.0, None if null == 3 else out.ctypes.data_as(_lib.vp))
    for kw in (dict(eye=(np.nan, 0, 0)), dict(target=(0, np.inf, 0)), dict(up=(0, 1, np.nan)), dict(fku=np.inf), dict(target=(0, 0, 0)), dict(up=(0, 0, 0)),
               dict(up=(0, 0, 2.5)), dict(up=(0, 0, -1)), dict(up=(0, 1e-14, 1)), dict(null=0), dict(null=1), dict(null=2), dict(null=3)):
        assert call(**kw) == _lib.SL2_ERR_INVALID and "sl2_view_look_at" in L.sl2_last_error().decode(), kw
    assert not out.view(np.uint8).any()
    assert call() == _lib.SL2_OK and out[0]["q"].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert call(up=(0, 1e-6, 1)) == _lib.SL2_OK          # nearly parallel is still a direction


# ------------------------------------------------------------------------------------------------- the arithmetic
def test_glyph_edges_are_the_header_s():
    """12 box edges, each along one axis between two corners of the box, every edge once; 4 lens edges in a ring."""
    box = [wc.glyph_edge(e) for e in range(12)]
    seen = set()
    for e, (a, b) in enumerate(box):
        diff = [k for k in range(3) if a[k] != b[k]]
        assert diff == [e // 4] and a[e // 4] == wc.BOX_LO[e // 4] and b[e // 4] == wc.BOX_HI[e // 4]
        assert all(a[k] in (wc.BOX_LO[k], wc.BOX_HI[k]) for k in range(3))
        seen.add((tuple(a), tuple(b)))
    assert len(seen) == 12
    lens = [wc.glyph_edge(e) for e in range(12, 16)]
    assert all(lens[k][1] == lens[(k + 1) % 4][0] for k in range(4)) and all(a[2] == b[2] == -0.017 for a, b in lens)
    assert sorted({tuple(a[:2]) for a, _ in lens}) == [(-0.012, -0.012), (-0.012, 0.012), (0.012, -0.012), (0.012, 0.012)]
    # qWO = qWR * (0, 0, 1, 0): Hamilton's product, written out
    q = np.array([0.3, -0.5, 0.7, 0.2])
    w1, x1, y1, z1 = q
    w2, x2, y2, z2 = 0.0, 0.0, 1.0, 0.0
    prod = [w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
            w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2]
    assert prod == [-q[2], -q[3], q[0], q[1]]
    # the lens looks along the camera's +z: the glyph's -z (where the lens sits) is the camera's viewing direction
    xv = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    assert wc.glyph_world(xv, [0.0, 0.0, -0.017]) == [0.0, 0.0, 0.017]


def test_view_frame_covariance_bounds_the_sampled_ellipsoid():
    """Anchored independently of any implementation: the 3-sigma ellipsoid (Y - y)^T Pyy^-1 (Y - y) = 9 is sampled IN THE WORLD,
    20 000 points, and every point goes through the view by itself.  With the unrounded centre every sample satisfies the
    ring's form at <= rhs (1 + 1e-9) - inside or on the outline - and the largest reaches >= 0.999 rhs: the extreme samples lie
    on it (the bounds of the rectified view's conic test)."""
    rng = np.random.default_rng(77)
    u = rng.normal(size=(20000, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    done = straddle = behind = 0
    k = 0
    while done < 120:
        k += 1
        view = wc.look_at(rng.uniform(-2, 2, 3), rng.uniform(-2, 2, 3), (0.0, 1.0, 0.2), dict(fku=rng.uniform(100, 400), fkv=rng.uniform(100, 400), u0=160.0, v0=120.0))
        q = np.array(view["q"])
        R = np.array(rc._quat_to_rot(rc._quat_inverse([float(v) for v in q]))).reshape(3, 3)
        m_want = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), rng.uniform(-0.5, 3.0)])
        y = np.array(view["r"]) + R.T @ m_want
        G = rng.normal(size=(3, 3)) * rng.uniform(0.005, 0.08)
        Pyy = G @ G.T + 1e-8 * np.eye(3)
        m, _, Jy = rc.zeroed_jac(wc._pose(view), y)
        Sg = wc.world_sigma(Jy, Pyy)
        assert np.allclose(Sg, R @ Pyy @ R.T, rtol=1e-12, atol=1e-18) and np.allclose(m, m_want, atol=1e-12)
        Y = y + 3.0 * u @ np.linalg.cholesky(Pyy).T
        X = (Y - np.array(view["r"])) @ R.T
        got = rc.conic(wc._cam(view), m, Sg)
        if got is None:
            # no ring: the ellipsoid reaches the view plane, or lies wholly behind it
            assert X[:, 2].min() <= 1e-9 * np.abs(X[:, 2]).max() + 1e-4 or m[2] <= 0
            straddle += X[:, 2].min() < 0 < X[:, 2].max()
            behind += X[:, 2].max() < 0
            continue
        assert (X[:, 2] > 0).all()
        (cx, cy), (A, B, C, rhs) = got
        du = view["u0"] - view["fku"] * X[:, 0] / X[:, 2] - cx
        dv = view["v0"] - view["fkv"] * X[:, 1] / X[:, 2] - cy
        form = A * du * du + B * du * dv + C * dv * dv
        assert form.max() <= rhs * (1 + 1e-9) and form.max() >= 0.999 * rhs, form.max() / rhs
        done += 1
    assert straddle >= 5 and behind >= 5, (straddle, behind, k)


def test_host_forms_match_and_stay_inside_exactly_sized_blocks_under_asan(tmp_path):
    """tests/world_view_host.cpp: a program of its own (nothing loaded into Python), built with the address and
    undefined-behaviour sanitizers; it compares sl2_world_view_dev.hpp with what the restatement expects, bit for bit, and the
    pick rule with the coverage found by drawing."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = os.path.join(str(tmp_path), "world_view_host")
    casefile = os.path.join(str(tmp_path), "cases.bin")
    cases = wc.math_cases()
    rings = edges = straddle = behind = clicks = 0
    draw = lambda f, it, p: overlay.draw_items_host(f, it, p)
    with open(casefile, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for view, xv, y, Pyy in cases:
            f.write(np.ascontiguousarray(view).tobytes())
            for a in (xv, y, Pyy):
                f.write(np.ascontiguousarray(a, np.float64).tobytes())
            m, _, Jy = rc.zeroed_jac(wc._pose(view), y)
            S = wc.world_sigma(Jy, Pyy)
            f.write(struct.pack("<12d", *(list(m) + [v for row in S for v in row])))
            items = wc.feature_items(view, y, Pyy, wc.FEATURES | wc.UNCERTAINTIES, oc.RED, 1)
            marker = [it for it in items if int(it["kind"]) == rc.RECT]
            ring = [it for it in items if int(it["kind"]) == rc.RING]
            f.write(struct.pack("<6i", *([1, int(marker[1]["a"][0]), int(marker[1]["a"][1])] if marker else [0, 0, 0]) +
                                        ([1, int(ring[0]["a"][0]), int(ring[0]["a"][1])] if ring else [0, 0, 0])))
            f.write(struct.pack("<4d", *(ring[0]["q"].tolist() if ring else [0.0] * 4)))
            rings += len(ring)
            sd = 3.0 * np.sqrt(S[2][2])
            straddle += (not ring) and m[2] - sd < 0 < m[2] + sd
            behind += (not ring) and m[2] + sd < 0
            glyph = dict(wc.glyph_segments(view, xv))
            edges += len(glyph)
            for e in range(16):
                f.write(struct.pack("<5i", *([1] + glyph[e] if e in glyph else [0] * 5)))
            ext = [0.0] * 6
            wc.extend(ext, xv)
            wc.extend(ext, y)
            f.write(struct.pack("<6d", *ext))
            axes = dict(wc.axes_segments(view, ext))
            for k in range(3):
                f.write(struct.pack("<5i", *([1] + axes[k] if k in axes else [0] * 5)))
        f.write(struct.pack("<i", len(wc.PICK_CASES)))
        patches = np.arange(5 * 121, dtype=np.uint8).reshape(5, 121)
        for c in wc.PICK_CASES:
            w, h = c["size"]
            f.write(struct.pack("<5i", w, h, len(c["items"]), c["npatches"], len(c["clicks"])))
            f.write(c["items"].tobytes())
            f.write(np.array(c["clicks"], np.int64).astype(np.int32).tobytes())
            want = [wc.pick(draw, c["items"], w, h, x, y, patches[:c["npatches"]] if c["npatches"] else None) for x, y in c["clicks"]]
            f.write(np.array(want, np.int32).tobytes())
            clicks += len(want)
    assert len(cases) >= 36 and rings >= 10 and straddle >= 5 and behind >= 5 and 100 < edges < 16 * len(cases), (rings, straddle, behind, edges)
    src = os.path.join(ROOT, "tests", "world_view_host.cpp")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src])
    res = subprocess.run([exe, casefile], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip() == "ok %d math cases %d rings %d glyph edges %d pick cases %d clicks" % (len(cases), rings, edges, len(wc.PICK_CASES), clicks)


# ------------------------------------------------------------------------------------------------- picking
@pytest.mark.parametrize("case", wc.PICK_CASES, ids=[c["name"] for c in wc.PICK_CASES])
def test_pick_host_form_equals_the_rule_over_drawn_coverage(case):
    """An item covers a pixel iff sl2_draw_items_host of that item alone gives the same colour there over an all-0 and an
    all-255 frame; the pick is the last labelled item with a covered pixel in the clipped 7 x 7 window."""
    w, h = case["size"]
    patches = np.arange(5 * 121, dtype=np.uint8).reshape(5, 121)[:case["npatches"]] if case["npatches"] else None
    draw = lambda f, it, p: overlay.draw_items_host(f, it, p)
    for x, y in case["clicks"]:
        want = wc.pick(draw, case["items"], w, h, x, y, patches)
        if not -2 ** 31 <= x < 2 ** 31:
            continue
        assert world_view.pick_items_host(w, h, case["items"], x, y, case["npatches"]) == want, (case["name"], x, y)


def test_pick_rule_does_what_its_words_say():
    by = {c["name"]: c for c in wc.PICK_CASES}
    assert [len(by["count_%d" % n]["items"]) for n in (0, 1, 63, 64, 65, 130)] == [0, 1, 63, 64, 65, 130]
    pick = lambda name, x, y: world_view.pick_items_host(*by[name]["size"], by[name]["items"], x, y, by[name]["npatches"])
    # the later of two labelled items wins where both are in the window; each alone where only it is
    assert pick("later_of_two_wins", 20, 10) == (9, 1) and pick("later_of_two_wins_reversed", 20, 10) == (4, 1)
    assert pick("later_of_two_wins", 10, 17) == (4, 0) and pick("later_of_two_wins", 40, 12) == (9, 1)
    assert pick("later_of_two_wins", 33, 25) == (4, 0) and pick("later_of_two_wins", 34, 25) == (-1, -1)          # 3 pixels off the rim, then 4
    # an unlabelled item on top neither counts nor hides
    assert pick("unlabelled_on_top_does_not_hide", 10, 10) == (4, 0) and pick("unlabelled_on_top_does_not_hide", 36, 10) == (-1, -1)
    # a ring is its rim: the interior more than 3 pixels from it picks nothing
    assert pick("inside_a_large_ring", 35, 18) == (-1, -1) and pick("inside_a_large_ring", 35, 8) == (7, 0) and pick("inside_a_large_ring", 45, 18) == (7, 0)
    assert pick("inside_a_large_ring", 53, 18) == (-1, -1)
    # a segment's tie pixels are the header's: at x = 5 the line 4,4 .. 12,8 passes midway and takes the larger y
    # (the window of (8, 1) is x 5 .. 11, y 0 .. 4: it holds (5, 4), not (5, 5); that of (8, 11) starts at y 8 and ends at x 11: it holds (11, 8))
    assert pick("segment_ties", 1, 1) == (2, 0) and pick("segment_ties", 8, 1) == (-1, -1) and pick("segment_ties", 8, 2) == (2, 0)
    assert pick("segment_ties", 8, 11) == (2, 0) and pick("segment_ties", 8, 12) == (-1, -1)
    assert [pick("segment_ties", x, y) for x, y in by["segment_ties"]["clicks"]] == [pick("segment_ties_reversed", x, y) for x, y in by["segment_ties"]["clicks"]]
    # windows partly off the image are clipped; a click off the image answers nothing and is not refused
    assert pick("window_partly_off", 0, 0) == (1, 0) and pick("window_partly_off", 5, 5) == (1, 0) and pick("window_partly_off", 6, 6) == (-1, -1)
    assert pick("window_partly_off", 0, 17) == (-1, -1) and pick("window_partly_off", 69, 3) == (-1, -1)          # items wholly off the image
    assert all(pick("click_off_the_image", x, y) == (-1, -1) for x, y in by["click_off_the_image"]["clicks"])
    # what draws nothing is never picked
    assert all(pick("items_that_draw_nothing", x, y) == (-1, -1) for x, y in by["items_that_draw_nothing"]["clicks"])
    assert pick("items_that_draw_nothing_over_one_that_does", 25, 18) == (8, 0)
    assert pick("unknown_kinds", 5, 5) == (12, 0)
    assert pick("patches_and_indices_outside", 40, 15) == (-1, -1) and pick("patches_and_indices_outside", 55, 15) == (-1, -1)
    assert pick("patches_and_indices_outside", 30, 28) == (9, 3) and pick("no_patches_at_all", 20, 15) == (2, 1)
    # a PATCH covers its 13 x 13 square: 6 + 3 pixels from the centre still picks, 10 does not
    assert pick("patch_square_is_covered_whole", 29, 24) == (6, 0) and pick("patch_square_is_covered_whole", 30, 25) == (-1, -1)
    assert pick("patch_square_is_covered_whole", 11, 6) == (6, 0) and pick("patch_square_is_covered_whole", 10, 5) == (-1, -1)


# ------------------------------------------------------------------------------------------------- the test scenes, on the oracle
def _oracle_state(s):
    kinds = s.feature_kinds()
    feats = []
    for k in range(len(kinds)):
        f = s.feature(k)
        feats.append(dict(label=int(kinds[k, 2]), full=bool(kinds[k, 1]), size=int(kinds[k, 0]), selected=f["selected"], success=f["success"]))
    return dict(x=s.total_state(), P=s.total_covariance(), feats=feats, traj=s.trajectory())


def test_builder_on_the_oracle_s_run_of_the_gpu_scenes_skips_no_field(oracle):
    """The scenes of tests/test_gpu_world_view.py, run by the CPU oracle, through the fixed test views: no coordinate that gets
    rounded lies within 1e-6 of a half-integer (the GPU test compares every integer field and asserts the same), every kind of
    item appears, the view inside the map cuts and drops what lies behind it, and the view turned away lists nothing."""
    from mapping_helpers import make_mapping_sequence, oracle_for
    from slam_helpers import Pair
    import display_helpers as rs
    pr = Pair(4, rs.SHIPPED_STEPS + 1, batch=1, make_engine=False)
    for k in range(rs.SHIPPED_STEPS):
        pr.oracles[0].go_one_step(pr.frames[0][k], True)
    state = _oracle_state(pr.oracles[0])
    for name, view in VIEWS.items():
        for layers in (wc.ALL, wc.FEATURES | wc.CAMERA):
            items, rounded, ext = wc.world_list(state, view, layers, marked=1)
            assert rc.skipped_fields(rounded) == 0, (name, layers)
        items, rounded, ext = wc.world_list(state, view, wc.ALL, marked=1)
        kinds, rgbs = items["kind"].tolist(), [tuple(v) for v in items["rgb"].tolist()]
        if name == "away":
            assert items.size == 0
            continue
        if name in ("reference", "side"):
            assert rgbs.count(wc.GREY) == 16 and rgbs.count(wc.WHITE) == 3 and kinds.count(rc.RECT) == 8 and kinds.count(rc.RING) == 4
            assert kinds[:16] == [rc.SEGMENT] * 16 and rgbs[-3:] == [wc.WHITE] * 3
            assert tuple(items[items["label"] == 1][0]["rgb"]) == oc.GREEN
        assert items.size <= wc.world_item_bound(4, 1)
    # the extents: the camera's position and the four features, with 0 taken in
    x = state["x"]
    pts = np.vstack([np.zeros(3), x[0:3]] + [x[13 + 3 * k:16 + 3 * k] for k in range(4)])
    _, _, ext = wc.world_list(state, VIEWS["reference"], wc.ALL)
    assert np.array_equal(ext, np.stack([pts.min(axis=0), pts.max(axis=0)], axis=1).reshape(-1))
    _, _, ext = wc.world_list(state, VIEWS["reference"], wc.ALL & ~wc.FEATURES)
    assert np.array_equal(ext, np.stack([pts[:2].min(axis=0), pts[:2].max(axis=0)], axis=1).reshape(-1))
    # the view inside the map: something lies behind it and something in front
    inside = wc.world_list(state, VIEWS["inside"], wc.ALL)[0]
    full = wc.world_list(state, VIEWS["side"], wc.ALL)[0]
    assert 0 < inside.size < full.size
    cam, params, spec, frames, templates = make_mapping_sequence(seed=rs.MAPPING_SEED, n_known=rs.MAPPING_KNOWN, n_frames=rs.MAPPING_FRAMES)
    mviews = wc.fixed_views(cam)
    for victim in (None, 2):          # (sequence 1 of the GPU test's engine has feature 2 deleted by hand before step 6)
        s = oracle_for(cam, params, spec, templates, oracle)
        seen_ray = 0
        for k in range(1, rs.MAPPING_FRAMES):
            if victim is not None and k == 6:
                assert s.delete_feature(victim)
            s.go_one_step(frames[k], True, True)
            if k < 8:
                continue
            state = _oracle_state(s)
            for name, view in mviews.items():
                items, rounded, ext = wc.world_list(state, view, wc.ALL)
                assert rc.skipped_fields(rounded) == 0, (k, name)
                if name in ("reference", "side"):
                    rays = [it for it in items if int(it["kind"]) == rc.SEGMENT and int(it["label"]) >= 0]
                    assert len(rays) == sum(not f["full"] for f in state["feats"])
                    seen_ray += len(rays)
                assert items.size <= wc.world_item_bound(rs.MAPPING_MAX_FEATURES, 1)
        assert seen_ray > 0


def test_the_large_map_of_the_gpu_test_skips_no_field():
    """The 70-feature engine of the GPU test is never stepped: its state is what this builds (wc.large_map), so the check of the
    half-integers can be made here."""
    state = wc.large_map()
    assert len(state["feats"]) == 70
    for name, view in VIEWS.items():
        items, rounded, ext = wc.world_list(state, view, wc.ALL)
        assert rc.skipped_fields(rounded) == 0, name
    items = wc.world_list(state, VIEWS["side"], wc.ALL)[0]
    assert items["kind"].tolist().count(rc.RING) >= 60


# ------------------------------------------------------------------------------------------------- source, build, adapters, documents
def test_kernel_source_and_build():
    csrc = os.path.join(ROOT, "scenelib2_amd", "csrc")
    src = open(os.path.join(csrc, "sl2_world_view.hip")).read()
    kernels = list(re.finditer(r"__global__[^{;]*?\b(k_\w+)\s*\(([^{;]*?)\)\s*\{", src, flags=re.S))
    assert [m.group(1) for m in kernels] == ["k_world_list", "k_pick_items"]
    args = kernels[0].group(2)
    assert "const SeqArrays S" in args and "CameraParams" not in args and "sl2_view view" not in args and "const sl2_view* __restrict__ views" in args
    for word in ("wave_min", "wave_max", "hipMemsetAsync", "pick_item_hits(", "pick_host_body(", "list_trajectory(", "list_feature(", "draw_call("):
        assert word in src, word
    # the list writer the three list kernels share, and the chain the three drawing calls share
    writer = open(os.path.join(csrc, "sl2_drawlist_dev.hpp")).read()
    for word in ("__ballot", "__shfl_up", "__device__", "void list_trajectory(", "void list_feature("):
        assert word in writer, word
    assert writer.count("at < item_stride") == 1 and "\nSL2_HD " not in writer          # every store goes through the one guarded put(); device code only
    for name in ("sl2_overlay.hip", "sl2_rectify.hip", "sl2_world_view.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert "sl2_drawlist_dev.hpp" in text and "at < item_stride" not in text, name          # no store of its own
    chain = open(os.path.join(csrc, "sl2_display.hpp")).read()
    assert "launch_draw(" in chain and "int draw_call(" in chain and "int items_call(" in chain
    dev = open(os.path.join(csrc, "sl2_world_view_dev.hpp")).read()
    assert "SL2_HD bool pick_item_hits" in dev and "overlay_prepare(" in dev and "overlay_hit(" in dev and "scene_conic(" in dev and "scene_segment(" in dev
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert mk.count("sl2_world_view.hip") == 1 and "sl2_world_view_dev.hpp" in mk
    assert not re.search(r"^sl2_world_view\.o:", mk, flags=re.M)          # the default flags: -ffp-contract=off
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^#+ *8j\b", design, flags=re.M)
    assert m
    sec = design[m.start():]
    for word in ("k_world_list", "k_pick_items", "coverage", "scratch", "registers", "Left out", "world_view_bench.json"):
        assert word in sec, word
    assert "OpenGL drawing and the 3-D view" in design


def test_adapters_example_and_documents_know_the_feature(tmp_path):
    from scenelib2_amd import MonoSLAM
    assert list(inspect.signature(MonoSLAM.Draw3dScene).parameters) == ["self", "view", "out_rgb", "width", "height", "chk_display_trajectory",
                                                                        "chk_display_3d_features", "chk_display_3d_uncertainties"]
    assert list(inspect.signature(MonoSLAM.Picker).parameters) == ["self", "x", "y", "threed"]
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(str(tmp_path), "use_adapter.cpp")
    with open(src, "w") as f:
        f.write("#include <scenelib2_amd_monoslam.hpp>\n"
                "int use(SceneLib2Amd::MonoSLAM& m, const sl2_view& v, uint8_t* rgb) {\n"
                "  void (SceneLib2Amd::MonoSLAM::*p)(const sl2_view&, uint8_t*, int, int, bool, bool, bool) = &SceneLib2Amd::MonoSLAM::Draw3dScene;\n"
                "  (m.*p)(v, rgb, 480, 360, true, false, true);\n"
                "  int (SceneLib2Amd::MonoSLAM::*q)(int, int, bool) = &SceneLib2Amd::MonoSLAM::Picker;\n"
                "  m.mark_feature_by_lab((m.*q)(3, 4, true) - 1);\n"
                "  return m.Picker(3, 4, false);\n}\n")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src])
    hpp = open(os.path.join(ROOT, "include", "scenelib2_amd_monoslam.hpp")).read()
    body = hpp[hpp.find("void Draw3dScene("):]
    body = re.sub(r"\s+", " ", body[:body.find("\n  }")])
    assert "sl2_draw_world" in body and "marked_feature_label_" in body and "SL2_WORLD_CAMERA" in body
    for box, bit in (("chk_display_trajectory", "SL2_WORLD_TRAJECTORY"), ("chk_display_3d_features", "SL2_WORLD_FEATURES | SL2_WORLD_AXES"),
                     ("chk_display_3d_uncertainties", "SL2_WORLD_UNCERTAINTIES")):
        assert "(%s ? %s : 0)" % (box, bit) in body, box
    body = hpp[hpp.find("int Picker("):]
    body = body[:body.find("\n  }")]
    assert "sl2_pick_items_host" in body and "sl2_world_items" in body and "picked[0] + 1" in body
    ref = open(os.path.join(ROOT, "examples", "ref_binding", "monoslam_amd.h")).read()
    assert "void Draw3dScene(const sl2_view& view, cv::Mat& out_rgb, int width, int height, const bool& chk_display_trajectory" in ref
    assert "impl_.Draw3dScene(" in ref and "int Picker(int x, int y, const bool& threed)" in ref
    mk = open(os.path.join(ROOT, "examples", "Makefile")).read()
    assert re.search(r"^all:.*\bworld_view_monoslam\b", mk, flags=re.M) and "world_view_monoslam.cpp" in mk
    ex = open(os.path.join(ROOT, "examples", "world_view_monoslam.cpp")).read()
    for call in ("sl2_draw_world", "sl2_world_items", "sl2_world_item_bound", "sl2_view_look_at", "sl2_pick_items_batch", "sl2_delete_features", "sl2_go_one_step"):
        assert call in ex, call
    assert "sl2_draw_world" in open(os.path.join(ROOT, "README.md")).read()
    assert "sl2_draw_world" in open(os.path.join(ROOT, "INTEGRATION.md")).read() and "sl2_pick_items_batch" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert os.path.exists(os.path.join(ROOT, "scripts", "bench_world_view.py"))
