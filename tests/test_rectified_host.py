"""The rectified view, host side: SL2_ITEM_SEGMENT through sl2_draw_items_host and sl2_rectify_frame_host byte for byte against a
NumPy restatement of the header's pixel rules (rectified_cases.py; it calls nothing of the library), the properties the rules
promise; the scene's arithmetic - Pzeroedyigraphics against central differences, the conic against sampled ellipsoids, the 3-D
segment rule on anchors, the list builder on the oracle's run of the GPU test's scenes; the refusals, the symbols, and the
stand-alone program over the same cases (the scene's arithmetic bit for bit) under the address and undefined-behaviour
sanitizers.  (The kernels: tests/test_gpu_rectified.py.)"""
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
import rectified_cases as rc

from scenelib2_amd import _lib, overlay, rectified

NEW = ["sl2_rectify_frames", "sl2_rectify_frame_host", "sl2_scene_item_bound", "sl2_scene_items", "sl2_draw_rectified"]


def _header():
    return open(os.path.join(ROOT, "include", "scenelib2_amd.h")).read()


def test_case_lists_hold_what_the_contract_names():
    names = [c[0] for c in rc.SEGMENT_CASES] + [c[0] for c in rc.REMAP_CASES]
    assert len(names) == len(set(names))
    assert rc.SIZES == ((70, 37), (64, 16))
    for w, h in rc.SIZES:
        for stem in ["seg_octant_%d" % k for k in range(8)] + ["seg_octant_%d_reversed" % k for k in range(8)] + [
                "seg_horizontal", "seg_vertical", "seg_diagonals", "seg_single_pixel", "seg_half_ties", "seg_across_tile_edges", "seg_one_end_off",
                "seg_both_ends_off", "seg_beyond_far", "seg_over_ring", "seg_under_ring", "seg_other_kinds_draw_nothing", "seg_many"]:
            assert "%s_%dx%d" % (stem, w, h) in names, stem
        for centre in ("inside", "border", "nondyadic"):
            for kd in ("zero", "shipped", "strong", "negative", "corners_lost"):
                assert "remap_%s_%s_%dx%d" % (centre, kd, w, h) in names
    assert max(len(c[2]) for c in rc.SEGMENT_CASES) > 2 * 256          # more than two rounds of the kernel's staging
    assert any(c[2] == (162.3, 125.7) for c in rc.REMAP_CASES) and rc.SHIPPED_KD1 == 9e-06


@pytest.mark.parametrize("case", rc.SEGMENT_CASES, ids=[c[0] for c in rc.SEGMENT_CASES])
def test_segments_host_form_equals_the_restated_rule(case):
    name, (w, h), items, patches = case
    frame = oc.frame_of(w, h, seed=len(name))
    want = rc.reference(frame, items, patches)
    got = overlay.draw_items_host(frame, oc.items_array(items), patches)
    assert np.array_equal(got, want), (name, np.argwhere((got != want).any(axis=2))[:5].tolist())


def test_segment_rule_draws_what_its_words_say():
    """The restated rule itself, on anchors small enough to check by hand."""
    w, h = 70, 37
    pts = lambda a: sorted((int(x), int(y)) for y, x in np.argwhere(rc.segment_mask(a, w, h)))
    assert pts((3, 5, 7, 5)) == [(x, 5) for x in range(3, 8)] == pts((7, 5, 3, 5))
    assert pts((9, 2, 9, 6)) == [(9, y) for y in range(2, 7)] == pts((9, 6, 9, 2))
    assert pts((2, 2, 6, 6)) == [(k, k) for k in range(2, 7)]
    assert pts((6, 2, 2, 6)) == [(8 - k, k) for k in range(2, 7)][::-1]
    assert pts((5, 5, 5, 5)) == [(5, 5)] and pts((w, 3, w, 3)) == [] and pts((-1, -1, -1, -1)) == []
    # (0,0) .. (4,2): y = floor((4 x + 4) / 8) = 0, 1, 1, 2, 2 - the exact halves at x = 1 and x = 3 go to the larger y; the
    # reverse is the same item once its ends are exchanged
    assert pts((0, 0, 4, 2)) == [(0, 0), (1, 1), (2, 1), (3, 2), (4, 2)]
    assert pts((4, 2, 0, 0)) == [(0, 0), (1, 1), (2, 1), (3, 2), (4, 2)]
    assert rc.half_ties((0, 0, 4, 2)) == (True, [1, 3]) and rc.half_ties((0, 0, 2, 1)) == (True, [1])
    # a floored, not truncated, division: (0,2) .. (4,0) has numerators 4, 0, -4, -8, -12 over 8: 0, 0, -1, -1, -2
    assert pts((0, 2, 4, 0)) == [(0, 2), (1, 2), (2, 1), (3, 1), (4, 0)]
    # one pixel per major step, ends included, whatever the octant; both directions agree away from exact halves
    rng = np.random.default_rng(5)
    for _ in range(300):
        a = [int(v) for v in rng.integers(0, 37, 4)]
        m = rc.segment_mask(a, w, h)
        assert m.sum() == max(abs(a[2] - a[0]), abs(a[3] - a[1])) + 1
        assert m[a[1], a[0]] and m[a[3], a[2]]
        back = rc.segment_mask((a[2], a[3], a[0], a[1]), w, h)
        xmajor, ties = rc.half_ties(a)
        diff = np.argwhere(m != back)
        assert all((x if xmajor else y) in ties for y, x in diff), a
    # (the exchange of the ends makes the two directions one item, so under this rule they agree at the halves too)
    assert pts((0, 0, 2, 1)) == [(0, 0), (1, 1), (2, 1)] == pts((2, 1, 0, 0))
    # ends beyond 2^20 are pulled in first: the slope is that of the clamped ends
    assert np.array_equal(rc.segment_mask((-2 ** 30, 4, 2 ** 30, 4), w, h), rc.segment_mask((-rc.FAR, 4, rc.FAR, 4), w, h))
    assert rc.segment_mask((-2 ** 30, 4, 2 ** 30, 4), w, h)[4].all()
    # the painter's rule, both ways
    f = np.zeros((h, w), np.uint8)
    by = {c[0]: c for c in rc.SEGMENT_CASES}
    over, under = (rc.reference(f, by["seg_%s_ring_70x37" % k][2]) for k in ("over", "under"))
    seg = rc.segment_mask(by["seg_over_ring_70x37"][2][1]["a"], w, h)
    ring, _ = oc.covers(by["seg_over_ring_70x37"][2][0], w, h, None)
    assert (seg & ring).sum() >= 2 and (over[seg] == oc.GREEN).all() and (under[ring] == oc.RED).all() and (over != under).any()
    none = rc.reference(f, by["seg_other_kinds_draw_nothing_70x37"][2])
    assert none.any(axis=2).sum() == 4 and none[1, 1:5].any(axis=1).all()


def test_segment_kind_in_header_python_and_host_checks():
    h = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert "SL2_ITEM_RING = 1, SL2_ITEM_PATCH = 2, SL2_ITEM_RECT = 3, SL2_ITEM_SEGMENT = 5" in h
    assert _lib.SL2_ITEM_SEGMENT == rectified.SL2_ITEM_SEGMENT == rc.SEGMENT == 5
    it = rectified.segment(1, 2, 3, 4, oc.RED, label=7)
    assert it.dtype == oc.ITEM and it == rc.segment(1, 2, 3, 4, oc.RED, label=7) and int(it["patch"]) == -1 and not it["q"].any()
    # a host-resident list with a segment is accepted by the batch call's checks (kind 4 is still refused); they precede the device
    L = _lib.load()
    p = lambda a: a.ctypes.data_as(_lib.vp)
    f, out, cnt = np.zeros((1, 8, 8), np.uint8), np.full((1, 8, 8, 3), 7, np.uint8), np.ones(1, np.int32)
    for kind, ok in ((5, True), (4, False), (0, False), (6, False)):
        items = oc.items_array([rc.segment(0, 0, 7, 7)])
        items["kind"] = kind
        code = L.sl2_draw_items_batch(0, None, p(f), 0, 1, 8, 8, 64, p(items), 1, p(cnt), 0, None, 0, 0, p(out), 192, 0)
        if ok:
            assert code == (_lib.SL2_OK if _lib.device_count() > 0 else _lib.SL2_ERR_NO_DEVICE)
        else:
            assert code == _lib.SL2_ERR_INVALID and "kind" in L.sl2_last_error().decode() and (out == 7).all()


@pytest.mark.parametrize("case", rc.REMAP_CASES, ids=[c[0] for c in rc.REMAP_CASES])
def test_remap_host_form_equals_the_restated_rule(case):
    name, (w, h), (u0, v0), kd1 = case
    frame = rc.remap_frame(w, h, seed=len(name))
    want = rc.rectify(frame, u0, v0, kd1)
    got = rectified.rectify_frame_host(frame, u0, v0, kd1)
    assert got.shape == (h, w) and got.dtype == np.uint8
    assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5].tolist())


def test_remap_rule_does_what_its_words_say():
    by = {c[0]: c for c in rc.REMAP_CASES}
    for w, h in rc.SIZES:
        sfx = "_%dx%d" % (w, h)
        f = rc.remap_frame(w, h, 3)
        for centre in ("inside", "border", "nondyadic"):
            _, _, (u0, v0), _ = by["remap_%s_zero%s" % (centre, sfx)]
            assert np.array_equal(rc.rectify(f, u0, v0, 0.0), f)          # kd1 = 0: the input, exactly
        _, _, (u0, v0), kd1 = by["remap_inside_shipped" + sfx]
        assert kd1 == 9e-06
        # kd1 > 0 pulls the sampling position towards the principal point: nothing is sampled off the image, no border shows
        _, _, (u0, v0), kd1 = by["remap_inside_strong" + sfx]
        strong = rc.rectify(f, u0, v0, kd1)
        assert (strong > 0).all() and not np.array_equal(strong, f)
        # kd1 < 0 pushes it outwards: the far corners read the border, the neighbourhood of the principal point does not move
        _, _, (u0, v0), kd1 = by["remap_inside_negative" + sfx]
        neg = rc.rectify(f, u0, v0, kd1)
        cy, cx = int(v0), int(u0)
        assert np.array_equal(neg[cy - 1:cy + 2, cx - 1:cx + 2], f[cy - 1:cy + 2, cx - 1:cx + 2])
        _, _, (u0, v0), kd1 = by["remap_inside_corners_lost" + sfx]
        lost = rc.rectify(f, u0, v0, kd1)
        ys, xs = np.mgrid[0:h, 0:w]
        fac = 1.0 + 2.0 * kd1 * ((xs - u0) ** 2 + (ys - v0) ** 2)
        assert (fac[[0, 0, -1, -1], [0, -1, 0, -1]] <= 0).all() and (fac[h // 2, w // 2] > 0)
        assert (lost[fac <= 0] == 0).all() and lost[h // 2, w // 2] > 0
    # a constant image stays constant wherever all four taps are inside; a half-pixel shift averages neighbours
    g = np.full((16, 64), 200, np.uint8)
    out = rc.rectify(g, 31.5, 7.5, 2e-4)
    assert (out == 200).all()
    # the bilinear weights: a source position half-way between 10 and 30 reads 20 - a frame with a step, sampled through a
    # camera whose distortion moves x = 40 (cx = 8 from u0 = 32) by exactly -0.5: s = 8 / 7.5, f = s^2, kd1 = (f - 1) / (2 * 64)
    kd1 = ((8.0 / 7.5) ** 2 - 1.0) / 128.0
    step = np.zeros((16, 64), np.uint8)
    step[:, :40], step[:, 40:] = 10, 30
    assert int(rc.rectify(step, 32.0, 8.0, kd1)[8, 40]) == 20


def _host_rc(frame, w, h, u0, v0, kd1, out):
    p = lambda a: None if a is None else a.ctypes.data_as(_lib.vp)
    return _lib.load().sl2_rectify_frame_host(p(frame), w, h, u0, v0, kd1, p(out))


def test_refusals():
    L = _lib.load()
    f, out = np.ones((8, 8), np.uint8), np.full((8, 8), 7, np.uint8)
    assert _host_rc(f, 8, 8, 4.0, 4.0, 0.0, out) == _lib.SL2_OK and (out == 1).all()
    out[:] = 7
    nan, inf = float("nan"), float("inf")
    for args in ((None, 8, 8, 4.0, 4.0, 0.0, out), (f, 8, 8, 4.0, 4.0, 0.0, None), (f, 0, 8, 4.0, 4.0, 0.0, out), (f, 8, 0, 4.0, 4.0, 0.0, out),
                 (f, 32769, 1, 4.0, 4.0, 0.0, out), (f, 8, -1, 4.0, 4.0, 0.0, out), (f, 8, 8, nan, 4.0, 0.0, out), (f, 8, 8, 4.0, inf, 0.0, out),
                 (f, 8, 8, 4.0, 4.0, -inf, out), (f, 8, 8, 4.0, 4.0, nan, out)):
        assert _host_rc(*args) == _lib.SL2_ERR_INVALID, args[1:6]
        assert "sl2_rectify_frame_host" in L.sl2_last_error().decode()
    assert (out == 7).all()
    buf = np.zeros(64, np.uint8)
    for od in (0, 1):
        assert L.sl2_rectify_frames(None, 0, 1, buf.ctypes.data_as(_lib.vp), 64, od, buf.ctypes.data_as(_lib.vp), 64, od) == _lib.SL2_ERR_INVALID
        assert "sl2_rectify_frames" in L.sl2_last_error().decode()
    assert not buf.any()


def test_symbols_signatures_and_python_names():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    flat = re.sub(r"\s+", " ", text)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, text), "%s is not declared" % name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name) and hasattr(_lib.load_testing(), name)
        assert getattr(L, name).argtypes, "%s has no ctypes signature" % name
    for sig in ("int sl2_rectify_frames(sl2_engine* e, int seq0, int nseq, const uint8_t* frames, size_t seq_stride, int frames_on_device, "
                "uint8_t* out, size_t out_stride, int out_on_device);",
                "int sl2_rectify_frame_host(const uint8_t* frame, int width, int height, double u0, double v0, double kd1, uint8_t* out);",
                "size_t sl2_scene_item_bound(int max_features, int partial_slots);",
                "int sl2_scene_items(sl2_engine* e, int seq0, int nseq, int layers, const int32_t* marked , sl2_overlay_item* items, "
                "int item_stride, int32_t* counts, int on_device);",
                "int sl2_draw_rectified(sl2_engine* e, int seq0, int nseq, const uint8_t* frames, size_t seq_stride, int frames_on_device, "
                "int layers, const int32_t* marked, uint8_t* out, size_t out_stride, int out_on_device);"):
        assert sig in flat, sig
    assert "#define SL2_API_VERSION 5" in _header()
    history = _header()[:_header().find("#define SL2_API_VERSION")]
    assert all(name in history for name in NEW + ["SL2_ITEM_SEGMENT"])
    from scenelib2_amd import Engine
    p = inspect.signature(Engine.rectify_frames).parameters
    assert list(p) == ["self", "frames", "seq0", "nseq", "on_device", "seq_stride", "out_stride"]
    assert callable(Engine.rectify_frames_device) and callable(rectified.rectify_frame_host) and callable(rectified.segment)
    for name in ("scene_items", "draw_rectified", "draw_rectified_device", "scene_item_bound"):
        assert callable(getattr(Engine, name))
    p = inspect.signature(Engine.scene_items).parameters
    assert list(p) == ["self", "seq0", "nseq", "layers", "marked"] and p["layers"].default == 7 and p["marked"].default is None
    assert "SL2_SCENE_TRAJECTORY = 1, SL2_SCENE_FEATURES = 2, SL2_SCENE_UNCERTAINTIES = 4" in text
    assert (_lib.SL2_SCENE_TRAJECTORY, _lib.SL2_SCENE_FEATURES, _lib.SL2_SCENE_UNCERTAINTIES, _lib.SL2_SCENE_ALL) == (1, 2, 4, 7)
    assert (rc.TRAJECTORY, rc.FEATURES, rc.UNCERTAINTIES) == (1, 2, 4)


def test_scene_bound_and_null_engine_refusals():
    L = _lib.load()
    for N, k in ((16, 1), (100, 4), (676, 4), (0, 0)):
        assert L.sl2_scene_item_bound(N, k) == 3 * N + k + 999 == rc.scene_item_bound(N, k)
    assert L.sl2_scene_item_bound(-1, 1) == 0 and L.sl2_scene_item_bound(4, -1) == 0
    buf = np.zeros(64 * 40, np.uint8)
    cnt = np.zeros(1, np.int32)
    for on_device in (0, 1):
        assert L.sl2_scene_items(None, 0, 1, 7, None, buf.ctypes.data_as(_lib.vp), 2000, cnt.ctypes.data_as(_lib.vp), on_device) == _lib.SL2_ERR_INVALID
        assert "sl2_scene_items" in L.sl2_last_error().decode()
        assert L.sl2_draw_rectified(None, 0, 1, buf.ctypes.data_as(_lib.vp), 16, 0, 7, None, buf.ctypes.data_as(_lib.vp), 48, on_device) == _lib.SL2_ERR_INVALID
        assert "sl2_draw_rectified" in L.sl2_last_error().decode()
    assert not buf.any() and cnt[0] == 0


def _zeroed_np(v):
    """zeroedyi of the stacked (xp, y), plain NumPy, as the function the reference's Jacobians are the derivative of: RRW from
    the CONJUGATE of q (dqbar_by_dq, feature_model.cpp:152-162) in the homogeneous form of the rotation matrix, diagonal
    w^2 + x^2 - y^2 - z^2 ... (dR_by_dq0 .. dR_by_dqz, feature_model.cpp:196-238).  On the unit sphere it is the value the
    library computes (Quaterniond::inverse, toRotationMatrix)."""
    r, q, y = v[0:3], v[3:7], v[7:10]
    w, x, yy, z = q[0], -q[1], -q[2], -q[3]
    R = np.array([[w * w + x * x - yy * yy - z * z, 2 * (x * yy - w * z), 2 * (x * z + w * yy)],
                  [2 * (x * yy + w * z), w * w - x * x + yy * yy - z * z, 2 * (yy * z - w * x)],
                  [2 * (x * z - w * yy), 2 * (yy * z + w * x), w * w - x * x - yy * yy + z * z]])
    return R @ (y - r)


def test_pzeroedyigraphics_against_central_differences():
    """Sigma = J P J^T with J the central-difference Jacobian of zeroedyi with respect to (xp, y) and P the joint covariance:
    relative 1e-6 (the differences' own error: step 1e-6 on quantities of order one, third derivatives of order one).  At unit
    quaternions, where the filter keeps the state: the reference's dzeroedyi_by_dq is the derivative of the homogeneous
    rotation matrix of the conjugate; Quaterniond::inverse() and toRotationMatrix(), which it EVALUATES, agree with that only on
    the sphere, so along q's radius the reference's Jacobian is not the derivative of what it evaluates (with those in
    _zeroed_np the two Sigma differ by a third under a covariance that has variance along the radius)."""
    cases = [c for c in rc.scene_math_cases() if abs(float(c[1][3:7] @ c[1][3:7]) - 1.0) < 1e-12]
    assert len(cases) >= 40
    for cam, xp, y, Pxx, Pxy, Pyy in cases:
        m, Jx, Jy = rc.zeroed_jac(xp, y)
        S = np.array(rc.sigma(Jx, Jy, Pxx, Pxy, Pyy))
        v = np.concatenate([xp, y])
        assert np.allclose(m, _zeroed_np(v), rtol=0, atol=1e-13)
        J = np.zeros((3, 10))
        for k in range(10):
            d = np.zeros(10)
            d[k] = 1e-6
            J[:, k] = (_zeroed_np(v + d) - _zeroed_np(v - d)) / 2e-6
        P = np.block([[Pxx, Pxy], [Pxy.T, Pyy]])
        want = J @ P @ J.T
        assert np.linalg.norm(S - want) <= 1e-6 * np.linalg.norm(want), (np.linalg.norm(S - want) / np.linalg.norm(want))
        assert np.abs(S - S.T).max() <= 1e-12 * np.abs(S).max() and np.linalg.eigvalsh((S + S.T) / 2).min() > 0


def test_the_conic_is_the_outline_of_the_projected_ellipsoid():
    """Anchored independently of any implementation: for 200 random (m, Sigma) with d > 0, 20 000 points of the surface
    (X - m)^T Sigma^-1 (X - m) = 9 are projected; with the unrounded centre every one satisfies the ring's form at
    <= rhs (1 + 1e-9) - they lie inside or on the outline - and the largest reaches >= 0.999 rhs - the outline is tight."""
    rng = np.random.default_rng(2026)
    cam = dict(rc.SHIPPED)
    done, worst_in, least_max = 0, 0.0, np.inf
    u = rng.normal(size=(20000, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    while done < 200:
        m = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.4, 0.4), rng.uniform(0.3, 3.0)])
        G = rng.normal(size=(3, 3)) * rng.uniform(0.005, 0.08)
        Sg = G @ G.T + 1e-8 * np.eye(3)
        got = rc.conic(cam, m, [[float(v) for v in row] for row in Sg])
        if got is None:
            assert m[2] * m[2] - 9.0 * Sg[2, 2] <= 0
            continue
        assert rc.conic(cam, -m, [[float(v) for v in row] for row in Sg]) is None          # the same ellipsoid behind the camera: d > 0, no ring
        (cx, cy), (A, B, C, rhs) = got
        assert rhs > 0 and A > 0 and C > 0 and 4 * A * C - B * B > 0
        X = m + 3.0 * u @ np.linalg.cholesky(Sg).T
        assert (X[:, 2] > 0).all()          # d > 0: wholly in front of the camera plane
        du = cam["u0"] - cam["fku"] * X[:, 0] / X[:, 2] - cx
        dv = cam["v0"] - cam["fkv"] * X[:, 1] / X[:, 2] - cy
        form = A * du * du + B * du * dv + C * dv * dv
        worst_in, least_max = max(worst_in, form.max() / rhs), min(least_max, form.max() / rhs)
        assert form.max() <= rhs * (1 + 1e-9), form.max() / rhs
        assert form.max() >= 0.999 * rhs, form.max() / rhs
        done += 1
    print("conic: largest form / rhs over the surfaces between %.9f and %.12f" % (least_max, worst_in))


def test_scene_segment_rule_on_anchors():
    cam = dict(rc.SHIPPED)
    # in front: the two projections, rounded
    assert rc.scene_segment(cam, [0.0, 0.0, 1.0], [0.1, -0.1, 1.0]) == [162, 125, 143, 145]          # 162 - 19.5 = 142.5 -> 143, 125 + 19.5 -> 145
    # crossing the near plane: the end behind moves onto X[2] = 0.01 along the segment, whichever end it is
    fwd = rc.scene_segment(cam, [0.0, 0.0, 1.0], [0.0, 0.0, -1.0])
    assert fwd == [162, 125, 162, 125]
    a, b = [0.001, 0.0, 0.51], [0.001, 0.0, -0.49]
    assert rc.scene_segment(cam, a, b) == [162, 125, 143, 125] and rc.scene_segment(cam, b, a) == [143, 125, 162, 125]          # t = 0.5: x/z = 0.1
    # behind, both: omitted; touching the plane counts as in front
    assert rc.scene_segment(cam, [0, 0, 0.0099], [1, 1, -3]) is None and rc.scene_segment(cam, [0, 0, 0.01], [0, 0, 0.01]) == [162, 125, 162, 125]
    # the guard square: a segment far outside is omitted, one leaving is cut at +-32767
    assert rc.scene_segment(cam, [400.0, 0, 1], [800.0, 0, 1]) is None
    cut = rc.scene_segment(cam, [0.0, 0.0, 1.0], [400.0, 0.0, 1.0])
    assert cut == [162, 125, -32766, 125]          # int(-32767 + 0.5) by C truncation
    assert rc.scene_segment(cam, [float("nan"), 0, 1], [0, 0, 1]) is None


def _oracle_view(s, cam):
    kinds = s.feature_kinds()
    feats = []
    for k in range(len(kinds)):
        f = s.feature(k)
        feats.append(dict(label=int(kinds[k, 2]), full=bool(kinds[k, 1]), size=int(kinds[k, 0]), selected=f["selected"], success=f["success"]))
    return dict(cam=cam, x=s.total_state(), P=s.total_covariance(), feats=feats, traj=s.trajectory())


def test_builder_on_the_oracle_s_run_of_the_gpu_scenes_skips_no_field(oracle):
    """The scenes of tests/test_gpu_rectified.py, run by the CPU oracle: the shipped four-feature scene after a few steps and
    the mapping scene while a partial feature is in flight.  Every kind of item appears, and no coordinate that gets rounded
    lies within 1e-6 of a half-integer: the GPU test compares every integer field."""
    from mapping_helpers import make_mapping_sequence, oracle_for
    from slam_helpers import Pair
    import display_helpers as rs
    pr = Pair(4, rs.SHIPPED_STEPS + 1, batch=1, make_engine=False)
    for k in range(rs.SHIPPED_STEPS):
        pr.oracles[0].go_one_step(pr.frames[0][k], True)
    items, rounded = rc.scene_list(_oracle_view(pr.oracles[0], pr.cam), 7, marked=1)
    assert rc.skipped_fields(rounded) == 0 and len(rounded) >= 4 * 4
    kinds = items["kind"].tolist()
    assert kinds.count(rc.RECT) == 8 and kinds.count(rc.RING) == 4
    # (trajectory_store_ holds the stale rRES_ of the reference, SURVEY Q12 - here the starting position, five times; the camera
    # has moved forward, so it lies behind the near plane and every segment is omitted.  Seen from half a metre further back
    # the four segments are there, as single pixels.)
    assert kinds.count(rc.SEGMENT) == 0 and len(pr.oracles[0].trajectory()) == rs.SHIPPED_STEPS
    view = _oracle_view(pr.oracles[0], pr.cam)
    view["x"] = view["x"].copy()
    view["x"][2] -= 0.5
    moved, rounded = rc.scene_list(view, rc.TRAJECTORY)
    assert moved["kind"].tolist() == [rc.SEGMENT] * (rs.SHIPPED_STEPS - 1) and rc.skipped_fields(rounded) == 0
    assert tuple(items[items["label"] == 1][0]["rgb"]) == oc.GREEN
    cam, params, spec, frames, templates = make_mapping_sequence(seed=rs.MAPPING_SEED, n_known=rs.MAPPING_KNOWN, n_frames=rs.MAPPING_FRAMES)
    for victim in (None, 2):          # (sequence 1 of the GPU test's engine has feature 2 deleted by hand before step 6)
        s = oracle_for(cam, params, spec, templates, oracle)
        seen_ray = 0
        for k in range(1, rs.MAPPING_FRAMES):
            if victim is not None and k == 6:
                assert s.delete_feature(victim)
            s.go_one_step(frames[k], True, True)
            view = _oracle_view(s, cam)
            items, rounded = rc.scene_list(view, 7)
            assert rc.skipped_fields(rounded) == 0, k
            rays = [it for it in items if int(it["kind"]) == rc.SEGMENT and int(it["label"]) >= 0]
            assert len(rays) == sum(not f["full"] for f in view["feats"])
            seen_ray += len(rays)
            assert items.size <= rc.scene_item_bound(rs.MAPPING_MAX_FEATURES, 1)
        assert seen_ray > 0


def test_kernel_source_and_build():
    csrc = os.path.join(ROOT, "scenelib2_amd", "csrc")
    src = open(os.path.join(csrc, "sl2_rectify.hip")).read()
    kernels = list(re.finditer(r"__global__[^{;]*?\b(k_\w+)\s*\(([^{;]*?)\)\s*\{", src, flags=re.S))
    assert [m.group(1) for m in kernels] == ["k_rectify", "k_scene_list"]
    for m in kernels:
        assert "CameraParams" not in m.group(2) and "const SeqArrays S" in m.group(2), m.group(1)          # no camera by value
    assert "load_cam(S.seq_cam" in src and "rectify_pixel(" in src and "rectify_host_body(" in src
    dev = open(os.path.join(csrc, "sl2_rectify_dev.hpp")).read()
    assert "rectify_host_body" in dev and "SL2_HD uint8_t rectify_pixel" in dev          # one source for both forms
    odev = open(os.path.join(csrc, "sl2_overlay_dev.hpp")).read()
    assert "SL2_ITEM_SEGMENT" in odev and "overlay_segment_covers" in odev and "long long" in odev
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert mk.count("sl2_rectify.hip") == 1 and "sl2_rectify_dev.hpp" in mk
    assert not re.search(r"^sl2_rectify\.o:", mk, flags=re.M)          # the default flags: -ffp-contract=off
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^#+ *8i\b", design, flags=re.M)
    sec = design[re.search(r"^#+ *8i\b", design, flags=re.M).start():]
    assert "k_scene_list(const SeqArrays S" not in src.replace("k_scene_list(const SeqArrays S", "", 1) and "scene_sigma(" in src and "scene_conic(" in src
    for word in ("k_rectify", "k_scene_list", "SL2_ITEM_SEGMENT", "through the caches", "scratch", "Left out", "rectified_bench.json"):
        assert word in sec, word


def test_host_bodies_match_and_stay_inside_exactly_sized_blocks_under_asan(tmp_path):
    """tests/rectified_host.cpp: a program of its own (nothing loaded into Python), built with the address and undefined-behaviour
    sanitizers, over the same cases with exactly sized heap blocks; it compares with what the restated rules expect."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = os.path.join(str(tmp_path), "rectified_host")
    casefile = os.path.join(str(tmp_path), "cases.bin")
    with open(casefile, "wb") as f:
        f.write(struct.pack("<i", len(rc.SEGMENT_CASES)))
        for name, (w, h), items, patches in rc.SEGMENT_CASES:
            frame = oc.frame_of(w, h, seed=len(name))
            n, stride = (0, 0) if patches is None else patches.shape
            f.write(struct.pack("<5i", w, h, len(items), n, stride))
            f.write(frame.tobytes())
            f.write(oc.items_array(items).tobytes())
            if n:
                f.write(patches.tobytes()[:(n - 1) * stride + 121])
            f.write(rc.reference(frame, items, patches).tobytes())
        f.write(struct.pack("<i", len(rc.REMAP_CASES)))
        for name, (w, h), (u0, v0), kd1 in rc.REMAP_CASES:
            frame = rc.remap_frame(w, h, seed=len(name))
            f.write(struct.pack("<2i3d", w, h, u0, v0, kd1))
            f.write(frame.tobytes())
            f.write(rc.rectify(frame, u0, v0, kd1).tobytes())
        scenes, segs = rc.scene_math_cases(), rc.segment3d_cases()
        f.write(struct.pack("<i", len(scenes)))
        for cam, xp, y, Pxx, Pxy, Pyy in scenes:
            f.write(struct.pack("<4d", cam["fku"], cam["fkv"], cam["u0"], cam["v0"]))
            for a in (xp, y, Pxx, Pxy, Pyy):
                f.write(np.ascontiguousarray(a, np.float64).tobytes())
            m, Jx, Jy = rc.zeroed_jac(xp, y)
            S = rc.sigma(Jx, Jy, Pxx, Pxy, Pyy)
            got = rc.conic(cam, m, S)
            f.write(struct.pack("<12d", *(list(m) + [v for row in S for v in row])))
            f.write(struct.pack("<i6d", *((0, 0, 0, 0, 0, 0, 0) if got is None else (1,) + tuple(got[0]) + tuple(got[1]))))
        f.write(struct.pack("<i", len(segs)))
        for cam, a, b in segs:
            f.write(struct.pack("<10d", cam["fku"], cam["fkv"], cam["u0"], cam["v0"], *(list(a) + list(b))))
            got = rc.scene_segment(cam, a, b)
            f.write(struct.pack("<5i", *((0, 0, 0, 0, 0) if got is None else [1] + got)))
    src = os.path.join(ROOT, "tests", "rectified_host.cpp")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, src])
    res = subprocess.run([exe, casefile], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.startswith("ok %d segment cases %d remap cases %d scene cases %d 3-D segments" % (
        len(rc.SEGMENT_CASES), len(rc.REMAP_CASES), len(scenes), len(segs)))
    assert sum(rc.conic(c[0], rc.zeroed_jac(c[1], c[2])[0], rc.sigma(*rc.zeroed_jac(c[1], c[2])[1:], c[3], c[4], c[5])) is not None for c in scenes) >= 15
    assert 10 <= sum(rc.scene_segment(*c) is not None for c in segs) <= len(segs) - 10


def test_adapters_example_and_documents_know_the_feature(tmp_path):
    from scenelib2_amd import MonoSLAM
    assert list(inspect.signature(MonoSLAM.DrawRectifiedAR).parameters) == ["self", "frame", "out_rgb", "chk_display_trajectory",
                                                                            "chk_display_3d_features", "chk_display_3d_uncertainties"]
    assert list(inspect.signature(MonoSLAM.DrawAR).parameters)[:4] == ["self", "frame", "out_rgb", "chk_rectify_image_display"]
    # include/scenelib2_amd_monoslam.hpp: both members type-check with the reference's argument order, and each check box maps to its bit
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    src = os.path.join(str(tmp_path), "use_adapter.cpp")
    with open(src, "w") as f:
        f.write("#include <scenelib2_amd_monoslam.hpp>\n"
                "void use(SceneLib2Amd::MonoSLAM& m, const SceneLib2Amd::Frame& fr, uint8_t* rgb) {\n"
                "  void (SceneLib2Amd::MonoSLAM::*p)(const SceneLib2Amd::Frame&, uint8_t*, bool, bool, bool) = &SceneLib2Amd::MonoSLAM::DrawRectifiedAR;\n"
                "  (m.*p)(fr, rgb, true, false, true);\n"
                "  m.DrawAR(fr, rgb, true, true, true, true, false, false, false);\n}\n")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src])
    hpp = open(os.path.join(ROOT, "include", "scenelib2_amd_monoslam.hpp")).read()
    body = hpp[hpp.find("void DrawRectifiedAR("):]
    body = re.sub(r"\s+", " ", body[:body.find("\n  }")])
    assert "sl2_draw_rectified" in body and "marked_feature_label_" in body
    for box, bit in (("chk_display_trajectory", "SL2_SCENE_TRAJECTORY"), ("chk_display_3d_features", "SL2_SCENE_FEATURES"),
                     ("chk_display_3d_uncertainties", "SL2_SCENE_UNCERTAINTIES")):
        assert "(%s ? %s : 0)" % (box, bit) in body, box
    ref = open(os.path.join(ROOT, "examples", "ref_binding", "monoslam_amd.h")).read()
    assert "void DrawRectifiedAR(cv::Mat frame, cv::Mat& out_rgb, const bool& chk_display_trajectory" in ref and "impl_.DrawRectifiedAR(" in ref
    assert "void DrawAR(cv::Mat frame, cv::Mat& out_rgb, const bool& chk_rectify_image_display" in ref
    mk = open(os.path.join(ROOT, "examples", "Makefile")).read()
    assert re.search(r"^all:.*\brectified_monoslam\b", mk, flags=re.M) and "rectified_monoslam.cpp" in mk
    ex = open(os.path.join(ROOT, "examples", "rectified_monoslam.cpp")).read()
    for call in ("sl2_draw_rectified", "sl2_scene_items", "sl2_scene_item_bound", "sl2_rectify_frames", "sl2_go_one_step"):
        assert call in ex, call
    assert "sl2_draw_rectified" in open(os.path.join(ROOT, "README.md")).read()
    assert "sl2_draw_rectified" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("rectified_bench.json", "rectified_ab.json"):
        assert os.path.exists(os.path.join(ROOT, "profiles", name)), name
