"""The world view and picking on the device (include/scenelib2_amd.h, "the world view and picking").

sl2_world_items against world_view_cases.world_list, a builder that works ONLY from public accessors (total state, total
covariance, features, trajectory) in the header's order of operations - every field exact, q byte for byte, the extents exact -
on the shipped four-feature scene, a mapping scene with a partial feature in flight, a map of 70 features (two rounds of lanes)
and a trajectory of 66 entries (two ballot rounds); through the reference example's view, a view per sequence, a view inside the
map and one turned away.  sl2_draw_world against sl2_draw_items_host of the device's own list over a constant frame.
sl2_pick_items_batch against sl2_pick_items_host (which tests/test_world_view_host.py holds to a coverage found by drawing)."""
import numpy as np
import pytest

import display_helpers as dh
import overlay_cases as oc
import rectified_cases as rc
import world_view_cases as wc
from display_helpers import SENTINEL, assert_lists_equal, engine_state
from mapping_helpers import make_mapping_sequence
from scenelib2_amd import Engine, _lib, overlay, world_view
from slam_helpers import Pair

pytestmark = pytest.mark.gpu

ALL = wc.ALL
SIZES = ((70, 37), (64, 32), (320, 240))


def states_of(e):
    return [engine_state(e, b) for b in range(e.batch)]


def check_world(S, seq0, nseq, views, layers, marked=None, size=None, background=0):
    """sl2_world_items against the builder (every field and the extents, no skips: asserted); with `size`, sl2_draw_world against
    sl2_draw_items_host of the device's own list over a constant frame."""
    e = S["e"]
    views = np.atleast_1d(np.asarray(views, wc.VIEW))
    lists, extents = e.world_items(views, seq0, nseq, layers, marked)
    built = []
    for i in range(nseq):
        view = views[0 if views.size == 1 else i]
        want, rounded, ext = wc.world_list(S["states"][seq0 + i], view, layers, -1 if marked is None else int(marked[i]))
        assert rc.skipped_fields(rounded) == 0, "a rounded coordinate lies within 1e-6 of a half-integer: choose another scene or view"
        assert_lists_equal(lists[i], want, "sequence %d, layers %d" % (seq0 + i, layers))
        assert extents[i].tobytes() == ext.tobytes(), (seq0 + i, layers, extents[i].tolist(), ext.tolist())          # min and max do not round
        assert want.size <= e.world_item_bound()
        built.append(want)
    if size is not None:
        w, h = size
        imgs = e.draw_world(views, w, h, seq0, nseq, background, layers, marked)
        for i in range(nseq):
            host = overlay.draw_items_host(np.full((h, w), background, np.uint8), lists[i], None)
            assert np.array_equal(imgs[i], host), (seq0 + i, layers, np.argwhere((imgs[i] != host).any(axis=2))[:5].tolist())
    return built


@pytest.fixture(scope="module")
def shipped_scene():
    for e, pr in dh.shipped_scene():
        yield dict(e=e, states=states_of(e), views=wc.fixed_views(pr.cam), cam=pr.cam)


@pytest.fixture(scope="module")
def mapping_scene():
    for e, frames, cam in dh.mapping_scene():
        states = states_of(e)
        for b in range(e.batch):          # the builder's six numbers are sl2_get_partial_feature's
            st, pos = states[b], 13
            for f in st["feats"]:
                if not f["full"]:
                    pf = e.partial_feature(b, 0)["pf"]
                    assert pf is not None and pf["label"] == f["label"] and np.array_equal(pf["y"], st["x"][pos:pos + 6])
                pos += f["size"]
        yield dict(e=e, states=states, views=wc.fixed_views(cam), cam=cam)


@pytest.fixture(scope="module")
def large_map():
    for e, state, cam in dh.large_map():
        yield dict(e=e, states=[state], views=wc.fixed_views(cam), cam=cam)


@pytest.fixture(scope="module")
def long_trajectory():
    """Four known features first seen from four places, stepped 66 times with the trajectory saved, the last feature of the list
    deleted twice on the way: trajectory_store_ (the stale rRES_ of the reference, SURVEY Q12: the place the LAST feature was
    first seen from) holds 66 entries of three different values - 65 segments, a second ballot round with one live lane."""
    pr = Pair(4, 4, batch=1, make_engine=False)
    e = Engine(pr.cam, pr.params, 1, 4)
    spec = pr.specs[0]
    e.set_vehicle_state(spec.xv0[None], spec.Pxx0[None])
    xo = np.tile(spec.poses[0], (4, 1))
    xo[:, 2] += (0.0, 0.3, 0.15, -0.3)
    xo[:, 0] += 0.02 * np.arange(4)
    e.add_known_features(spec.feat_y[None], xo[None], pr.templates[0][None])
    for k in range(66):
        e.go_one_step(pr.frame_batch(k % 4), save_trajectory=True)
        if k in (19, 41):
            assert e.delete_features([3 if k == 19 else 2]).all()
    states = states_of(e)
    assert len(states[0]["traj"]) == 66 and len(np.unique(states[0]["traj"], axis=0)) == 3
    yield dict(e=e, states=states, views=wc.fixed_views(pr.cam), cam=pr.cam)
    e.close()


# ------------------------------------------------------------------------------------------------- the lists
def test_world_lists_of_the_shipped_scene_through_the_reference_view(shipped_scene):
    S = shipped_scene
    built = check_world(S, 0, 3, S["views"]["reference"], ALL, np.array([1, -1, 3], np.int32), size=(320, 240))
    for b in built:
        kinds, rgbs = b["kind"].tolist(), [tuple(v) for v in b["rgb"].tolist()]
        assert kinds[:16] == [rc.SEGMENT] * 16 and rgbs[:16] == [wc.GREY] * 16 and rgbs[-3:] == [wc.WHITE] * 3
        assert kinds.count(rc.RECT) == 8 and kinds.count(rc.RING) == 4 and rgbs.count(oc.YELLOW) >= dh.SHIPPED_STEPS - 2
        # (a known feature's Pyy stays 0 until the filter correlates it: its world-frame ellipsoid is a point or nearly one, and a
        # form that is not positive definite is listed and draws nothing - the large map below has proper ellipsoids)
    assert tuple(built[0][built[0]["label"] == 1][0]["rgb"]) == oc.GREEN and tuple(built[2][built[2]["label"] == 3][-1]["rgb"]) == oc.GREEN


def test_a_view_per_sequence_against_one_shared_view(shipped_scene, mapping_scene):
    S = shipped_scene
    V = S["views"]
    per = np.array([V["side"], V["reference"], V["inside"]], wc.VIEW)
    built = check_world(S, 0, 3, per, ALL, size=(70, 37), background=200)
    shared = check_world(S, 0, 3, V["reference"], ALL)
    assert built[1].tobytes() == shared[1].tobytes() and built[0].tobytes() != shared[0].tobytes()
    M = mapping_scene
    check_world(M, 0, 2, np.array([M["views"]["inside"], M["views"]["side"]], wc.VIEW), ALL, np.array([-1, 2], np.int32), size=(64, 32))


def test_view_inside_the_map_and_view_turned_away(shipped_scene, mapping_scene, large_map):
    for S in (shipped_scene, mapping_scene, large_map):
        n = S["e"].batch
        inside = check_world(S, 0, n, S["views"]["inside"], ALL, size=(70, 37))
        side = check_world(S, 0, n, S["views"]["side"], ALL)
        assert all(0 < a.size < b.size for a, b in zip(inside, side))          # something lies behind it, something in front
        away = check_world(S, 0, n, S["views"]["away"], ALL & ~(wc.CAMERA | wc.AXES), size=(64, 32), background=200)
        assert all(a.size == 0 for a in away)
        lists, _ = S["e"].world_items(S["views"]["away"], 0, n, ALL)
        assert [len(l) for l in lists] == [0] * n          # the camera and the axes lie behind it too
    # the view inside the mapping scene cuts a ray at its near plane: an end of the segment far outside the image
    M = mapping_scene
    rays = [it for b in check_world(M, 0, 2, M["views"]["inside"], wc.FEATURES) for it in b if int(it["kind"]) == rc.SEGMENT]
    assert rays and any(np.abs(it["a"]).max() > 1000 for it in rays)


def test_large_map_two_rounds_of_slots(large_map):
    S = large_map
    for name in ("reference", "side"):
        built = check_world(S, 0, 1, S["views"][name], ALL, np.array([66], np.int32), size=(320, 240) if name == "side" else None)
        b = built[0]
        assert b["kind"].tolist().count(rc.RECT) == 140 and b["kind"].tolist().count(rc.RING) >= 60
        labels = [int(it["label"]) for it in b if int(it["kind"]) == rc.RECT][::2]
        assert labels == list(range(70))          # slot order across the two rounds
        assert all(oc.ring_valid(it["q"]) for it in b if int(it["kind"]) == rc.RING)
        assert tuple(b[b["label"] == 66][0]["rgb"]) == oc.GREEN
    # ellipsoids that straddle the inside view's plane yield a marker and no ring, or neither
    b = check_world(S, 0, 1, S["views"]["inside"], wc.FEATURES | wc.UNCERTAINTIES)[0]
    rings = {int(it["label"]) for it in b if int(it["kind"]) == rc.RING}
    markers = {int(it["label"]) for it in b if int(it["kind"]) == rc.RECT}
    assert markers - rings and len(markers) < 70
    # the extents take the features in with FEATURES only
    with_f = S["e"].world_items(S["views"]["side"], 0, 1, wc.FEATURES)[1][0]
    without = S["e"].world_items(S["views"]["side"], 0, 1, wc.UNCERTAINTIES | wc.AXES)[1][0]
    y = wc.large_map()["y"]
    assert with_f[1] == y[:, 0].max() and with_f[4] == min(y[:, 2].min(), -0.11) and with_f[5] == y[:, 2].max()
    assert without.tolist() == [0.0, 0.021, 0.0, 0.013, -0.11, 0.0]


def test_long_trajectory_two_ballot_rounds(long_trajectory):
    S = long_trajectory
    b = check_world(S, 0, 1, S["views"]["side"], wc.TRAJECTORY, size=(320, 240))[0]
    assert b.size == 65 and set(b["kind"].tolist()) == {rc.SEGMENT}
    assert len({tuple(a) for a in b["a"].tolist()}) >= 4          # the two jumps of the store are two long segments among the points
    check_world(S, 0, 1, S["views"]["reference"], ALL)
    check_world(S, 0, 1, S["views"]["inside"], ALL)


@pytest.mark.parametrize("layers", range(32))
def test_every_subset_of_the_layers(shipped_scene, mapping_scene, layers):
    S, M = shipped_scene, mapping_scene
    check_world(S, 0, 3, S["views"]["side"], layers, size=(64, 32) if layers in (0, 21) else None)
    built = check_world(M, 0, 2, M["views"]["reference"], layers, np.array([-1, 2], np.int32), size=(70, 37) if layers in (10, 31) else None, background=200)
    if layers == 0:
        assert all(b.size == 0 for b in built)
    if layers & wc.FEATURES:
        assert all(any(int(it["kind"]) == rc.SEGMENT and int(it["label"]) >= 0 for it in b) for b in built), "no ray of a partial feature"
    if layers == wc.UNCERTAINTIES:
        assert all(set(b["kind"].tolist()) == {rc.RING} for b in built)
    if layers == wc.AXES:
        assert all(b.size == 3 and [tuple(v) for v in b["rgb"].tolist()] == [wc.WHITE] * 3 for b in built)
    if layers == wc.CAMERA:
        assert all(b.size == 16 for b in built)


def test_own_camera_as_the_view_gives_the_scene_list(shipped_scene, mapping_scene):
    """The cross-check against shipped code: with the sequence's own (r, q) and camera numbers as the view and the layers
    TRAJECTORY | FEATURES, every item is computed by the same expressions as sl2_scene_items computes it - item for item.  (The
    ray of a partial feature is the exception in the last bit: the scene list adds 10 hhat in the camera frame, the world list
    in the world; its integer fields are compared, the mapping scene's rounding permitting: asserted here.)"""
    for S in (shipped_scene, mapping_scene):
        e = S["e"]
        n = e.batch
        cams = e.get_cameras(0, n)
        views = np.array([wc.make_view(S["states"][b]["x"][0:3], S["states"][b]["x"][3:7], cams[b]) for b in range(n)], wc.VIEW)
        world, _ = e.world_items(views, 0, n, wc.TRAJECTORY | wc.FEATURES)
        scene = e.scene_items(0, n, rc.TRAJECTORY | rc.FEATURES)
        for b in range(n):
            assert_lists_equal(world[b], scene[b], "sequence %d" % b)
            assert world[b].size > 0


# ------------------------------------------------------------------------------------------------- drawing
def _draw_raw(e, views_arr, nviews, w, h, bg, layers, marked, seq0, nseq, on_device, out_pad):
    """One sl2_draw_world call in the given residency with sentinels round every buffer; returns [nseq][h][w][3]."""
    L, vp = e.L, _lib.vp
    out_stride = 3 * w * h + out_pad
    out = np.full((nseq + 2, out_stride), SENTINEL, np.uint8)          # a guard image before and behind
    v = np.ascontiguousarray(views_arr[:nviews])
    m = np.ascontiguousarray(marked, np.int32)
    bufs = []
    if on_device:
        dv, dm, do = _lib.DeviceBuffer(v.nbytes), _lib.DeviceBuffer(m.nbytes), _lib.DeviceBuffer(out.nbytes)
        dv.upload(v); dm.upload(m); do.upload(out)
        bufs = [dv, dm, do]
        _lib.check(L.sl2_draw_world(e.h, seq0, nseq, vp(dv.ptr), nviews, w, h, bg, layers, vp(dm.ptr), vp(do.ptr + out_stride), out_stride, 1), L)
        out = do.download(out.shape, np.uint8)          # (a blocking copy on the null stream: behind the launches)
    else:
        _lib.check(L.sl2_draw_world(e.h, seq0, nseq, v.ctypes.data_as(vp), nviews, w, h, bg, layers, m.ctypes.data_as(vp),
                                    vp(out.ctypes.data + out_stride), out_stride, 0), L)
    for b in bufs:
        b.free()
    assert (out[0] == SENTINEL).all() and (out[-1] == SENTINEL).all() and (out[:, 3 * w * h:] == SENTINEL).all(), "bytes round the images were written"
    return out[1:-1, :3 * w * h].reshape(nseq, h, w, 3)


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("on_device", [0, 1], ids=["host", "device"])
def test_draw_world_equals_the_host_rasteriser_in_every_residency(shipped_scene, size, on_device):
    S = shipped_scene
    e, V = S["e"], S["views"]
    w, h = size
    per = np.array([V["side"], V["reference"], V["inside"]], wc.VIEW)
    marked = np.array([1, -1, 3], np.int32)
    lists, _ = e.world_items(per, 0, 3, ALL, marked)
    for bg, pad in ((0, 0), (200, 7)):
        got = _draw_raw(e, per, 3, w, h, bg, ALL, marked, 0, 3, on_device, pad)
        for i in range(3):
            host = overlay.draw_items_host(np.full((h, w), bg, np.uint8), lists[i], None)
            assert np.array_equal(got[i], host), (i, bg, np.argwhere((got[i] != host).any(axis=2))[:5].tolist())
        if size == (320, 240):          # (the views keep the camera's principal point: the small images show a corner of the pane)
            assert (got == (150, 150, 150)).all(axis=3).any() and (got[0] == (0, 255, 0)).all(axis=2).any() and not (got[1] == (0, 255, 0)).all(axis=2).any()
    # one shared view, a late seq0
    lists, _ = e.world_items(V["side"], 1, 2, ALL)
    got = _draw_raw(e, np.array([V["side"]], wc.VIEW), 1, w, h, 31, ALL, np.array([-1, -1], np.int32), 1, 2, on_device, 4)
    for i in range(2):
        assert np.array_equal(got[i], overlay.draw_items_host(np.full((h, w), 31, np.uint8), lists[i], None))


def test_world_items_device_form_writes_nothing_behind_the_lists(mapping_scene):
    S = mapping_scene
    e, V = S["e"], S["views"]
    L, vp = e.L, _lib.vp
    stride = e.world_item_bound() + 3
    views = np.array([V["side"], V["reference"]], wc.VIEW)
    marked = np.array([2, -1], np.int32)
    host, host_ext = e.world_items(views, 0, 2, ALL, marked)
    bufs = [_lib.DeviceBuffer(n) for n in (64 * stride * 2, 8, 8, views.nbytes, 8 * 14)]
    d_items, d_counts, d_marked, d_views, d_ext = bufs
    d_items.upload(np.full(64 * stride * 2, SENTINEL, np.uint8))
    d_marked.upload(marked)
    d_views.upload(views)
    d_ext.upload(np.full(14, -7.0))
    _lib.check(L.sl2_world_items(e.h, 0, 2, vp(d_views.ptr), 2, ALL, vp(d_marked.ptr), vp(d_items.ptr), stride, vp(d_counts.ptr), vp(d_ext.ptr + 8), 1), L)
    counts = d_counts.download((2,), np.int32)
    items = d_items.download((2, stride), oc.ITEM)
    ext = d_ext.download((14,), np.float64)
    for i in range(2):
        assert counts[i] == host[i].size and items[i, :counts[i]].tobytes() == host[i].tobytes()
        assert (items[i, counts[i]:].view(np.uint8) == SENTINEL).all()          # nothing behind the list was written
    assert ext[0] == -7.0 and ext[13] == -7.0 and ext[1:13].tobytes() == host_ext.tobytes()
    # extents may be NULL, in both forms
    _lib.check(L.sl2_world_items(e.h, 0, 2, vp(d_views.ptr), 2, ALL, vp(d_marked.ptr), vp(d_items.ptr), stride, vp(d_counts.ptr), None, 1), L)
    assert np.array_equal(d_counts.download((2,), np.int32), counts)
    # sl2_draw_items_batch and sl2_pick_items_batch take the device lists as they are
    W, H = 70, 37
    want = np.stack([overlay.draw_items_host(np.zeros((H, W), np.uint8), host[i], None) for i in range(2)])
    d_f, d_o = _lib.DeviceBuffer(2 * W * H), _lib.DeviceBuffer(want.nbytes)
    d_f.upload(np.zeros((2, H, W), np.uint8))
    _lib.check(L.sl2_draw_items_batch(0, None, vp(d_f.ptr), 1, 2, W, H, W * H, vp(d_items.ptr), stride, vp(d_counts.ptr), 1, None, 0, 0, vp(d_o.ptr),
                                      3 * W * H, 1), L)
    assert np.array_equal(d_o.download(want.shape, np.uint8), want)
    for d in bufs + [d_f, d_o]:
        d.free()


# ------------------------------------------------------------------------------------------------- picking
def _pick_batch(lists, clicks, w, h, npatches, on_device, item_pad=0):
    L, vp = _lib.load(), _lib.vp
    n = len(lists)
    stride = max([a.size for a in lists] + [1]) + item_pad
    items = np.zeros((n, stride), oc.ITEM)
    counts = np.zeros(n, np.int32)
    for i, a in enumerate(lists):
        items[i, :a.size] = a
        items[i, a.size:] = wc._lab(oc.rect(0, 0, w - 1, h - 1), 99)          # what lies behind a list's count is not part of it
        counts[i] = a.size
    c = np.ascontiguousarray(clicks, np.int32).reshape(n, 2)
    out = np.full((n + 2, 2), 77, np.int32)
    if on_device:
        bufs = [_lib.DeviceBuffer(a.nbytes) for a in (items, counts, c, out)]
        for b, a in zip(bufs, (items, counts, c, out)):
            b.upload(a)
        rc_ = L.sl2_pick_items_batch(0, None, n, w, h, vp(bufs[0].ptr), stride, vp(bufs[1].ptr), npatches, vp(bufs[2].ptr), vp(bufs[3].ptr + 8), 1)
        out = bufs[3].download(out.shape, np.int32)
        for b in bufs:
            b.free()
    else:
        rc_ = L.sl2_pick_items_batch(0, None, n, w, h, items.ctypes.data_as(vp), stride, counts.ctypes.data_as(vp), npatches, c.ctypes.data_as(vp),
                                     vp(out.ctypes.data + 8), 0)
    assert (out[0] == 77).all() and (out[-1] == 77).all()
    return rc_, out[1:-1]


@pytest.mark.parametrize("on_device", [0, 1], ids=["host", "device"])
def test_pick_batch_equals_the_host_form_on_the_host_cases(on_device):
    """Every click of every case an image of one launch (per patch count).  A host-resident batch refuses a list with an item of
    unknown kind or a patch index outside the array, as sl2_draw_items_batch does: those cases go by device lists, and the
    refusal is asserted."""
    L = _lib.load()
    for npatches in sorted({c["npatches"] for c in wc.PICK_CASES}):
        lists, clicks, want, names = [], [], [], []
        for c in wc.PICK_CASES:
            if c["npatches"] != npatches:
                continue
            w, h = c["size"]
            if c["refused_on_host"] and not on_device:
                code, out = _pick_batch([c["items"]], [c["clicks"][0]], w, h, npatches, 0)
                assert code == _lib.SL2_ERR_INVALID and "sl2_pick_items_batch: image 0" in L.sl2_last_error().decode() and (out == 77).all()
                continue
            for x, y in c["clicks"]:
                if not -2 ** 31 <= x < 2 ** 31:
                    continue
                lists.append(c["items"]); clicks.append((x, y)); names.append(c["name"])
                want.append(world_view.pick_items_host(w, h, c["items"], x, y, npatches))
        if not lists:
            continue
        for pad in (0, 3):
            code, got = _pick_batch(lists, clicks, w, h, npatches, on_device, item_pad=pad)
            assert code == _lib.SL2_OK, L.sl2_last_error().decode()
            bad = [(names[i], clicks[i], got[i].tolist(), want[i]) for i in range(len(lists)) if tuple(got[i]) != want[i]]
            assert not bad, bad[:5]
    assert np.array_equal(world_view.pick_items(70, 37, [wc.PICK_CASES[0]["items"]] * 2, [(20, 10), (0, 0)]), [[9, 1], [-1, -1]])


def test_pick_device_count_is_clamped():
    """A device count cannot be looked at: below 0 it is 0, above item_stride it is item_stride."""
    items = oc.items_array([wc._lab(oc.rect(1, 1, 5, 5), 3), wc._lab(oc.rect(1, 1, 5, 5), 4)])
    L, vp = _lib.load(), _lib.vp
    both = np.stack([items, items, items])
    counts = np.array([-5, 2 ** 30, 1], np.int32)
    clicks = np.array([[1, 1]] * 3, np.int32)
    out = np.zeros((3, 2), np.int32)
    bufs = [_lib.DeviceBuffer(a.nbytes) for a in (both, counts, clicks, out)]
    for b, a in zip(bufs, (both, counts, clicks, out)):
        b.upload(a)
    _lib.check(L.sl2_pick_items_batch(0, None, 3, 10, 10, vp(bufs[0].ptr), 2, vp(bufs[1].ptr), 0, vp(bufs[2].ptr), vp(bufs[3].ptr), 1), L)
    assert bufs[3].download((3, 2), np.int32).tolist() == [[-1, -1], [4, 1], [3, 0]]
    for b in bufs:
        b.free()


def test_a_click_on_each_marker_of_the_engine_s_lists_picks_a_feature_that_covers_it(shipped_scene, mapping_scene, large_map):
    draw = lambda f, it, p: overlay.draw_items_host(f, it, p)
    w, h = 320, 240
    for S in (shipped_scene, mapping_scene, large_map):
        lists, _ = S["e"].world_items(S["views"]["reference"], 0, 1, ALL)
        items = lists[0]
        marks = [(k, it) for k, it in enumerate(items) if int(it["kind"]) == rc.RECT and it["a"][0] == it["a"][2]
                 and 0 <= it["a"][0] < w and 0 <= it["a"][1] < h][:12]
        assert len(marks) >= 4
        got = world_view.pick_items(w, h, [items] * len(marks), [(int(it["a"][0]), int(it["a"][1])) for _, it in marks])
        for (k, it), (label, index) in zip(marks, got.tolist()):
            x, y = int(it["a"][0]), int(it["a"][1])
            assert index >= k and label == int(items[index]["label"]) >= 0          # the marker itself covers its pixel: nothing earlier wins
            assert wc.coverage(draw, items[index], w, h)[max(y - 3, 0):y + 4, max(x - 3, 0):x + 4].any()
            assert (label, index) == world_view.pick_items_host(w, h, items, x, y)
        assert any(label == int(it["label"]) for (k, it), (label, index) in zip(marks, got.tolist()))


# ------------------------------------------------------------------------------------------------- ranges, groups, refusals
def test_late_seq0_paused_sequence_and_groups(shipped_scene, mapping_scene):
    S = shipped_scene
    e, V = S["e"], S["views"]
    check_world(S, 2, 1, V["side"], ALL, np.array([0], np.int32), size=(70, 37))
    check_world(S, 1, 2, np.array([V["reference"], V["side"]], wc.VIEW), ALL)
    e.set_active([0, 1, 0])          # the mask is not consulted: a paused sequence is listed like any other
    try:
        check_world(S, 0, 3, V["reference"], ALL, size=(64, 32))
    finally:
        e.set_active([1, 1, 1])
    M = mapping_scene
    m = M["e"]
    m.set_groups(2)
    try:
        check_world(M, 0, 2, M["views"]["side"], ALL, size=(70, 37))
        check_world(M, 1, 1, M["views"]["reference"], ALL, np.array([3], np.int32))
    finally:
        m.set_groups(1)


def test_refusals_queue_nothing(mapping_scene):
    S = mapping_scene
    e = S["e"]
    L, vp = e.L, _lib.vp
    bound = e.world_item_bound()
    views = np.array([S["views"]["side"], S["views"]["reference"]], wc.VIEW)
    three = np.array([S["views"]["side"]] * 3, wc.VIEW)
    nan_view = views.copy()
    nan_view[1]["q"][2] = np.nan
    inf_view = views.copy()
    inf_view[0]["fku"] = np.inf
    cnt = np.zeros(2, np.int32)
    buf = np.zeros((2, bound), oc.ITEM)
    ext = np.zeros((2, 6))
    W, H = 70, 37
    out = np.full((2, 3 * W * H), 7, np.uint8)
    d_items = _lib.DeviceBuffer(64 * bound * 2 + 64)
    d_views = _lib.DeviceBuffer(views.nbytes + 8)
    def items_rc(seq0=0, nseq=2, v=views, nv=2, layers=ALL, ip=buf.ctypes.data, st=bound, cp=cnt.ctypes.data, dev=0, vptr=None):
        return (L.sl2_world_items(e.h, seq0, nseq, vp(vptr) if vptr else (v.ctypes.data_as(vp) if v is not None else None), nv, layers, None,
                                  vp(ip) if ip else None, st, vp(cp) if cp else None, ext.ctypes.data_as(vp) if not dev else None, dev),
                L.sl2_last_error().decode())
    for kw, word in ((dict(ip=None), "null"), (dict(cp=None), "null"), (dict(v=None), "null views"), (dict(nseq=0), "nseq"), (dict(nseq=-2), "nseq"),
                     (dict(seq0=1), "batch"), (dict(seq0=-1), "batch"), (dict(seq0=2, nseq=1, nv=1), "batch"), (dict(nv=0), "nviews"),
                     (dict(v=three, nv=3), "nviews"), (dict(layers=32), "layers"), (dict(layers=-1), "layers"), (dict(st=bound - 1), "item_stride"),
                     (dict(st=e.scene_item_bound()), "item_stride"), (dict(ip=d_items.ptr + 4, dev=1, vptr=d_views.ptr), "aligned"),
                     (dict(ip=d_items.ptr, dev=1, vptr=d_views.ptr + 4), "aligned"), (dict(v=nan_view), "sequence 1: its view"),
                     (dict(v=inf_view), "sequence 0: its view"), (dict(v=nan_view[1:], nv=1), "sequences 0 .. 1: the view"),
                     (dict(v=nan_view, seq0=1, nseq=1, nv=1), None)):
        code, msg = items_rc(**kw)
        if word is None:          # the second view is not looked at with nviews == 1
            assert code == _lib.SL2_OK, msg
            cnt[:] = 0; buf[:] = 0; ext[:] = 0
            continue
        assert code == _lib.SL2_ERR_INVALID and "sl2_world_items: sequence" in msg and word in msg, (kw, msg)
    assert not cnt.any() and not buf.view(np.uint8).any() and not ext.any()
    def draw_rc(seq0=0, nseq=2, v=views, nv=2, w=W, h=H, bg=0, layers=ALL, op=out.ctypes.data, os_=3 * W * H):
        return (L.sl2_draw_world(e.h, seq0, nseq, v.ctypes.data_as(vp) if v is not None else None, nv, w, h, bg, layers, None, vp(op) if op else None, os_, 0),
                L.sl2_last_error().decode())
    for kw, word in ((dict(v=None), "null"), (dict(op=None), "null"), (dict(nseq=0), "nseq"), (dict(seq0=2), "batch"), (dict(nv=3, v=three), "nviews"),
                     (dict(layers=32), "layers"), (dict(w=0), "width"), (dict(h=32769), "height"), (dict(w=-4), "width"), (dict(bg=256), "background"),
                     (dict(bg=-1), "background"), (dict(os_=3 * W * H - 1), "out_stride"), (dict(v=nan_view), "sequence 1: its view")):
        code, msg = draw_rc(**kw)
        assert code == _lib.SL2_ERR_INVALID and "sl2_draw_world: sequence" in msg and word in msg, (kw, msg)
    assert (out == 7).all()
    code, msg = draw_rc()
    assert code == _lib.SL2_OK and not (out == 7).all()
    d_items.free()
    d_views.free()


def test_a_device_view_that_is_not_finite_lists_nothing_it_touches(shipped_scene):
    """A device-resident view cannot be looked at: NaN in its pose omits every item, an infinite focal length too; the count
    is 0, nothing is written, and the other sequence's list is untouched by it."""
    S = shipped_scene
    e = S["e"]
    L, vp = e.L, _lib.vp
    stride = e.world_item_bound()
    views = np.array([S["views"]["side"]] * 3, wc.VIEW)
    views[0]["r"][1] = np.nan
    views[2]["fku"] = np.inf
    good, _ = e.world_items(S["views"]["side"], 1, 1, ALL)
    bufs = [_lib.DeviceBuffer(n) for n in (64 * stride * 3, 12, views.nbytes)]
    bufs[0].upload(np.full(64 * stride * 3, SENTINEL, np.uint8))
    bufs[2].upload(views)
    _lib.check(L.sl2_world_items(e.h, 0, 3, vp(bufs[2].ptr), 3, ALL, None, vp(bufs[0].ptr), stride, vp(bufs[1].ptr), None, 1), L)
    counts = bufs[1].download((3,), np.int32)
    items = bufs[0].download((3, stride), oc.ITEM)
    assert counts[0] == 0 and counts[1] == good[0].size and items[1, :counts[1]].tobytes() == good[0].tobytes()
    assert (items[0].view(np.uint8) == SENTINEL).all()
    assert all(int(it["kind"]) != rc.RING or not oc.ring_valid(it["q"]) for it in items[2, :counts[2]])          # whatever is listed draws nothing finite
    for b in bufs:
        b.free()


def test_world_calls_between_replayed_steps_of_a_captured_graph():
    """set_graph_mode(1): world lists, drawings and picks in every form between the steps cost no capture, and the engine's
    state stays bit-identical to a twin that never draws."""
    T = _lib.load_testing()
    pr = Pair(12, 6, batch=2, n_select=6, make_engine=False)
    engines = [pr.make_engine_for(0, 2, 12) for _ in range(2)]
    for e in engines:
        e.set_graph_mode(True)
    W, H = pr.cam["width"], pr.cam["height"]
    fb = W * H
    V = wc.fixed_views(pr.cam)
    views = np.array([V["side"], V["reference"]], wc.VIEW)
    bufs = [_lib.DeviceBuffer(2 * fb) for _ in range(2)]
    d_out, d_views = _lib.DeviceBuffer(2 * 3 * 70 * 37), _lib.DeviceBuffer(views.nbytes)
    d_views.upload(views)
    for k in range(6):
        buf = bufs[k & 1]
        frames = np.ascontiguousarray(pr.frame_batch(k), dtype=np.uint8).reshape(2, H, W)
        buf.upload(frames)
        for e in engines:
            e.go_one_step(buf.ptr, on_device=True, seq_stride=fb, save_trajectory=True)
        e = engines[0]
        e.draw_world_device(d_views.ptr, 2, 70, 37, d_out.ptr, background=9)          # queued behind the step, no wait in between
        dev = d_out.download((2, 37, 70, 3), np.uint8)
        S = dict(e=e, states=states_of(e))
        check_world(S, 0, 2, views, ALL, np.array([k, -1], np.int32), size=(64, 32))
        assert np.array_equal(dev, e.draw_world(views, 70, 37, 0, 2, 9))
        lists, _ = e.world_items(views, 0, 2, ALL)
        world_view.pick_items(70, 37, lists, [(35, 18), (3, 3)])
        for q in engines:
            q.synchronize()
        assert T.sl2_debug_graph_captures(engines[0].h) == T.sl2_debug_graph_captures(engines[1].h) == min(k + 1, 2)
    a, b = engines[0].save_sequences(0, 2), engines[1].save_sequences(0, 2)
    assert [bytes(x) for x in a] == [bytes(x) for x in b]
    for d in bufs + [d_out, d_views]:
        d.free()
    for e in engines:
        e.close()


# ------------------------------------------------------------------------------------------------- the adapter
def test_monoslam_draw3dscene_and_picker():
    """MonoSLAM.Draw3dScene(view, out, width, height, trajectory, features, uncertainties): the camera is always drawn, the
    axes go with the features box; Picker answers label + 1 from the list of the last call, 0 where nothing lies."""
    from scenelib2_amd import MonoSLAM
    cam, params, spec, frames, templates = make_mapping_sequence(n_frames=8)
    m = MonoSLAM(max_features=16).InitFromValues(cam, params, spec.xv0, spec.Pxx0)
    xo = spec.xp_org()
    for i in range(spec.n_features):
        m.AddNewKnownFeature(spec.feat_y[i], xo[i], templates[i])
    for k in range(1, 5):
        m.GoOneStep(frames[k], save_trajectory=True)
    assert m.Picker(10, 10, True) == 0 and m.Picker(10, 10, False) == 0          # nothing drawn yet
    view = world_view.reference_view(cam)
    eng = m._engine
    m.marked_feature_label_ = 1
    W, H = 200, 150
    view = world_view.look_at(wc.REFERENCE_EYE, wc.REFERENCE_TARGET, wc.REFERENCE_UP, 120.0, 120.0, 100.0, 75.0)
    for t in (0, 1):
        for f in (0, 1):
            for u in (0, 1):
                layers = (wc.TRAJECTORY if t else 0) | (wc.FEATURES | wc.AXES if f else 0) | (wc.UNCERTAINTIES if u else 0) | wc.CAMERA
                out = np.zeros((H, W, 3), np.uint8)
                img = m.Draw3dScene(view, out, W, H, bool(t), bool(f), bool(u))
                want = eng.draw_world(view, W, H, 0, 1, 0, layers, [1])[0]
                assert np.array_equal(img, want) and np.array_equal(out, want), (t, f, u)
    assert m.Draw3dScene(view).shape == (cam["height"], cam["width"], 3)
    m.Draw3dScene(view, None, W, H, True, True, False)
    items = eng.world_items(view, 0, 1, wc.TRAJECTORY | wc.FEATURES | wc.AXES | wc.CAMERA)[0][0]
    marks = [it for it in items if int(it["kind"]) == rc.RECT and it["a"][0] == it["a"][2] and 0 <= it["a"][0] < W and 0 <= it["a"][1] < H]
    assert marks
    for it in marks:
        x, y = int(it["a"][0]), int(it["a"][1])
        name = m.Picker(x, y, True)
        assert name == world_view.pick_items_host(W, H, items, x, y)[0] + 1 >= 1
    assert m.Picker(0, H - 1, True) == world_view.pick_items_host(W, H, items, 0, H - 1)[0] + 1
    assert m.Picker(-5, 3, True) == 0
    # the reference's reading: mark what was clicked, then delete it
    name = m.Picker(int(marks[0]["a"][0]), int(marks[0]["a"][1]), True)
    m.mark_feature_by_lab(name - 1)
    assert m.marked_feature_label_ == name - 1 and m.delete_feature()
    assert all(f.label_ != name - 1 for f in m.feature_list_)
    # the 2-D picker works on the list of the last DrawAR call
    m.DrawAR(frames[4], None, True, True, True, False)
    scene = eng.scene_items(0, 1, rc.TRAJECTORY | rc.FEATURES)[0]
    mk = [it for it in scene if int(it["kind"]) == rc.RECT and it["a"][0] == it["a"][2]][0]
    assert m.Picker(int(mk["a"][0]), int(mk["a"][1]), False) == world_view.pick_items_host(cam["width"], cam["height"], scene, int(mk["a"][0]), int(mk["a"][1]))[0] + 1 >= 1
    m.DrawAR(frames[4], None, False)
    raw = eng.overlay_items(0, 1, 7)[0]
    pt = [it for it in raw if int(it["kind"]) == oc.PATCH][0]
    assert m.Picker(int(pt["a"][0]), int(pt["a"][1]), False) == world_view.pick_items_host(cam["width"], cam["height"], raw, int(pt["a"][0]), int(pt["a"][1]), npatches=16)[0] + 1 >= 1
