"""The rectified view on the device (include/scenelib2_amd.h, "the rectified view").

The line primitive: the segment cases of rectified_cases.py through sl2_draw_items_batch, a whole size a launch, in every
residency and with strides above the minimum - byte-equal to sl2_draw_items_host (which tests/test_rectified_host.py holds to
a NumPy restatement of the header's rule).

The undistorted frame: the remap cases through sl2_rectify_frames, EVERY case of a size a sequence of one engine with its own
camera (sl2_set_cameras) in one call, in every residency and with padded strides - byte-equal to sl2_rectify_frame_host.
sl2_create takes no image below 22 rows, so the 64 x 16 cases run at 64 x 32: still one tile wide, two tiles high, with rows
that go out as dwords (70 x 37 has the remainders on both axes and rows that do not).

The scene: sl2_scene_items against rectified_cases.scene_list, a builder that works ONLY from public accessors (total state,
total covariance, features, trajectory, cameras) in the header's order of operations - every field exact, q included - on the
shipped four-feature scene and a mapping scene with a partial feature in flight; sl2_draw_rectified against
sl2_rectify_frame_host followed by sl2_draw_items_host on the device's own list."""
import numpy as np
import pytest

import display_helpers as dh
import overlay_cases as oc
import rectified_cases as rc
from display_helpers import SENTINEL, assert_images, assert_lists_equal, engine_state
from scenelib2_amd import Engine, _lib, overlay, rectified, synth
from slam_helpers import Pair

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------- the line primitive
@pytest.fixture(scope="module")
def seg_batches():
    out = {}
    for name, (w, h), items, patches in rc.SEGMENT_CASES:
        g = out.setdefault((w, h), dict(names=[], frames=[], lists=[], patches=None))
        g["names"].append(name)
        g["frames"].append(oc.frame_of(w, h, seed=len(name)))
        g["lists"].append(oc.items_array(items))
        if patches is not None:
            g["patches"] = patches
    for g in out.values():
        g["want"] = np.stack([overlay.draw_items_host(f, l, g["patches"]) for f, l in zip(g["frames"], g["lists"])])
        g["frames"] = np.stack(g["frames"])
    return out


def _draw(g, w, h, *residency, **pads):
    """(A host-resident list with an item of unknown kind is refused, tests/test_rectified_host.py: that case goes by device lists.)"""
    return dh.draw_items_batch(g, w, h, *residency, filler=rc.segment(0, 0, w - 1, h - 1, oc.GREEN), refused_prefix="seg_other_kinds", **pads)


@pytest.mark.parametrize("size", rc.SIZES)
@pytest.mark.parametrize("residency", ["host", "device", "frames_on_device", "lists_and_out_on_device"])
def test_segment_cases_equal_the_host_form(seg_batches, size, residency):
    w, h = size
    fd, idv, od = dict(host=(0, 0, 0), device=(1, 1, 1), frames_on_device=(1, 0, 0), lists_and_out_on_device=(0, 1, 1))[residency]
    assert_images(_draw(seg_batches[size], w, h, fd, idv, od))


@pytest.mark.parametrize("size", rc.SIZES)
def test_segment_cases_with_strides_above_the_minimum(seg_batches, size):
    w, h = size
    for res in ((1, 1, 1), (0, 0, 0)):
        for pads in ((13, 3, 7), (4, 1, 4)):
            assert_images(_draw(seg_batches[size], w, h, *res, seq_pad=pads[0], item_pad=pads[1], out_pad=pads[2]))


# ------------------------------------------------------------------------------------------------- the undistorted frame
GPU_SIZES = ((70, 37), (64, 32))


def _remap_cases(size):
    """The cases of rectified_cases.py for this size; 64 x 32 takes the principal points and coefficients of 64 x 16."""
    w, h = size
    src = (64, 16) if size == (64, 32) else size
    return [(name, (u0, v0), kd1) for name, s, (u0, v0), kd1 in rc.REMAP_CASES if s == src]


@pytest.fixture(scope="module", params=GPU_SIZES, ids=["%dx%d" % s for s in GPU_SIZES])
def remap_engine(request):
    """An engine with one sequence per remap case, each with the case's camera, and the host form's images."""
    w, h = request.param
    cases = _remap_cases(request.param)
    assert len(cases) == 15
    base = dict(width=w, height=h, fku=60.0, fkv=60.0, u0=w / 2.0, v0=h / 2.0, kd1=0.0, sd=1)
    e = Engine(base, synth.default_params(4), len(cases) + 2, 8)
    cams = [dict(base, u0=u0, v0=v0, kd1=kd1) for _, (u0, v0), kd1 in cases]
    e.set_cameras(cams, seq0=1)          # sequence 0 and the last one keep the engine's camera (kd1 = 0)
    frames = np.stack([rc.remap_frame(w, h, seed=k) for k in range(len(cases) + 2)])
    want = np.stack([frames[0]] + [rectified.rectify_frame_host(frames[1 + k], u0, v0, kd1) for k, (_, (u0, v0), kd1) in enumerate(cases)] + [frames[-1]])
    yield dict(e=e, w=w, h=h, names=["engine_camera"] + [c[0] for c in cases] + ["engine_camera"], frames=frames, want=want)
    e.close()


def _rectify(R, seq0, nseq, frames_dev, out_dev, seq_pad=0, out_pad=0):
    e, w, h = R["e"], R["w"], R["h"]
    L = _lib.load()
    seq_stride, out_stride = w * h + seq_pad, w * h + out_pad
    frames = np.full((nseq, seq_stride), 77, np.uint8)
    frames[:, :w * h] = R["frames"][seq0:seq0 + nseq].reshape(nseq, -1)
    out = np.full((nseq, out_stride), SENTINEL, np.uint8)
    bufs = []
    def dev(a):
        b = _lib.DeviceBuffer(a.nbytes)
        b.upload(a)
        bufs.append(b)
        return b
    fp = dev(frames).ptr if frames_dev else frames.ctypes.data
    dout = dev(out) if out_dev else None
    op = dout.ptr if out_dev else out.ctypes.data
    vp = _lib.vp
    _lib.check(L.sl2_rectify_frames(e.h, seq0, nseq, vp(fp), seq_stride, int(frames_dev), vp(op), out_stride, int(out_dev)), L)
    if out_dev:
        out = dout.download(out.shape, np.uint8)          # (a blocking copy on the null stream: behind the launch)
    for b in bufs:
        b.free()
    assert (out[:, w * h:] == SENTINEL).all(), "bytes between the images were written"
    return out[:, :w * h].reshape(nseq, h, w)


def _assert_frames(R, got, seq0):
    for i in range(len(got)):
        want = R["want"][seq0 + i]
        assert np.array_equal(got[i], want), (R["names"][seq0 + i], np.argwhere(got[i] != want)[:5].tolist())


@pytest.mark.parametrize("residency", ["host", "device", "frames_on_device", "out_on_device"])
def test_remap_cases_equal_the_host_form_each_sequence_with_its_own_camera(remap_engine, residency):
    R = remap_engine
    fd, od = dict(host=(0, 0), device=(1, 1), frames_on_device=(1, 0), out_on_device=(0, 1))[residency]
    n = len(R["names"])
    got = _rectify(R, 0, n, fd, od)
    _assert_frames(R, got, 0)
    # (the cameras differ in what they give; a principal point far outside with kd1 < 0 leaves nothing but border, more than once)
    assert len({g.tobytes() for g in got}) >= n - 4


def test_remap_with_strides_above_the_minimum_and_late_ranges(remap_engine):
    """Strides that keep the dword stores (pads of 4) and ones that do not, and ranges that do not begin at sequence 0: the
    camera is that of sequence seq0 + i, the image that of index i."""
    R = remap_engine
    n = len(R["names"])
    for res in ((1, 1), (0, 0)):
        for pads in ((13, 7), (4, 4), (1, 2)):
            _assert_frames(R, _rectify(R, 0, n, *res, seq_pad=pads[0], out_pad=pads[1]), 0)
        _assert_frames(R, _rectify(R, 5, 3, *res), 5)
        _assert_frames(R, _rectify(R, n - 1, 1, *res), n - 1)
    e = R["e"]
    assert np.array_equal(e.rectify_frames(R["frames"][3:9], 3, 6), R["want"][3:9])          # the Python wrapper
    d_in, d_out = _lib.DeviceBuffer(R["frames"].nbytes), _lib.DeviceBuffer(R["frames"].nbytes)
    d_in.upload(R["frames"])
    e.rectify_frames_device(d_in.ptr, d_out.ptr)
    assert np.array_equal(d_out.download(R["frames"].shape, np.uint8), R["want"])
    d_in.free()
    d_out.free()


def test_rectify_refusals_queue_nothing(remap_engine):
    R = remap_engine
    e, w, h = R["e"], R["w"], R["h"]
    L = _lib.load()
    n = len(R["names"])
    f = np.ascontiguousarray(R["frames"][:2])
    out = np.full((2, w * h), 7, np.uint8)
    vp = _lib.vp
    call = lambda seq0=0, nseq=2, fp=f.ctypes.data, ss=w * h, op=out.ctypes.data, os_=w * h: (
        L.sl2_rectify_frames(e.h, seq0, nseq, vp(fp) if fp else None, ss, 0, vp(op) if op else None, os_, 0), L.sl2_last_error().decode())
    for kw, word in ((dict(fp=None), "null"), (dict(op=None), "null"), (dict(nseq=0), "nseq"), (dict(nseq=-1), "nseq"), (dict(seq0=-1), "batch"),
                     (dict(seq0=n - 1), "batch"), (dict(seq0=n), "batch"), (dict(ss=w * h - 1), "seq_stride"), (dict(os_=w * h - 1), "out_stride")):
        code, msg = call(**kw)
        assert code == _lib.SL2_ERR_INVALID and "sl2_rectify_frames: sequences" in msg and word in msg, (kw, msg)
    assert (out == 7).all()
    assert call()[0] == _lib.SL2_OK and np.array_equal(out.reshape(2, h, w), R["want"][:2])


def test_rectify_between_replayed_steps_of_a_captured_graph():
    """set_graph_mode(1), device frames in two alternating buffers: rectify calls in every form between the steps, and a camera
    change on the way, cost no capture; the warp uses the cameras as the setters queued so far leave them, and the engine's
    state stays bit-identical to a twin that never rectifies."""
    T = _lib.load_testing()
    pr = Pair(12, 6, batch=2, n_select=6, make_engine=False)
    engines = [pr.make_engine_for(0, 2, 12) for _ in range(2)]
    for e in engines:
        e.set_graph_mode(True)
    W, H = pr.cam["width"], pr.cam["height"]
    fb = W * H
    bufs = [_lib.DeviceBuffer(2 * fb) for _ in range(2)]
    d_out = _lib.DeviceBuffer(2 * fb)
    for k in range(6):
        buf = bufs[k & 1]
        frames = np.ascontiguousarray(pr.frame_batch(k), dtype=np.uint8).reshape(2, H, W)
        buf.upload(frames)
        for e in engines:
            e.go_one_step(buf.ptr, on_device=True, seq_stride=fb, save_trajectory=True)
            if k == 2:
                e.set_cameras([dict(pr.cam, kd1=-3e-6, u0=150.5)], seq0=1)
        e = engines[0]
        e.rectify_frames_device(buf.ptr, d_out.ptr)          # queued behind the step, no wait in between
        dev = d_out.download((2, H, W), np.uint8)
        cams = e.get_cameras()
        want = np.stack([rectified.rectify_frame_host(frames[b], cams[b]["u0"], cams[b]["v0"], cams[b]["kd1"]) for b in range(2)])
        assert np.array_equal(dev, want) and not np.array_equal(dev, frames)
        assert np.array_equal(e.rectify_frames(buf.ptr, on_device=True), want) and np.array_equal(e.rectify_frames(frames), want)
        for q in engines:
            q.synchronize()
        assert T.sl2_debug_graph_captures(engines[0].h) == T.sl2_debug_graph_captures(engines[1].h) == min(k + 1, 2)
    assert cams[1]["kd1"] == -3e-6 and cams[0]["kd1"] == pr.cam["kd1"] != 0.0
    a, b = engines[0].save_sequences(0, 2), engines[1].save_sequences(0, 2)
    assert [bytes(x) for x in a] == [bytes(x) for x in b]
    for d in bufs + [d_out]:
        d.free()
    for e in engines:
        e.close()


# ------------------------------------------------------------------------------------------------- the scene lists
TRAJ, FEAT, UNC = rectified.SL2_SCENE_TRAJECTORY, rectified.SL2_SCENE_FEATURES, rectified.SL2_SCENE_UNCERTAINTIES


def check_scene(e, frames, seq0, nseq, layers, marked=None, draw=True):
    """sl2_scene_items against the builder (every field, no skips: asserted); sl2_draw_rectified against sl2_rectify_frame_host
    followed by sl2_draw_items_host on the device's own list."""
    lists = e.scene_items(seq0, nseq, layers, marked)
    built = []
    for i in range(nseq):
        want, rounded = rc.scene_list(engine_state(e, seq0 + i), layers, -1 if marked is None else int(marked[i]))
        assert rc.skipped_fields(rounded) == 0, "a rounded coordinate lies within 1e-6 of a half-integer: choose another scene"
        assert_lists_equal(lists[i], want, "sequence %d, layers %d" % (seq0 + i, layers))
        assert want.size <= e.scene_item_bound()
        built.append(want)
    if draw:
        imgs = e.draw_rectified(frames[seq0:seq0 + nseq], seq0, nseq, layers, marked)
        cams = e.get_cameras(seq0, nseq)
        for i in range(nseq):
            grey = rectified.rectify_frame_host(frames[seq0 + i], cams[i]["u0"], cams[i]["v0"], cams[i]["kd1"])
            host = overlay.draw_items_host(grey, lists[i], None)
            assert np.array_equal(imgs[i], host), (seq0 + i, layers, np.argwhere((imgs[i] != host).any(axis=2))[:5].tolist())
    return built


@pytest.fixture(scope="module")
def shipped_scene():
    """display_helpers.shipped_scene with three cameras' worth of distortion for the frame (the scene's projection uses fku, fkv,
    u0, v0 alone)."""
    for e, pr in dh.shipped_scene():
        e.set_cameras([dict(pr.cam, kd1=4e-5), dict(pr.cam, kd1=-2e-5, u0=150.25)], seq0=1)
        yield dict(e=e, frames=pr.frame_batch(dh.SHIPPED_STEPS - 1), pr=pr)


@pytest.fixture(scope="module")
def mapping_scene():
    for e, frames, cam in dh.mapping_scene():
        yield dict(e=e, frames=frames, cam=cam)


@pytest.fixture(scope="module")
def large_map():
    for e, state, cam in dh.large_map():
        yield dict(e=e, cam=cam)


def test_scene_lists_of_the_shipped_scene(shipped_scene):
    e, frames = shipped_scene["e"], shipped_scene["frames"]
    built = check_scene(e, frames, 0, 3, TRAJ | FEAT | UNC, np.array([1, -1, 3], np.int32))
    kinds = [b["kind"].tolist() for b in built]
    assert kinds[0] == [rc.RECT, rc.RECT, rc.RING] * 4          # (its trajectory lies behind it: tests/test_rectified_host.py)
    assert kinds[1][:dh.SHIPPED_STEPS - 1] == [rc.SEGMENT] * (dh.SHIPPED_STEPS - 1) and kinds[1].count(rc.RING) == 4
    assert tuple(built[0][built[0]["label"] == 1][0]["rgb"]) == oc.GREEN and tuple(built[2][built[2]["label"] == 3][-1]["rgb"]) == oc.GREEN
    assert all(oc.ring_valid(it["q"]) for b in built for it in b if int(it["kind"]) == rc.RING)


def test_large_map_two_rounds_of_slots(large_map):
    """70 fully initialised features with proper ellipsoids, one sequence: a second round of 64 slots with 6 live lanes, placed
    behind the first in slot order."""
    e, cam = large_map["e"], large_map["cam"]
    frames = oc.frame_of(cam["width"], cam["height"], seed=5)[None]
    b = check_scene(e, frames, 0, 1, TRAJ | FEAT | UNC, np.array([66], np.int32))[0]
    kinds = b["kind"].tolist()
    assert kinds.count(rc.RECT) == 140 and kinds.count(rc.RING) >= 60 and kinds.count(rc.SEGMENT) == 0
    assert [int(it["label"]) for it in b if int(it["kind"]) == rc.RECT][::2] == list(range(70))          # slot order across the two rounds
    assert all(oc.ring_valid(it["q"]) for it in b if int(it["kind"]) == rc.RING)
    assert tuple(b[b["label"] == 66][0]["rgb"]) == oc.GREEN and tuple(b[b["label"] == 65][0]["rgb"]) == oc.YELLOW
    check_scene(e, frames, 0, 1, UNC, draw=False)


@pytest.mark.parametrize("layers", range(8))
def test_every_subset_of_the_layers(shipped_scene, mapping_scene, layers):
    check_scene(shipped_scene["e"], shipped_scene["frames"], 0, 3, layers, draw=layers in (0, 5))
    built = check_scene(mapping_scene["e"], mapping_scene["frames"], 0, 2, layers, np.array([-1, 2], np.int32), draw=layers in (2, 7))
    if layers == 0:
        assert all(b.size == 0 for b in built)
    if layers & FEAT:
        assert all(any(int(it["kind"]) == rc.SEGMENT and int(it["label"]) >= 0 for it in b) for b in built), "no ray of a partial feature"
    if layers == UNC:
        assert all(set(b["kind"].tolist()) == {rc.RING} for b in built)


def test_late_seq0_paused_sequence_and_groups(shipped_scene, mapping_scene):
    e, frames = shipped_scene["e"], shipped_scene["frames"]
    check_scene(e, frames, 2, 1, 7, np.array([0], np.int32))
    check_scene(e, frames, 1, 2, 7)
    e.set_active([0, 1, 0])          # the mask is not consulted: a paused sequence is listed like any other
    check_scene(e, frames, 0, 3, 7)
    e.set_active([1, 1, 1])
    m = mapping_scene["e"]
    m.set_groups(2)
    try:
        check_scene(m, mapping_scene["frames"], 0, 2, 7)
        check_scene(m, mapping_scene["frames"], 1, 1, 7, np.array([3], np.int32))
    finally:
        m.set_groups(1)


def test_camera_turned_away_and_trajectory_across_the_near_plane():
    """Its own engine (the state is overwritten).  trajectory_store_ holds the stale rRES_ of the reference: the
    place the LAST feature of the list was first seen from.  Four known features first seen from four places along the viewing
    axis, the last one deleted after every step: the store runs from 0.3 m behind the camera to 0.15 m and 0.3 m in front of
    it, so its first segment crosses the near plane and is cut at X[2] = 0.01.  Then sequence 0 is put behind the whole store and
    turned by half a turn about y: every feature and the whole trajectory lie behind it - every item omitted, count 0."""
    pr = Pair(4, 4, batch=2, make_engine=False)
    e = Engine(pr.cam, pr.params, 2, 4)
    e.set_vehicle_state(np.stack([s.xv0 for s in pr.specs]), np.stack([s.Pxx0 for s in pr.specs]))
    for b, spec in enumerate(pr.specs):
        xo = np.tile(spec.poses[0], (4, 1))
        xo[:, 2] += (0.0, 0.3, 0.15, -0.3)
        xo[:, 0] += 0.02 * np.arange(4)
        e.add_known_features(spec.feat_y[None], xo[None], pr.templates[b][None], seq0=b)
    for k in range(3):
        e.go_one_step(pr.frame_batch(k), save_trajectory=True)
        assert e.delete_features([3 - k, 3 - k]).all()
    frames = pr.frame_batch(2)
    traj = e.trajectory(0)
    cf = np.array([rc.zeroed_jac(e.total_state(0)[:7], t)[0] for t in traj])
    assert len(traj) == 3 and cf[0, 2] < rc.NEAR < cf[1, 2] < cf[2, 2], cf.tolist()
    built = check_scene(e, frames, 0, 2, 7)
    assert built[0]["kind"].tolist() == [rc.SEGMENT, rc.SEGMENT, rc.RECT, rc.RECT, rc.RING]          # both segments, the one feature left
    cut, whole = built[0][0]["a"], built[0][1]["a"]
    assert tuple(cut[2:]) == tuple(whole[:2])          # the cut segment ends where the next begins ...
    p = rc.project(e.get_cameras(0, 1)[0], cf[1])
    assert tuple(cut[2:]) == (rc.c_round(p[0]), rc.c_round(p[1])) and np.abs(cut[:2] - cut[2:]).max() > 100          # ... and starts far out, on the near plane
    xv, Pxx = e.get_vehicle_state(0, 2)
    xv[0, 0:3] = [0.0, 0.0, -1.0]          # sequence 0 steps back behind the whole store and looks the other way; sequence 1 stays
    xv[0, 3:7] = [0.0, 0.0, 1.0, 0.0]
    e.set_vehicle_state(xv, Pxx)
    built = check_scene(e, frames, 0, 2, 7)
    assert built[0].size == 0 and built[1].size == 5
    assert [len(l) for l in e.scene_items(0, 2, 7)] == [0, 5]
    img = e.draw_rectified(frames, 0, 2, 7)
    cam = e.get_cameras(0, 1)[0]
    grey = rectified.rectify_frame_host(frames[0], cam["u0"], cam["v0"], cam["kd1"])
    assert np.array_equal(img[0], np.repeat(grey[:, :, None], 3, axis=2))          # nothing drawn: the rectified frame alone
    e.close()


def test_scene_residency_refusals_and_the_rasteriser_takes_the_lists(mapping_scene):
    e, frames = mapping_scene["e"], mapping_scene["frames"]
    L = _lib.load()
    vp = _lib.vp
    stride = e.scene_item_bound() + 3
    host = e.scene_items(0, 2, 7, np.array([2, -1], np.int32))
    # device form: items, counts and marked on the device, one launch, no wait; strides above the bound
    d_items, d_counts, d_marked = _lib.DeviceBuffer(64 * stride * 2), _lib.DeviceBuffer(8), _lib.DeviceBuffer(8)
    d_items.upload(np.full(64 * stride * 2, SENTINEL, np.uint8))
    d_marked.upload(np.array([2, -1], np.int32))
    _lib.check(L.sl2_scene_items(e.h, 0, 2, 7, vp(d_marked.ptr), vp(d_items.ptr), stride, vp(d_counts.ptr), 1), L)
    counts = d_counts.download((2,), np.int32)
    items = d_items.download((2, stride), oc.ITEM)
    for i in range(2):
        assert counts[i] == host[i].size and items[i, :counts[i]].tobytes() == host[i].tobytes()
        assert (items[i, counts[i]:].view(np.uint8) == SENTINEL).all()          # nothing behind the list was written
    # sl2_draw_items_batch accepts the lists as they are, host- and device-resident
    W, H = mapping_scene["cam"]["width"], mapping_scene["cam"]["height"]
    want = np.stack([overlay.draw_items_host(frames[i], host[i], None) for i in range(2)])
    assert np.array_equal(overlay.draw_items(frames, host, None), want)
    d_f, d_o = _lib.DeviceBuffer(frames.nbytes), _lib.DeviceBuffer(want.nbytes)
    d_f.upload(frames)
    _lib.check(L.sl2_draw_items_batch(0, None, vp(d_f.ptr), 1, 2, W, H, W * H, vp(d_items.ptr), stride, vp(d_counts.ptr), 1, None, 0, 0, vp(d_o.ptr),
                                      3 * W * H, 1), L)
    assert np.array_equal(d_o.download(want.shape, np.uint8), want)
    # sl2_draw_rectified, device form, equals its host form
    e.draw_rectified_device(d_f.ptr, d_o.ptr, layers=7, marked_ptr=d_marked.ptr)
    assert np.array_equal(d_o.download(want.shape, np.uint8), e.draw_rectified(frames, 0, 2, 7, np.array([2, -1], np.int32)))
    assert np.array_equal(e.draw_rectified(d_f.ptr, 0, 2, 7, on_device=True), e.draw_rectified(frames, 0, 2, 7))
    # refusals: nothing queued, the message names the sequences
    cnt = np.zeros(2, np.int32)
    buf = np.zeros((2, stride), oc.ITEM)
    out = np.full((2, 3 * W * H), 7, np.uint8)
    def items_rc(seq0=0, nseq=2, layers=7, ip=buf.ctypes.data, st=stride, cp=cnt.ctypes.data, dev=0):
        return L.sl2_scene_items(e.h, seq0, nseq, layers, None, vp(ip) if ip else None, st, vp(cp) if cp else None, dev), L.sl2_last_error().decode()
    for kw, word in ((dict(ip=None), "null"), (dict(cp=None), "null"), (dict(nseq=0), "nseq"), (dict(seq0=1), "batch"), (dict(seq0=-1), "batch"),
                     (dict(layers=8), "layers"), (dict(layers=-1), "layers"), (dict(st=e.scene_item_bound() - 1), "item_stride"),
                     (dict(ip=d_items.ptr + 4, dev=1), "aligned")):
        code, msg = items_rc(**kw)
        assert code == _lib.SL2_ERR_INVALID and "sl2_scene_items: sequences" in msg and word in msg, (kw, msg)
    def draw_rc(seq0=0, nseq=2, layers=7, fp=frames.ctypes.data, ss=W * H, op=out.ctypes.data, os_=3 * W * H):
        return (L.sl2_draw_rectified(e.h, seq0, nseq, vp(fp) if fp else None, ss, 0, layers, None, vp(op) if op else None, os_, 0),
                L.sl2_last_error().decode())
    for kw, word in ((dict(fp=None), "null"), (dict(op=None), "null"), (dict(nseq=0), "nseq"), (dict(seq0=2), "batch"), (dict(layers=16), "layers"),
                     (dict(ss=W * H - 1), "seq_stride"), (dict(os_=3 * W * H - 1), "out_stride")):
        code, msg = draw_rc(**kw)
        assert code == _lib.SL2_ERR_INVALID and "sl2_draw_rectified: sequences" in msg and word in msg, (kw, msg)
    assert (out == 7).all() and not cnt.any() and not buf.view(np.uint8).any()
    for d in (d_items, d_counts, d_marked, d_f, d_o):
        d.free()


def test_scene_calls_between_replayed_steps_of_a_captured_graph():
    """set_graph_mode(1): scene lists and rectified drawings in every form between the steps cost no capture, and the engine's
    state stays bit-identical to a twin that never draws."""
    T = _lib.load_testing()
    pr = Pair(12, 6, batch=2, n_select=6, make_engine=False)
    engines = [pr.make_engine_for(0, 2, 12) for _ in range(2)]
    for e in engines:
        e.set_graph_mode(True)
    W, H = pr.cam["width"], pr.cam["height"]
    fb = W * H
    bufs = [_lib.DeviceBuffer(2 * fb) for _ in range(2)]
    d_out = _lib.DeviceBuffer(2 * 3 * fb)
    for k in range(6):
        buf = bufs[k & 1]
        frames = np.ascontiguousarray(pr.frame_batch(k), dtype=np.uint8).reshape(2, H, W)
        buf.upload(frames)
        for e in engines:
            e.go_one_step(buf.ptr, on_device=True, seq_stride=fb, save_trajectory=True)
        e = engines[0]
        e.draw_rectified_device(buf.ptr, d_out.ptr)          # queued behind the step, no wait in between
        dev = d_out.download((2, H, W, 3), np.uint8)
        check_scene(e, frames, 0, 2, 7, np.array([k, -1], np.int32))
        assert np.array_equal(dev, e.draw_rectified(frames, 0, 2, 7))
        for q in engines:
            q.synchronize()
        assert T.sl2_debug_graph_captures(engines[0].h) == T.sl2_debug_graph_captures(engines[1].h) == min(k + 1, 2)
    a, b = engines[0].save_sequences(0, 2), engines[1].save_sequences(0, 2)
    assert [bytes(x) for x in a] == [bytes(x) for x in b]
    for d in bufs + [d_out]:
        d.free()
    for e in engines:
        e.close()
