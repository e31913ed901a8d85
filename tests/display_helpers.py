"""What the GPU tests of the three display views (annotated frames, the rectified view, the world view) share: the driver of
sl2_draw_items_batch, the comparisons, the public state of a sequence, and the scenes - as plain generator functions; each test
module keeps its own fixture around them.  The scenes' constants are also what the host tests run through the CPU oracle, to show
that no rounded coordinate of theirs lies at a half-integer."""
import numpy as np

import overlay_cases as oc
import world_view_cases as wc
from mapping_helpers import make_mapping_sequence
from scenelib2_amd import Engine, _lib, synth
from slam_helpers import Pair

SENTINEL = 0xA5
SHIPPED_STEPS = 5          # the shipped four-feature scene (slam_helpers.Pair(4, ...)) after this many steps, trajectory saved
MAPPING_SEED, MAPPING_KNOWN, MAPPING_FRAMES, MAPPING_MAX_FEATURES = 7, 12, 24, 24          # mapping_helpers.make_mapping_sequence


# ------------------------------------------------------------------------------------------------- the rasteriser
def draw_items_batch(g, w, h, frames_dev, items_dev, out_dev, filler, refused_prefix, seq_pad=0, item_pad=0, out_pad=0):
    """One sl2_draw_items_batch call over a whole group g (names, frames, lists, patches, want); returns (the group drawn, its
    images [n][h][w][3]) after checking the guard bytes.  `filler` is the item put behind every list's count: it is not part of
    the list.  A host-resident list with a bad item is refused (the host tests), so the cases whose names start with
    `refused_prefix` go by device lists only."""
    L = _lib.load()
    if not items_dev:
        keep = [i for i, name in enumerate(g["names"]) if not name.startswith(refused_prefix)]
        g = dict(names=[g["names"][i] for i in keep], lists=[g["lists"][i] for i in keep], frames=g["frames"][keep], want=g["want"][keep],
                 patches=g["patches"])
    n = len(g["lists"])
    seq_stride, out_stride = w * h + seq_pad, 3 * w * h + out_pad
    stride = max(a.size for a in g["lists"]) + item_pad
    items = np.zeros((n, stride), oc.ITEM)
    counts = np.zeros(n, np.int32)
    for i, a in enumerate(g["lists"]):
        items[i, :a.size] = a
        items[i, a.size:] = filler
        counts[i] = a.size
    frames = np.full((n, seq_stride), 77, np.uint8)
    frames[:, :w * h] = g["frames"].reshape(n, -1)
    out = np.full((n, out_stride), SENTINEL, np.uint8)
    P = g["patches"]
    bufs = []
    def dev(a):
        b = _lib.DeviceBuffer(a.nbytes)
        b.upload(a)
        bufs.append(b)
        return b
    fp = dev(frames).ptr if frames_dev else frames.ctypes.data
    ip, cp, pp = (dev(items).ptr, dev(counts).ptr, dev(P).ptr) if items_dev else (items.ctypes.data, counts.ctypes.data, P.ctypes.data)
    dout = dev(out) if out_dev else None
    op = dout.ptr if out_dev else out.ctypes.data
    vp = _lib.vp
    _lib.check(L.sl2_draw_items_batch(0, None, vp(fp), int(frames_dev), n, w, h, seq_stride, vp(ip), stride, vp(cp), int(items_dev), vp(pp),
                                      P.shape[1], P.shape[0], vp(op), out_stride, int(out_dev)), L)
    if out_dev:
        out = dout.download(out.shape, np.uint8)          # (a blocking copy on the null stream: behind the launch)
    for b in bufs:
        b.free()
    assert (out[:, 3 * w * h:] == SENTINEL).all(), "bytes between the images were written"
    return g, out[:, :3 * w * h].reshape(n, h, w, 3)


def assert_images(g_got):
    g, got = g_got
    assert len(got) == len(g["names"]) > 20
    for i, name in enumerate(g["names"]):
        assert np.array_equal(got[i], g["want"][i]), (name, np.argwhere((got[i] != g["want"][i]).any(axis=2))[:5].tolist())


# ------------------------------------------------------------------------------------------------- the lists
def assert_lists_equal(got, want, what):
    assert got.size == want.size, (what, got.size, want.size, got["kind"].tolist(), want["kind"].tolist())
    for name in ("kind", "label", "a", "patch", "rgb", "pad"):
        assert np.array_equal(got[name], want[name]), (what, name, got[name].tolist(), want[name].tolist())
    # the headers fix the order of every operation behind q, so equality is exact
    assert got["q"].tobytes() == want["q"].tobytes(), (what, "q", got["q"].tolist(), want["q"].tolist())


def engine_state(e, seq):
    """What rectified_cases.scene_list and world_view_cases.world_list want, from public accessors only.  (A partial feature's six
    states are the entries of the total state at its place in feature_list_ order.)"""
    feats = [dict(label=f["label"], full=f["fully_initialised"], size=f["state_size"], selected=f["selected"], success=f["success"])
             for f in e.features(seq)]
    return dict(cam=e.get_cameras(seq, 1)[0], x=e.total_state(seq), P=e.total_covariance(seq), feats=feats, traj=e.trajectory(seq))


# ------------------------------------------------------------------------------------------------- the scenes
def shipped_scene():
    """The shipped four-feature scene after a few steps, batch 3.  Sequence 1 is then seen from half a metre further back, so that
    its trajectory lies in front of it; sequence 2 sits out the last step.  Yields (engine, pair) and closes the engine."""
    pr = Pair(4, SHIPPED_STEPS + 1, batch=3)
    e = pr.engine
    for k in range(SHIPPED_STEPS):
        if k == SHIPPED_STEPS - 1:
            e.set_active([1, 1, 0])
        e.go_one_step(pr.frame_batch(k), save_trajectory=True)
    e.set_active([1, 1, 1])
    xv, Pxx = e.get_vehicle_state(1, 1)
    xv[0, 2] -= 0.5
    e.set_vehicle_state(xv, Pxx, seq0=1)
    yield e, pr
    e.close()


def mapping_scene():
    """The mapping scene stepped until a partially initialised feature is in flight in both sequences (asserted), batch 2;
    sequence 1 has one feature deleted by hand on the way, so that the two maps and lists differ.  Yields (engine, the frames last
    shown, camera) and closes the engine."""
    cam, params, spec, frames, templates = make_mapping_sequence(seed=MAPPING_SEED, n_known=MAPPING_KNOWN, n_frames=MAPPING_FRAMES)
    B = 2
    e = Engine(cam, params, B, MAPPING_MAX_FEATURES)
    e.set_vehicle_state(np.tile(spec.xv0, (B, 1)), np.tile(spec.Pxx0, (B, 1, 1)))
    e.add_known_features(np.tile(spec.feat_y, (B, 1, 1)), np.tile(spec.xp_org(), (B, 1, 1)), np.tile(templates, (B, 1, 1, 1)))
    last = 0
    for k in range(1, MAPPING_FRAMES):
        if k == 6:
            assert e.delete_features([-1, 2])[1]
        e.go_one_step(np.tile(frames[k], (B, 1, 1)), save_trajectory=True, enable_mapping=True)
        last = k
        if k >= 8 and all(any(not f["fully_initialised"] for f in e.features(b)) for b in range(B)):
            break
    assert all(any(not f["fully_initialised"] for f in e.features(b)) for b in range(B)), "no partial feature in flight"
    yield e, np.tile(frames[last], (B, 1, 1)), cam
    e.close()


def large_map():
    """70 known features, never stepped, random positive definite Pyy (world_view_cases.large_map): one sequence, two rounds of
    64 slots, the second with 6 live lanes.  Yields (engine, its public state, camera) and closes the engine."""
    m = wc.large_map()
    cam = synth.default_camera()
    e = Engine(cam, synth.default_params(4), 1, 70)
    e.set_vehicle_state(m["xv"][None], m["Pxx"][None])
    xo = np.tile(np.array([0.0, 0.0, -0.6, 1.0, 0.0, 0.0, 0.0]), (1, 70, 1))
    e.add_known_features(m["y"][None], xo, np.full((1, 70, 11, 11), 128, np.uint8))
    e.set_feature_covariances(m["Pyy"][None])
    state = engine_state(e, 0)
    assert np.array_equal(state["x"], m["x"]) and np.array_equal(state["P"], m["P"])          # the state tests/test_world_view_host.py checked
    yield e, state, cam
    e.close()
