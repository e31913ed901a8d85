"""The per-sequence camera calibration on the device (sl2_set_cameras, sl2_get_cameras): every sequence of a batch
projects and unprojects with its own fku, fkv, u0, v0, kd1, sd - physically different cameras of one image size in one batch.

Every sequence has its OWN scene: synth renders the frames, places the features and cuts the templates for that sequence's
camera on the CPU.  Three cameras: c0 the default 320 x 240 one; c1 with fku x 1.07, fkv x 0.94, u0 + 9.5, v0 - 6.25, kd1 x 2;
c2 with fku x 0.9, kd1 = 0 (no distortion: the oracle takes it), sd = 2.  Three map shapes: four features at capacity 8 (the fused
three-launch step), 100 features (n = 313: the ten-launch path), a dozen with mapping on and room for two more (region, create,
partial prediction, finish).  Tolerances are the project's own against the oracle: search results, selection, counters, flags and
z exact, state 1e-12 (max-abs), covariance 1e-11 (relative Frobenius).

So that no comparison passes on sequences that never measure, the oracle alone was run first on the CPU over these scenes: every
camera matches at least half of its selected features in every frame (the worst: c1, 9 of 12 on the dozen shape, 93 of 100 on
the 100-feature shape), and on the dozen shape every camera initialises a partial feature in frame 0 and converts it by frame 5
(c0: frame 3), so eight frames see all three convert.  The tests assert exactly that of oracle and engine."""
import gc

import numpy as np
import pytest

import oracle_api as oa
from conftest import golden_path, rel_fro, shipped_patches
from scenelib2_amd import Engine, _lib, synth
from scenelib2_amd.config import load_config
from test_gpu_checkpoint import compare_with_oracle, header_of
from test_gpu_seq_dt import accessors, compare_mapping_tight, same

pytestmark = pytest.mark.gpu

TOL_X, TOL_P = 1e-12, 1e-11
CAM_CHUNK = 64          # sequences one launch of sl2_set_cameras carries (kCamChunk, sl2_engine.hip; tests/test_seq_camera_host.py pins it)

C0 = synth.default_camera(320, 240)
C1 = dict(C0, fku=C0["fku"] * 1.07, fkv=C0["fkv"] * 0.94, u0=C0["u0"] + 9.5, v0=C0["v0"] - 6.25, kd1=C0["kd1"] * 2)
C2 = dict(C0, fku=C0["fku"] * 0.9, kd1=0.0, sd=2)
CAMS = [C0, C1, C2]
FRAMES = {"four": 6, "hundred": 6, "dozen": 8}


@pytest.fixture(autouse=True)
def release_engines():
    yield
    gc.collect()


# ------------------------------------------------------------------------------------------------------------------ scenes
class Scene:
    """One sequence as ONE camera sees it: initial state, known features, templates and frames, made for that camera."""

    def __init__(self, cam, params, xv0, Pxx0, feat_y, xp_org, templates, frames, capacity, sigma=0.0, mapping=False):
        self.cam, self.params = dict(cam), dict(params)
        self.xv0, self.Pxx0 = np.asarray(xv0, np.float64), np.asarray(Pxx0, np.float64).reshape(13, 13)
        self.feat_y, self.xp_org = np.asarray(feat_y, np.float64), np.asarray(xp_org, np.float64)
        self.templates = np.asarray(templates, np.uint8)
        self.frames = list(frames)
        self.capacity, self.sigma, self.mapping = capacity, sigma, mapping
        self.N = self.feat_y.shape[0]

    def oracle(self, cam=None):
        o = oa.OracleSLAM(cam or self.cam, self.params["delta_t"], self.params["number_of_features_to_select"])
        if self.mapping:
            o.set_mapping_params(self.params)
        o.set_state(self.xv0, self.Pxx0)
        for i in range(self.N):
            o.add_known_feature(self.feat_y[i], self.xp_org[i], self.templates[i])
        if self.sigma > 0.0:
            for i in range(self.N):
                o.set_feature_Pyy(i, np.eye(3) * self.sigma ** 2)
        return o


_TEX = []
_SCENES = {}


def scene(shape, cam):
    """The scene of `shape` for camera `cam`, built once: the same path and texture for every camera, the features on the same
    pixel grid of each camera's own first view (so the world points differ from camera to camera)."""
    key = (shape, tuple(sorted(cam.items())))
    if key in _SCENES:
        return _SCENES[key]
    if not _TEX:
        _TEX.append(synth.make_texture())
    tex = _TEX[0]
    n_frames = FRAMES[shape]
    if shape == "dozen":      # the recipe of tests/mapping_helpers.py (a camera faster than the 0.2 m/s gate), room for two more features
        N = 12
        params = dict(synth.default_params(N), number_of_features_to_keep_visible=14)
        spec = synth.SequenceSpec(cam, N, n_frames, synth.BASE_SEED + 7, v_amp=0.45, w_amp=0.05)
        capacity, sigma, mapping = 32, 0.0, True
    else:
        N = 4 if shape == "four" else 100
        params = synth.default_params(N)
        spec = synth.SequenceSpec(cam, N, n_frames, synth.BASE_SEED + (0 if shape == "four" else 3))
        capacity, sigma, mapping = (8, 0.0, False) if shape == "four" else (N, 0.005, False)
    frames = synth.render_host(cam, tex, spec.tex_extent, spec.tex_origin, spec.poses)      # frames[k] = pose k
    templates = synth.cut_templates(frames[0], spec.feat_px)
    sc = Scene(cam, params, spec.xv0, spec.Pxx0, spec.feat_y, spec.xp_org(), templates, frames[1:], capacity, sigma, mapping)
    _SCENES[key] = sc
    return sc


def engine_of(scenes, cams=None, create_cam=None, lib=None):
    """One engine whose sequence b holds scenes[b]; created with create_cam (default: the first scene's camera), every
    sequence then given cams[b] (default: its scene's camera; cams=False: nothing set)."""
    B, s0 = len(scenes), scenes[0]
    e = Engine(create_cam or s0.cam, s0.params, B, s0.capacity, lib=lib)
    if cams is not False:
        e.set_cameras(cams or [s.cam for s in scenes])
    e.set_vehicle_state(np.stack([s.xv0 for s in scenes]), np.stack([s.Pxx0 for s in scenes]))
    e.add_known_features(np.stack([s.feat_y for s in scenes]), np.stack([s.xp_org for s in scenes]),
                         np.stack([s.templates for s in scenes]))
    if s0.sigma > 0.0:
        e.set_feature_covariances(np.tile(np.eye(3) * s0.sigma ** 2, (B, s0.N, 1, 1)))
    return e


def batch(scenes, k):
    return np.stack([s.frames[k] for s in scenes])


def cam_equal(a, b):
    return all(a[k] == b[k] for k in ("width", "height", "fku", "fkv", "u0", "v0", "kd1", "sd")) and set(a) == set(b)


def header_camera(blob):
    c = header_of(blob).camera
    return dict(width=c.width, height=c.height, fku=c.fku, fkv=c.fkv, u0=c.u0, v0=c.v0, kd1=c.kd1, sd=c.sd)


class Stepper:
    """One way of issuing a step, applied alike to every engine of a comparison."""

    def __init__(self, form, fb):
        self.form, self.fb, self.bufs = form, fb, {}

    def prepare(self, e):
        if self.form == "unfused":
            e.set_step_fusion(0)
        if self.form == "graph":
            e.set_graph_mode(True)
        if self.form == "groups":
            e.set_groups(2)

    def __call__(self, e, frames, nsel, mapping=False):
        if self.form == "seams":
            e.kalman_filter_predict()
            e.auto_select_n_features(nsel)
            e.make_measurements(frames)
            e.kalman_filter_update()
            e.finish_step(False)
        elif self.form == "graph":
            buf = self.bufs.setdefault(id(e), _lib.DeviceBuffer(e.batch * self.fb, 0))
            e.synchronize()
            buf.upload(frames)
            e.go_one_step(buf.ptr, on_device=True, seq_stride=self.fb, enable_mapping=mapping)
        else:
            e.go_one_step(frames, enable_mapping=mapping)

    def free(self):
        for b in self.bufs.values():
            b.free()


def check_against_oracle(e, b, o, sc, k, tag):
    """Sequence b of e against oracle o after frame k: exact integers, state and covariance to tolerance.  Returns (dx, dP)."""
    if sc.mapping:
        dx, dP = compare_mapping_tight(e, b, o, k)
    else:
        assert int(e.total_state_sizes(b, 1)[0]) == o.total_state_size
        dx = float(np.abs(o.total_state() - e.total_state(b)).max())
        dP = rel_fro(e.total_covariance(b), o.total_covariance())
    print("%s frame %d seq %d: |dx| %.3e  rel |dP| %.3e" % (tag, k, b, dx, dP))
    assert dx <= TOL_X and dP <= TOL_P, (tag, k, b, dx, dP)
    if not sc.mapping:
        compare_with_oracle(e, b, o, TOL_X, TOL_P)
    return dx, dP


# ------------------------------------------------------------------------------------------------------------ 1: defaults
def test_defaults_are_the_create_camera():
    sc = scene("four", C1)
    e = engine_of([sc] * 3, cams=False)
    got = e.get_cameras()
    assert len(got) == 3 and all(cam_equal(g, C1) for g in got)
    assert len(e.get_cameras(1, 2)) == 2 and cam_equal(e.get_cameras(2, 1)[0], C1)
    e.go_one_step(batch([sc] * 3, 0))
    blobs = e.save_sequences()
    assert all(cam_equal(header_camera(b), C1) for b in blobs)
    assert all(cam_equal(g, C1) for g in e.get_cameras())
    e.close()


# --------------------------------------------------------------------- 2: a set camera equals an engine created with it
@pytest.mark.parametrize("form,shape", [("fused", "four"), ("unfused", "four"), ("seams", "four"), ("graph", "four"),
                                        ("groups", "four"), ("fused", "hundred"), ("seams", "hundred"), ("graph", "hundred"),
                                        ("mapping", "dozen"), ("graph", "dozen")])
def test_a_set_camera_equals_an_engine_created_with_it(form, shape):
    """The record changes no arithmetic: sequence b of the mixed engine - created with a camera nobody keeps, except that
    sequence 0 is left on the create camera in the `fused` form - is bit for bit the batch-1 engine created with camera b."""
    cams = CAMS + [C1] if form == "groups" else CAMS            # groups = 2 with B = 4: a record per group's first sequence
    scenes = [scene(shape, c) for c in cams]
    sc = scenes[0]
    fb = sc.cam["width"] * sc.cam["height"]
    nsel = sc.params["number_of_features_to_select"]
    step = Stepper(form, fb)
    if form == "fused":
        e = engine_of(scenes, cams=False)
        e.set_cameras(cams[1:], seq0=1)
    else:
        e = engine_of(scenes, create_cam=dict(C0, fku=211.0, u0=150.0, sd=3))
    step.prepare(e)
    singles = [engine_of([s], cams=False) for s in scenes]
    for s in singles:
        if form in ("unfused", "graph"):
            step.prepare(s)
    for k in range(6):
        step(e, batch(scenes, k), nsel, sc.mapping)
        for b, s in enumerate(singles):
            step(s, batch(scenes[b:b + 1], k), nsel, sc.mapping)
            a, w = accessors(e, b), accessors(s, 0)
            for key in a:
                assert same(a[key], w[key]), "%s %s frame %d sequence %d: %s differs from the engine created with its camera" % (
                    form, shape, k, b, key)
    assert len({e.total_state(b).tobytes() for b in range(3)}) == 3           # three cameras, three filters
    if sc.mapping:
        assert all(s.partial_feature(0)["info"]["initialised"] >= 1 for s in singles)
    for q in [e] + singles:
        assert not q.status_flags().any()
        q.close()
    step.free()


# --------------------------------------------------------------------------- 3: every sequence on an oracle with its own camera
@pytest.mark.parametrize("shape", ["four", "hundred", "dozen"])
def test_each_sequence_follows_an_oracle_with_its_own_camera(shape):
    """Worst errors measured on an MI355X: see DESIGN 8e."""
    scenes = [scene(shape, c) for c in CAMS]
    sc = scenes[0]
    e = engine_of(scenes, create_cam=dict(C0, fku=211.0, u0=150.0, sd=3))      # nobody keeps the engine's own camera
    e.set_profiling(2)
    oracles = [s.oracle() for s in scenes]
    worst = [0.0, 0.0]
    n_frames = FRAMES[shape]
    for k in range(n_frames):
        e.go_one_step(batch(scenes, k), enable_mapping=sc.mapping)
        for b, o in enumerate(oracles):
            o.go_one_step(scenes[b].frames[k], False, sc.mapping)
            dx, dP = check_against_oracle(e, b, o, sc, k, shape)
            worst = [max(worst[0], dx), max(worst[1], dP)]
            # the condition: the sequence measures - at least half of what it selected, in oracle and engine alike
            sel, counters = e.selection(b)
            for matched, selected in ((o.measurement_size // 2, o.num_selected), (counters["measurement_size"] // 2, counters["selected"])):
                assert selected >= (10 if shape != "four" else 4) and 2 * matched >= selected, (shape, k, b, matched, selected)
                if shape == "hundred":
                    assert matched >= 10
    assert len({e.total_state(b).tobytes() for b in range(3)}) == 3
    t = e.kernel_times()
    if shape == "hundred":
        assert t["k_predict"]["launches"] == n_frames and t["k_feature_prediction"]["launches"] == n_frames and "k_syrk" in t, sorted(t)
    else:
        assert t["k_small_front"]["launches"] == n_frames and "k_predict" not in t, sorted(t)
    if shape == "dozen":      # every camera initialised a partial feature and converted one - in eight frames all three do
        for b, o in enumerate(oracles):
            info, got = o.mapping_info(), e.partial_feature(b)["info"]
            assert info["initialised"] >= 1 and info["converted"] >= 1, (b, info)
            assert got["initialised"] == info["initialised"] and got["converted"] == info["converted"], (b, got, info)
        assert t["k_map_find"]["launches"] >= 1 and t["k_map_particles"]["launches"] >= 1, sorted(t)
        assert "k_map_create" in t or "k_map_finish" in t, sorted(t)
    assert not e.status_flags().any()
    print("%s worst: |dx| %.3e  rel |dP| %.3e" % (shape, worst[0], worst[1]))
    e.close()


# ------------------------------------------------------------------------------ 4: a change in mid-run reaches a replayed graph
def switched_oracle(sc0, sc1, frames_before):
    """An oracle of scene sc0 that ran frames_before frames under sc0's camera and goes on under sc1's.  The oracle has no camera
    setter, so its filter is moved into a fresh oracle created with the new camera - which is exact here and only here: known
    features without a prior carry no uncertainty (AddNewKnownFeature leaves Pyy and Pxy zero, and rows of zeros stay zero through
    every update), so x_v, P_xx, the features' positions and their counters ARE the filter.  Asserted below."""
    a = sc0.oracle()
    for k in range(frames_before):
        a.go_one_step(sc0.frames[k], False, False)
    P = a.total_covariance()
    assert not P[13:, :].any() and not P[:, 13:].any()
    assert a.total_state()[13:].tobytes() == sc0.feat_y.reshape(-1).tobytes()
    xv, Pxx = a.get_state()
    o = oa.OracleSLAM(sc1.cam, sc0.params["delta_t"], sc0.params["number_of_features_to_select"])
    o.set_state(xv, Pxx)
    for i in range(sc0.N):
        o.add_known_feature(sc0.feat_y[i], sc0.xp_org[i], sc0.templates[i])
        f = a.feature(i)
        o.set_feature_counters(i, f["attempted"], f["successful"])
    return o


@pytest.mark.parametrize("mapping", [False, True])
def test_a_change_in_mid_run_reaches_a_replayed_graph(mapping):
    """Graph mode, B = 2, device-resident frames in two alternating buffers: three steps under c0, then sequence 1 becomes c1 and
    is fed c1's frames, three more.  The setter costs no capture (sl2_debug_graph_captures of the TEST build); sequence 0 is bit
    for bit the run without the call; sequence 1 is bit for bit the same schedule issued as direct launches, and - mapping off -
    on an oracle whose camera was switched at the same step.  With mapping on the oracle cannot be switched (a feature the
    particle filter initialised has covariance no oracle call can set), so there the direct launches are the judge; they are
    themselves held to per-camera oracles by the test above."""
    shape = "dozen" if mapping else "four"
    s0, s1 = scene(shape, C0), scene(shape, C1)
    fb = C0["width"] * C0["height"]
    T = _lib.load_testing()
    bufs = [_lib.DeviceBuffer(2 * fb, 0) for _ in range(2)]
    runs = {}
    for name, graph, change in (("graph", True, True), ("direct", False, True), ("kept", True, False)):
        e = engine_of([s0, s0], cams=False, lib=T)
        e.set_graph_mode(graph)
        for k in range(6):
            feed = [s0, s1 if (change and k >= 3) else s0]
            if k == 3:
                before = T.sl2_debug_graph_captures(e.h)
                assert before >= 2 if graph else before == 0
                if change:
                    e.set_cameras([C1], seq0=1)
                    assert T.sl2_debug_graph_captures(e.h) == before
                    assert cam_equal(e.get_cameras(1, 1)[0], C1) and cam_equal(e.get_cameras(0, 1)[0], C0)
            e.synchronize()
            bufs[k & 1].upload(batch(feed, k))
            e.go_one_step(bufs[k & 1].ptr, on_device=True, seq_stride=fb, enable_mapping=mapping)
            if k == 3:
                after_setter = T.sl2_debug_graph_captures(e.h)
        e.synchronize()
        if not mapping:
            assert T.sl2_debug_graph_captures(e.h) == (2 if graph else 0), "the setter cost a capture"
        runs[name] = dict(acc=[accessors(e, b) for b in range(2)], after_setter=after_setter)
        if name == "graph" and not mapping:
            o = switched_oracle(s0, s1, 3)
            for k in range(3, 6):
                o.go_one_step(s1.frames[k], False, False)
            check_against_oracle(e, 1, o, s0, 5, "switched")
            assert o.measurement_size >= 4                       # it still measures under the new camera
        assert not e.status_flags().any()
        e.close()
    assert runs["graph"]["after_setter"] == runs["kept"]["after_setter"], "the setter cost a capture"
    assert runs["direct"]["after_setter"] == 0
    for b in range(2):
        assert same(runs["graph"]["acc"][b], runs["direct"]["acc"][b]), b
    assert same(runs["graph"]["acc"][0], runs["kept"]["acc"][0])                 # sequence 0 never noticed
    assert not same(runs["graph"]["acc"][1]["x"], runs["kept"]["acc"][1]["x"])   # sequence 1 did
    for b in bufs:
        b.free()


# -------------------------------------------------------------------------------------------------------- 5: visibility edge
def test_visibility_edge_follows_the_sequence_s_own_principal_point():
    """A fifth feature 26 px from the left edge under c0 (inside the 20 px search boundary) is 14 px from it - outside - for a
    camera whose u0 is 12 px smaller.  Same scene, same frame, two cameras: the visible counts, the flags and the selection
    differ between the sequences and equal each oracle's exactly."""
    base = scene("four", C0)
    spec = synth.SequenceSpec(C0, 4, FRAMES["four"], synth.BASE_SEED + 0)
    px = np.array([[26, 120]])
    c0, c1 = px[0, 0] - C0["u0"], px[0, 1] - C0["v0"]
    factor = np.sqrt(1 - 2 * C0["kd1"] * (c0 * c0 + c1 * c1))
    ray = np.array([(c0 / factor) / -C0["fku"], (c1 / factor) / -C0["fkv"], 1.0])
    r0 = spec.poses[0, :3]
    y5 = np.array([r0[0] - r0[2] * ray[0], r0[1] - r0[2] * ray[1], 0.0])
    frame0 = synth.render_host(C0, _TEX[0], spec.tex_extent, spec.tex_origin, spec.poses[0:1])[0]
    sc = Scene(C0, dict(base.params, number_of_features_to_select=5), base.xv0, base.Pxx0, np.vstack([base.feat_y, y5]),
               np.vstack([base.xp_org, base.xp_org[:1]]), np.concatenate([base.templates, synth.cut_templates(frame0, px)]),
               base.frames, capacity=8)
    shifted = dict(C0, u0=C0["u0"] - 12.0)
    e = engine_of([sc, sc], cams=[C0, shifted])
    oracles = [sc.oracle(C0), sc.oracle(shifted)]
    for k in range(2):
        e.go_one_step(batch([sc, sc], k))
        vis = []
        for b, o in enumerate(oracles):
            o.go_one_step(sc.frames[k], False, False)
            check_against_oracle(e, b, o, sc, k, "edge")
            sel, counters = e.selection(b)
            assert counters["visible"] == o.num_visible and list(sel) == list(o.selected_labels())
            flags = [f["visible"] for f in e.features(b)]
            assert sum(flags) == o.num_visible
            vis.append((counters["visible"], flags, list(sel)))
        if k == 0:      # (from the second frame on the filter under the shifted camera has moved its pose to explain the frame)
            assert vis[0][0] == 5 and vis[0][1] == [True] * 5 and 4 in vis[0][2], vis
            assert vis[1][0] == 4 and vis[1][1] == [True] * 4 + [False] and 4 not in vis[1][2], vis
    e.close()


# -------------------------------------------------------------------------------------------------------- 6: checkpoint rule
def test_checkpoints_record_the_sequence_s_camera_and_loads_check_it():
    s0, s1 = scene("four", C0), scene("four", C1)
    src = engine_of([s0, s1])
    for k in range(3):
        src.go_one_step(batch([s0, s1], k))
    blobs = src.save_sequences()
    assert cam_equal(header_camera(blobs[0]), C0) and cam_equal(header_camera(blobs[1]), C1)
    dst = engine_of([s0, s0], cams=False)
    dst.go_one_step(batch([s0, s0], 0))
    before = dst.save_sequences()
    for attempt in (lambda: dst.load_sequences(blobs[1], seq0=1), lambda: dst.copy_sequences(src, 1, 1, 1),
                    lambda: dst.load_sequences([blobs[0], blobs[1]], seq0=0)):      # (a good blob in front of the bad one)
        with pytest.raises(_lib.Sl2Error) as ei:
            attempt()
        assert ei.value.code == _lib.SL2_ERR_INVALID and "camera" in str(ei.value), str(ei.value)
        assert dst.save_sequences() == before
    dst.set_cameras([C1], seq0=1)
    dst.load_sequences(blobs[1], seq0=1)
    assert dst.save_sequences(1, 1)[0][24:header_of(blobs[1]).off_pos_log] == blobs[1][24:header_of(blobs[1]).off_pos_log]
    twin = engine_of([s0], cams=[C1])
    twin.copy_sequences(src, 1, 1, 0)
    with pytest.raises(_lib.Sl2Error) as ei:
        twin.copy_sequences(src, 0, 1, 0)                  # source sequence 0 ran under c0
    assert ei.value.code == _lib.SL2_ERR_INVALID and "camera" in str(ei.value)
    for k in range(3, 6):
        src.go_one_step(batch([s0, s1], k))
        dst.go_one_step(batch([s0, s1], k))
        twin.go_one_step(batch([s1], k))
        a = accessors(src, 1)
        for name, w in (("loaded", accessors(dst, 1)), ("copied", accessors(twin, 0))):
            for key in a:
                assert same(a[key], w[key]), "frame %d: the %s sequence's %s differs from the source continuing" % (k, name, key)
    dst.reset_sequences(1, 1)
    got = dst.get_cameras()
    assert cam_equal(got[0], C0) and cam_equal(got[1], C1)
    assert cam_equal(header_camera(dst.save_sequences(1, 1)[0]), C1)          # the empty sequence is still that camera's
    for q in (src, dst, twin):
        q.close()


# ---------------------------------------------------------------------------------------------------------------- 7: refusals
def test_refusals_change_nothing():
    s0, s1 = scene("four", C0), scene("four", C1)
    scenes = [s0, s1, s0]
    e = engine_of(scenes)
    ref = engine_of(scenes)
    cams0 = e.get_cameras()
    good = dict(C2)

    def refused(fn):
        with pytest.raises(_lib.Sl2Error) as ei:
            fn()
        assert ei.value.code == _lib.SL2_ERR_INVALID
        assert all(cam_equal(a, b) for a, b in zip(e.get_cameras(), cams0))

    arr = (_lib.sl2_camera * 3)(*[_lib.make_camera(good)] * 3)
    refused(lambda: e._ck(e.L.sl2_set_cameras(e.h, 0, 3, None)))                          # a null pointer
    refused(lambda: e._ck(e.L.sl2_get_cameras(e.h, 0, 3, None)))
    refused(lambda: e.set_cameras([good] * 3, seq0=1))                                    # a range outside the batch
    refused(lambda: e.set_cameras([good], seq0=3))
    refused(lambda: e.set_cameras([good], seq0=-1))
    refused(lambda: e._ck(e.L.sl2_set_cameras(e.h, 0, 0, arr)))
    refused(lambda: e.get_cameras(2, 2))
    bad = [dict(good, width=640), dict(good, height=239), dict(good, fku=0.0), dict(good, fkv=-0.0), dict(good, sd=-1)]
    for key in ("fku", "fkv", "u0", "v0", "kd1"):
        bad += [dict(good, **{key: v}) for v in (np.nan, np.inf, -np.inf)]
    for b in bad:
        refused(lambda: e.set_cameras([b]))
        refused(lambda: e.set_cameras([good, good, b]))                                   # only the last entry of the range is bad
        refused(lambda: e.set_cameras([b, good], seq0=1))
    # ... and a step's results are what they are without any of those calls
    for k in range(2):
        e.go_one_step(batch(scenes, k))
        ref.go_one_step(batch(scenes, k))
        for b in range(3):
            assert same(accessors(e, b), accessors(ref, b)), (k, b)
    e.set_cameras([dict(good, fku=-180.0, kd1=-1e-6, sd=0)])                              # all of that is a calibration
    e.close()
    ref.close()


# --------------------------------------------------------------------- 8: more sequences than one launch of the host form carries
def test_more_sequences_than_one_launch_of_the_host_form_carries():
    """The host form travels in kernel arguments, CAM_CHUNK sequences a launch: CAM_CHUNK + 3 sequences take two launches with a
    ragged second one.  The shipped four-feature scene, every sequence with its own u0."""
    cfg = load_config(golden_path("scenelib2_shipped.cfg"))
    frame = np.load(golden_path("oracle_shipped.npz"))["frame"]
    B = CAM_CHUNK + 3
    cams = [dict(cfg["cam"], u0=cfg["cam"]["u0"] + 0.25 * (b + 1)) for b in range(B)]
    sc = Scene(cfg["cam"], cfg["params"], cfg["xv"], cfg["Pxx"], [f["y"] for f in cfg["features"]],
               [f["xp_org"] for f in cfg["features"]], shipped_patches(), [frame], capacity=8)
    e = engine_of([sc] * B, cams=cams)
    got = e.get_cameras()
    assert len(got) == B and all(cam_equal(g, c) for g, c in zip(got, cams))
    e.set_cameras(cams[1:B - 1], seq0=2)                       # a range that starts and ends inside chunks
    want = cams[:2] + cams[1:B - 1]
    assert all(cam_equal(g, c) for g, c in zip(e.get_cameras(), want))
    e.go_one_step(batch([sc] * B, 0))
    for b in (0, 2, CAM_CHUNK - 1, CAM_CHUNK, CAM_CHUNK + 1, B - 1):
        o = sc.oracle(want[b])
        o.go_one_step(frame, False, False)
        check_against_oracle(e, b, o, sc, 0, "chunks")
        assert cam_equal(header_camera(e.save_sequences(b, 1)[0]), want[b])
    assert len({e.total_state(b).tobytes() for b in range(2, B)}) == B - 2
    e.close()


# ---------------------------------------------------------------------------------------------- 9: the mask is not consulted
def test_a_paused_sequence_takes_a_camera_and_resumes_under_it():
    s0, s1 = scene("four", C0), scene("four", C1)
    e = engine_of([s0, s1], cams=False)                          # sequence 1 holds c1's scene; its camera is still the engine's
    e.set_active([1, 0])
    e.set_cameras([C1], seq0=1)                                  # paused: the setter does not ask
    assert cam_equal(e.get_cameras(1, 1)[0], C1)
    before = accessors(e, 1)
    x_before, P_before = e.total_state(1), e.total_covariance(1)
    e.go_one_step(batch([s0, s1], 0))
    after = accessors(e, 1)
    assert same(after["x"], before["x"]) and same(after["P"], before["P"]) and same(after["features"], before["features"])
    assert e.total_state(1).tobytes() == x_before.tobytes() and e.total_covariance(1).tobytes() == P_before.tobytes()
    e.set_active([1, 1])
    o = s1.oracle()
    for k in range(3):
        e.go_one_step(batch([s0, s1], k))
        o.go_one_step(s1.frames[k], False, False)
        check_against_oracle(e, 1, o, s1, k, "resumed")
    assert o.measurement_size >= 4
    e.close()
