"""Save / restore / copy / reset of sequences on the GPU (sl2_save_sequences, sl2_load_sequences, sl2_copy_sequences,
sl2_reset_sequences): a restored sequence continues bit for bit in an engine of the same shape, tracks the oracle in an engine
of another shape or another age, survives graph replay, and a refused blob leaves the engine untouched."""
import ctypes as C
import gc
import os
import subprocess

import numpy as np
import pytest

import oracle_api as oa
from conftest import ROOT
from mapping_helpers import make_mapping_sequence, oracle_for
from scenelib2_amd import Engine, _lib
from slam_helpers import Pair

pytestmark = pytest.mark.gpu

TOL_X, TOL_P = 1e-12, 1e-11            # known features only (tests/test_gpu_slam.py)
TOL_X_MAP, TOL_P_MAP = 1e-11, 1e-10    # with feature initialisation (tests/test_gpu_mapping.py)
SMALL_STEP_REFUSED = 8


@pytest.fixture(autouse=True)
def release_engines():
    """Engines that ended up in reference cycles (a caught exception keeps its frames) are destroyed here, not at some later
    collection in the middle of another test's measurement of free device memory."""
    yield
    gc.collect()


def same(a, b):
    """Exact equality of nested accessor results (dicts, lists, numpy arrays, ctypes structures, scalars)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(p, q) for p, q in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
    if isinstance(a, C.Structure):
        return bytes(a) == bytes(b)
    if isinstance(a, float) and isinstance(b, float) and a != a and b != b:
        return True
    return a == b


def state_of(e, b):
    """What the issue compares after every frame: x, P, features, selection, trajectory (+ the partial features)."""
    return dict(x=e.total_state(b), P=e.total_covariance(b), features=e.features(b, include_deleted=True),
                selection=e.selection(b), trajectory=e.trajectory(b), partial=e.partial_features(b))


def all_accessors(e, b):
    d = state_of(e, b)
    d["snapshot"] = e.snapshot(b)
    d["status"] = e.status_flags()
    d["info"] = e.partial_feature(b)["info"]
    return d


def header_of(blob):
    return _lib.sl2_sequence_blob_header.from_buffer_copy(blob[:256])


def compare_with_oracle(e, b, o, tol_x, tol_P):
    """Pair.compare_state for ONE sequence of an engine against any oracle."""
    n = o.total_state_size
    assert int(e.total_state_sizes(b, 1)[0]) == n
    xo, xe = o.total_state(), e.total_state(b)
    Po, Pe = o.total_covariance(), e.total_covariance(b)
    dx = float(np.abs(xo - xe).max())
    dP = float(np.linalg.norm(Po - Pe) / max(np.linalg.norm(Po), 1e-300))
    assert dx <= tol_x, "state differs by %g (seq %d)" % (dx, b)
    assert dP <= tol_P, "covariance rel-Frobenius differs by %g (seq %d)" % (dP, b)
    feats = e.features(b)
    assert len(feats) == o.num_features
    sel, counters = e.selection(b)
    assert counters["visible"] == o.num_visible
    assert list(sel) == list(o.selected_labels())
    for i, fe in enumerate(feats):
        fo = o.feature(i)
        assert fe["label"] == fo["label"] and fe["attempted"] == fo["attempted"] and fe["successful"] == fo["successful"]
        assert fe["selected"] == fo["selected"]
        if fe["selected"]:
            assert fe["success"] == fo["success"]
            if fo["success"]:
                assert np.array_equal(fe["z"], fo["z"])
    return dx, dP


def compare_mapping(e, b, s, k):
    """One sequence with feature initialisation against its oracle: events, labels, search results exact; state to tolerance."""
    info, got = s.mapping_info(), e.partial_feature(b)
    for key in ("initialised", "converted", "deleted", "n_partial"):
        assert got["info"][key] == info[key], (k, key, got["info"], info)
    pf = s.partial_feature(0)
    if pf is not None:
        g = got["pf"]
        assert g["label"] == pf["label"] and g["n_particles"] == pf["n_particles"] and g["attempts"] == pf["attempts"], k
        assert np.array_equal(g["particles"][:, 0], pf["particles"][:, 0]), k
        if pf["making"]:
            assert np.array_equal(g["particles"][:, 11], pf["particles"][:, 11]), k
    x0, P0 = s.total_state(), s.total_covariance()
    assert e.total_state_sizes(b, 1)[0] == x0.size, k
    x1, P1 = e.total_state(b), e.total_covariance(b)
    dx = float(np.abs(x1 - x0).max())
    dP = float(np.linalg.norm(P1 - P0) / max(np.linalg.norm(P0), 1e-12))
    assert dx < TOL_X_MAP, (k, dx)
    assert dP <= TOL_P_MAP, (k, dP)
    kinds = s.feature_kinds()
    feats = e.features(b)
    assert [f["label"] for f in feats] == list(kinds[:, 2]) and [f["state_size"] for f in feats] == list(kinds[:, 0]), k
    for f in feats:                                  # counters of every feature in the list
        assert f["attempted"] >= f["successful"] >= 0
    return dx, dP


def fresh_like(pr, batch=None, max_features=None):
    return Engine(pr.cam, pr.params, batch or pr.B, max_features or pr.engine.max_features)


def mapping_engine(cam, params, spec, templates, max_features, batch=1):
    e = Engine(cam, params, batch, max_features)
    e.set_vehicle_state(np.tile(spec.xv0, (batch, 1)), np.tile(spec.Pxx0, (batch, 1, 1)))
    e.add_known_features(np.tile(spec.feat_y, (batch, 1, 1)), np.tile(spec.xp_org(), (batch, 1, 1)), np.tile(templates, (batch, 1, 1, 1)))
    return e


# ------------------------------------------------------------------------------------------------- 4: same shape, no mapping
def test_same_shape_continues_bit_identically_in_permuted_slots():
    pr = Pair(12, 60, batch=4)
    A = pr.engine
    B = fresh_like(pr)
    B.set_vehicle_state(np.stack([s.xv0 for s in pr.specs]), np.stack([s.Pxx0 for s in pr.specs]))
    for b in range(4):
        B.add_known_features(pr.specs[b].feat_y[None], np.tile(pr.specs[b].poses[0], (1, 12, 1)), pr.templates[b][None], seq0=b)
    for k in range(25):
        pr.step_both(k, True)
        B.go_one_step(pr.frame_batch(k), True)
    pr.compare_state(TOL_X, TOL_P)
    blobs = B.save_sequences()
    assert all(header_of(b).n_slots == 12 and header_of(b).sequence_steps == 25 and header_of(b).mapping_in_use == 0 for b in blobs)
    B.close()
    perm = [2, 0, 3, 1]                              # sequence b of run A lives in slot perm[b] of the new engine
    B2 = fresh_like(pr)
    for b in range(4):
        B2.load_sequences([blobs[b]], seq0=perm[b])
    inv = [perm.index(s) for s in range(4)]
    worst = dict(x=0.0, P=0.0)
    for k in range(25, 60):
        pr.step_both(k, True)
        fb = pr.frame_batch(k)
        B2.go_one_step(fb[inv], True)
        for b in range(4):
            assert same(state_of(A, b), state_of(B2, perm[b])), "frame %d sequence %d" % (k, b)
        w = pr.compare_state(TOL_X, TOL_P)
        worst = {q: max(worst[q], w[q]) for q in worst}
    print("worst against the oracle after the restore: |dx| %.3e, rel |dP| %.3e" % (worst["x"], worst["P"]))
    assert [B2.snapshot(perm[b])["header"].sequence_steps for b in range(4)] == [60] * 4
    assert B2.snapshot(0)["header"].steps_done == 35
    # the position log: the engine is 35 steps old, the sequences 60; what is shown are their last 35 positions
    la, lb = A.position_log(), B2.position_log()
    assert la.shape == (4, 60, 3) and lb.shape == (4, 35, 3)
    for b in range(4):
        assert np.array_equal(la[b, 25:], lb[perm[b]])


# --------------------------------------------------------------------------------------------- 5 - 7: with feature initialisation
@pytest.fixture(scope="module")
def mapping_run():
    """The uninterrupted run of tests 5 - 7: engine A (max_features 16) and the oracle over frames 1 .. 59, a blob taken after
    frame 27, A's accessor state and the oracle's (x, P, events) after every later frame."""
    cam, params, spec, frames, templates = make_mapping_sequence(n_frames=60)
    s = oracle_for(cam, params, spec, templates, oa)
    A = mapping_engine(cam, params, spec, templates, 16)
    run = dict(cam=cam, params=params, spec=spec, frames=frames, templates=templates, states={}, blobs={}, positions=[])
    for k in range(1, 28):
        s.go_one_step(frames[k], True, True)
        A.go_one_step(frames[k][None], save_trajectory=True, enable_mapping=True)
        run["positions"].append(s.total_state()[:3].copy())
    compare_mapping(A, 0, s, 27)
    run["partial_at_27"] = len(A.partial_features(0))
    run["labels_at_27"] = A.snapshot(0)["header"].next_free_label
    run["blob"] = A.save_sequences(0, 1)[0]
    run["A"], run["oracle"], run["next_frame"] = A, s, 28
    yield run
    A.close()


def advance(run, upto):
    """Step engine A and the oracle of the shared run up to frame `upto` (each frame once, whichever test asks first)."""
    A, s, frames = run["A"], run["oracle"], run["frames"]
    while run["next_frame"] <= upto:
        k = run["next_frame"]
        s.go_one_step(frames[k], True, True)
        A.go_one_step(frames[k][None], save_trajectory=True, enable_mapping=True)
        compare_mapping(A, 0, s, k)
        run["states"][k] = state_of(A, 0)
        run["blobs"][k] = A.save_sequences(0, 1)[0]
        run["positions"].append(s.total_state()[:3].copy())
        run["oracle_at"] = run.get("oracle_at", {})
        run["oracle_at"][k] = dict(x=s.total_state(), P=s.total_covariance(), info=s.mapping_info(), kinds=s.feature_kinds().copy(),
                                   selected=list(s.selected_labels()), visible=s.num_visible,
                                   counters=[(s.feature(i)["label"], s.feature(i)["attempted"], s.feature(i)["successful"])
                                             for i in range(s.num_features)])
        run["next_frame"] = k + 1


def against_recorded_oracle(e, b, rec, k):
    """compare_mapping against what the oracle held after frame k of the shared run."""
    info = e.partial_feature(b)["info"]
    for key in ("initialised", "converted", "deleted", "n_partial"):
        assert info[key] == rec["info"][key], (k, key)
    x1, P1 = e.total_state(b), e.total_covariance(b)
    assert x1.size == rec["x"].size, k
    dx = float(np.abs(x1 - rec["x"]).max())
    dP = float(np.linalg.norm(P1 - rec["P"]) / max(np.linalg.norm(rec["P"]), 1e-12))
    assert dx < TOL_X_MAP, (k, dx)
    assert dP <= TOL_P_MAP, (k, dP)
    feats = e.features(b)
    assert [f["label"] for f in feats] == list(rec["kinds"][:, 2]) and [f["state_size"] for f in feats] == list(rec["kinds"][:, 0]), k
    assert [(f["label"], f["attempted"], f["successful"]) for f in feats] == rec["counters"], k
    sel, counters = e.selection(b)
    assert list(sel) == rec["selected"] and counters["visible"] == rec["visible"], k
    return dx, dP


def test_mapping_restore_is_bit_identical_and_labels_continue(mapping_run):
    run = mapping_run
    assert run["partial_at_27"] == 1
    h = header_of(run["blob"])
    assert h.magic == _lib.SL2_BLOB_MAGIC and h.mapping_in_use == 1 and h.sequence_steps == 27 and h.n_partial_slots == 1
    assert h.src_max_features == 16 and h.n_slots <= 16 and h.bytes == len(run["blob"])
    B = Engine(run["cam"], run["params"], 1, 16)
    B.load_sequences([run["blob"]])
    assert B.snapshot(0)["header"].next_free_label == run["labels_at_27"]
    assert len(B.partial_features(0)) == 1
    advance(run, 59)
    for k in range(28, 60):
        B.go_one_step(run["frames"][k][None], save_trajectory=True, enable_mapping=True)
        assert same(state_of(B, 0), run["states"][k]), "frame %d" % k
        assert B.save_sequences(0, 1)[0] == run["blobs"][k], "frame %d: blobs differ" % k      # particles, drand48, every counter
        against_recorded_oracle(B, 0, run["oracle_at"][k], k)
    last = run["oracle_at"][59]["info"]
    assert last["converted"] >= 4 and B.snapshot(0)["header"].next_free_label > run["labels_at_27"]
    assert not B.status_flags().any()


def test_mapping_blob_in_an_engine_of_another_shape(mapping_run):
    run = mapping_run
    advance(run, 59)
    cam, params, spec, frames, templates = (run[q] for q in ("cam", "params", "spec", "frames", "templates"))
    E = mapping_engine(cam, params, spec, templates, 40, batch=3)      # slots 0 and 1: the same sequence from its start
    E.load_sequences([run["blob"]], seq0=2)
    worst = [0.0, 0.0]
    for k in range(28, 60):
        E.go_one_step(np.stack([frames[k - 27], frames[k - 27], frames[k]]), save_trajectory=True, enable_mapping=True)
        dx, dP = against_recorded_oracle(E, 2, run["oracle_at"][k], k)
        worst = [max(worst[0], dx), max(worst[1], dP)]
        assert not (E.status_flags() & SMALL_STEP_REFUSED).any(), k
        assert same(state_of(E, 0), state_of(E, 1)), k                 # the neighbours are not disturbed (and equal each other)
    print("another shape: worst |dx| %.3e, rel |dP| %.3e" % tuple(worst))
    assert E.snapshot(2)["header"].sequence_steps == 59 and E.snapshot(0)["header"].sequence_steps == 32


@pytest.mark.parametrize("batch", [1, 4])
@pytest.mark.parametrize("age", [3, 70])
def test_mapping_blob_in_an_engine_of_another_age(mapping_run, batch, age):
    run = mapping_run
    advance(run, 59)
    cam, params, spec, frames, templates = (run[q] for q in ("cam", "params", "spec", "frames", "templates"))
    E = mapping_engine(cam, params, spec, templates, 16, batch=batch)
    for k in range(age):
        E.go_one_step(np.tile(frames[1 + k % 20][None], (batch, 1, 1)), save_trajectory=True, enable_mapping=True)
    slot = batch - 1
    E.load_sequences([run["blob"]], seq0=slot)
    for k in range(28, 60):
        fb = np.tile(frames[1 + (age + k) % 20][None], (batch, 1, 1))
        fb[slot] = frames[k]
        E.go_one_step(fb, save_trajectory=True, enable_mapping=True)
        against_recorded_oracle(E, slot, run["oracle_at"][k], k)
        assert not (E.status_flags()[slot] & SMALL_STEP_REFUSED), k
    assert E.snapshot(slot)["header"].sequence_steps == 59 and E.snapshot(slot)["header"].steps_done == age + 32
    # the position log shows min(engine steps, 1000) entries; of those, the sequence's own are its last min(that, 59)
    log = E.position_log(slot, 1)[0]
    assert log.shape == (age + 32, 3)
    own = min(age + 32, 59)
    want = np.array(run["positions"][59 - own:59])
    assert np.abs(log[-own:] - want).max() < TOL_X_MAP
    assert not log[:-own].any()                       # before the sequence existed


# ------------------------------------------------------------------------------------------------------------- 8: graph mode
def test_load_under_graph_replay_of_the_fused_small_step():
    pr = Pair(10, 12, batch=2, n_select=10, max_features=32)             # ld = 128: the fused small-map step
    donor = Pair(20, 12, batch=1, n_select=10, max_features=32, seq0=5)
    for k in range(4):
        donor.step_both(k, True)
    donor.compare_state(TOL_X, TOL_P)
    blob = donor.engine.save_sequences(0, 1)[0]
    assert header_of(blob).n_slots == 20
    e = pr.engine
    e.set_graph_mode(True)
    W, H = pr.cam["width"], pr.cam["height"]
    bufs = [_lib.DeviceBuffer(2 * W * H, 0) for _ in range(2)]
    for k in range(4):                                                   # replays with a map of 10 slots (64-column panel)
        for b in range(2):
            pr.oracles[b].go_one_step(pr.frames[b][k], True)
        bufs[k & 1].upload(pr.frame_batch(k))
        e.go_one_step(bufs[k & 1].ptr, save_trajectory=True, on_device=True, seq_stride=W * H)
        e.synchronize()
    pr.compare_state(TOL_X, TOL_P)
    e.load_sequences([blob], seq0=1)                                     # 20 slots: the captured steps no longer fit
    for k in range(4, 12):
        pr.oracles[0].go_one_step(pr.frames[0][k], True)
        donor.oracles[0].go_one_step(donor.frames[0][k], True)
        bufs[k & 1].upload(np.stack([pr.frames[0][k], donor.frames[0][k]]))
        e.go_one_step(bufs[k & 1].ptr, save_trajectory=True, on_device=True, seq_stride=W * H)
        e.synchronize()
        compare_with_oracle(e, 0, pr.oracles[0], TOL_X, TOL_P)
        compare_with_oracle(e, 1, donor.oracles[0], TOL_X, TOL_P)
        assert not e.status_flags().any(), k


# ------------------------------------------------------------------------------------------------------------------- 9: copy
def test_copy_within_an_engine_and_between_engines():
    pr = Pair(12, 20, batch=4)
    e = pr.engine
    for k in range(10):
        pr.step_both(k, True)
    before = e.save_sequences()
    e.copy_sequences(e, 0, 1, 2)                                         # sequence 0 -> slot 2
    other = fresh_like(pr, batch=2)                                      # its own stream
    assert other.stream != e.stream
    other.copy_sequences(e, 0, 2, 0)                                     # sequences 0, 1 -> the other engine
    after = e.save_sequences()
    assert after[0] == before[0] and after[1] == before[1] and after[3] == before[3]      # the source is unchanged
    assert after[2] == before[0]
    assert other.save_sequences() == before[:2]
    with pytest.raises(_lib.Sl2Error) as ei:
        e.copy_sequences(e, 0, 2, 1)                                     # [0, 2) onto [1, 3)
    assert ei.value.code == _lib.SL2_ERR_INVALID and "overlap" in str(ei.value)
    assert e.save_sequences() == after
    for k in range(10, 20):
        fb = pr.frame_batch(k)
        fb[2] = fb[0]
        e.go_one_step(fb, True)
        other.go_one_step(fb[:2], True)
        assert same(state_of(e, 2), state_of(e, 0)), k
        for b in range(2):
            assert same(state_of(other, b), state_of(e, b)), (k, b)
    assert e.save_sequences(2, 1)[0] == e.save_sequences(0, 1)[0]


# ------------------------------------------------------------------------------------------------------------------ 10: reset
def test_reset_gives_the_slot_to_a_new_sequence():
    pr = Pair(12, 35, batch=4)
    untouched = Pair(12, 35, batch=4)
    new = Pair(9, 15, batch=2, seq0=10, n_select=12, make_engine=False)
    e = pr.engine
    for k in range(20):
        e.go_one_step(pr.frame_batch(k), True)
        untouched.engine.go_one_step(pr.frame_batch(k), True)
    empty = fresh_like(pr).save_sequences(0, 1)[0]
    for j, slot in enumerate((1, 3)):
        e.reset_sequences(slot, 1)
        blob = e.save_sequences(slot, 1)[0]
        assert header_of(blob).n_slots == 0 and header_of(blob).sequence_steps == 0
        assert blob == empty                                             # what sl2_create left, bit for bit
        e.set_vehicle_state(new.specs[j].xv0[None], new.specs[j].Pxx0[None], seq0=slot)
        e.add_known_features(new.specs[j].feat_y[None], np.tile(new.specs[j].poses[0], (1, 9, 1)), new.templates[j][None], seq0=slot)
    assert [f["label"] for f in e.features(1)] == list(range(9))        # next_free_label_ started at 0 again
    for k in range(15):
        fb = pr.frame_batch(20 + k)
        untouched.engine.go_one_step(fb, True)
        fb = fb.copy()
        for j, slot in enumerate((1, 3)):
            fb[slot] = new.frames[j][k]
            new.oracles[j].go_one_step(new.frames[j][k], True)
        e.go_one_step(fb, True)
        for j, slot in enumerate((1, 3)):
            compare_with_oracle(e, slot, new.oracles[j], TOL_X, TOL_P)
        for b in (0, 2):
            assert same(state_of(e, b), state_of(untouched.engine, b)), (k, b)
    assert [e.snapshot(b)["header"].sequence_steps for b in range(4)] == [35, 15, 35, 15]
    assert e.trajectory(1).shape == new.oracles[0].trajectory().shape == (15, 3)      # trajectory_store_ started again


# ------------------------------------------------------------------------------------------------------- 11: round trip at rest
def test_round_trip_at_rest_and_between_the_seams(mapping_run):
    run = mapping_run
    E = Engine(run["cam"], run["params"], 1, 16)
    E.load_sequences([run["blob"]])                                      # a partially initialised feature in flight
    acc1 = all_accessors(E, 0)
    s1 = E.save_sequences(0, 1)[0]
    assert s1 == run["blob"]
    E.load_sequences([s1])
    assert E.save_sequences(0, 1)[0] == s1
    assert same(all_accessors(E, 0), acc1)
    # between kalman_filter_predict and finish_step
    pr = Pair(12, 6, batch=2)
    e = pr.engine
    for k in range(3):
        pr.step_both(k, True)
    e.kalman_filter_predict()
    e.auto_select_n_features(12)
    e.make_measurements(pr.frame_batch(3))
    acc = [all_accessors(e, b) for b in range(2)]
    blobs = e.save_sequences()
    e.load_sequences(blobs)
    assert e.save_sequences() == blobs
    assert same([all_accessors(e, b) for b in range(2)], acc)
    f = fresh_like(pr)
    f.load_sequences(blobs)
    assert f.save_sequences() == blobs
    for q in (e, f):                                                     # ... and the step ends as if nothing had happened
        q.kalman_filter_update()
        q.finish_step(True)
    for b in range(2):
        pr.oracles[b].go_one_step(pr.frames[b][3], True)
        assert same(state_of(e, b), state_of(f, b))
    pr.compare_state(TOL_X, TOL_P)


# ------------------------------------------------------------------------------------------------------------- 12: refusals
def test_refused_blobs_leave_the_engine_untouched(mapping_run):
    run = mapping_run
    pr = Pair(12, 4, batch=2)
    e = pr.engine
    for k in range(3):
        pr.step_both(k, True)
    before = e.save_sequences()
    good = before[0]

    def refused(blob, code, word, engine=e, seq0=1):
        with pytest.raises(_lib.Sl2Error) as ei:
            engine.load_sequences([blob], seq0=seq0)
        assert ei.value.code == code and word in str(ei.value), str(ei.value)
        assert engine.save_sequences() == (before if engine is e else engine_before)

    bad = bytearray(good); bad[0] ^= 0xFF
    refused(bytes(bad), _lib.SL2_ERR_INVALID, "magic")
    refused(good[:len(good) - 4096], _lib.SL2_ERR_INVALID, "truncated")
    refused(good[:200], _lib.SL2_ERR_INVALID, "truncated")               # not even a header
    h = header_of(good); h.camera.fku += 1.0
    refused(bytes(h) + good[256:], _lib.SL2_ERR_INVALID, "camera")
    h = header_of(good); h.params.delta_t *= 2
    refused(bytes(h) + good[256:], _lib.SL2_ERR_INVALID, "params")
    h = header_of(good); h.off_P += 64
    refused(bytes(h) + good[256:], _lib.SL2_ERR_INVALID, "offsets")
    # a second blob that is bad: the first one must not have been written either
    with pytest.raises(_lib.Sl2Error):
        e.load_sequences([before[1], bytes(bad)], seq0=0)
    assert e.save_sequences() == before
    # n_slots > N
    small = Engine(pr.cam, pr.params, 1, 8)
    engine_before = small.save_sequences()
    refused(good, _lib.SL2_ERR_CAPACITY, "n_slots", engine=small, seq0=0)
    # more partial slots than kpart: a blob written with max_features_to_init_at_once = 2 and two partial features in flight
    cam, params, spec, frames, templates = (run[q] for q in ("cam", "params", "spec", "frames", "templates"))
    params = dict(params); params["number_of_features_to_keep_visible"] = 14
    p2 = dict(params); p2["max_features_to_init_at_once"] = 2
    two = mapping_engine(cam, p2, spec, templates, 16)
    blob2 = None
    for k in range(1, 40):
        two.go_one_step(frames[k][None], enable_mapping=True)
        if len(two.partial_features(0)) == 2:
            blob2 = two.save_sequences(0, 1)[0]
            break
    assert blob2 is not None and header_of(blob2).n_partial_slots == 2
    one = mapping_engine(cam, params, spec, templates, 16)
    engine_before = one.save_sequences()
    refused(blob2, _lib.SL2_ERR_CAPACITY, "n_partial_slots", engine=one, seq0=0)
    # ... while an engine with room takes it (the two parameters that may differ, differ)
    p4 = dict(params); p4["max_features_to_init_at_once"] = 4
    roomy = Engine(cam, p4, 1, 16)
    roomy.load_sequences([blob2])
    assert len(roomy.partial_features(0)) == 2
    # bad arguments
    with pytest.raises(_lib.Sl2Error):
        e.reset_sequences(1, 2)
    with pytest.raises(_lib.Sl2Error):
        e.copy_sequences(e, 0, 1, 2)
    assert e.save_sequences() == before


def test_sequence_groups_save_and_load_but_refuse_blobs_with_mapping(mapping_run):
    """Groups are offsets into the same arrays: everything works with sl2_set_groups > 1 except a blob with mapping in use,
    which is refused as mapping itself is."""
    pr = Pair(12, 12, batch=4)
    A = pr.engine
    A.set_groups(2)
    for k in range(5):
        A.go_one_step(pr.frame_batch(k), True)
    blobs = A.save_sequences()
    B = fresh_like(pr)
    B.set_groups(2)
    B.load_sequences(blobs)
    assert B.save_sequences() == blobs
    for k in range(5, 12):
        for q in (A, B):
            q.go_one_step(pr.frame_batch(k), True)
        for b in range(4):
            assert same(state_of(A, b), state_of(B, b)), (k, b)
    run = mapping_run
    E = mapping_engine(run["cam"], run["params"], run["spec"], run["templates"], 16, batch=2)
    E.set_groups(2)
    before = E.save_sequences()
    with pytest.raises(_lib.Sl2Error, match="sequence groups"):
        E.load_sequences([run["blob"]], seq0=1)
    assert E.save_sequences() == before


# -------------------------------------------------------------------------------------------------------- 13: large shapes once
@pytest.mark.parametrize("n_features,batch", [(100, 8), (500, 2)])
def test_large_shapes_continue_bit_identically(n_features, batch):
    pr = Pair(n_features, 5, batch=batch, n_select=min(n_features, 100), make_engine=True)
    A = pr.engine
    for k in range(2):
        A.go_one_step(pr.frame_batch(k), True)
    blobs = A.save_sequences()
    assert header_of(blobs[0]).state_size == 13 + 3 * n_features
    B = fresh_like(pr)
    # through device memory as well: save to a device buffer, load from it
    cap = A.sequence_blob_capacity()
    assert cap % 64 == 0 and cap >= len(blobs[0])
    dev = _lib.DeviceBuffer(cap * batch, 0)
    A.save_sequences_device(dev.ptr, cap)
    A.synchronize()
    assert bytes(dev.download((len(blobs[1]),), np.uint8, offset=cap)) == blobs[1]
    B.load_sequences_device(dev.ptr, cap)
    assert B.save_sequences() == blobs
    C2 = fresh_like(pr)
    C2.load_sequences(blobs)
    for k in range(2, 5):
        fb = pr.frame_batch(k)
        for q in (A, B, C2):
            q.go_one_step(fb, True)
        for b in range(batch):
            xa, Pa = A.total_state(b), A.total_covariance(b)
            for q in (B, C2):
                assert np.array_equal(xa, q.total_state(b)) and np.array_equal(Pa, q.total_covariance(b)), (k, b)
    assert A.save_sequences() == B.save_sequences() == C2.save_sequences()
    assert not A.status_flags().any()
    dev.free()


# --------------------------------------------------------------------------------------------------- 14: the C++ adapter's file
@pytest.mark.parametrize("mapping", [False, True])
def test_resume_example_prints_what_the_uninterrupted_adapter_prints(tmp_path, mapping):
    """examples/resume_monoslam: 13 frames, SaveState, a NEW object, LoadState, the remaining frames - the output of
    examples/monoslam_adapter on the same scene, line for line."""
    from test_gpu_headless_example import _write_scene
    exe = os.path.join(ROOT, "examples", "resume_monoslam")
    ref = os.path.join(ROOT, "examples", "monoslam_adapter")
    if not (os.path.exists(exe) and os.path.exists(ref)):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    cam, params, spec, frames, templates = make_mapping_sequence(n_frames=30)
    cfg, fd = _write_scene(str(tmp_path), cam, params, spec, frames, templates)
    flags = ["--mapping"] if mapping else []
    a = subprocess.run([ref, "--cfg", cfg, "--frames", fd] + flags, capture_output=True, text=True, timeout=300)
    b = subprocess.run([exe, "--cfg", cfg, "--frames", fd, "--save-at", "13", "--state", os.path.join(str(tmp_path), "seq.blob")] + flags,
                       capture_output=True, text=True, timeout=300)
    assert a.returncode == 0, a.stdout + a.stderr
    assert b.returncode == 0, b.stdout + b.stderr
    assert "saved after 13 frames" in b.stderr and "restored" in b.stderr
    la, lb = a.stdout.splitlines(), b.stdout.splitlines()
    assert len([l for l in la if l.startswith("frame ")]) == 3 and "[Robot covariance]" in la
    assert la == lb
