"""Stepping a subset of the batch (sl2_set_active_sequences): a paused sequence is left exactly as it was by every form the
step takes, its neighbours do not notice, a resumed sequence goes on as the oracle does when it is handed the next frame, and
sequences of unequal length are fed by sl2_ingest_next_ragged.

"Blob" below = the bytes of sl2_save_sequences: the complete state of a sequence by construction.  core(blob) leaves out the
two things that follow the ENGINE's clock - the header's sequence_steps and the position log - which are checked on their own.
A masked engine is fed per sequence: every sequence gets ITS next frame in the steps it is active for (a camera that dropped
a frame, a sequence that waited), so sequence b after j of its own frames must equal, bit for bit, the same sequence after j
steps of an engine that never paused anybody.  Tolerances against the oracle are those of tests/test_gpu_slam.py and
tests/test_gpu_mapping.py."""
import ctypes as C
import gc
import os
import subprocess
import time

import numpy as np
import pytest

import oracle_api as oa
from conftest import ROOT
from mapping_helpers import make_mapping_sequence, oracle_for
from scenelib2_amd import Engine, _lib, ingest, synth
from slam_helpers import Pair
from test_gpu_checkpoint import compare_mapping, compare_with_oracle, header_of, mapping_engine

pytestmark = pytest.mark.gpu

TOL_X, TOL_P = 1e-12, 1e-11            # tests/test_gpu_slam.py
TOL_P_LARGE = 1e-10                    # tests/test_gpu_slam.py, n = 613
SMALL_STEP_REFUSED = 8


@pytest.fixture(autouse=True)
def release_engines():
    yield
    gc.collect()


def core(blob):
    """A blob without what follows the engine's clock: sequence_steps (bytes 16 .. 23 of the header) and the position log (the
    last section)."""
    return bytes(blob[:16]) + bytes(blob[24:header_of(blob).off_pos_log])


def steps_of(blob):
    return header_of(blob).sequence_steps


def engine_of(pr, batch=None, max_features=None, lib=None, seqs=None):
    """A fresh engine that holds sequences `seqs` of the pair (default: all of them, tiled up to `batch`)."""
    B = batch or pr.B
    seqs = [b % pr.B for b in range(B)] if seqs is None else seqs
    e = Engine(pr.cam, pr.params, B, max_features or pr.N, lib=lib)
    e.set_vehicle_state(np.stack([pr.specs[s].xv0 for s in seqs]), np.stack([pr.specs[s].Pxx0 for s in seqs]))
    for b, s in enumerate(seqs):
        nf = pr.specs[s].feat_y.shape[0]
        e.add_known_features(pr.specs[s].feat_y[None], np.tile(pr.specs[s].poses[0], (1, nf, 1)), pr.templates[s][None], seq0=b)
        if getattr(pr, "sigma", 0.0) > 0.0:
            e.set_feature_covariances(np.tile(np.eye(3) * pr.sigma ** 2, (1, nf, 1, 1)), seq0=b)
    return e


def oracles_of(pr, n_select=None):
    out = []
    for b in range(pr.B):
        s = oa.OracleSLAM(pr.cam, pr.params["delta_t"], n_select or pr.params["number_of_features_to_select"])
        s.set_state(pr.specs[b].xv0, pr.specs[b].Pxx0)
        for i in range(pr.specs[b].feat_y.shape[0]):
            s.add_known_feature(pr.specs[b].feat_y[i], pr.specs[b].poses[0], pr.templates[b][i])
        if getattr(pr, "sigma", 0.0) > 0.0:
            for i in range(pr.specs[b].feat_y.shape[0]):
                s.set_feature_Pyy(i, np.eye(3) * pr.sigma ** 2)
        out.append(s)
    return out


def masks_for(B, n, always=(1, 4, 7), seed=5):
    """A mask per step that changes every step: sequences `always` never pause, the others do about two steps in five -
    sequence 0 among them; step 3 pauses everybody who can be paused."""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n):
        m = (rng.rand(B) < 0.6).astype(np.uint8)
        if k == 3:
            m[:] = 0
        if k == 0:
            m[0] = 0                                # sequence 0 is paused in the very first step
        for a in always:
            if a < B:
                m[a] = 1
        if out and np.array_equal(out[-1], m):
            m[B - 1 if (B - 1) not in always else 0] ^= 1
        out.append(m)
    return out


def plain_step(eng, batch, save_trajectory=True):
    eng.go_one_step(batch, save_trajectory)


def seam_step(eng, batch, save_trajectory=True):
    eng.kalman_filter_predict()
    eng.auto_select_n_features(eng.params_n_select)
    eng.make_measurements(batch)
    eng.kalman_filter_update()
    eng.finish_step(save_trajectory)


def masked_run(pr, eng, masks, step=plain_step, oracles=None, tol=(TOL_X, TOL_P)):
    """Step `eng` under one mask per step, every sequence fed its own next frame.  After every step: each paused sequence's blob
    equals its blob from before the step outside the position log, sequence_steps stands still, the position log repeats the
    last position and the trajectory store has not grown; each active sequence equals its oracle (if given).  An engine of more
    sequences than the pair has holds copies: sequence b >= pr.B is a copy of sequence b % pr.B and must stay one.  Returns, per
    sequence, its blobs after each of ITS frames, and the blobs of all sequences after every step."""
    B = eng.batch
    seen = [0] * B
    own = [[] for _ in range(B)]
    per_step = []
    before = eng.save_sequences()
    for k, mask in enumerate(masks):
        mask = np.asarray(mask, np.uint8)
        traj_before = [eng.trajectory(b).shape[0] for b in range(min(B, pr.B))]
        eng.set_active(mask)
        batch = np.stack([pr.frames[b % pr.B][min(seen[b], pr.n_frames - 1)] for b in range(B)])
        step(eng, batch)
        after = eng.save_sequences()
        assert np.array_equal(eng.active(), mask)
        log = eng.position_log(capacity=2)
        xv, _ = eng.get_vehicle_state()
        for b in range(B):
            if not mask[b]:
                assert core(after[b]) == core(before[b]), "step %d: paused sequence %d changed" % (k, b)
                assert steps_of(after[b]) == steps_of(before[b]), (k, b)
                assert np.array_equal(log[b, -1], xv[b, :3]), (k, b)
                if k >= 1:
                    assert np.array_equal(log[b, -1], log[b, -2]), "step %d: the log of paused sequence %d does not repeat" % (k, b)
                if b < pr.B:
                    assert eng.trajectory(b).shape[0] == traj_before[b], (k, b)
            else:
                assert steps_of(after[b]) == steps_of(before[b]) + 1, (k, b)
                if oracles is not None and b < pr.B:
                    oracles[b].go_one_step(pr.frames[b][seen[b]], True)
                    compare_with_oracle(eng, b, oracles[b], tol[0], tol[1])
                seen[b] += 1
                own[b].append(after[b])
            if b >= pr.B:
                assert after[b] == after[b % pr.B], "step %d: sequence %d left its twin %d" % (k, b, b % pr.B)
        per_step.append(after)
        before = after
    assert not eng.status_flags().any()
    return own, per_step


@pytest.fixture(scope="module")
def small_pair():
    """Eight different sequences of a dozen features, 30 frames (rendered once for the module)."""
    pr = Pair(12, 30, batch=8, make_engine=False)
    pr.sigma = 0.0
    return pr


@pytest.fixture(scope="module")
def all_active(small_pair):
    """The engine that never pauses anybody: the blobs of every sequence after every step."""
    pr = small_pair
    e = engine_of(pr)
    blobs = []
    for k in range(pr.n_frames):
        e.go_one_step(pr.frame_batch(k), True)
        blobs.append(e.save_sequences())
    e.close()
    return blobs


# ------------------------------------------------------------------------------------------ 1 - 3: untouched, neighbours, oracle
def test_paused_means_untouched_neighbours_unaffected_oracle_parity(small_pair, all_active):
    pr = small_pair
    eng = engine_of(pr)
    assert np.array_equal(eng.active(), np.ones(8, np.uint8))
    masks = masks_for(8, 30)
    assert not masks[0][0] and all(not np.array_equal(masks[k], masks[k + 1]) for k in range(29))
    own, per_step = masked_run(pr, eng, masks, oracles=oracles_of(pr))
    paused_steps = [int(sum(1 - m[b] for m in masks)) for b in range(8)]
    assert paused_steps[1] == paused_steps[4] == paused_steps[7] == 0 and min(paused_steps[b] for b in (0, 2, 3, 5, 6)) >= 5
    for b in range(8):
        for j, blob in enumerate(own[b]):
            if paused_steps[b] == 0:       # never paused: the very blob of the all-active engine, position log and step count included
                assert blob == all_active[j][b], "sequence %d differs from the all-active engine after step %d" % (b, j)
            else:                          # paused now and then: after j + 1 of ITS frames, what the all-active engine held after j + 1 steps
                assert core(blob) == core(all_active[j][b]), "sequence %d differs after its frame %d" % (b, j)
                assert steps_of(blob) == j + 1
    eng.close()


# ------------------------------------------------------------------------------------------------- 4: every form of the step
@pytest.mark.parametrize("form", ["fusion0", "fusion1", "fusion2", "back_only", "exact_search", "groups2", "groups2_fusion0", "seams"])
def test_same_results_under_every_step_form(small_pair, all_active, form):
    pr = small_pair
    B = 264 if form == "back_only" else 8          # more than 256 sequences of a small capacity: the back side alone is fused
    n = 6 if form == "back_only" else 12
    eng = engine_of(pr, batch=B)
    eng.params_n_select = pr.params["number_of_features_to_select"]
    step = plain_step
    if form in ("fusion0", "groups2_fusion0"):
        eng.set_step_fusion(0)
    if form == "fusion2":
        eng.set_step_fusion(2)
    if form == "exact_search":
        eng.set_search_variant(0)
    if form in ("groups2", "groups2_fusion0"):
        eng.set_groups(2)
    if form == "seams":
        step = seam_step
    eng.set_profiling(2)
    masks = [np.tile(m, B // 8) for m in masks_for(8, n)]
    own, _ = masked_run(pr, eng, masks, step=step, oracles=oracles_of(pr))
    t = eng.kernel_times()
    fused_front, fused_back, plain = (t.get(q, {}).get("launches", 0) for q in ("k_small_front", "k_small_back", "k_finalize"))
    want = {"fusion0": (0, 0, n), "groups2_fusion0": (0, 0, 2 * n), "seams": (0, 0, n), "back_only": (0, n, 0), "groups2": (2 * n, 2 * n, 0)}.get(form, (n, n, 0))
    assert (fused_front, fused_back, plain) == want, t
    # the search and the front end are the same code in every form, and the one-stage and the fused update differ in rounding
    # only: against the all-active engine (fused) the forms that fuse are bit-identical, the others within the oracle's tolerance
    for b in range(8):
        for j, blob in enumerate(own[b]):
            if form in ("fusion1", "fusion2", "exact_search", "groups2"):
                assert core(blob) == core(all_active[j][b]), (form, b, j)
    eng.close()


def test_graph_replay_under_a_changing_mask_equals_direct_launches(small_pair):
    """A captured step replays under any mask: the mask is device data, not part of the graph's key.  Two engines on device
    frames, one in graph mode: the same blobs after every step, and no graph is dropped or re-captured by the mask."""
    pr = small_pair
    fb = pr.cam["width"] * pr.cam["height"]
    dev = _lib.DeviceBuffer(2 * 8 * fb, 0)
    direct, graph = engine_of(pr), engine_of(pr)
    graph.set_graph_mode(True)
    masks = masks_for(8, 14)
    seen = [0] * 8
    for k, mask in enumerate(masks):
        batch = np.stack([pr.frames[b][seen[b]] for b in range(8)])
        off = (k & 1) * 8 * fb
        direct.synchronize()
        graph.synchronize()
        dev.upload(batch, off)
        before = graph.save_sequences()
        for e in (direct, graph):
            e.set_active(mask)
            e.go_one_step(dev.ptr + off, True, on_device=True, seq_stride=fb)
        a, g = direct.save_sequences(), graph.save_sequences()
        assert a == g, "step %d: graph replay differs from direct launches" % k
        for b in range(8):
            if not mask[b]:
                assert core(g[b]) == core(before[b]) and steps_of(g[b]) == steps_of(before[b]), (k, b)
            else:
                seen[b] += 1
    assert len(set(seen)) > 1
    for e in (direct, graph):
        assert not e.status_flags().any()
        e.close()
    dev.free()


# ---------------------------------------------------------------- 5: sequence 0 paused while a map outgrows the fused step
@pytest.mark.parametrize("grow", [1, 0])
def test_sequence_zero_paused_while_a_map_outgrows_the_fused_step_known_features(grow):
    """Two sequences of 36 features step fused.  Sequence 0 is paused and four features are added to sequence `grow`
    (sl2_add_known_features ignores the mask): the engine must move to the one-stage kernels and stay there - with grow = 0 it
    is the PAUSED sequence whose map size the mailbox has to keep reporting, from the workgroup of sequence 0 which is itself
    paused - so that nothing is refused when sequence 0 is resumed."""
    pr = Pair(40, 12, batch=2, n_select=16, max_features=64, feature_counts=[40, 40], feature_sigma=0.004, make_engine=False)
    eng = Engine(pr.cam, pr.params, 2, 64)
    eng.set_vehicle_state(np.stack([s.xv0 for s in pr.specs]), np.stack([s.Pxx0 for s in pr.specs]))
    ora = []
    for b in range(2):
        o = oa.OracleSLAM(pr.cam, pr.params["delta_t"], 16)
        o.set_state(pr.specs[b].xv0, pr.specs[b].Pxx0)
        ora.append(o)

    def add(b, lo, hi):
        eng.add_known_features(pr.specs[b].feat_y[None, lo:hi], np.tile(pr.specs[b].poses[0], (1, hi - lo, 1)), pr.templates[b][None, lo:hi], seq0=b)
        for i in range(lo, hi):
            ora[b].add_known_feature(pr.specs[b].feat_y[i], pr.specs[b].poses[0], pr.templates[b][i])

    seen = [0, 0]

    def step(mask):
        eng.set_active(mask)
        eng.go_one_step(np.stack([pr.frames[b][seen[b]] for b in range(2)]), False)
        for b in range(2):
            if mask[b]:
                ora[b].go_one_step(pr.frames[b][seen[b]], False)
                seen[b] += 1
                assert np.abs(eng.total_state(b) - ora[b].total_state()).max() <= TOL_X, (b, seen)
                Po, Pe = ora[b].total_covariance(), eng.total_covariance(b)
                assert np.linalg.norm(Pe - Po) <= TOL_P * np.linalg.norm(Po), (b, seen)
                assert [f["successful"] for f in eng.features(b)] == [ora[b].feature(i)["successful"] for i in range(ora[b].num_features)]

    for b in range(2):
        add(b, 0, 36)
    eng.set_profiling(2)
    for _ in range(2):
        step([1, 1])
    t = eng.kernel_times()
    assert t["k_small_back"]["launches"] == 2 and "k_syrk" not in t, t
    eng.set_active([0, 1])
    add(grow, 36, 40)
    assert np.array_equal(eng.active(), [0, 1])
    frozen = core(eng.save_sequences(0, 1)[0])
    for _ in range(5):
        step([0, 1])
        assert core(eng.save_sequences(0, 1)[0]) == frozen
    t = eng.kernel_times()
    assert t["k_small_back"]["launches"] == 2 and t["k_syrk"]["launches"] == 5 and t["k_finalize"]["launches"] == 5, t
    for _ in range(3):
        step([1, 1])
    t = eng.kernel_times()
    assert t["k_small_back"]["launches"] == 2 and t["k_finalize"]["launches"] == 8, t
    assert seen == [5, 10]
    assert not (eng.status_flags() & SMALL_STEP_REFUSED).any() and not eng.status_flags().any()
    eng.close()


def test_sequence_zero_paused_while_a_map_outgrows_the_fused_step_with_mapping():
    """The same with feature initialisation: sequence 1 starts with 34 features and initialises more (with feature initialisation
    on, the host's bound on the map sizes runs two slots ahead of what the device last reported: 34 + 2 = 36 slots is the fused
    update's limit, and the first feature made - frame 14 in the oracle - crosses it); sequence 0 stands still.
    The step moves from k_small_back to the one-stage kernels when the map of sequence 1 reaches the fused update's limit
    (per-launch profiling shows both), no sequence is refused, sequence 1 follows its oracle and sequence 0, resumed at the
    end, follows its own."""
    cam, params, spec, frames, templates = make_mapping_sequence(n_known=34, n_frames=30)
    params = dict(params, number_of_features_to_select=16, number_of_features_to_keep_visible=60)
    s0, s1 = (oracle_for(cam, params, spec, templates, oa) for _ in range(2))
    eng = mapping_engine(cam, params, spec, templates, 64, batch=2)
    eng.set_profiling(2)
    eng.set_active([0, 1])
    frozen = None
    for k in range(1, 26):
        s1.go_one_step(frames[k], True, True)
        eng.go_one_step(np.stack([frames[k], frames[k]]), save_trajectory=True, enable_mapping=True)
        compare_mapping(eng, 1, s1, k)
        if k == 1:
            frozen = core(eng.save_sequences(0, 1)[0])           # (taken after the first step: the header's mapping_in_use is the ENGINE's and turns 1 with it)
            fresh = mapping_engine(cam, params, spec, templates, 64, batch=1)
            b0 = fresh.save_sequences()[0]
            assert frozen[256 - 8:] == core(b0)[256 - 8:] and steps_of(eng.save_sequences(0, 1)[0]) == 0      # everything behind the header: a sequence no step has touched
            fresh.close()
        assert core(eng.save_sequences(0, 1)[0]) == frozen, k
    t = eng.kernel_times()
    fused, plain = t.get("k_small_back", {}).get("launches", 0), t.get("k_finalize", {}).get("launches", 0)
    print("25 mapping steps with sequence 0 paused: %d fused, %d on the one-stage kernels" % (fused, plain))
    assert fused + plain == 25 and fused >= 5 and plain >= 5, t
    assert s1.mapping_info()["initialised"] >= 2
    eng.set_active([1, 0])
    frozen1 = core(eng.save_sequences(1, 1)[0])
    for k in range(1, 6):
        s0.go_one_step(frames[k], True, True)
        eng.go_one_step(np.stack([frames[k], frames[k]]), save_trajectory=True, enable_mapping=True)
        compare_mapping(eng, 0, s0, k)
        assert core(eng.save_sequences(1, 1)[0]) == frozen1, k
    assert not eng.status_flags().any()
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 6: mapping on
def test_paused_with_a_partial_feature_in_flight_then_resumed():
    """Two copies of the mapping sequence in one engine.  Sequence 1 is paused for four steps while its partially initialised
    feature is in flight, then goes on with the frames it missed: particles, drand48 stream, labels and events continue as its
    oracle's do (compare_mapping: events, labels, particle depths and search results exact), and it ends bit-identical to
    sequence 0 as it was after the same number of frames."""
    cam, params, spec, frames, templates = make_mapping_sequence(n_frames=45)
    s = [oracle_for(cam, params, spec, templates, oa) for _ in range(2)]
    eng = mapping_engine(cam, params, spec, templates, 16, batch=2)
    seen = [0, 0]
    blobs0 = {}
    paused_left, paused_done = 0, False
    for k in range(1, 41):
        if not paused_done and paused_left == 0 and k >= 5 and s[1].mapping_info()["n_partial"] == 1 and s[1].partial_feature(0)["attempts"] >= 2:
            paused_left, paused_done = 4, True
            assert len(eng.partial_features(1)) == 1
        mask = [1, 0 if paused_left else 1]
        before = eng.save_sequences(1, 1)[0]
        eng.set_active(mask)
        eng.go_one_step(np.stack([frames[seen[0] + 1], frames[seen[1] + 1]]), save_trajectory=True, enable_mapping=True)
        for b in range(2):
            if mask[b]:
                seen[b] += 1
                s[b].go_one_step(frames[seen[b]], True, True)
                compare_mapping(eng, b, s[b], k)
        blobs0[seen[0]] = eng.save_sequences(0, 1)[0]
        after = eng.save_sequences(1, 1)[0]
        if paused_left:
            assert core(after) == core(before) and steps_of(after) == steps_of(before), k
            paused_left -= 1
        else:
            assert core(after) == core(blobs0[seen[1]]), "frame %d of sequence 1 differs from frame %d of sequence 0" % (seen[1], seen[1])
    assert paused_done and seen == [40, 36]
    assert s[1].mapping_info()["converted"] >= 2
    assert not eng.status_flags().any()
    eng.close()


def test_one_sequence_paused_and_resumed_with_mapping_keeps_the_launch_rules():
    """tests/test_gpu_mapping.py: test_launches_follow_the_partial_features_the_previous_step_reported, with the one sequence
    paused in two steps out of seven.  A paused step still reports (the count its partial features stand at, from the paused
    path of k_map_update / k_map_finish), so every step - paused or not - is issued with exactly the launches the count
    before it asks for, and the run equals the oracle's over the frames the sequence saw."""
    cam, params, spec, frames, templates = make_mapping_sequence(n_frames=80)
    kpart = int(params["max_features_to_init_at_once"])
    s = oracle_for(cam, params, spec, templates, oa)
    eng = Engine(cam, params, 1, 128)
    eng.set_vehicle_state(spec.xv0[None], spec.Pxx0[None])
    eng.add_known_features(spec.feat_y[None], spec.xp_org()[None], templates[None])
    eng.set_profiling(2)
    states, n_partial_before, seen, paused = [], 0, 0, 0
    for k in range(1, 91):
        active = 0 if (k % 7 in (3, 4)) else 1
        states.append(0 if k == 1 else (1 if n_partial_before == 0 else (2 if n_partial_before >= kpart else 0)))
        eng.set_active([active])
        before = eng.save_sequences()[0]
        eng.go_one_step(frames[seen + 1][None], save_trajectory=True, enable_mapping=True)
        if active:
            seen += 1
            s.go_one_step(frames[seen], True, True)
            compare_mapping(eng, 0, s, k)
            n_partial_before = s.mapping_info()["n_partial"]
        else:
            paused += 1
            after = eng.save_sequences()[0]
            assert core(after) == core(before) and steps_of(after) == steps_of(before), k
    assert seen == 64 and paused == 26
    t = eng.kernel_times()
    n = lambda name: t.get(name, {}).get("launches", 0)
    want = {"k_map_find": states.count(0) + states.count(1), "k_map_create": states.count(0), "k_map_finish": states.count(1),
            "k_map_particles": states.count(0) + states.count(2), "k_map_me_search": states.count(0) + states.count(2),
            "k_map_update": states.count(0) + states.count(2)}
    have = {name: n(name) for name in want}
    print("90 waited mapping steps (26 paused): %d with every launch, %d starting without a partial feature, %d with every slot taken" %
          (states.count(0), states.count(1), states.count(2)), have)
    assert have == want and states.count(1) >= 10 and states.count(2) >= 10, (have, want)
    assert s.mapping_info()["converted"] >= 3
    assert not eng.status_flags().any()
    eng.close()


# ---------------------------------------------------------------------------------------------------------- 7: large maps
@pytest.mark.parametrize("n_features,batch,n_frames,panel", [(200, 4, 6, False), (288, 4, 4, True)])
def test_large_maps_two_sequences_paused_on_alternating_steps(n_features, batch, n_frames, panel):
    """640 x 480, 200 features (n = 613), four sequences, sequence 1 paused on the even steps and sequence 3 on the odd ones:
    the one-launch Cholesky and substitution of 13 blocks; then 288 features, whose 18 blocks are factored panel-wise and
    substituted in groups (k_chol_syrk, k_fwd_gemm: profiling shows them)."""
    cam = synth.default_camera(640, 480)
    pr = Pair(n_features, n_frames, batch=batch, cam=cam, feature_sigma=0.005, make_engine=False)
    pr.sigma = 0.005
    eng = engine_of(pr)
    eng.set_profiling(2)
    masks = [np.array([1, k % 2, 1, 1 - k % 2], np.uint8) for k in range(n_frames)]
    masked_run(pr, eng, masks, oracles=oracles_of(pr), tol=(TOL_X, TOL_P_LARGE))
    t = eng.kernel_times()
    assert ("k_chol_syrk" in t and "k_fwd_gemm" in t) == panel, sorted(t)
    assert t["k_syrk"]["launches"] == len(masks)
    _, cnt = eng.selection(0)
    assert cnt["measurement_size"] > 1.5 * n_features
    eng.close()


# ----------------------------------------------------------------------------------------------- 8: with the checkpoint calls
def test_reset_load_and_copy_into_a_paused_sequence(small_pair, all_active):
    pr = small_pair
    eng = engine_of(pr, batch=3)
    for k in range(10):
        eng.go_one_step(pr.frame_batch(k)[:3], True)
    src = eng.save_sequences(0, 1)[0]
    assert src == all_active[9][0]
    eng.set_active([1, 1, 0])
    eng.reset_sequences(2, 1)
    assert np.array_equal(eng.active(), [1, 1, 0])
    assert header_of(eng.save_sequences(2, 1)[0]).n_slots == 0
    eng.load_sequences([src], seq0=2)
    assert np.array_equal(eng.active(), [1, 1, 0])
    loaded = eng.save_sequences(2, 1)[0]
    assert core(loaded) == core(src) and steps_of(loaded) == 10
    for k in range(10, 13):                                   # three steps: sequences 0 and 1 go on, the loaded one stands still
        eng.go_one_step(pr.frame_batch(k)[:3], True)
        now = eng.save_sequences()
        assert core(now[2]) == core(src) and steps_of(now[2]) == 10, k
        assert now[0] == all_active[k][0] and now[1] == all_active[k][1], k
    eng.set_active([0, 0, 1])                                 # ... then it alone continues as the source did: frames 10, 11, 12 of sequence 0
    for j in range(10, 13):
        batch = pr.frame_batch(j)[:3].copy()
        batch[2] = pr.frames[0][j]
        eng.go_one_step(batch, True)
        now = eng.save_sequences(2, 1)[0]
        assert core(now) == core(all_active[j][0]) and steps_of(now) == j + 1, j
    # a copy into a paused sequence: taken, and the mask stays the destination engine's own
    eng.copy_sequences(eng, 2, 1, 0)
    assert np.array_equal(eng.active(), [0, 0, 1])
    assert core(eng.save_sequences(0, 1)[0]) == core(eng.save_sequences(2, 1)[0])
    assert not eng.status_flags().any()
    eng.close()


# ------------------------------------------------------------------------------------------------------------ 9: host side
def test_host_side_of_the_mask(small_pair):
    pr = small_pair
    L = _lib.load()
    eng = engine_of(pr, batch=4)
    assert np.array_equal(eng.active(), [1, 1, 1, 1])
    one = np.ones(8, np.uint8)
    for seq0, nseq in ((-1, 1), (0, 0), (0, 5), (3, 2), (4, 1)):
        assert L.sl2_set_active_sequences(eng.h, seq0, nseq, _lib.u8p(one), 0) == _lib.SL2_ERR_INVALID
        assert L.sl2_get_active_sequences(eng.h, seq0, nseq, _lib.u8p(one)) == _lib.SL2_ERR_INVALID
    assert L.sl2_set_active_sequences(eng.h, 0, 4, None, 0) == _lib.SL2_ERR_INVALID
    assert L.sl2_get_active_sequences(eng.h, 0, 4, None) == _lib.SL2_ERR_INVALID
    assert L.sl2_set_active_sequences(None, 0, 1, _lib.u8p(one), 0) == _lib.SL2_ERR_INVALID
    assert np.array_equal(eng.active(), [1, 1, 1, 1])
    eng.set_active([0, 7, 0], seq0=1)                         # any non-zero byte is "active"; a sub-range leaves the rest alone
    assert np.array_equal(eng.active(), [1, 0, 1, 0])
    assert np.array_equal(eng.active(1, 2), [0, 1])
    dev = _lib.DeviceBuffer(4, 0)
    dev.upload(np.array([0, 1, 255, 0], np.uint8))
    eng.set_active((dev.ptr, 4), on_device=True)
    assert np.array_equal(eng.active(), [0, 1, 1, 0])
    twin = engine_of(pr, batch=4)
    twin.set_active([0, 1, 1, 0])
    for k in range(3):
        eng.go_one_step(pr.frame_batch(k)[:4], True)
        twin.go_one_step(pr.frame_batch(k)[:4], True)
    assert eng.save_sequences() == twin.save_sequences()      # the device form and the host form are the same mask
    # sl2_get_step_work counts the active sequences only: the engine of four with two paused does the work of an engine of those two
    half = engine_of(pr, seqs=[1, 2], batch=2)
    for k in range(3):
        half.go_one_step(pr.frame_batch(k)[1:3], True)
    w4, w2 = eng.step_work(), half.step_work()
    assert w4 == w2 and w2["searched"] > 0 and w2["sum_n"] == 2 * (13 + 3 * 12), (w4, w2)
    for e in (eng, twin, half):
        e.close()
    dev.free()


def test_a_mask_set_behind_queued_steps_applies_to_later_steps_only(small_pair):
    """The engine's stream is held by a host function while 20 steps, a mask that pauses sequence 1, and 5 more steps are queued:
    the call returns without waiting (the queue is still held when it does), the caller's array may change at once, and the
    result is that of an engine that was never held - sequence 1 saw 20 steps, the others 25."""
    pr = small_pair
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipLaunchHostFunc.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    st = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(st)) == 0
    released = []
    hold = C.CFUNCTYPE(None, C.c_void_p)(lambda _arg: (time.sleep(0.3), released.append(1)) and None)
    fb = pr.cam["width"] * pr.cam["height"]
    frames = np.stack([pr.frame_batch(k)[:3] for k in range(25)])
    dev = _lib.DeviceBuffer(frames.nbytes, 0)
    dev.upload(frames)
    held = Engine(pr.cam, pr.params, 3, 12, stream=st.value)
    ref = engine_of(pr, batch=3)
    held.set_vehicle_state(np.stack([pr.specs[s].xv0 for s in range(3)]), np.stack([pr.specs[s].Pxx0 for s in range(3)]))
    for b in range(3):
        held.add_known_features(pr.specs[b].feat_y[None], np.tile(pr.specs[b].poses[0], (1, 12, 1)), pr.templates[b][None], seq0=b)
    held.synchronize()
    assert hip.hipLaunchHostFunc(st, C.cast(hold, C.c_void_p), None) == 0
    for k in range(20):
        held.go_one_step(dev.ptr + k * 3 * fb, True, on_device=True, seq_stride=fb)
    mask = np.array([1, 0, 1], np.uint8)
    held.set_active(mask)
    still_held = not released
    mask[:] = 1                                               # consumed before the call returned
    for k in range(20, 25):
        held.go_one_step(dev.ptr + k * 3 * fb, True, on_device=True, seq_stride=fb)
    assert still_held, "the queue drained before the mask was set: nothing was queued ahead of it"
    for k in range(25):
        if k == 20:
            ref.set_active([1, 0, 1])
        ref.go_one_step(frames[k], True)
    got, want = held.save_sequences(), ref.save_sequences()
    assert [steps_of(b) for b in got] == [25, 20, 25]
    assert got == want
    held.close()
    ref.close()
    dev.free()


# --------------------------------------------------------------------------------------------------------- 10: ragged ingest
def _ragged_dirs(tmp_path, W, H, counts):
    rng = np.random.RandomState(11)
    dirs, want = [], []
    for s, n in enumerate(counts):
        d = os.path.join(str(tmp_path), "seq%d" % s)
        os.makedirs(d)
        imgs = rng.randint(0, 256, size=(n, H, W)).astype(np.uint8)
        for k in range(n):
            ingest.write_pgm(os.path.join(d, "%05d.pgm" % k), imgs[k])
        dirs.append(d)
        want.append(imgs)
    return dirs, want


@pytest.mark.parametrize("zero_copy", [False, True])
def test_ragged_ingest_hands_out_until_the_longest_sequence_ends(tmp_path, zero_copy):
    W, H, counts = 64, 48, [5, 3, 4]
    dirs, want = _ragged_dirs(tmp_path, W, H, counts)
    L = _lib.load()
    g = ingest.FrameIngest(dirs, W, H, depth=4)
    if not zero_copy:
        g.set_zero_copy(0)
    assert list(g.frame_counts) == counts and g.frame_count == 3
    for k in range(5):
        ptr, stride, have = g.next_ragged()
        assert stride == W * H
        assert list(have) == [1 if k < n else 0 for n in counts], k
        host = np.zeros((3, H, W), np.uint8)
        _lib.check(L.sl2_dev_download(0, host.ctypes.data_as(_lib.vp), _lib.vp(ptr), host.nbytes))
        for s in range(3):
            if have[s]:
                assert np.array_equal(host[s], want[s][k]), (k, s)
    with pytest.raises(_lib.Sl2Error) as ei:
        g.next_ragged()
    assert ei.value.code == _lib.SL2_ERR_CAPACITY
    with pytest.raises(_lib.Sl2Error) as ei:                  # the two next-calls are not mixed on one grabber
        g.next()
    assert ei.value.code == _lib.SL2_ERR_INVALID
    g.close()
    g = ingest.FrameIngest(dirs, W, H, depth=4)               # an identical grabber: sl2_ingest_next keeps its meaning
    if not zero_copy:
        g.set_zero_copy(0)
    for k in range(3):
        ptr, stride = g.next()
        host = np.zeros((3, H, W), np.uint8)
        _lib.check(L.sl2_dev_download(0, host.ctypes.data_as(_lib.vp), _lib.vp(ptr), host.nbytes))
        for s in range(3):
            assert np.array_equal(host[s], want[s][k]), (k, s)
    with pytest.raises(_lib.Sl2Error) as ei:
        g.next()
    assert ei.value.code == _lib.SL2_ERR_CAPACITY
    with pytest.raises(_lib.Sl2Error) as ei:
        g.next_ragged()
    assert ei.value.code == _lib.SL2_ERR_INVALID
    g.close()


# ------------------------------------------------------------------------------------------------------- 11: the new example
@pytest.mark.parametrize("mapping", [False, True])
def test_ragged_example_prints_what_three_single_runs_print(tmp_path, mapping):
    """examples/ragged_monoslam on directories of 5, 3 and 4 frames (with --mapping: 25, 12 and 18, so that features are
    initialised) in one batch under the mask next_ragged hands out: per sequence the line examples/monoslam_adapter prints for
    the last frame of a run on that directory alone."""
    from test_gpu_headless_example import _write_scene
    exe = os.path.join(ROOT, "examples", "ragged_monoslam")
    ref = os.path.join(ROOT, "examples", "monoslam_adapter")
    if not (os.path.exists(exe) and os.path.exists(ref)):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    counts = [25, 12, 18] if mapping else [5, 3, 4]
    cam, params, spec, frames, templates = make_mapping_sequence(n_frames=max(counts) + 1)
    cfg, _ = _write_scene(str(tmp_path), cam, params, spec, frames, templates)
    dirs = []
    for s, n in enumerate(counts):
        d = os.path.join(str(tmp_path), "frames%d" % s)
        os.makedirs(d)
        for k in range(1, n + 1):
            ingest.write_pgm(os.path.join(d, "%05d.pgm" % k), frames[k])
        dirs.append(d)
    flags = ["--mapping"] if mapping else []
    args = [exe, "--cfg", cfg]
    for d in dirs:
        args += ["--frames", d]
    r = subprocess.run(args + flags, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("sequence ")]
    assert len(lines) == 3, r.stdout
    for s, d in enumerate(dirs):
        a = subprocess.run([ref, "--cfg", cfg, "--frames", d] + flags, capture_output=True, text=True, timeout=300)
        assert a.returncode == 0, a.stdout + a.stderr
        last = [l for l in a.stdout.splitlines() if l.startswith("frame ")][-1]
        assert lines[s] == "sequence %d  %s" % (s, last), (lines[s], last)
