"""The fused small-map step (sl2_small.hip: k_small_front, the search, k_small_back) under graph replay and with misplaced
recorded feature positions (Q28).

The fused step is the default for the reference's own workload (at most 16 features measured, one partially initialised
feature at a time, live maps of at most 36 slots).  Two things of it are decided per step and are invisible to a test that
only runs it eagerly on a map of fixed size:
  - k_small_back's LDS panel is 64 or 128 columns wide, chosen by the host from its bound on the live map; a captured step
    bakes the choice in, so a map that grows past it between two replays must get a step captured anew;
  - a known feature added behind a partially initialised one is three columns off in H once that one converts
    (feature.cpp:254); the fused update must place its block where the ten-launch step and the reference do.

Fused modes (sl2_step_plan.hpp: small_step_mode): 1 = both sides of the search fused (a few sequences), 2 = the back side only
(more than 256 sequences at a capacity with ld < 256: three distinct sequences tiled to 300, a sample of them compared).
Every test shows by per-launch profiling on a directly launched engine that the fused kernels ran."""
import numpy as np
import pytest

import oracle_api as oa
from conftest import rel_fro
from mapping_helpers import make_mapping_sequence, oracle_for
from scenelib2_amd import Engine, _lib
from slam_helpers import Pair

pytestmark = pytest.mark.gpu

TOL_X, TOL_P = 1e-12, 1e-11            # tests/test_gpu_slam.py: engine against the oracle
TOL_X_MAP, TOL_P_MAP = 1e-11, 1e-10    # tests/test_gpu_mapping.py: the same with feature initialisation on
TWIN_X, TWIN_P = 1e-13, 1e-12          # fused step against the ten-launch step

BATCH = {1: 3, 2: 300}                 # fused mode -> batch that reaches it
SAMPLE = {1: (0, 1, 2), 2: (0, 1, 2, 151, 299)}
FEATURE_KEYS = ("label", "active", "selected", "success", "attempted", "successful", "pos", "fully_initialised", "state_size")


def _tile(arrays, B):
    """Per-sequence arrays of the three distinct sequences -> [B][...], sequence b = distinct sequence b % 3."""
    return np.stack([arrays[b % len(arrays)] for b in range(B)])


def _assert_fused_ran(eng, mode):
    t = eng.kernel_times()
    assert "k_small_back" in t and "k_syrk" not in t and "k_build_AS" not in t, sorted(t)
    if mode == 1:
        assert "k_small_front" in t and "k_predict" not in t, sorted(t)
    else:
        assert "k_small_front" not in t and "k_predict" in t, sorted(t)


def _assert_same_features(a, b, seqs, exact=True):
    for s in seqs:
        fa, fb = a.features(s, include_deleted=True), b.features(s, include_deleted=True)
        assert len(fa) == len(fb), s
        for p, q in zip(fa, fb):
            for key in FEATURE_KEYS:
                assert p[key] == q[key], (s, p["label"], key, p[key], q[key])
            assert np.array_equal(p["z"], q["z"]), (s, p["label"])
            if exact:
                assert np.array_equal(p["h"], q["h"]), (s, p["label"])
        sa, ca = a.selection(s)
        sb, cb = b.selection(s)
        assert list(sa) == list(sb) and ca == cb, s


def _assert_near(a, b, seqs):
    """Fused engine a against the ten-launch engine b: integer outputs identical, state and covariance within rounding."""
    _assert_same_features(a, b, seqs, exact=False)
    for s in seqs:
        assert np.abs(a.total_state(s) - b.total_state(s)).max() <= TWIN_X, s
        assert rel_fro(a.total_covariance(s), b.total_covariance(s)) <= TWIN_P, s


def _assert_oracle(eng, oracles, seqs, tol_x, tol_p):
    for s in seqs:
        o = oracles[s % len(oracles)]
        assert int(eng.total_state_sizes(s, 1)[0]) == o.total_state_size, s
        assert np.abs(eng.total_state(s) - o.total_state()).max() <= tol_x, s
        assert rel_fro(eng.total_covariance(s), o.total_covariance()) <= tol_p, s
        feats = eng.features(s)
        assert [f["label"] for f in feats] == [o.feature(i)["label"] for i in range(o.num_features)], s
        assert [(f["attempted"], f["successful"], f["pos"]) for f in feats] == \
               [(o.feature(i)["attempted"], o.feature(i)["successful"], o.feature(i)["pos"]) for i in range(o.num_features)], s


class GraphTwin:
    """Two engines with identical inputs: engine 0 replays captured steps (graph mode, device-resident frames from two
    alternating buffers), engine 1 launches the same steps directly, with per-launch profiling.  Between steps the same calls
    go to both (`both`)."""

    def __init__(self, cam, params, B, capacity, setup, lib=None):
        self.W, self.H, self.B = cam["width"], cam["height"], B
        self.engines = []
        for graph in (True, False):
            e = Engine(cam, params, B, capacity, lib=lib)
            setup(e)
            e.set_graph_mode(graph)
            if not graph:
                e.set_profiling(2)
            self.engines.append(e)
        self.bufs = [_lib.DeviceBuffer(B * self.W * self.H, 0) for _ in range(2)]
        self.k = 0

    @property
    def eager(self):
        return self.engines[1]

    def both(self, fn):
        return [fn(e) for e in self.engines]

    def step(self, frames, mapping=False):
        buf = self.bufs[self.k & 1]
        self.k += 1
        buf.upload(np.ascontiguousarray(frames, dtype=np.uint8))
        for e in self.engines:
            e.go_one_step(buf.ptr, save_trajectory=True, enable_mapping=mapping, on_device=True, seq_stride=self.W * self.H)
            e.synchronize()

    def compare(self, seqs):
        g, d = self.engines
        assert not g.status_flags().any() and not d.status_flags().any(), (np.flatnonzero(g.status_flags()), np.flatnonzero(d.status_flags()))
        for s in seqs:
            assert np.array_equal(g.total_state(s), d.total_state(s)), s
            assert np.array_equal(g.total_covariance(s), d.total_covariance(s)), s
            assert np.array_equal(g.trajectory(s), d.trajectory(s)), s
        _assert_same_features(g, d, seqs)


class KnownFeatures:
    """Three distinct synthetic sequences (slam_helpers.Pair's frames) whose known features are added in ranges, to the
    engines (tiled to the batch) and to one oracle per distinct sequence alike."""

    def __init__(self, n_features, n_frames, n_select, B):
        self.pr = Pair(n_features, n_frames, batch=3, n_select=n_select, make_engine=False)
        self.B = B
        self.oracles = []
        for spec in self.pr.specs:
            o = oa.OracleSLAM(self.pr.cam, self.pr.params["delta_t"], n_select)
            o.set_state(spec.xv0, spec.Pxx0)
            self.oracles.append(o)

    def setup(self, e):
        e.set_vehicle_state(_tile([s.xv0 for s in self.pr.specs], self.B), _tile([s.Pxx0 for s in self.pr.specs], self.B))

    def add(self, engines, lo, hi):
        specs, tpl = self.pr.specs, self.pr.templates
        y = _tile([s.feat_y[lo:hi] for s in specs], self.B)
        xp = _tile([np.tile(s.poses[0], (hi - lo, 1)) for s in specs], self.B)
        p = _tile([t[lo:hi] for t in tpl], self.B)
        for e in engines:
            e.add_known_features(y, xp, p)
        for j, o in enumerate(self.oracles):
            for i in range(lo, hi):
                o.add_known_feature(specs[j].feat_y[i], specs[j].poses[0], tpl[j][i])

    def frames(self, k):
        return _tile(list(self.pr.frame_batch(k)), self.B)

    def step_oracles(self, k):
        for j, o in enumerate(self.oracles):
            o.go_one_step(self.pr.frames[j][k], True)


# ---------------------------------------------------------------- A: graph replay across host-side map changes

@pytest.mark.parametrize("mode", [1, 2])
def test_graph_replay_follows_known_features_across_the_panel_width(mode):
    """12 known features (k_small_back's panel: 64 columns) step under graph replay; sl2_add_known_features then takes every
    sequence to 18 slots (13 + 54 + 1 > 64: the kernel needs the 128-column panel).  The step captured at 12 slots must not be
    replayed: graph and direct launches bit-identical, and the direct one the oracle's, before and after."""
    B = BATCH[mode]
    kf = KnownFeatures(18, 10, 10, B)
    tw = GraphTwin(kf.pr.cam, kf.pr.params, B, 40, kf.setup)
    kf.add(tw.engines, 0, 12)
    for k in range(10):
        if k == 4:
            kf.add(tw.engines, 12, 18)
        tw.step(kf.frames(k))
        kf.step_oracles(k)
        tw.compare(SAMPLE[mode])
        _assert_oracle(tw.eager, kf.oracles, SAMPLE[mode][:3], TOL_X, TOL_P)
    assert all(int(n) == 13 + 3 * 18 for n in tw.eager.total_state_sizes())
    _assert_fused_ran(tw.eager, mode)
    assert tw.eager.kernel_times()["k_small_back"]["launches"] == 10


@pytest.mark.parametrize("mode", [1, 2])
def test_graph_replay_follows_a_map_that_grows_with_a_partial_feature_in_flight(mode):
    """Feature initialisation on: the map grows by itself, and with a partially initialised feature in flight (six more
    columns) the kernel needs the 128-column panel from 15 slots on.  12 known features, three distinct sequences; the run
    must cross from 14 slots to 15 with a partial feature in flight under graph replay, bit-identical to direct launches,
    and the direct launches equal the oracle's event for event."""
    B, F = BATCH[mode], 16
    seqs = [make_mapping_sequence(seed=7 + j, n_known=12, n_frames=F) for j in range(3)]
    cam = seqs[0][0]
    params = dict(seqs[0][1])
    params["number_of_features_to_keep_visible"] = 16          # 12 visible known features must not shut the gate
    oracles = [oracle_for(cam, params, spec, tpl, oa) for _, _, spec, _, tpl in seqs]

    def setup(e):
        e.set_vehicle_state(_tile([q[2].xv0 for q in seqs], B), _tile([q[2].Pxx0 for q in seqs], B))
        e.add_known_features(_tile([q[2].feat_y for q in seqs], B), _tile([q[2].xp_org() for q in seqs], B),
                             _tile([q[4] for q in seqs], B))

    tw = GraphTwin(cam, params, B, 40, setup)
    reached = []                                               # (slots, partial features in flight) of sequence 0 per step
    for k in range(1, F + 1):
        tw.step(_tile([q[3][k] for q in seqs], B), mapping=True)
        for o, q in zip(oracles, seqs):
            o.go_one_step(q[3][k], True, True)
        tw.compare(SAMPLE[mode])
        _assert_oracle(tw.eager, oracles, SAMPLE[mode][:3], TOL_X_MAP, TOL_P_MAP)
        for s in SAMPLE[mode]:
            info, want = tw.eager.partial_feature(s)["info"], oracles[s % 3].mapping_info()
            assert [info[key] for key in ("initialised", "converted", "deleted", "n_partial")] == \
                   [want[key] for key in ("initialised", "converted", "deleted", "n_partial")], (k, s)
        reached.append((len(tw.eager.features(0, include_deleted=True)), tw.eager.partial_feature(0)["info"]["n_partial"]))
    print("slots, partial features in flight:", reached)
    assert any(n <= 14 for n, _ in reached) and any(n >= 15 and p == 1 for n, p in reached), reached
    _assert_fused_ran(tw.eager, mode)
    assert tw.eager.kernel_times()["k_small_back"]["launches"] == F


@pytest.mark.parametrize("mode", [1, 2])
def test_graph_replay_follows_a_map_out_of_the_fused_step(mode):
    """30 known features step fused under graph replay; ten more take the map past the fused update's 36 slots and the step
    to the ten launches (test_gpu_slam.py::test_step_kernels_follow_the_live_map_size, here under graph replay)."""
    B = BATCH[mode]
    kf = KnownFeatures(40, 8, 16, B)
    tw = GraphTwin(kf.pr.cam, kf.pr.params, B, 48, kf.setup)     # (ld = 192: mode 2 at 300 sequences)
    kf.add(tw.engines, 0, 30)
    for k in range(8):
        if k == 4:
            _assert_fused_ran(tw.eager, mode)
            kf.add(tw.engines, 30, 40)
        tw.step(kf.frames(k))
        kf.step_oracles(k)
        tw.compare(SAMPLE[mode])
        _assert_oracle(tw.eager, kf.oracles, SAMPLE[mode][:3], TOL_X, TOL_P)
    t = tw.eager.kernel_times()
    assert t["k_small_back"]["launches"] == 4 and t["k_syrk"]["launches"] == 4 and t["k_finalize"]["launches"] == 4, t


@pytest.mark.parametrize("mode", [1, 2])
def test_graph_replay_after_calls_that_change_the_map_between_steps(mode):
    """Calls between steps that change the device state but not which launches the step consists of: delete_features,
    set_feature_covariances, set_vehicle_state and a manual initialise_feature.  After each, the replayed step must still
    equal the directly launched one bit for bit (and the direct one the oracle's as long as the oracle can follow:
    up to and including the deletion)."""
    B = BATCH[mode]
    seqs = [make_mapping_sequence(seed=7 + j, n_known=12, n_frames=14) for j in range(3)]
    cam, params = seqs[0][0], seqs[0][1]
    oracles = [oracle_for(cam, params, spec, tpl, oa) for _, _, spec, _, tpl in seqs]

    def setup(e):
        e.set_vehicle_state(_tile([q[2].xv0 for q in seqs], B), _tile([q[2].Pxx0 for q in seqs], B))
        e.add_known_features(_tile([q[2].feat_y for q in seqs], B), _tile([q[2].xp_org() for q in seqs], B),
                             _tile([q[4] for q in seqs], B))

    tw = GraphTwin(cam, params, B, 40, setup)
    labels = np.full(B, -1, dtype=np.int32)
    labels[0::3] = 6                                           # one sequence in three loses its feature 6
    for k in range(1, 15):
        if k == 3:
            done = tw.both(lambda e: e.delete_features(labels))
            assert np.array_equal(done[0], labels >= 0) and np.array_equal(done[1], labels >= 0)
            oracles[0].delete_feature(6)
        elif k == 5:
            Pyy = np.tile(np.diag([2e-5, 1e-5, 3e-5]), (B, 4, 1, 1))
            tw.both(lambda e: e.set_feature_covariances(Pyy))
        elif k == 7:
            xv, Pxx = tw.engines[1].get_vehicle_state()
            xv[:, 0:3] += 1e-3
            Pxx[:, 0:3, 0:3] += np.eye(3) * 1e-6
            tw.both(lambda e: e.set_vehicle_state(xv, Pxx))
        elif k == 10:
            uv = np.tile([[171, 97], [-1, -1], [150, 110]], (B // 3, 1))
            created = tw.both(lambda e: e.initialise_feature(_tile([q[3][k - 1] for q in seqs], B), uv))
            assert np.array_equal(created[0], created[1]) and created[0][0]
        tw.step(_tile([q[3][k] for q in seqs], B))
        if k < 5:
            for o, q in zip(oracles, seqs):
                o.go_one_step(q[3][k], True, False)
            _assert_oracle(tw.eager, oracles, SAMPLE[mode][:3], TOL_X, TOL_P)
        tw.compare(SAMPLE[mode])
    assert tw.eager.partial_feature(0)["info"]["initialised"] >= 1
    _assert_fused_ran(tw.eager, mode)


def test_graph_replay_captures_once_per_buffer_and_step_plan():
    """A captured step is keyed by its frame buffer and its step plan (sl2_step_plan.hpp).  One sequence at capacity 128
    (ld = 448), frames alternating between two device buffers; sl2_add_known_features - which drops no captured step - puts the
    map at 4 slots (k_small_back with the 64-column panel), then 20 (the 128-column panel), then 40 (the one-stage kernels), six
    steps in each.  sl2_debug_graph_captures of the TEST build must read 2, 4 and 6: one capture per (buffer, plan), none for a
    repeat, none lost to eviction - and every step bit-identical to direct launches."""
    T = _lib.load_testing()
    kf = KnownFeatures(40, 18, 10, 1)
    tw = GraphTwin(kf.pr.cam, kf.pr.params, 1, 128, kf.setup, lib=T)
    k, lo = 0, 0
    for hi, captures in ((4, 2), (20, 4), (40, 6)):
        kf.add(tw.engines, lo, hi)
        lo = hi
        for _ in range(6):
            tw.step(kf.frames(k))
            tw.compare((0,))
            k += 1
        assert [T.sl2_debug_graph_captures(e.h) for e in tw.engines] == [captures, 0], hi
    assert int(tw.eager.total_state_sizes()[0]) == 13 + 3 * 40
    t = tw.eager.kernel_times()
    assert t["k_small_front"]["launches"] == 12 and t["k_small_back"]["launches"] == 12 and t["k_syrk"]["launches"] == 6, t


# ---------------------------------------------------------------- B: Q28 offsets on the fused update

@pytest.mark.parametrize("mode", [1, 2])
def test_q28_on_the_fused_update_inside_the_vehicle_state_and_below_column_zero(mode):
    """test_gpu_slam.py::test_q28_block_inside_the_vehicle_state_and_below_column_zero on an engine that fuses (24 features,
    12 measured: one 32-row block).  Recorded positions forced through the test hooks put dh_by_dy blocks at columns 10, 7,
    4 and 1 (the last two overwrite pose coefficients, monoslam.cpp:562-565) in sequence 0: against the oracle's set_block
    overwrite and against the ten-launch step; then one block below column 0 in sequence 1, which raises
    SL2_STATUS_REFERENCE_OUT_OF_BOUNDS for that sequence only and nothing else."""
    B, N = BATCH[mode], 24
    pr = Pair(N, 6, batch=3, n_select=12, feature_sigma=0.004, make_engine=False)
    engs = []
    for fused in (1, 0):
        e = Engine(pr.cam, pr.params, B, N)
        e.set_step_fusion(fused)
        e.set_vehicle_state(_tile([s.xv0 for s in pr.specs], B), _tile([s.Pxx0 for s in pr.specs], B))
        e.add_known_features(_tile([s.feat_y for s in pr.specs], B), _tile([np.tile(s.poses[0], (N, 1)) for s in pr.specs], B),
                             _tile(pr.templates, B))
        e.set_feature_covariances(np.tile(np.eye(3) * 0.004 ** 2, (B, N, 1, 1)))
        e.set_profiling(2)
        engs.append(e)
    eng, twin = engs

    def step(k):
        frames = _tile(list(pr.frame_batch(k)), B)
        for e in engs:
            e.go_one_step(frames, False)
        for b in range(3):
            pr.oracles[b].go_one_step(pr.frames[b][k], False)
        _assert_near(eng, twin, SAMPLE[mode])
        for b in range(3):
            o = pr.oracles[b]
            assert np.abs(eng.total_state(b) - o.total_state()).max() <= TOL_X, (k, b)
            assert rel_fro(eng.total_covariance(b), o.total_covariance()) <= TOL_P, (k, b)

    step(0)
    for slot, hc in ((2, 10), (3, 7), (4, 4), (5, 1)):
        for e in engs:
            e.debug_set_position_error(0, slot, 13 + 3 * slot - hc)
        pr.oracles[0].set_feature_position(slot, hc)
    for k in range(1, 4):
        step(k)
        feats = eng.features(0)
        assert [feats[s]["pos"] for s in (2, 3, 4, 5)] == [10, 7, 4, 1]
        assert sum(1 for s in (2, 3, 4, 5) if feats[s]["selected"] and feats[s]["success"]) >= 3, "the misplaced blocks were never measured"
    assert not eng.status_flags().any() and not twin.status_flags().any()
    # below column 0: t = slot - err / 3 <= -5  <=>  13 + 3 t < 0
    for e in engs:
        e.debug_set_position_error(1, 1, 18 + 3)                  # slot 1: t = 1 - 7 = -6
        e.go_one_step(_tile(list(pr.frame_batch(4)), B), False)
    for e in engs:
        st = e.status_flags()
        assert st[1] == 4 and not np.delete(st, 1).any(), np.flatnonzero(st)
    xe, Pe = eng.get_vehicle_state()
    assert np.isfinite(xe).all() and np.isfinite(Pe).all()
    _assert_near(eng, twin, SAMPLE[mode])
    _assert_fused_ran(eng, mode)


def test_q28_through_the_public_api_on_the_fused_update():
    """No hooks: feature initialisation on (one feature at a time, as shipped), and two known features added while a partially
    initialised feature is in flight.  They land in slots behind it; when it converts, the reference records their positions
    three columns low (feature.cpp:254) and from then on places their dh_by_dy blocks there (monoslam.cpp:564).  The fused step
    (7 features measured: one 32-row block) against the mapping oracle and against the ten-launch step, through the
    conversion and the measurements of the misplaced features that follow."""
    F, n0, n_known = 16, 5, 7
    cam, params, spec, frames, templates = make_mapping_sequence(n_known=n_known, n_frames=F)
    xo = spec.xp_org()
    o = oa.OracleSLAM(cam, params["delta_t"], params["number_of_features_to_select"])
    o.set_mapping_params(params)
    o.set_state(spec.xv0, spec.Pxx0)
    engs = []
    for fused in (1, 0):
        e = Engine(cam, params, 1, 32)
        e.set_step_fusion(fused)
        e.set_vehicle_state(spec.xv0[None], spec.Pxx0[None])
        e.set_profiling(2)
        engs.append(e)
    eng, twin = engs

    def add(lo, hi):
        for e in engs:
            e.add_known_features(spec.feat_y[None, lo:hi], xo[None, lo:hi], templates[None, lo:hi])
        for i in range(lo, hi):
            o.add_known_feature(spec.feat_y[i], xo[i], templates[i])

    add(0, n0)
    added_at, converted_at_add, misplaced, measured = None, None, 0, 0
    for k in range(1, F + 1):
        if added_at is None and k >= 2 and eng.partial_feature(0)["info"]["n_partial"] == 1:
            assert o.mapping_info()["n_partial"] == 1
            converted_at_add = o.mapping_info()["converted"]
            add(n0, n_known)
            added_at = k
        o.go_one_step(frames[k], True, True)
        for e in engs:
            e.go_one_step(frames[k][None], save_trajectory=True, enable_mapping=True)
        info, got = o.mapping_info(), eng.partial_feature(0)["info"]
        assert [got[key] for key in ("initialised", "converted", "deleted", "n_partial")] == \
               [info[key] for key in ("initialised", "converted", "deleted", "n_partial")], (k, got, info)
        _assert_oracle(eng, [o], (0,), TOL_X_MAP, TOL_P_MAP)
        _assert_near(eng, twin, (0,))
        kinds = o.feature_kinds()
        slot_of = {f["label"]: s for s, f in enumerate(eng.features(0, include_deleted=True))}
        pos = 13
        for i, fe in enumerate(eng.features(0)):
            fo = o.feature(i)
            if fo["pos"] != pos:                               # a recorded position off its true one: Q28
                assert fe["pos"] == fo["pos"] and fe["pos"] != 13 + 3 * slot_of[fe["label"]], (k, fe["label"], fe["pos"])
                misplaced += 1
                measured += int(fe["selected"] and fe["success"])
            pos += int(kinds[i][0])
    assert added_at is not None and o.mapping_info()["converted"] > converted_at_add, "the partial feature never converted"
    assert misplaced > 0, "Q28 never showed"
    assert measured > 0, "no feature with a misplaced position was measured: the fused update's H placement went untested"
    assert not eng.status_flags().any() and not twin.status_flags().any()
    _assert_fused_ran(eng, 1)
