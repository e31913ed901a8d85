"""k_build_AS_ahead against k_build_AS, bit for bit (sl2_update_build.hip).

The form that keeps a batch of rows of P in flight computes every entry of A^T and S by the expression of k_build_AS, so two
engines on the same inputs that differ in nothing but the form (TEST build: SL2_BUILD_SPLIT=1 gives one workgroup per sequence
at any batch size, SL2_BUILD_AHEAD=0 | 1 picks the form; step fusion off, so that every map goes through the one-stage path)
must agree exactly after every step: total state, total covariance and every field of sl2_get_features.

Shapes: ld = 64 with N = 5 .. 8 (every N mod 4: one full batch and a partial batch of 1 - 3, two full batches), ld = 320
with 100 features (25 full batches; also held to the oracle at the tolerances of tests/test_gpu_slam.py), ld = 1024 (N = 334,
the batch of two features).  Events: m mod 32 of 2, 16 and 18 (padding rows of A^T, identity part of S), a sequence without a
measurement, Q28 position errors beyond and inside the pose columns, a feature deleted in the middle of the map, a paused
sequence."""
import numpy as np
import pytest

from scenelib2_amd import _lib
from slam_helpers import Pair, compare_state

pytestmark = pytest.mark.gpu

TOL_X, TOL_P = 1e-12, 1e-11           # tests/test_gpu_slam.py: engine against the oracle
FEATURE_SIGMA = 0.004                 # a dense P: every live entry of A^T and S changes


def twins(pr, batch, max_features, monkeypatch, form="ahead<4>"):
    """(engine with k_build_AS, engine with k_build_AS_ahead), one workgroup per sequence in both: their update plans
    (sl2_update_plan.hpp, read back through the TEST build's hook) are k_build_AS<1,4> and the given ahead form, the dynamic
    LDS each form asks for, and otherwise the same plan."""
    lib = _lib.load_testing()
    out = []
    for ahead in ("0", "1"):
        monkeypatch.setenv("SL2_BUILD_SPLIT", "1")
        monkeypatch.setenv("SL2_BUILD_AHEAD", ahead)
        try:
            e = pr.make_engine_for(0, batch, max_features, feature_sigma=FEATURE_SIGMA, lib=lib)
        finally:
            monkeypatch.delenv("SL2_BUILD_SPLIT", raising=False)
            monkeypatch.delenv("SL2_BUILD_AHEAD", raising=False)
        e.set_step_fusion(False)
        out.append(e)
    p0, p1 = (e.debug_update_plan() for e in out)
    ld = (13 + 3 * max_features + 6 + 1 + 63) // 64 * 64
    nsel = min(pr.params["number_of_features_to_select"], max_features)
    assert (p0["build"], p1["build"]) == ("<1,4>", form), (p0, p1)
    assert p0["build_lds_bytes"] == 8 * 2 * 4 * ld and p1["build_lds_bytes"] == 8 * (2 * int(form[6]) * ld + 24 * nsel), (p0, p1)
    assert {k for k in p0 if p0[k] != p1[k]} == {"build", "build_lds_bytes"}, (p0, p1)
    assert p0["build_nsplit"] == 1 and p0["build_threads"] == ld
    return out


def assert_identical(e0, e1, batch, what):
    for b in range(batch):
        assert np.array_equal(e0.total_state(b), e1.total_state(b)), "%s seq %d: total state differs" % (what, b)
        assert np.array_equal(e0.total_covariance(b), e1.total_covariance(b)), "%s seq %d: total covariance differs" % (what, b)
        f0, f1 = e0.features(b, include_deleted=True), e1.features(b, include_deleted=True)
        assert len(f0) == len(f1), "%s seq %d: feature count differs" % (what, b)
        for a, c in zip(f0, f1):
            for key in a:
                assert np.array_equal(a[key], c[key]), "%s seq %d feature %d: %s differs" % (what, b, a["label"], key)
    assert np.array_equal(e0.status_flags(), e1.status_flags())


def seam_frame(engines, frames, n):
    for e in engines:
        e.kalman_filter_predict()
        e.auto_select_n_features(n)
        e.make_measurements(frames)
        e.kalman_filter_update()
        e.finish_step(False)


def measured(e, batch):
    return [e.selection(b)[1]["measurement_size"] for b in range(batch)]


@pytest.mark.parametrize("N", [5, 6, 7, 8])
def test_small_maps_every_remainder_of_the_batch(N, monkeypatch):
    """ld = 64: N = 5, 6, 7 are one full batch and a partial one of 1, 2, 3 features; N = 8 is two full batches."""
    B = 2
    pr = Pair(N, 3, batch=B, make_engine=False, feature_sigma=FEATURE_SIGMA)
    e0, e1 = twins(pr, B, N, monkeypatch)
    seen = set()
    for k in range(3):
        seam_frame((e0, e1), pr.frame_batch(k), N)
        seen.update(measured(e1, B))
        assert_identical(e0, e1, B, "N = %d frame %d" % (N, k))
    print("build-ahead N=%d m seen %s" % (N, sorted(seen)))
    assert 2 * N in seen, sorted(seen)
    assert not e1.status_flags().any()


def test_headline_map_full_batches_and_oracle(monkeypatch):
    """100 features, all selected: ld = 320, 25 full batches of four.  Both forms against each other exactly, the new one
    against the oracle at the tolerances of the parity tests."""
    B, N = 2, 100
    pr = Pair(N, 2, batch=B, make_engine=False, feature_sigma=FEATURE_SIGMA)
    e0, e1 = twins(pr, B, N, monkeypatch)
    for k in range(2):
        for b in range(B):
            pr.oracles[b].go_one_step(pr.frames[b][k], False)
        for e in (e0, e1):
            e.go_one_step(pr.frame_batch(k), False)
        ms = measured(e1, B)
        print("build-ahead N=100 frame %d m %s" % (k, ms))
        assert max(ms) >= 160, ms                      # (most of the 25 batches are live)
        assert_identical(e0, e1, B, "N = 100 frame %d" % k)
        worst = compare_state(pr.oracles, e1, TOL_X, TOL_P)
        print("build-ahead N=100 frame %d against the oracle: |dx| %.3e, rel |dP| %.3e" % (k, worst["x"], worst["P"]))
    assert not e1.status_flags().any()


def test_largest_ld(monkeypatch):
    """334 slots: ld = 1024, the largest the form takes (two features per batch there); 24 live features, m = 48 then 18."""
    B = 2
    pr = Pair(24, 2, batch=B, make_engine=False, feature_sigma=FEATURE_SIGMA)
    e0, e1 = twins(pr, B, 334, monkeypatch, form="ahead<2>")
    seen = set()
    for k, n in enumerate((24, 9)):
        seam_frame((e0, e1), pr.frame_batch(k), n)
        seen.update(measured(e1, B))
        assert_identical(e0, e1, B, "ld = 1024 frame %d" % k)
    print("build-ahead ld=1024 m seen %s" % sorted(seen))
    assert {48, 18} <= seen, sorted(seen)
    assert not e1.status_flags().any()


def test_events_on_one_batch(monkeypatch):
    """Three sequences of 24, 0 and 24 features (the second measures nothing on any frame).  Frames 0 - 3 select 24, 9, 8, 1:
    m mod 32 = 16, 18, 16, 2.  Then Q28 position errors on four features of sequence 0 - two blocks beyond the pose columns
    (columns 10 and 7), two inside them (4 and 1) -, a feature deleted in the middle of the map, and sequence 2 paused for a
    frame and resumed."""
    B, N = 3, 24
    counts = [N, 0, N]
    pr = Pair(N, 9, batch=B, make_engine=False, feature_counts=counts, feature_sigma=FEATURE_SIGMA)
    e0, e1 = twins(pr, B, N, monkeypatch)
    both = (e0, e1)
    residues = set()
    for k, n in enumerate((24, 9, 8, 1)):
        seam_frame(both, pr.frame_batch(k), n)
        ms = measured(e1, B)
        print("build-ahead events frame %d m %s" % (k, ms))
        assert ms[1] == 0
        residues.update(m % 32 for m in ms if m)
        assert_identical(e0, e1, B, "events frame %d" % k)
    assert {2, 16, 18} <= residues, sorted(residues)
    # Q28
    wrong = ((2, 10), (3, 7), (4, 4), (5, 1))
    for slot, hc in wrong:
        for e in both:
            e.debug_set_position_error(0, slot, 13 + 3 * slot - hc)
    hit = set()
    for k in (4, 5):
        seam_frame(both, pr.frame_batch(k), N)
        feats = e1.features(0)
        assert [feats[s]["pos"] for s, _ in wrong] == [hc for _, hc in wrong]
        hit.update(hc for s, hc in wrong if feats[s]["selected"] and feats[s]["success"])
        assert_identical(e0, e1, B, "events frame %d (Q28)" % k)
    print("build-ahead events Q28 columns measured %s" % sorted(hit))
    assert hit & {10, 7} and hit & {4, 1}, "the misplaced blocks were not measured on both sides of column 7: %s" % sorted(hit)
    # a feature deleted in the middle of the map
    for e in both:
        done = e.delete_features(np.array([12, -1, 12], dtype=np.int32))
        assert done[0] and done[2]
    seam_frame(both, pr.frame_batch(6), N)
    assert_identical(e0, e1, B, "events frame 6 (after a deletion)")
    # a paused sequence
    for e in both:
        e.set_active([1, 1, 0])
    frozen = (e1.total_state(2), e1.total_covariance(2))
    seam_frame(both, pr.frame_batch(7), N)
    assert np.array_equal(e1.total_state(2), frozen[0]) and np.array_equal(e1.total_covariance(2), frozen[1])
    assert_identical(e0, e1, B, "events frame 7 (sequence 2 paused)")
    for e in both:
        e.set_active([1, 1, 1])
    seam_frame(both, pr.frame_batch(8), N)
    assert_identical(e0, e1, B, "events frame 8 (resumed)")
    assert not e1.status_flags().any()
