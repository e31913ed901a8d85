"""The streaming accesses of the dense EKF update (load_stream / store_stream, sl2_update_dev.hpp): k_build_AS_ahead reads the
rows of P and writes A^T with them, k_fwdsub_lds reads A^T and writes V^T with them.  A hint changes no value, so what is held
here is what the kernels' edges must leave behind whatever the cache policy: the oracle's state, a bitwise symmetric P, zeros
in everything of P that is not live state, and a paused sequence left alone.  (Values bit for bit: tests/test_gpu_build_as_ahead.py
and tests/test_gpu_ekf_update_edges.py.)

The engines are the TEST build's with SL2_BUILD_SPLIT=1, SL2_BUILD_AHEAD=1 (one workgroup per sequence at any batch size: the form
the headline batch takes, as in tests/test_gpu_build_as_ahead.py), SL2_NO_KSPLIT (k_fwdsub_lds instead of the small batches'
k_fwdsub_ksplit) and step fusion off; the plan is read back and asserted.

Shapes (every feature of every active sequence is measured, asserted):
  * ld = 128, 25 slots, four sequences of 25, 23, 24 and 25 features, the last paused in the second step: m = 50, 46 and 48 are
    two 32-row blocks - the second over half, a half block with a short tail, exactly a half block; the build's partial batch
    holds 1, 3 and 0 features behind six or five full ones; k_fwdsub_lds<2> has J = 1 and its half block row; k_syrk has the
    off-diagonal tile (0, 1) with its mirror and, in tile (1, 1), the quarter that holds column ld - 1; the sequences of 23 and 24
    features leave never-used slots.
  * ld = 64, 7 slots, three sequences of 7, 5 and 6 features (m = 14, 10, 12 <= 16: one block, less than half), the last paused
    in the second step."""
import numpy as np
import pytest

from scenelib2_amd import _lib
from slam_helpers import Pair, compare_state

pytestmark = pytest.mark.gpu

TOL_X, TOL_P = 1e-12, 1e-11           # tests/test_gpu_slam.py: engine against the oracle
FEATURE_SIGMA = 0.004                 # a dense P: every live entry of A^T, V^T and P changes


def hinted_engine(pr, max_features, monkeypatch):
    switches = {"SL2_BUILD_SPLIT": "1", "SL2_BUILD_AHEAD": "1", "SL2_NO_KSPLIT": "1"}
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    try:
        e = pr.make_engine_for(0, pr.B, max_features, feature_sigma=FEATURE_SIGMA, lib=_lib.load_testing())
    finally:
        for k in switches:
            monkeypatch.delenv(k, raising=False)
    e.set_step_fusion(False)
    return e


@pytest.mark.parametrize("counts, ld, blocks", [((25, 23, 24, 25), 128, 2), ((7, 5, 6), 64, 1)], ids=["ld128", "ld64"])
def test_two_steps_with_a_paused_sequence(counts, ld, blocks, monkeypatch):
    B, slots, last = len(counts), max(counts), len(counts) - 1
    assert (13 + 3 * slots + 6 + 1 + 63) // 64 * 64 == ld and slots % 4
    pr = Pair(slots, 2, batch=B, make_engine=False, feature_counts=list(counts), feature_sigma=FEATURE_SIGMA)
    e = hinted_engine(pr, slots, monkeypatch)
    plan = e.debug_update_plan()
    assert (plan["build"], plan["build_nsplit"], plan["build_threads"]) == ("ahead<4>", 1, ld), plan
    assert (plan["chol"], plan["fwd"], plan["fwd_nb"]) == ("left", "lds", blocks), plan

    frozen = None
    for k in range(2):
        active = [1] * B
        if k == 1:
            active[last] = 0
            frozen = (e.total_state(last), e.debug_raw_covariance(last))
        e.set_active(active)
        for b in range(B):
            if active[b]:
                pr.oracles[b].go_one_step(pr.frames[b][k], False)
        e.go_one_step(pr.frame_batch(k), False)
        ms = [e.selection(b)[1]["measurement_size"] for b in range(B)]
        print("update-streams ld=%d frame %d m %s" % (ld, k, ms))
        assert all(ms[b] == 2 * counts[b] for b in range(B) if active[b]), ms
        worst = compare_state(pr.oracles, e, TOL_X, TOL_P)
        print("update-streams ld=%d frame %d against the oracle: |dx| %.3e, rel |dP| %.3e" % (ld, k, worst["x"], worst["P"]))

    for b in range(B):
        P = e.debug_raw_covariance(b)
        assert P.shape == (ld, ld)
        assert np.array_equal(P, P.T), "seq %d: P is not bitwise symmetric" % b
        n = 13 + 3 * counts[b]
        # never-used slots, the partially initialised features' columns (no mapping here) and the padding up to ld, with the
        # innovation's column ld - 1 of A^T and V^T among it
        assert not P[n:, :].any() and not P[:, n:].any(), "seq %d: P is not zero outside the live state" % b
    assert np.array_equal(e.total_state(last), frozen[0]), "the paused sequence's state changed"
    assert np.array_equal(e.debug_raw_covariance(last), frozen[1]), "the paused sequence's covariance changed"
    assert not e.status_flags().any()
