"""sl2_get_step_stats (Engine.step_stats): the per-step filter-consistency record of a whole batch in one call.

Truth is independent of the kernel under test.  An engine is stepped by the seams - predict, select, make_measurements -;
features(seq) and total_covariance(seq) then hold the measurement Jacobians, the innovations and the PRIOR covariance.  H and
S = H P H^T + R are built in np.longdouble, S is factored by a hand-written Cholesky and L w = nu is solved in
np.longdouble as well (tests/ekf_update_truth.py, shared with the posterior's truth); only then does the engine's
kalman_filter_update run, and step_stats is read.

Tolerances: nis, min_pivot, max_pivot: relative error <= 8 m 2^-53 cond(S), the forward-error shape of a Cholesky
solve; log_det_S: absolute error <= 8 m 2^-53 (cond(S) + sum |log L_rr|); cond(S) by np.linalg.cond in the test.  worst_feature_d2
(a 2 x 2 solve per feature): relative error <= 8 * 2 * 2^-53 cond(S_i).  Integer fields, worst_label, position_var and every
determinism statement: exact equality.  Each test asserts the `dof` it means to hit."""
import numpy as np
import pytest

from ekf_update_truth import chol_solve_longdouble, innovation_system, measured_features
from mapping_helpers import make_mapping_sequence
from scenelib2_amd import Engine, _lib, synth
from slam_helpers import Pair

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
INT_FIELDS = ("stepped", "status_flags", "sequence_steps", "n_features", "n_partial", "n_visible", "n_selected", "n_matched",
              "dof", "worst_label")
DBL_FIELDS = ("nis", "log_det_S", "min_pivot", "max_pivot", "worst_feature_d2", "position_var")


def truth_before_update(e, b):
    """Call between make_measurements and kalman_filter_update: what the record of sequence b must say after the update."""
    ok = measured_features(e, b)                                   # feature_list_ order = slot order = the rows' order
    m = 2 * len(ok)
    t = dict(dof=m, n_matched=len(ok), worst_label=-1, worst_feature_d2=0.0, nis=0.0, log_det_S=0.0, min_pivot=0.0, max_pivot=0.0,
             cond=1.0, sum_abs_log=0.0, cond_worst=1.0)
    if not m:
        return t
    _, S, nu = innovation_system(e.total_covariance(b), ok)        # tests/ekf_update_truth.py: H P, S and nu in np.longdouble
    L, w = chol_solve_longdouble(S, nu)
    d = np.diag(L)
    t.update(nis=float(w @ w), log_det_S=float(2 * np.log(d).sum()), min_pivot=float(d.min()), max_pivot=float(d.max()),
             cond=float(np.linalg.cond(S.astype(np.float64))), sum_abs_log=float(np.abs(np.log(d)).sum()))
    d2 = []
    for f in ok:
        Si, ni = f["S"].astype(np.longdouble), f["nu"].astype(np.longdouble)
        det = Si[0, 0] * Si[1, 1] - Si[0, 1] * Si[1, 0]
        d2.append(float((ni[0] * (Si[1, 1] * ni[0] - Si[0, 1] * ni[1]) + ni[1] * (Si[0, 0] * ni[1] - Si[1, 0] * ni[0])) / det))
    k = int(np.argmax(d2))                     # (the first of equals: the lower slot)
    t.update(worst_label=ok[k]["label"], worst_feature_d2=d2[k], cond_worst=float(np.linalg.cond(ok[k]["S"])))
    return t


def check_against_truth(r, t, what):
    """One record against its truth at the tolerances of the module docstring; the figures are printed before they are asserted."""
    m = t["dof"]
    assert int(r["stepped"]) == 1 and int(r["dof"]) == m and int(r["n_matched"]) == t["n_matched"], (what, r, t)
    assert int(r["worst_label"]) == t["worst_label"], (what, r, t)
    if not m:
        assert all(float(r[k]) == 0.0 for k in DBL_FIELDS if k != "position_var"), (what, r)
        return
    bound = 8 * m * EPS * t["cond"]
    rel = lambda a, b: abs(a - b) / abs(b)
    dev = dict(nis=rel(float(r["nis"]), t["nis"]) / bound,
               pivot=max(rel(float(r["min_pivot"]), t["min_pivot"]), rel(float(r["max_pivot"]), t["max_pivot"])) / bound,
               log_det_S=abs(float(r["log_det_S"]) - t["log_det_S"]) / (8 * m * EPS * (t["cond"] + t["sum_abs_log"])),
               d2=rel(float(r["worst_feature_d2"]), t["worst_feature_d2"]) / (16 * EPS * t["cond_worst"]))
    print("%s: m = %d, cond(S) = %.3g, deviation / bound: nis %.3g, pivots %.3g, log det S %.3g, worst d2 %.3g; nis = %.6g" % (
        what, m, t["cond"], dev["nis"], dev["pivot"], dev["log_det_S"], dev["d2"], float(r["nis"])))
    for k, v in dev.items():
        assert v <= 1.0, (what, k, v, r, t)


def position_var_of(e, b):
    Pxx = e.get_vehicle_state(b, 1)[1][0]
    return (Pxx[0, 0] + Pxx[1, 1]) + Pxx[2, 2]


def seam_frame(e, frames, n_select, seqs):
    """One frame through the seams of engine e; returns {seq: truth} for `seqs`, taken in front of the update."""
    e.kalman_filter_predict()
    e.auto_select_n_features(n_select)
    e.make_measurements(frames)
    truth = {b: truth_before_update(e, b) for b in seqs}
    e.kalman_filter_update()
    return truth


def device_records(e, seq0=0, nseq=None):
    nseq = e.batch - seq0 if nseq is None else nseq
    buf = _lib.DeviceBuffer(96 * nseq)
    e.step_stats_device(buf.ptr, seq0, nseq)
    e.synchronize()
    out = buf.download((nseq,), _lib.STEP_STATS_DTYPE)
    buf.free()
    return out


def launched(e, name):
    return e.kernel_times().get(name, dict(launches=0))["launches"]


# ------------------------------------------------------------------------------------------------- mixed maps, determinism
def test_mixed_maps_in_one_launch_and_the_bytes_of_a_record():
    """B = 3 with 0, 4 and 12 features: m = 0, 8 and 24 in one launch, three frames.  The rows of the sub-range (1, 2) are the
    full range's rows byte for byte, the device form is the host form, a second call repeats the first, and regrouping the
    batch (no step in between) changes nothing."""
    pr = Pair(12, 3, batch=3, feature_counts=[0, 4, 12])
    e = pr.engine
    assert list(e.step_stats()["stepped"]) == [0, 0, 0]                  # nobody has stepped since sl2_create
    for k in range(3):
        truth = seam_frame(e, pr.frame_batch(k), 12, (0, 1, 2))
        rec = e.step_stats()
        assert [int(v) for v in rec["dof"]] == [0, 8, 24], rec["dof"]
        for b in range(3):
            check_against_truth(rec[b], truth[b], "mixed frame %d seq %d" % (k, b))
            assert float(rec[b]["position_var"]) == position_var_of(e, b)
            h = e.snapshot(b)["header"]
            assert (int(rec[b]["n_features"]), int(rec[b]["n_partial"]), int(rec[b]["n_visible"]), int(rec[b]["n_selected"]),
                    int(rec[b]["sequence_steps"]), int(rec[b]["status_flags"])) == (
                h.n_features, h.n_partial, h.number_of_visible_features, h.n_selected, h.sequence_steps, h.status_flags)
            assert 2 * int(rec[b]["n_matched"]) == h.successful_measurement_vector_size
        assert e.step_stats(1, 2).tobytes() == rec[1:].tobytes()
        assert e.step_stats(2, 1).tobytes() == rec[2:].tobytes()
        assert device_records(e).tobytes() == rec.tobytes()
        assert device_records(e, 1, 2).tobytes() == rec[1:].tobytes()
        assert e.step_stats().tobytes() == rec.tobytes()
        if k == 1:
            e.set_groups(2)
            assert e.step_stats().tobytes() == rec.tobytes()
            e.set_groups(1)
        e.finish_step(False)
        after = e.step_stats()                     # the update's figures outlive the end of the step; the clock has moved on
        for name in INT_FIELDS + DBL_FIELDS:
            if name not in ("sequence_steps", "position_var", "n_selected", "n_features"):
                assert after[name].tobytes() == rec[name].tobytes(), name
        assert [int(v) for v in after["sequence_steps"]] == [k + 1] * 3
    assert not e.status_flags().any()


# -------------------------------------------------------------------------------------------- the substitution's variants
@pytest.mark.parametrize("n_features", [1, 16, 17, 40])
def test_across_the_32_row_block_edge_through_ksplit(n_features):
    """m = 2, 32 (one full block), 34 (two blocks) and 80 (a ragged third block), one sequence: k_fwdsub_ksplit."""
    pr = Pair(n_features, 2, batch=1)
    e = pr.engine
    e.set_profiling(2)
    for k in range(2):
        truth = seam_frame(e, pr.frame_batch(k), n_features, (0,))
        rec = e.step_stats()
        assert int(rec[0]["dof"]) == 2 * n_features
        check_against_truth(rec[0], truth[0], "ksplit %d features frame %d" % (n_features, k))
        assert float(rec[0]["position_var"]) == position_var_of(e, 0)
        e.finish_step(False)
    assert launched(e, "k_fwdsub_ksplit") == 2 and launched(e, "k_fwdsub_lds") == 0 and launched(e, "k_step_stats") >= 2


def test_through_fwdsub_lds():
    """24 sequences of 12 features at a capacity of 16 (ld = 128): B ld / 16 = 192 > 160, so the substitution is
    k_fwdsub_lds<1>.  Truth for the first, a middle and the last sequence."""
    pr = Pair(12, 1, batch=24, max_features=16)
    e = pr.engine
    e.set_profiling(2)
    truth = seam_frame(e, pr.frame_batch(0), 12, (0, 11, 23))
    rec = e.step_stats()
    assert launched(e, "k_fwdsub_lds") == 1 and launched(e, "k_fwdsub_ksplit") == 0
    assert [int(v) for v in rec["dof"]] == [24] * 24
    for b in (0, 11, 23):
        check_against_truth(rec[b], truth[b], "fwdsub_lds seq %d" % b)
    assert device_records(e, 11, 13).tobytes() == rec[11:].tobytes()


@pytest.mark.parametrize("n_features,kernel", [(224, "k_fwd_gemm"), (272, "k_chol_syrk")])
def test_large_maps(n_features, kernel):
    """640 x 480, one sequence, two frames.  224 features: 14 blocks, the grouped substitution (k_fwd_gemm between the groups);
    272 features: 17 blocks padded to 20, the panel-wise factorisation (k_chol_syrk) in front of it."""
    pr = Pair(n_features, 2, batch=1, cam=synth.default_camera(640, 480))
    e = pr.engine
    e.set_profiling(2)
    for k in range(2):
        truth = seam_frame(e, pr.frame_batch(k), n_features, (0,))
        rec = e.step_stats()
        assert int(rec[0]["dof"]) == 2 * n_features
        check_against_truth(rec[0], truth[0], "%d features frame %d" % (n_features, k))
        e.finish_step(False)
    assert launched(e, kernel) >= 2 and launched(e, "k_fwd_gemm") >= 2 and launched(e, "k_fwdsub_ksplit") == 0
    assert not e.status_flags().any()


# --------------------------------------------------------------------------------------------------------- the fused step
@pytest.mark.parametrize("n_features,n_select", [(4, 4), (12, 12), (16, 16), (20, 16)])
def test_fused_step_against_the_seam_engine(n_features, n_select):
    """One Pair's frames through two engines: one by the seams (the ten-launch chain; truth is computed from it), one by
    go_one_step under set_step_fusion(2) - k_small_back, which keeps w and L in LDS and stores what the query reads.  20
    features with 16 selected: the 128-column panel."""
    pr = Pair(n_features, 3, batch=1, n_select=n_select)
    seam = pr.engine
    fused = pr.make_engine_for(0, 1, n_features)
    fused.set_step_fusion(2)
    fused.set_profiling(2)
    for k in range(3):
        truth = seam_frame(seam, pr.frame_batch(k), n_select, (0,))
        seam.finish_step(False)
        fused.go_one_step(pr.frame_batch(k))
        rs, rf = seam.step_stats()[0], fused.step_stats()[0]
        assert int(rf["dof"]) == 2 * n_select
        check_against_truth(rs, truth[0], "seam engine, %d / %d frame %d" % (n_features, n_select, k))
        check_against_truth(rf, truth[0], "fused engine, %d / %d frame %d" % (n_features, n_select, k))
        for name in INT_FIELDS:
            assert int(rs[name]) == int(rf[name]), (name, rs, rf)
        assert float(rf["position_var"]) == position_var_of(fused, 0)
    assert launched(fused, "k_small_back") == 3 and launched(fused, "k_fwdsub_ksplit") == 0
    assert not fused.status_flags().any()


@pytest.mark.parametrize("n_features,n_select", [(12, 12), (20, 16)])
def test_fused_step_under_graph_replay(n_features, n_select):
    """set_graph_mode(1) with device-resident frames in two alternating buffers: the records of captured and replayed steps are
    those of the same steps launched directly, byte for byte, in the host and in the device form."""
    pr = Pair(n_features, 6, batch=2, n_select=n_select, make_engine=False)
    engines = [pr.make_engine_for(0, 2, n_features) for _ in range(2)]
    for e in engines:
        e.set_step_fusion(2)
    engines[0].set_graph_mode(True)
    fb = pr.cam["width"] * pr.cam["height"]
    bufs = [_lib.DeviceBuffer(2 * fb) for _ in range(2)]
    for k in range(6):                             # frames 0, 1 capture (one graph per buffer), 2 .. 5 replay
        buf = bufs[k & 1]
        buf.upload(np.ascontiguousarray(pr.frame_batch(k), dtype=np.uint8))
        recs = []
        for e in engines:
            e.go_one_step(buf.ptr, on_device=True, seq_stride=fb)
            recs.append(e.step_stats())
            assert device_records(e).tobytes() == recs[-1].tobytes()
            e.synchronize()
        assert [int(v) for v in recs[0]["dof"]] == [2 * n_select] * 2 and [int(v) for v in recs[0]["stepped"]] == [1, 1]
        assert recs[0].tobytes() == recs[1].tobytes(), k
    for b in bufs:
        b.free()


# -------------------------------------------------------------------------------------------------------------- staleness
def _zeros_but_live(r):
    return (int(r["stepped"]) == 0 and int(r["dof"]) == 0 and int(r["worst_label"]) == -1 and
            all(float(r[k]) == 0.0 for k in DBL_FIELDS if k != "position_var"))


def test_a_record_is_of_the_last_update_the_sequence_took_part_in():
    """Pause, reset, load and copy: the sequence reads stepped = 0, dof = 0 until it steps again, its counts stay live, and its
    neighbours' records are what they are in a twin engine nobody paused.  A blank frame: stepped = 1, dof = 0, no worst feature."""
    pr = Pair(12, 5, batch=3, make_engine=False)
    e, twin = pr.make_engine_for(0, 3, 12), pr.make_engine_for(0, 3, 12)
    for q in (e, twin):
        q.go_one_step(pr.frame_batch(0))
    r0 = e.step_stats()
    assert r0.tobytes() == twin.step_stats().tobytes() and [int(v) for v in r0["dof"]] == [24] * 3
    # ---- paused
    e.set_active([1, 0, 1])
    assert e.step_stats().tobytes() == r0.tobytes()                      # the last update is still the one all three took part in
    for q in (e, twin):
        q.go_one_step(pr.frame_batch(1))
    r1, t1 = e.step_stats(), twin.step_stats()
    assert _zeros_but_live(r1[1]), r1[1]
    assert int(r1[1]["sequence_steps"]) == 1 and int(r1[1]["n_features"]) == 12 and int(r1[1]["n_matched"]) == 12
    assert float(r1[1]["position_var"]) == position_var_of(e, 1)
    assert r1[0].tobytes() == t1[0].tobytes() and r1[2].tobytes() == t1[2].tobytes()
    assert [int(v) for v in r1["dof"]] == [24, 0, 24] and [int(v) for v in t1["dof"]] == [24] * 3
    # ---- resumed: it steps again
    e.set_active([1, 1, 1])
    for q in (e, twin):
        q.go_one_step(pr.frame_batch(2))
    r2 = e.step_stats()
    assert [int(v) for v in r2["stepped"]] == [1, 1, 1] and int(r2[1]["dof"]) > 0 and int(r2[1]["sequence_steps"]) == 2
    assert r2[0].tobytes() == twin.step_stats()[0].tobytes()
    # ---- reset, load, copy into slot 1: nothing has stepped there
    blob = e.save_sequences(0, 1)
    e.reset_sequences(1, 1)
    r = e.step_stats()
    assert _zeros_but_live(r[1]) and int(r[1]["n_features"]) == 0 and int(r[1]["sequence_steps"]) == 0 and int(r[1]["n_matched"]) == 0
    assert r[0].tobytes() == r2[0].tobytes() and r[2].tobytes() == r2[2].tobytes()
    e.load_sequences(blob, seq0=1)
    r = e.step_stats()
    assert _zeros_but_live(r[1]) and int(r[1]["n_features"]) == 12 and int(r[1]["sequence_steps"]) == 3
    assert r[0].tobytes() == r2[0].tobytes() and r[2].tobytes() == r2[2].tobytes()
    e.reset_sequences(1, 1)
    e.copy_sequences(e, 2, 1, 1)
    r = e.step_stats()
    assert _zeros_but_live(r[1]) and int(r[1]["n_features"]) == 12 and int(r[1]["sequence_steps"]) == 3
    assert float(r[1]["position_var"]) == float(r[2]["position_var"])
    assert r[0].tobytes() == r2[0].tobytes() and r[2].tobytes() == r2[2].tobytes()
    # ---- the copy steps with its source's frame: both say the same
    f3 = pr.frame_batch(3)
    f3[1] = f3[2]
    e.go_one_step(f3)
    r3 = e.step_stats()
    assert [int(v) for v in r3["stepped"]] == [1, 1, 1] and int(r3[1]["dof"]) > 0
    assert r3[1].tobytes() == r3[2].tobytes()
    # ---- a blank frame for sequence 0
    f4 = pr.frame_batch(4)
    f4[1] = f4[2]
    f4[0] = 128
    e.go_one_step(f4)
    r4 = e.step_stats()
    assert int(r4[0]["stepped"]) == 1 and int(r4[0]["dof"]) == 0 and int(r4[0]["worst_label"]) == -1 and int(r4[0]["n_matched"]) == 0
    assert all(float(r4[0][k]) == 0.0 for k in DBL_FIELDS if k != "position_var") and int(r4[0]["n_selected"]) > 0
    assert int(r4[1]["dof"]) > 0 and r4[1].tobytes() == r4[2].tobytes()
    assert not e.status_flags().any()


# ---------------------------------------------------------------------------------------------------------------- mapping
def test_counts_follow_the_snapshot_header_while_the_map_grows():
    """enable_mapping with a dozen known features: n_partial and n_features are the snapshot header's after every step, with a
    partially initialised feature in flight (which feature_list_ counts)."""
    cam, params, spec, frames, templates = make_mapping_sequence(n_known=12, n_frames=16)
    params["number_of_features_to_keep_visible"] = 16             # 12 visible known features must not shut the gate
    e = Engine(cam, params, 1, 40)
    e.set_vehicle_state(spec.xv0[None], spec.Pxx0[None])
    e.add_known_features(spec.feat_y[None], spec.xp_org()[None], templates[None])
    seen_partial, seen_grown = False, False
    for k in range(1, 17):
        e.go_one_step(frames[k][None], True, True)
        r = e.step_stats()[0]
        h = e.snapshot(0)["header"]
        assert (int(r["n_partial"]), int(r["n_features"]), int(r["n_selected"]), int(r["n_visible"]), int(r["sequence_steps"])) == (
            h.n_partial, h.n_features, h.n_selected, h.number_of_visible_features, h.sequence_steps), k
        assert int(r["stepped"]) == 1 and int(r["dof"]) == 2 * int(r["n_matched"])
        seen_partial = seen_partial or h.n_partial > 0
        seen_grown = seen_grown or h.n_features > 12
    assert seen_partial and seen_grown, "the run must carry a partially initialised feature"

