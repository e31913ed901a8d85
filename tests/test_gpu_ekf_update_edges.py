"""The dense EKF update (sl2_ekf_update.hip walking sl2_update_{build,chol,fwdsub,syrk}.hip: k_build_AS -> k_chol_left | panels -> k_fwdsub_ksplit | k_fwdsub_lds<NB> | grouped ->
k_syrk) held to an extended-precision truth and to the oracle on every case of tests/ekf_update_cases.py: each of the thirteen
k_fwdsub_lds<NB>, partly and fully live; m at every remainder of the 32-row block and of k_syrk's 16-row chunk, falling and
rising on one engine so that rows of a larger system sit in the padding of the workspaces; mixed systems and a paused sequence
in one launch; both sides of every dispatch boundary, the kernels asserted by name; the forms of k_build_AS; the live-tile rules
of k_syrk.  tests/test_ekf_update_cases_host.py shows on the CPU that every schedule reaches the m it exists for: no case skips.

Every frame runs through the seams.  Between make_measurements and kalman_filter_update the truth of tests/ekf_update_truth.py
is taken from the engine's own prior x, P and feature records; after the update and BEFORE finish_step (which normalises and
symmetrises) total_state and the full total_covariance are compared with it:

    |P+ - truth|_F <= C m 2^-53 cond(S) |P_prior|_F,     max |x+ - truth| <= C m 2^-53 cond(S) max(1, |x|_inf),     C = 8

C = 8 is the constant of tests/test_gpu_step_stats.py.  Measured worst deviation / bound (profiles/ekf_update_edges.json): the
engine 0.058 (m = 2, where cond(S) = 1 and the bound is sixteen roundings on |P|_F), the oracle 0.84 at the same place: above
1/64, so C is not lowered.

Symmetry at that point: k_syrk computes the upper block triangle and stores every 32 x 32 block off the diagonal a second time,
transposed, FROM THE SAME ACCUMULATOR - elements at least 32 columns apart are therefore asserted exactly equal to their
mirror images.  Inside the diagonal 32 x 32 blocks the two halves are partly separate sums on a prior the predict step
leaves symmetric only to rounding: there |P - P^T|_F is held to twice the truth bound.

Then finish_step, the oracles' seams, and compare_state at TOL_X / TOL_P (TOL_P_LARGE from n = 613 on) for every sequence."""
import numpy as np
import pytest

import ekf_update_cases as uc
import ekf_update_truth as tr
from slam_helpers import compare_state

pytestmark = pytest.mark.gpu


def launched(e, name):
    return e.kernel_times().get(name, dict(launches=0))["launches"]


def check_symmetry(P, t, what):
    n = P.shape[0]
    i = np.arange(n)
    far = np.abs(i[:, None] - i[None, :]) >= 32
    assert np.array_equal(P[far], P.T[far]), "%s: mirrored blocks differ" % what
    bound = 2 * tr.bounds(t, uc.C_BOUND)[0]
    near = np.where(far, 0.0, P - P.T)
    assert np.linalg.norm(near) <= bound, "%s: |P - P^T|_F = %g inside the diagonal blocks, bound %g" % (what, np.linalg.norm(near), bound)


def run_case(case, monkeypatch):
    pr = uc.scene(case)
    oracles = uc.fresh_oracles(pr)
    e = uc.make_engine(case, pr, monkeypatch)
    # the plan launch_update makes for this engine is the table's (one host call; the kernels asserted by name below ran from it)
    assert uc.plan_in_table_words(e.debug_update_plan()) == (case.build, case.nsplit, case.chol, case.fwd), (case, e.debug_update_plan())
    e.set_profiling(2)
    ms_by_frame, worst = [], dict(P=0.0, x=0.0)
    for k, n in enumerate(case.schedule):
        active = case.active(k)
        if case.paused:
            e.set_active([int(b in active) for b in range(case.batch)])
        if k in case.delete:
            assert e.delete_features(np.full(case.batch, case.delete[k], dtype=np.int32)).all()
        frozen = {b: (e.total_state(b), e.total_covariance(b)) for b in range(case.batch) if b not in active}
        e.kalman_filter_predict()
        e.auto_select_n_features(n)                       # (the engine clamps n to its number_of_features_to_select)
        e.make_measurements(pr.frame_batch(k))
        truths = {b: tr.posterior_truth(e, b) for b in case.truth_seqs if b in active}
        e.kalman_filter_update()
        for b, t in truths.items():
            what = "%s frame %d seq %d (m = %d)" % (case.name, k, b, t["m"])
            x, P = e.total_state(b), e.total_covariance(b)
            rP, rx = tr.deviation_over_bound(x, P, t, uc.C_BOUND)
            uc.report(case, "engine", k, b, t, rP, rx)
            worst = dict(P=max(worst["P"], rP), x=max(worst["x"], rx))
            assert rP <= 1.0 and rx <= 1.0, "%s: deviation / bound = %g (P), %g (x)" % (what, rP, rx)
            if t["m"]:                                   # (m = 0: k_syrk leaves at once, P is the predict step's)
                check_symmetry(P, t, what)
        for b, (x0, P0) in frozen.items():                 # a paused sequence: not a bit of it moves, here or at the end of the step
            assert np.array_equal(e.total_state(b), x0) and np.array_equal(e.total_covariance(b), P0), (case, k, b)
        e.finish_step(False)
        for b, (x0, P0) in frozen.items():
            assert np.array_equal(e.total_state(b), x0) and np.array_equal(e.total_covariance(b), P0), (case, k, b)
        _, ms = uc.oracle_frame(case, pr, oracles, k)
        ms_by_frame.append(ms)
        for b, t in truths.items():
            assert t["m"] == ms[b], (case, k, b, t["m"], ms[b])
        compare_state(oracles, e, uc.TOL_X, case.tol_P)
    print("ekf-edge-worst group=%s case=%s who=engine P=%.3g x=%.3g" % (case.group, case.name, worst["P"], worst["x"]))
    uc.check_targets(case, ms_by_frame)                    # what the host test showed of the oracles holds for this run
    for name in case.must_run:
        assert launched(e, name) >= len(case.schedule), (case, name, e.kernel_times().keys())
    for name in case.must_not_run:
        assert launched(e, name) == 0, (case, name)
    if case.fwd == "grouped":                              # a launch per group of eight block rows, a product in front of all but the first
        groups = (case.nblk_max + 7) // 8
        assert launched(e, uc.LDS) == groups * len(case.schedule) and launched(e, uc.GEMM) == (groups - 1) * len(case.schedule)
    else:
        assert launched(e, uc.KSPLIT) + launched(e, uc.LDS) == len(case.schedule)
    assert not e.status_flags().any()
    return pr, e


def cases_of(group):
    return [c for c in uc.CASES if c.group == group]


@pytest.mark.parametrize("case", cases_of("a"), ids=repr)
def test_every_fwdsub_lds_instantiation_partly_live(case, monkeypatch):
    """k_fwdsub_lds<NB>, NB = 1 .. 13 (nblk_max = NB: number_of_features_to_select = 16 NB in an engine of max(24, 16 NB) slots),
    24 sequences of 24 features: m = 48 - two live blocks of NB -, then m = 18 - one block whose rows 16 .. 31 the kernel skips,
    over the rows the larger system left in V^T.  NB = 1 selects 16: m = 32, then 18."""
    run_case(case, monkeypatch)


@pytest.mark.parametrize("case", cases_of("b"), ids=repr)
def test_fwdsub_lds_with_every_block_live(case, monkeypatch):
    """NB = 3, 6, 8, 9, 13 with N = 16 NB features all measured, at the smallest batch of more than 160 strips, one frame (why one:
    tests/ekf_update_cases.py).  Truth up to n = 445; NB = 13 (n = 637) against the oracle alone, at TOL_P_LARGE."""
    run_case(case, monkeypatch)


@pytest.mark.parametrize("case", cases_of("c"), ids=repr)
def test_block_and_chunk_remainders_on_a_system_that_shrinks_and_grows(case, monkeypatch):
    """One engine of 64 features (NB = 4), twenty frames whose m alternates between large and small: every m mod 32 of
    {0, 2, 14, 16, 18, 30} with one, two and four live blocks, m mod 16 of {0, 2, 8, 10, 14} in k_syrk's last chunk (one to four
    live k-steps).  B = 24: k_fwdsub_lds<4>; B = 2: k_fwdsub_ksplit."""
    run_case(case, monkeypatch)


@pytest.mark.parametrize("case", cases_of("d"), ids=repr)
def test_mixed_systems_and_a_paused_sequence_in_one_launch(case, monkeypatch):
    """B = 9 with 0, 1, 8, 9, 16, 17, 40, 64 and 64 features: m = 0, 2, 16, 18, 32, 34, 80, 128, 128 next to each other; the last
    sequence sits frame 1 out and keeps x and P bit for bit.  Nine sequences are k_fwdsub_ksplit's; under SL2_NO_KSPLIT (TEST
    build) the same batch goes through k_fwdsub_lds<4>."""
    run_case(case, monkeypatch)


@pytest.mark.parametrize("case", cases_of("e"), ids=repr)
def test_both_sides_of_every_dispatch_boundary(case, monkeypatch):
    """160 | 168 strips (ksplit | lds); 8 | 9 blocks (ksplit | lds<9>); 13 | 14 blocks (lds<13> | groups of eight with k_fwd_gemm);
    16 | 20 blocks (k_chol_left | panels with k_chol_syrk), each with a live map of 24 features in a large engine; and
    SL2_PANEL_FROM=2 (TEST build): 144 features, 12 blocks in three panels and two groups, m = 288, 126, 256, 128, 258, 130, 254."""
    run_case(case, monkeypatch)


@pytest.mark.parametrize("case", cases_of("f"), ids=repr)
def test_build_AS_forms(case, monkeypatch):
    """N = 5 .. 8 (N mod 4; nsplit clamped to the two feature batches) and the same with one workgroup a sequence
    (SL2_BUILD_SPLIT=1, TEST build); ld = 1024 | 1088: k_build_AS<1,4> | <2,2>; a feature deleted in the middle of the map between
    the frames, so that slots and live features differ."""
    run_case(case, monkeypatch)


@pytest.mark.parametrize("case", cases_of("g"), ids=repr)
def test_syrk_live_tile_rules(case, monkeypatch):
    """Capacity 60 (ld = 256), 13 + 3 N = 28, 31, 34, 61, 64, 67: either side of the 32-column wave boundary and of the 64-column
    tile boundary.  Columns of P beyond the live map must stay exactly zero: afterwards the map is filled to capacity with new
    features (which writes no element of P), and the rows and columns that brings into view are read."""
    pr, e = run_case(case, monkeypatch)
    N, extra = case.counts[0], case.max_features - case.counts[0]
    n0 = 13 + 3 * N
    rng = np.random.default_rng(N)
    for b in range(case.batch):
        before = e.total_covariance(b)
        e.add_known_features(rng.uniform(-0.2, 0.2, (1, extra, 3)), np.tile(pr.specs[b].poses[0], (1, extra, 1)),
                             np.zeros((1, extra, 11, 11), dtype=np.uint8), seq0=b)
        P = e.total_covariance(b)
        assert P.shape == (13 + 3 * case.max_features,) * 2 and np.array_equal(P[:n0, :n0], before)
        assert not P[n0:, :].any() and not P[:, n0:].any(), (case, b)
