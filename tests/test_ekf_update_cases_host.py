"""The cases of tests/ekf_update_cases.py, shown on the CPU alone to be what they claim to be.  For every case the oracles run
the schedule through their seams, and
  1. the matched counts produce every m the case exists for (values, residues mod 32 per number of live blocks, residues mod 16,
     live block counts, a frame on which m falls): a schedule that misses a target is changed in the table, the GPU test of
     the case never skips;
  2. the oracle's own posterior lies inside the truth bound at C_BOUND: the bound is sane before a kernel is held to it;
  3. the truth of tests/ekf_update_truth.py reproduces the oracle's posterior at TOL_X and TOL_P (TOL_P_LARGE from n = 613 on);
  4. ld, mld, nblk_max, the form of k_build_AS and the kernels of the case are what the engine's own sizing and update plan
     (sl2_update_plan.hpp, compiled for the host) make of the case's arguments.
No GPU: tests/test_gpu_ekf_update_edges.py holds the engine to the same truth and the same oracles on the same cases."""
import numpy as np
import pytest

import ekf_update_cases as uc
import ekf_update_truth as tr
import update_plan_helpers as uh


@pytest.fixture(scope="module", autouse=True)
def _oracle_built(oracle):
    return oracle


# ------------------------------------------------------------------------------------------------------- the truth itself
def test_truth_on_a_system_with_a_known_answer():
    """n = 16, one feature measured with H = unit rows on its first two states and no pose columns: S = P_ff + R I and the
    posterior is the textbook P - P[:, f] S^-1 P[f, :], here in float64 by numpy.linalg."""
    rng = np.random.default_rng(5)
    G = rng.standard_normal((16, 16))
    P = G @ G.T + 16 * np.eye(16)
    x = rng.standard_normal(16)
    f = dict(dh_by_dxp=np.zeros((2, 7)), dh_by_dy=np.eye(2, 3), pos=13, R=0.25, nu=np.array([0.5, -1.0]))
    t = tr.posterior_from(x, P, [f])
    H = np.zeros((2, 16))
    H[0, 13] = H[1, 14] = 1.0
    S = H @ P @ H.T + 0.25 * np.eye(2)
    K = P @ H.T @ np.linalg.inv(S)
    assert t["m"] == 2 and abs(t["cond"] - np.linalg.cond(S)) <= 1e-12 * t["cond"] and t["norm_P"] == np.linalg.norm(P)
    assert np.abs((t["P"] - (P - K @ S @ K.T)).astype(np.float64)).max() <= 1e-13 * np.abs(P).max()
    assert np.abs((t["x"] - (x + K @ f["nu"])).astype(np.float64)).max() <= 1e-14
    rP, rx = tr.deviation_over_bound((x + K @ f["nu"]), P - K @ S @ K.T, t, uc.C_BOUND)
    assert rP <= 1.0 and rx <= 1.0
    t0 = tr.posterior_from(x, P, [])
    assert t0["m"] == 0 and np.array_equal(t0["P"].astype(np.float64), P) and np.array_equal(t0["x"].astype(np.float64), x)
    assert tr.deviation_over_bound(x, P, t0, uc.C_BOUND) == (0.0, 0.0)


# --------------------------------------------------------------------------------------------- 4: the sizes and the kernels
@pytest.mark.parametrize("case", uc.CASES, ids=repr)
def test_table_follows_from_the_sizing_rules(case):
    """The rules are the compiled ones: update_sizes and make_update_plan of sl2_update_plan.hpp, built for the host
    (tests/test_update_plan_host.py holds them to the rules of the code before the plan)."""
    sizes, plan = uh.plan_of_engine(case.max_features, case.n_select, case.batch, case.env, superseded=bool(case.env))
    assert sizes["admitted"] and (case.ld, case.mld, case.nblk_max) == (sizes["ld"], sizes["mld"], sizes["nblk_max"]), (case, sizes)
    assert (case.build, case.nsplit, case.chol, case.fwd) == uc.plan_in_table_words(plan), (case, plan)
    run, never = uc.chain_of(case.fwd, case.chol)
    assert set(case.must_run) == run and set(case.must_not_run) == never
    assert max(case.counts) <= case.max_features and len(case.schedule) >= 1


def test_table_covers_every_instantiation_and_both_sides_of_every_boundary():
    by = uc.BY_NAME
    assert {c.fwd for c in uc.CASES if c.group == "a"} == {"lds<%d>" % nb for nb in range(1, 14)}
    assert {c.nblk_max for c in uc.CASES if c.group == "b"} == {3, 6, 8, 9, 13}
    strips = lambda c: c.batch * (c.ld // 16)
    assert strips(by["e_strips_B20"]) == 160 and strips(by["e_strips_B21"]) == 168 and strips(by["d_mixed"]) <= 160
    assert (by["e_select128"].nblk_max, by["e_select129"].nblk_max) == (8, 9)
    assert (by["e_select208"].nblk_max, by["e_select209"].nblk_max) == (13, 14)
    assert (by["e_select256"].nblk_max, by["e_select257"].nblk_max) == (16, 20)
    assert (by["e_panel_from_2"].nblk_max, by["e_panel_from_2"].chol, by["e_panel_from_2"].fwd) == (12, "panels", "grouped")
    assert (by["f_build_ld1024"].build, by["f_build_ld1088"].build) == ("<1,4>", "<2,2>")
    assert {c.build for c in uc.CASES} == {"<1,4>", "<2,2>", "ahead<4>", "ahead<2>"}        # both plain forms, both ahead forms
    assert sorted(c.max_features % 4 for c in uc.CASES if c.name.startswith("f_build_N") and not c.env) == [0, 1, 2, 3]
    assert sorted(13 + 3 * c.counts[0] for c in uc.CASES if c.group == "g") == [28, 31, 34, 61, 64, 67]


# ------------------------------------------------------------------------------------ 1 - 3: schedules, bound, truth v oracle
@pytest.mark.parametrize("case", uc.CASES, ids=repr)
def test_schedule_hits_its_targets_and_truth_agrees_with_the_oracle(case):
    pr = uc.scene(case)
    oracles = uc.fresh_oracles(pr)
    ms_by_frame, worst = [], dict(P=0.0, x=0.0, dP=0.0, dx=0.0)
    for k in range(len(case.schedule)):
        truths, ms = uc.oracle_frame(case, pr, oracles, k, case.truth_seqs)
        ms_by_frame.append(ms)
        for b, t in truths.items():
            if t is None:
                continue
            rP, rx = tr.deviation_over_bound(t["x_oracle"], t["P_oracle"], t, uc.C_BOUND)
            uc.report(case, "oracle", k, b, t, rP, rx)
            dx = float(np.abs(t["x_oracle"] - t["x"].astype(np.float64)).max())
            dP = float(np.linalg.norm(t["P_oracle"] - t["P"].astype(np.float64)) / np.linalg.norm(t["P_oracle"]))
            worst = dict(P=max(worst["P"], rP), x=max(worst["x"], rx), dP=max(worst["dP"], dP), dx=max(worst["dx"], dx))
    print("ekf-edge-worst group=%s case=%s who=oracle P=%.3g x=%.3g relP=%.3g absx=%.3g" % (
        case.group, case.name, worst["P"], worst["x"], worst["dP"], worst["dx"]))
    uc.check_targets(case, ms_by_frame)
    assert worst["P"] <= 1.0 and worst["x"] <= 1.0, (case, worst)
    assert worst["dx"] <= uc.TOL_X and worst["dP"] <= case.tol_P, (case, worst)
    if case.delete:
        assert all(o.num_features == n - 1 for o, n in zip(oracles, case.counts))
