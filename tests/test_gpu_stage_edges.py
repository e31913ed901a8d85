"""The stages on either side of the search - feature_prediction_body, select_body, finalize_body (sl2_frontend_dev.hpp), as
k_feature_prediction / k_select / k_finalize and as the fused k_small_front / k_small_back - on maps built to sit ON their
edges (tests/stage_edge_cases.py; tests/test_stage_edge_cases_host.py shows on the CPU that each case is what it claims):

  1  visibility_test: each of its five ways to fail, alone, next to a twin a fraction of a pixel (1e-6 of the ratio, of a radian)
     on the other side; measurements exactly ON the upper bounds
  2  selection: bit-equal scores either side of every slice boundary of the rank split (ns = 63 .. 257, capacities larger than
     the map), a tie across the cut, a map of nothing but ties, scores of exactly zero, empty selections
  3  delete_bad_features: scheduled runs of every length 1 .. 5, at slot 0, at the last feature, around retired slots, across
     slot 128 (k_finalize's prefetch) and in a 257-slot map (its register strip), with the three counter edges
  4  a partially initialised feature between two scheduled ones
  5  more frame-sized search windows than the step's list of shared units holds

The checker is the CPU oracle throughout.  Selection order, visible count, flags, counters and labels are compared exactly;
state and covariance to the tolerances of tests/test_gpu_slam.py."""
import copy
import gc
import os
import re

import numpy as np
import pytest

import stage_edge_cases as sc
from conftest import ROOT, rel_fro
from scenelib2_amd import Engine, synth
from slam_helpers import Pair, compare_state
from test_gpu_checkpoint import header_of
from test_gpu_slam import TOL_P, TOL_P_LARGE, TOL_X

pytestmark = pytest.mark.gpu

CAMS = [synth.default_camera(), synth.default_camera(400, 300)]


@pytest.fixture(autouse=True)
def release_engines():
    yield
    gc.collect()


def engine_of(case, fusion=True):
    """One engine of one sequence holding the case.  (Created with sd >= 1 and then given the case's own calibration through
    sl2_set_cameras, which admits sd = 0.)"""
    e = Engine(dict(case.cam, sd=max(1, case.cam["sd"])), case.params, 1, case.capacity)
    e.set_cameras([case.cam])
    if not fusion:
        e.set_step_fusion(False)
    e.set_vehicle_state(case.xv0[None], case.Pxx0[None])
    e.add_known_features(case.y[None], case.xp_org[None], case.templates[None])
    if case.Pyy.any():
        e.set_feature_covariances(case.Pyy[None])
    return e


def seams(case, e, o, n=None):
    """kalman_filter_predict (where the case has one) and auto_select_n_features on both; everything the selection leaves
    behind compared.  Returns (engine features, visibility codes)."""
    n = case.n_select if n is None else n
    if case.predict:
        o.kalman_filter_predict()
        e.kalman_filter_predict()
        assert np.abs(e.total_state(0) - o.total_state()).max() <= TOL_X
        if not case.meta.get("nan"):             # (a covariance of NaN has no distance)
            assert rel_fro(e.total_covariance(0), o.total_covariance()) <= TOL_P
    n_vis = o.auto_select_n_features(n)
    e.auto_select_n_features(n)
    codes = case.vis_codes(o)
    sel, counters = e.selection(0)
    feats = e.features(0)
    assert len(feats) == case.N
    assert [f["visible"] for f in feats] == [c == 0 for c in codes]
    assert counters["visible"] == n_vis == sum(c == 0 for c in codes)
    assert list(sel) == list(o.selected_labels()), "selection order differs"
    assert counters["selected"] == o.num_selected
    assert [f["selected"] for f in feats] == [o.feature(i)["selected"] for i in range(case.N)]
    assert [f["label"] for f in feats] == list(range(case.N))
    return feats, codes


def whole_step_both_forms(case):
    """One GoOneStep of the case on the oracle, on an engine with step fusion (k_small_front / k_small_back) and on one without:
    both engines held to the oracle, and identical to each other in everything that is an integer."""
    assert case.capacity <= 35 and case.n_select <= 16
    o = case.oracle()
    o.go_one_step(case.frame)
    out = []
    for fusion in (True, False):
        e = engine_of(case, fusion)
        e.set_profiling(2)
        e.go_one_step(case.frame[None])
        compare_state([o], e, TOL_X, TOL_P)
        names = set(e.kernel_times())
        if fusion:
            assert {"k_small_front", "k_small_back"} <= names and not ({"k_select", "k_finalize"} & names), names
        else:
            assert {"k_feature_prediction", "k_select", "k_finalize"} <= names and not ({"k_small_front", "k_small_back"} & names), names
        out.append((e.features(0), e.selection(0), e))
    (fa, (sa, ca), _), (fb, (sb, cb), _) = out
    assert list(sa) == list(sb) and ca == cb
    for p, q in zip(fa, fb):
        for key in ("label", "visible", "selected", "success", "attempted", "successful", "pos"):
            assert p[key] == q[key], key
        assert np.array_equal(p["z"], q["z"]) and np.array_equal(p["h"], q["h"])
    return o, fa


# --------------------------------------------------------------------------------------------------------------- 1: visibility
@pytest.mark.parametrize("cam", CAMS, ids=lambda c: "%dx%d" % (c["width"], c["height"]))
def test_visibility_every_failure_and_its_twin(cam):
    """visible == (visibility_test == 0) for every feature of the scene - the four borders, behind the camera, length ratio 2
    and 1/2, 45 degrees - through the seam calls, then through a whole step in both step forms: the visible count and the
    selection are the oracle's, the visible features are measured, and no invisible feature's counters move."""
    case = sc.visibility_scene(cam)
    e, o = engine_of(case), case.oracle()
    feats, codes = seams(case, e, o)
    for a, b, bit in case.meta["pairs"]:
        assert feats[a]["visible"] and not feats[b]["visible"], (case.meta["names"][a], bit)
    assert not feats[case.meta["behind"]]["visible"]
    o2, fa = whole_step_both_forms(case)
    matched = 0
    for i, f in enumerate(fa):
        if codes[i] != 0:
            assert f["attempted"] == 0 and f["successful"] == 0 and not f["selected"], case.meta["names"][i]
        elif f["selected"]:
            assert f["attempted"] == 1
            matched += f["successful"]
    assert sum(f["selected"] for f in fa) == case.n_select and matched >= 1      # (so an update and normalise_state ran)


def test_visibility_exactly_on_the_upper_bounds():
    """h == width - 21 and h == height - 21 exactly: visible (the tests are `h > bound`).  h itself is compared exactly: the
    construction has no rounding in it (stage_edge_cases.on_the_bound_scene)."""
    case = sc.on_the_bound_scene()
    e, o = engine_of(case), case.oracle()
    feats, codes = seams(case, e, o)
    assert codes == [0, 0, 0, 0] and all(f["visible"] for f in feats)
    for f, want in zip(feats, case.meta["expect_h"]):
        if want is not None:
            assert tuple(f["h"]) == want


# ----------------------------------------------------------------------------------------------------- 2: ranks, ties, rank split
_RANK_CASES = {}


def rank_case(ns, capacity):
    if (ns, capacity) not in _RANK_CASES:
        _RANK_CASES[(ns, capacity)] = sc.rank_map(ns, capacity)
    return _RANK_CASES[(ns, capacity)]


@pytest.mark.parametrize("ns,capacity", sc.RANK_SIZES)
def test_selection_with_ties_across_the_rank_split(ns, capacity):
    """Tie groups with members in different slices of k_select's rank count (P = 4, 2, 1 groups of threads; the strided loop from
    257 slots), a tie pair the cut n_select falls into, invisible features in between: order, flags and counts are the oracle's.
    Then the whole map selected (n = ns): every tie group side by side in list order."""
    case = rank_case(ns, capacity)
    e, o = engine_of(case), case.oracle()
    feats, codes = seams(case, e, o)
    cut = case.meta["cut"]
    assert feats[cut[0]]["selected"] and not feats[cut[1]]["selected"]
    sel, _ = e.selection(0)
    assert sel[-1] == cut[0] and len(sel) == case.n_select
    for i, f in enumerate(feats):                 # the scores the ties rest on: bit-equal on the device too
        for g in case.meta["groups"]:
            if i in g[1:]:
                assert np.array_equal(f["S"], feats[g[0]]["S"])
    whole = copy.copy(case)                       # the same map with n_select = ns
    whole.n_select, whole.params = ns, synth.default_params(ns, sc.DT)
    e2, o2 = engine_of(whole), whole.oracle()
    seams(whole, e2, o2)
    sel2, cnt2 = e2.selection(0)
    assert list(sel2) == case.meta["full_order"] and cnt2["visible"] == len(sel2)


def test_selection_of_a_map_of_nothing_but_ties():
    case = sc.all_equal_map()
    e, o = engine_of(case), case.oracle()
    seams(case, e, o)
    assert list(e.selection(0)[0]) == list(range(case.n_select))


def test_selection_stops_at_the_first_zero_score():
    """sd = 0, Pxx = 0, no predict: S = 0 exactly for the features without a prior.  The oracle selects the 8 positive ones and
    stops (monoslam.cpp:241-249); so must the engine (s_zero_rank), with all 20 visible and n_select = 16."""
    case = sc.zero_score_map()
    e, o = engine_of(case), case.oracle()
    feats, _ = seams(case, e, o)
    sel, counters = e.selection(0)
    assert counters["visible"] == case.N and counters["selected"] == len(case.meta["positive"]) < case.n_select
    assert sorted(sel) == case.meta["positive"]
    for i in case.meta["zero"]:
        assert not feats[i]["S"].any() and not feats[i]["selected"]


def test_selection_with_nan_scores_keeps_list_order():
    """omega == 0 exactly: every score is NaN after the predict (key -0.5 in select_body), some features are invisible, and
    n_select cuts the visible ones: the first n_select visible features in list order, as the reference's insertion leaves them."""
    case = sc.nan_score_map()
    e, o = engine_of(case), case.oracle()
    feats, _ = seams(case, e, o)
    vis = [i for i in range(case.N) if i not in case.meta["invisible"]]
    assert list(e.selection(0)[0]) == vis[:case.n_select]
    assert all(np.isnan(feats[i]["S"][0, 0] + feats[i]["S"][1, 1]) for i in vis)


def test_empty_selections():
    """n_select = 0 with everything visible (the ABI admits it: sl2_auto_select_n_features takes any n), and a map on which
    nothing is visible - through the seams, and through a whole step in both step forms (no search, no update)."""
    case = sc.all_equal_map()
    e, o = engine_of(case), case.oracle()
    seams(case, e, o, n=0)
    assert e.selection(0)[1]["visible"] == case.N and e.selection(0)[1]["selected"] == 0
    case = sc.none_visible_map()
    e, o = engine_of(case), case.oracle()
    seams(case, e, o)
    assert e.selection(0)[1]["visible"] == 0 and e.selection(0)[1]["selected"] == 0
    _, fa = whole_step_both_forms(case)
    assert all(f["attempted"] == 0 and not f["visible"] for f in fa)


# ---------------------------------------------------------------------------------------------------------- 3: the deletion walk
def raw_covariance(e):
    """P of sequence 0 by SLOT, retired slots included (the sequence blob carries it so: sl2_save_sequences)."""
    blob = e.save_sequences(0, 1)[0]
    h = header_of(blob)
    n, pitch = h.state_size, h.row_pitch
    return np.frombuffer(blob, dtype=np.float64, count=n * pitch, offset=h.off_P).reshape(n, pitch)[:, :n].copy()


def assert_retired_rows_are_zero(e, labels):
    P = raw_covariance(e)
    for lab in labels:                 # (no squeeze has run: a feature's slot is its label)
        rows = slice(13 + 3 * lab, 16 + 3 * lab)
        assert not P[rows, :].any() and not P[:, rows].any(), "covariance of retired feature %d is not zero" % lab
    assert P[:13, :13].any()


@pytest.mark.parametrize("kind,fusion", [("ten", True), ("ten", False), ("ten_holes", True), ("ten_holes", False), ("130", True),
                                         ("257", True)])
def test_deletion_walk(kind, fusion):
    """Step, retire the plan's first features, step, set the counters, step: the features the reference's walk erases are gone -
    the 1st, 3rd, 5th of every scheduled run, runs counted over retired slots, the counter edges as `>=` and strict `<` say -
    their rows and columns of P exactly zero, everything else the oracle's; the skipped ones go a step later.  130: a run over
    slots 124 .. 129, either side of the 128 threads of k_finalize (flags prefetched / read).  257: 784 columns, beyond the
    6 x 128 the strip keeps in registers, with an update in the same step (TOL_P_LARGE from n = 613)."""
    plan = sc.deletion_plan(kind)
    tol_P = TOL_P_LARGE if 13 + 3 * plan["n"] >= 613 else TOL_P
    pr = sc.deletion_pair(plan, make_engine=True)
    e, o = pr.engine, pr.oracles[0]
    if not fusion:
        e.set_step_fusion(False)
    e.set_profiling(2)
    sc.step(pr, 0)
    pr.compare_state(TOL_X, tol_P)
    sc.set_counters(pr, {lab: sc.GO for lab in plan["first"]})
    sc.step(pr, 1)
    pr.compare_state(TOL_X, tol_P)
    live = [lab for lab in range(plan["n"]) if lab not in plan["first"]]
    assert [f["label"] for f in e.features(0)] == live
    sc.set_counters(pr, plan["counters"])
    sc.step(pr, 2)
    pr.compare_state(TOL_X, tol_P)
    after2 = [f["label"] for f in e.features(0)]
    assert sorted(set(live) - set(after2)) == plan["gone2"] and after2 == sc.oracle_labels(o)
    assert e.selection(0)[1]["measurement_size"] > 0                       # normalise_state ran in the step that deleted
    assert_retired_rows_are_zero(e, plan["first"] + plan["gone2"])
    sc.step(pr, 3)
    pr.compare_state(TOL_X, tol_P)
    after3 = [f["label"] for f in e.features(0)]
    assert sorted(set(after2) - set(after3)) == plan["gone3"]
    assert_retired_rows_are_zero(e, plan["first"] + plan["gone2"] + plan["gone3"])
    assert len(e.features(0, include_deleted=True)) == plan["n"]
    names = set(e.kernel_times())
    small = plan["n"] <= 35 and fusion
    assert ("k_small_back" in names) == small and ("k_finalize" in names) == (not small), names
    assert not e.status_flags().any()


# ------------------------------------------------------------------------------- 4: a partial feature inside a scheduled run
@pytest.mark.parametrize("mirror,fusion", [(False, True), (False, False), (True, True), (True, False)])
def test_partial_feature_ends_a_scheduled_run(mirror, fusion):
    """The list [A scheduled, P partially initialised, C scheduled]: P is an element of the reference's feature_list_, so it is
    the element that absorbs the skip after A's erase, and C is examined - and erased - in the same frame.  finalize_body used
    to step over P's slot (it carries FF_USED | FF_PARTIAL without FF_ACTIVE) as if it were retired, count A into C's run and
    keep C for a frame: this test failed on it (C, label 7, still listed after the step).  The walk now ends a run at a
    FF_PARTIAL slot.  mirror: [A scheduled, P, C unscheduled, D scheduled] - A and D go."""
    pr = sc.partial_run_pair(mirror, make_engine=True, fusion=fusion)
    e, o = pr.engine, pr.oracles[0]
    n = sc.PARTIAL_BASE + (3 if mirror else 2)
    feats = e.features(0)
    assert [f["label"] for f in feats] == list(range(n)) and [f["state_size"] for f in feats] == [int(k[0]) for k in o.feature_kinds()]
    assert not feats[sc.PARTIAL_BASE]["fully_initialised"] and e.partial_feature(0)["info"]["n_partial"] == 1
    e.set_profiling(2)
    sc.step(pr, 1, enable_mapping=True)
    gone = {5, 8} if mirror else {5, 7}
    assert sc.oracle_labels(o) == [lab for lab in range(n) if lab not in gone]
    assert [f["label"] for f in e.features(0)] == sc.oracle_labels(o), "the engine did not delete what the reference deletes"
    pr.compare_state(TOL_X, TOL_P)
    assert e.partial_feature(0)["info"]["n_partial"] == 1 == o.mapping_info()["n_partial"]
    assert_retired_rows_are_zero(e, sorted(gone))
    names = set(e.kernel_times())
    assert ("k_small_back" in names) == fusion and ("k_finalize" in names) == (not fusion), names
    sc.step(pr, 2, enable_mapping=True)
    pr.compare_state(TOL_X, TOL_P)
    assert [f["label"] for f in e.features(0)] == sc.oracle_labels(o)


# --------------------------------------------------------------------------------------------- 5: the full list of shared windows
def test_more_frame_sized_windows_than_the_shared_list_holds():
    """A camera position known to 0.3 m only (test_frame_sized_windows_are_shared_out_over_the_launch): every window of the
    first frame is the whole frame, 150 bands, cut into units of srch_unit_bands(150) = 4 bands: 38 units.  The step's list holds
    kSrchBigUnits = 16384 units per sequence group: 431 windows fit, the 432nd does not.  8 sequences x 60 features in ONE group
    select 480 windows: those that find the list full stay with their own wavefront, and what one of them had allocated below the
    capacity is stamped "nothing" (select_body).  Measurements bit-exact, candidate counts equal, 0 < shared < searched."""
    src = open(os.path.join(ROOT, "scenelib2_amd", "csrc", "sl2_common.hpp")).read()
    units_cap = int(re.search(r"constexpr int kSrchBigUnits = (\d+);", src).group(1))
    slots, min_bands = (int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("kSrchBigSlots", "kSrchBigMinBands"))
    bands = ((320 - 10 + 15) // 16 + 1) // 2 * ((240 - 10 + 15) // 16)      # (TU + 1) / 2 * TV of a window of 310 x 230 positions
    per = max((bands + slots - 1) // slots, min_bands)
    units = (bands + per - 1) // per
    assert (bands, per, units) == (150, 4, 38)
    B, N = 8, 60
    fit = units_cap // units
    assert fit == 431 and B * N > fit
    pr = Pair(N, 1, batch=B)
    xv, Pxx = [], []
    for b in range(B):
        P0 = pr.specs[b].Pxx0.copy()
        P0[0, 0] = P0[1, 1] = P0[2, 2] = 0.09
        pr.oracles[b].set_state(pr.specs[b].xv0, P0)
        xv.append(pr.specs[b].xv0)
        Pxx.append(P0)
    pr.engine.set_vehicle_state(np.stack(xv), np.stack(Pxx))
    pr.step_both(0, threads=min(16, B))
    pr.compare_state(1e-7, 1e-7)          # (that test's tolerances: the first update shrinks a prior 10^4 times the posterior)
    w = pr.engine.step_work()
    assert w["searched"] * units > units_cap, "too few windows to fill the list"
    assert w["search_tiles"] > 100 * w["searched"], "the windows of the first frame are not frame-sized"
    assert w["candidates"] == sum(o.diag()["candidates"] for o in pr.oracles)
    assert 0 < w["search_shared"] < w["searched"], w
