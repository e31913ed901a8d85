"""The cases of tests/stage_edge_cases.py, shown on the CPU oracle alone to be what they claim to be: every visibility bit
alone and every pair either side of its threshold, bit-equal innovation covariances inside every tie group with members either
side of every boundary of k_select's rank split, scores that are exactly zero, the scheduled runs of the deletion cases and what
the reference's walk does with them - and, for the list [A scheduled, P partially initialised, C scheduled], that the reference
deletes A AND C in one frame.  No GPU: tests/test_gpu_stage_edges.py holds the engine to the same oracle on the same cases."""
import numpy as np
import pytest

import stage_edge_cases as sc
from scenelib2_amd import synth

CAMS = [synth.default_camera(), synth.default_camera(400, 300)]


@pytest.fixture(scope="module", autouse=True)
def _oracle_built(oracle):
    return oracle


# --------------------------------------------------------------------------------------------------------------- 1: visibility
@pytest.mark.parametrize("cam", CAMS, ids=lambda c: "%dx%d" % (c["width"], c["height"]))
def test_visibility_scene_has_every_failure_alone_and_every_pair_straddles(cam):
    case = sc.visibility_scene(cam)
    o = case.oracle()
    n_vis = case.run_seams(o)
    assert np.array_equal(o.get_state()[0][:7], sc.predicted_pose())          # the pose the scene was built on, to the bit
    codes = case.vis_codes(o)
    for bit in (1, 2, 4, 8, 16):
        assert bit in codes, "no feature fails with bit %d alone: %s" % (bit, codes)
    for a, b, bit in case.meta["pairs"]:
        assert codes[a] == 0 and codes[b] == bit, (case.meta["names"][a], codes[a], case.meta["names"][b], codes[b])
    assert codes[case.meta["behind"]] == 16
    assert sum(c == 0 for c in codes) >= 4 and n_vis == sum(c == 0 for c in codes)
    W, H = cam["width"], cam["height"]
    for a, b, bit in case.meta["pairs"][:4]:                                   # the border pairs: a fraction of a pixel apart
        ha, hb = o.feature(a)["h"], o.feature(b)["h"]
        assert 0.05 < np.abs(ha - hb).max() < 0.2
        bound = {"left": 20.0, "right": W - 21.0, "top": 20.0, "bottom": H - 21.0}[case.meta["names"][a].split("_")[0]]
        k = 0 if bit == 1 else 1
        assert min(ha[k], hb[k]) < bound < max(ha[k], hb[k])
    assert n_vis > case.n_select                                              # the selection is a cut
    assert o.num_selected == case.n_select


def test_features_exactly_on_the_upper_bounds_are_visible():
    case = sc.on_the_bound_scene()
    o = case.oracle()
    assert case.run_seams(o) == 4
    for i, want in enumerate(case.meta["expect_h"]):
        if want is not None:
            assert tuple(o.feature(i)["h"]) == want                           # exactly: not a bit off the bound
    assert case.vis_codes(o) == [0, 0, 0, 0]


# ----------------------------------------------------------------------------------------------------- 2: ranks, ties, rank split
def test_rank_split_model_and_capacities():
    assert [sc.rank_split(ns)[0] for ns, _ in sc.RANK_SIZES] == [4, 4, 2, 2, 2, 1, 1, 1, 1, 1]
    assert sc.rank_split(64)[1] == [16, 32, 48] and sc.rank_split(127)[1] == [63] and sc.rank_split(63)[1] == [15, 31, 47]
    assert sum(cap > ns for ns, cap in sc.RANK_SIZES) * 2 >= len(sc.RANK_SIZES)


@pytest.mark.parametrize("ns,capacity", sc.RANK_SIZES)
def test_rank_maps_tie_where_they_say(ns, capacity):
    case = sc.rank_map(ns, capacity)
    m = case.meta
    o = case.oracle()
    n_vis = case.run_seams(o)
    codes = case.vis_codes(o)
    feats = [o.feature(i) for i in range(ns)]
    for g in m["groups"]:
        for k in g[1:]:
            assert np.array_equal(feats[k]["S"], feats[g[0]]["S"]), g        # bit-identical S, hence score
        assert all(codes[k] == 0 for k in g)
    # members either side of every boundary of the rank split; the triple in as many slices as there are
    slice_of = lambda s: sum(s >= b for b in m["bounds"])
    for b in m["bounds"]:
        assert any(g[0] == b - 1 and g[1] == b for g in m["groups"]), b
    triple = [g for g in m["groups"] if len(g) == 3][0]
    assert len({slice_of(s) for s in triple}) == min(3, m["P"])
    if ns > sc.SELECT_THREADS:
        assert any(g[0] < sc.SELECT_THREADS <= g[-1] for g in m["groups"])   # a tie across a thread's first and second feature
    # scores outside the groups are distinct, and the order is not list order
    score = np.array([f["S"][0, 0] + f["S"][1, 1] for f in feats])
    vis = [i for i in range(ns) if codes[i] == 0]
    grouped = {s for g in m["groups"] for s in g}
    loose = [i for i in vis if i not in grouped]
    assert len(set(score[loose])) == len(loose) and not (set(score[loose]) & set(score[list(grouped)]))
    assert n_vis == len(vis) and sorted(m["invisible"]) == [i for i in range(ns) if codes[i] != 0]
    assert codes[m["dup_invisible"]] == 4 and np.array_equal(case.y[m["dup_invisible"]], case.y[m["dup_of"]])
    full = m["full_order"]
    assert sorted(full) == vis and full != vis
    assert all(score[full[k]] >= score[full[k + 1]] for k in range(len(full) - 1)) and (score[vis] > 0).all()
    for g in m["groups"]:                                                    # ties keep list order, side by side
        at = [full.index(s) for s in g]
        assert at == list(range(at[0], at[0] + len(g)))
    # the cut falls inside the cut pair: its first member is the last feature selected
    sel = list(o.selected_labels())
    assert 0 < case.n_select < n_vis and sel == full[:case.n_select]
    assert sel[-1] == m["cut"][0] and m["cut"][1] not in sel and full[case.n_select] == m["cut"][1]


def test_all_equal_zero_scores_and_empty_selections():
    case = sc.all_equal_map()
    o = case.oracle()
    assert case.run_seams(o) == case.N
    S0 = o.feature(0)["S"]
    assert all(np.array_equal(o.feature(i)["S"], S0) for i in range(case.N))
    assert list(o.selected_labels()) == list(range(case.n_select))
    o = case.oracle()
    assert case.run_seams(o, 0) == case.N and o.num_selected == 0              # n_select = 0: all visible, none selected

    case = sc.zero_score_map()
    o = case.oracle()
    n_vis = case.run_seams(o)
    assert n_vis == case.N
    for i in case.meta["zero"]:
        S = o.feature(i)["S"]
        assert S[0, 0] + S[1, 1] == 0.0 and not S.any()
    scores = [o.feature(i)["S"][0, 0] + o.feature(i)["S"][1, 1] for i in case.meta["positive"]]
    assert min(scores) > 0.0
    sel = list(o.selected_labels())
    assert sorted(sel) == case.meta["positive"] and sel != case.meta["positive"]
    assert len(sel) < case.n_select < n_vis                                    # it stopped at the first zero, not at n

    case = sc.nan_score_map()
    o = case.oracle()
    n_vis = case.run_seams(o)
    vis = [i for i in range(case.N) if i not in case.meta["invisible"]]
    assert np.isfinite(o.get_state()[0]).all() and all(np.isnan(o.feature(i)["S"]).all() for i in vis)
    assert n_vis == len(vis) > case.n_select and list(o.selected_labels()) == vis[:case.n_select]     # list order

    case = sc.none_visible_map()
    o = case.oracle()
    assert case.run_seams(o) == 0 and o.num_selected == 0 and all(c == 1 for c in case.vis_codes(o))


# ---------------------------------------------------------------------------------------------------------- 3: the deletion walk
def test_reference_walk_model():
    assert sc.reference_walk(range(6), {0, 1, 2, 4}) == [0, 2, 4]
    assert sc.reference_walk(range(5), {0, 1, 2, 3, 4}) == [0, 2, 4]
    assert sc.reference_walk(range(4), {2, 3}) == [2]
    assert sc.AT_FRACTION[1] / sc.AT_FRACTION[0] == sc.FRACTION and sc.AT_MINIMUM[1] / sc.AT_MINIMUM[0] < sc.FRACTION


def run_lengths(labels, scheduled):
    runs, cur = [], 0
    for lab in labels:
        if lab in scheduled:
            cur += 1
        elif cur:
            runs.append(cur)
            cur = 0
    return runs + ([cur] if cur else [])


@pytest.mark.parametrize("kind", ["ten", "ten_holes", "130", "257"])
def test_deletion_plans_on_the_oracle(kind):
    plan = sc.deletion_plan(kind)
    live = [lab for lab in range(plan["n"]) if lab not in plan["first"]]
    sched = set(plan["scheduled"])
    if kind == "ten":
        assert run_lengths(live, sched) == [3, 1, 2] and live[0] in sched and live[-1] in sched
        assert plan["gone2"] == [0, 2, 4, 8] and plan["gone3"] == [1, 9]
        assert 6 not in sched and 7 not in sched                               # at the fraction exactly; one attempt short
    if kind == "ten_holes":
        assert run_lengths(live, sched) == [2, 1, 2] and plan["gone2"] == [0, 5, 8] and plan["gone3"] == [2, 9]
    if kind == "130":
        assert run_lengths(live, sched) == [2, 1, 3, 2, 4, 5, 2, 3, 6]
        assert {124, 126, 128} <= set(plan["gone2"])                           # the run over slots 124 .. 129
        assert {125, 129} <= set(plan["gone3"]) and 127 not in plan["gone3"]    # (what it leaves is a run of three)
    if kind == "257":
        assert plan["gone2"] == [0, 100, 102, 254, 256] and plan["gone3"] == [101, 255]
    pr = sc.deletion_pair(plan, make_engine=False)
    o = pr.oracles[0]
    sc.step(pr, 0)
    sc.set_counters(pr, {lab: sc.GO for lab in plan["first"]})
    sc.step(pr, 1)
    assert sc.oracle_labels(o) == live
    sc.set_counters(pr, plan["counters"])
    sc.step(pr, 2)
    assert sorted(set(live) - set(sc.oracle_labels(o))) == plan["gone2"]
    if kind == "257":
        assert o.measurement_size >= plan["n_select"]                          # most of the selected features matched: an update ran
    after2 = sc.oracle_labels(o)
    sc.step(pr, 3)
    assert sorted(set(after2) - set(sc.oracle_labels(o))) == plan["gone3"]
    for i in range(o.num_features):                                            # the extras were never measured
        f = o.feature(i)
        if f["label"] >= plan["base"]:
            assert (f["attempted"], f["successful"]) == plan["counters"].get(f["label"], (0, 0))


# ------------------------------------------------------------------------------- 4: a partial feature inside a scheduled run
@pytest.mark.parametrize("mirror", [False, True])
def test_reference_deletes_on_both_sides_of_a_partial_feature(mirror):
    pr = sc.partial_run_pair(mirror, make_engine=False)
    o = pr.oracles[0]
    kinds = o.feature_kinds()
    want = [3] * 6 + [6] + [3] * (2 if mirror else 1)
    assert list(kinds[:, 0]) == want and list(kinds[:, 2]) == list(range(len(want)))
    assert kinds[6, 1] == 0 and o.mapping_info()["n_partial"] == 1
    sc.step(pr, 1, enable_mapping=True)
    gone = {5, 8} if mirror else {5, 7}
    assert sc.oracle_labels(o) == [lab for lab in range(len(want)) if lab not in gone]      # both, in this one frame
    kinds = o.feature_kinds()
    assert [int(k[0]) for k in kinds if k[2] == 6] == [6] and o.mapping_info()["n_partial"] == 1   # P is left alone, still partial
