"""The case table of the dense EKF update's edges (sl2_ekf_update.hip and its phase units sl2_update_*.hip): every k_fwdsub_lds<NB> instantiation, the block and
chunk remainders of m, systems that shrink from one update to the next on one engine, mixed systems in one launch, both sides of
every dispatch boundary of the update plan (sl2_update_plan.hpp), the forms of k_build_AS and the live-tile rules of k_syrk.
Pure numpy and the CPU oracle: tests/test_ekf_update_cases_host.py shows on the oracle alone that every schedule reaches the m
values it exists for, that the truth of tests/ekf_update_truth.py agrees with the oracle, and that the sizes and kernels written
in the table are what the compiled plan makes of the case; tests/test_gpu_ekf_update_edges.py holds the engine to truth and
oracle on them, and the engine's own plan to the table.

A case is stepped by the seams (predict, auto_select_n_features(n), make_measurements, update, finish_step) with the n of its
schedule, one entry a frame; feature_sigma = 0.004 everywhere, so P is dense and every live tile changes.  The oracle has no
seam for the symmetrisation at the end of GoOneStep: its P keeps the rounding-level asymmetry of its update from frame to frame,
five decades below TOL_P.

Where the table departs from the shapes first proposed for it, the sizing rules are the reason (the host test asks the plan):
  * sl2_create clamps number_of_features_to_select to the capacity, so nblk_max = NB needs a capacity of at least 16 NB - 15
    slots: group a runs its 24 live features in engines of max(24, 16 NB) slots, and selects min(n, 16 NB) of them;
  * ld = roundup(13 + 3 N + 6 + 1, 64) is 1024 up to N = 334 and 1088 from 335 on: that pair is the k_build_AS<1,4> / <2,2> edge;
  * nine sequences at ld = 256 are 144 strips, inside k_fwdsub_ksplit's range: the mixed batch runs a second time under
    SL2_NO_KSPLIT so that k_fwdsub_lds sees it too.

  * group b steps ONE frame.  Measured at N = 128 and 144 (m = 256, 288; cond(S) = 3e3, then 1e3): after the first update the
    oracle (explicit S^-1) is 4e-14 |P| from the truth and the engine 2e-15; the second update, in which |P| shrinks eightfold,
    carries that difference of the two PRIORS to 0.9 .. 1.5e-11 between engine and oracle, while each stays on the truth of
    its own prior (engine 5e-15 .. 9e-15, oracle 3e-13 .. 8e-13).  A second frame there measures the oracle's inverse, not a kernel;
    every block of k_fwdsub_lds<NB> is live on the first.

THE CONSTANT C of the truth bound  |P+ - truth|_F <= C m 2^-53 cond(S) |P_prior|_F,  max |x+ - truth| <= C m 2^-53 cond(S)
max(1, |x|_inf):  profiles/ekf_update_edges.json holds the worst deviation / bound of every case group at C = 8, for the engine
(MI355X) and for the oracle (CPU).  The bound is tightest at m = 2, where S is 2 x 2, cond(S) = 1 and the whole budget is
sixteen roundings on |P|_F: there the oracle itself (explicit S^-1, sums over all n columns) uses 0.84 of it and the engine
0.058.  The engine's worst ratio is above 1/64, so C = 8 stays as proposed; at large m, where cond(S) is 1e2 .. 3e3, both are
three to six decades inside."""
import numpy as np

import ekf_update_truth as tr
import oracle_api as oa
from scenelib2_amd import synth
from slam_helpers import Pair

C_BOUND = 8.0
FEATURE_SIGMA = 0.004
TOL_X, TOL_P, TOL_P_LARGE = 1e-12, 1e-11, 1e-10        # tests/test_gpu_slam.py: engine against the oracle (n >= 613: TOL_P_LARGE)

BUILD, CHOL, KSPLIT, LDS, GEMM, SYRK = "k_build_AS", "k_chol_left", "k_fwdsub_ksplit", "k_fwdsub_lds", "k_fwd_gemm", "k_syrk"
CHOL_SOLVE, CHOL_SYRK = "k_fwdsub_lds@chol", "k_chol_syrk"
# (must have run, must not have run) of the four chains the dispatch can take
KSPLIT_CHAIN = ((BUILD, CHOL, KSPLIT, SYRK), (LDS, GEMM, CHOL_SOLVE, CHOL_SYRK))
LDS_CHAIN = ((BUILD, CHOL, LDS, SYRK), (KSPLIT, GEMM, CHOL_SOLVE, CHOL_SYRK))
GROUPED_CHAIN = ((BUILD, CHOL, LDS, GEMM, SYRK), (KSPLIT, CHOL_SOLVE, CHOL_SYRK))
PANEL_CHAIN = ((BUILD, CHOL, CHOL_SOLVE, CHOL_SYRK, LDS, GEMM, SYRK), (KSPLIT,))


class Case:
    def __init__(self, name, counts, max_features, n_select, schedule, ld, mld, fwd, chain, cam=(320, 240), env=None,
                 build="<1,4>", nsplit=None, chol="left", m=(), blocks=(), residues32=None, residues16=(), shrinks=False,
                 m_by_frame=None, paused=None, delete=None, truth=True, tol_P=TOL_P, unused_stay_zero=False):
        self.name, self.group = name, name[0]
        self.counts, self.batch = list(counts), len(counts)          # live features per sequence
        self.max_features, self.n_select = max_features, n_select    # the engine's capacity and number_of_features_to_select
        self.schedule = list(schedule)                               # n handed to auto_select_n_features, frame by frame
        self.cam = cam
        self.env = dict(env or {})                                   # switches of the TEST build, set around sl2_create only
        # what sl2_create and the dispatch must make of it
        self.ld, self.mld, self.nblk_max = ld, mld, mld // 32
        # fwd: "ksplit", "lds<NB>" or "grouped"; build: "<1,4>", "<2,2>" (k_build_AS), "ahead<4>" or "ahead<2>" (k_build_AS_ahead)
        self.fwd, self.chol, self.build, self.nsplit = fwd, chol, build, nsplit
        self.must_run, self.must_not_run = chain
        # what the schedule exists to hit
        self.m = set(m)                                              # values of m, each on some frame of some sequence
        self.blocks = set(blocks)                                    # numbers of live 32-row blocks
        self.residues32 = dict(residues32 or {})                     # {live blocks: residues of m mod 32}
        self.residues16 = set(residues16)                            # m mod 16: k_syrk's last chunk
        self.shrinks = shrinks                                       # some sequence's m falls from one frame to the next
        self.m_by_frame = m_by_frame                                 # {frame: [m of every sequence]}
        self.paused = dict(paused or {})                             # {frame: sequences that sit the frame out}
        self.delete = dict(delete or {})                             # {frame: label deleted in every sequence in front of it}
        self.truth, self.tol_P, self.unused_stay_zero = truth, tol_P, unused_stay_zero

    def __repr__(self):
        return self.name

    @property
    def truth_seqs(self):
        """Every sequence of a batch of up to four (and of the mixed batch); else the first, a middle and the last."""
        if not self.truth:
            return ()
        B = self.batch
        return tuple(range(B)) if B <= 4 or self.group == "d" else (0, B // 2, B - 1)

    def n_of(self, k):
        """What the engine selects on frame k: launch_select clamps n to the engine's number_of_features_to_select."""
        return min(self.schedule[k], self.n_select, self.max_features)

    def active(self, k):
        return [b for b in range(self.batch) if b not in self.paused.get(k, ())]


# --------------------------------------------------------------------------------------------------------------- the table
def _cases():
    out = []
    # a: every k_fwdsub_lds<NB>, partly live: two live blocks of NB, then one with a short tail (NB = 1: a full block, then the tail)
    for NB in range(1, 14):
        N = max(24, 16 * NB)
        out.append(Case("a_lds%d_partly_live" % NB, [24] * 24, N, 16 * NB, [24, 9], ld=(13 + 3 * N + 7 + 63) // 64 * 64,
                        mld=32 * NB, fwd="lds<%d>" % NB, chain=LDS_CHAIN, nsplit=min(128, (N + 3) // 4),
                        m=(32, 18) if NB == 1 else (48, 18), blocks=(1,) if NB == 1 else (2, 1), shrinks=True))
    # b: k_fwdsub_lds<NB> with all NB blocks live, at the smallest batch of more than 160 strips
    for NB, B, ld, cam, nsplit in [(3, 14, 192, (320, 240), 12), (6, 9, 320, (320, 240), 24), (8, 6, 448, (640, 480), 32),
                                   (9, 6, 512, (640, 480), 36), (13, 4, 704, (640, 480), 52)]:
        N = 16 * NB
        out.append(Case("b_lds%d_all_live" % NB, [N] * B, N, N, [N], ld=ld, mld=32 * NB, fwd="lds<%d>" % NB, chain=LDS_CHAIN,
                        cam=cam, nsplit=nsplit, blocks=(NB,), truth=13 + 3 * N <= 450, tol_P=TOL_P if 13 + 3 * N < 613 else TOL_P_LARGE))
    # c: remainders and shrinking systems, one schedule through both substitution kernels
    sched = [64, 17, 57, 8, 49, 1, 32, 9, 25, 7, 24, 16, 63, 15, 23, 31, 56, 12, 55, 21]
    edge = {0, 2, 14, 16, 18, 30}
    for B, fwd, chain in [(24, "lds<4>", LDS_CHAIN), (2, "ksplit", KSPLIT_CHAIN)]:
        out.append(Case("c_remainders_B%d" % B, [64] * B, 64, 64, sched, ld=256, mld=128, fwd=fwd, chain=chain, nsplit=16,
                        residues32={1: edge, 2: edge, 4: edge}, residues16=(0, 2, 8, 10, 14), shrinks=True))
    # d: mixed systems in one launch, the last sequence paused on frame 1
    counts = [0, 1, 8, 9, 16, 17, 40, 64, 64]
    for name, env, fwd, chain in [("d_mixed", None, "ksplit", KSPLIT_CHAIN), ("d_mixed_no_ksplit", {"SL2_NO_KSPLIT": "1"}, "lds<4>", LDS_CHAIN)]:
        out.append(Case(name, counts, 64, 64, [64, 64], ld=256, mld=128, fwd=fwd, chain=chain, env=env, nsplit=16,
                        m_by_frame={0: [0, 2, 16, 18, 32, 34, 80, 128, 128], 1: [0, 2, 16, 18, 32, 34, 80, 128, None]}, paused={1: (8,)}))
    # e: dispatch boundaries from both sides, small live maps in large engines
    for B, fwd, chain in [(20, "ksplit", KSPLIT_CHAIN), (21, "lds<2>", LDS_CHAIN)]:
        out.append(Case("e_strips_B%d" % B, [24] * B, 24, 24, [24, 9], ld=128, mld=64, fwd=fwd, chain=chain, nsplit=6, m=(48, 18)))
    for ns, cap, ld, mld, fwd, chain, chol, nsplit in [
            (128, 129, 448, 256, "ksplit", KSPLIT_CHAIN, "left", 33), (129, 129, 448, 288, "lds<9>", LDS_CHAIN, "left", 33),
            (208, 209, 704, 416, "lds<13>", LDS_CHAIN, "left", 53), (209, 209, 704, 448, "grouped", GROUPED_CHAIN, "left", 53),
            (256, 257, 832, 512, "grouped", GROUPED_CHAIN, "left", 65), (257, 257, 832, 640, "grouped", PANEL_CHAIN, "panels", 65)]:
        out.append(Case("e_select%d" % ns, [24], cap, ns, [24, 9], ld=ld, mld=mld, fwd=fwd, chain=chain, chol=chol, nsplit=nsplit, m=(48, 18)))
    out.append(Case("e_panel_from_2", [144, 144], 144, 144, [144, 63, 128, 64, 129, 65, 127], ld=512, mld=384, fwd="grouped", chain=PANEL_CHAIN,
                    chol="panels", cam=(640, 480), env={"SL2_PANEL_FROM": "2"}, nsplit=36, m=(126, 128, 130, 254, 256, 258, 288), shrinks=True))
    # f: k_build_AS
    for N in (5, 6, 7, 8):
        out.append(Case("f_build_N%d" % N, [N, N], N, N, [N, N], ld=64, mld=32, fwd="ksplit", chain=KSPLIT_CHAIN, nsplit=2, m=(2 * N,)))
        out.append(Case("f_build_N%d_one_workgroup" % N, [N, N], N, N, [N, N], ld=64, mld=32, fwd="ksplit", chain=KSPLIT_CHAIN,
                        env={"SL2_BUILD_SPLIT": "1"}, build="ahead<4>", nsplit=1, m=(2 * N,)))
    out.append(Case("f_build_ld1024", [24, 24], 334, 24, [24, 9], ld=1024, mld=64, fwd="ksplit", chain=KSPLIT_CHAIN, build="<1,4>", nsplit=84, m=(48, 18)))
    out.append(Case("f_build_ld1024_one_workgroup", [24, 24], 334, 24, [24, 9], ld=1024, mld=64, fwd="ksplit", chain=KSPLIT_CHAIN,
                    env={"SL2_BUILD_SPLIT": "1"}, build="ahead<2>", nsplit=1, m=(48, 18)))
    out.append(Case("f_build_ld1088", [24, 24], 335, 24, [24, 9], ld=1088, mld=64, fwd="ksplit", chain=KSPLIT_CHAIN, build="<2,2>", nsplit=84, m=(48, 18)))
    out.append(Case("f_build_deleted_slot", [12, 12], 12, 12, [12, 12], ld=64, mld=32, fwd="ksplit", chain=KSPLIT_CHAIN, nsplit=3, m=(24, 22),
                    delete={1: 5}, shrinks=True))
    # g: k_syrk's live-tile rules: 13 + 3 N = 28, 31, 34 | 61, 64, 67 inside ld = 256
    for N in (5, 6, 7, 16, 17, 18):
        out.append(Case("g_live_tiles_N%d" % N, [N, N], 60, N, [N, N], ld=256, mld=32 * ((2 * N + 31) // 32), fwd="ksplit", chain=KSPLIT_CHAIN,
                        nsplit=15, m=(2 * N,), unused_stay_zero=True))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ----------------------------------------------------------------------------------------------- the table and the plan
def plan_in_table_words(p):
    """A plan (Engine.debug_update_plan, update_plan_helpers.plan_of_engine) as the table writes it: build, nsplit, chol, fwd."""
    assert p["chol"] in ("left", "panels") and p["fwd"] in ("ksplit", "lds", "grouped"), p      # the product's forms only
    return p["build"], p["build_nsplit"], p["chol"], "lds<%d>" % p["fwd_nb"] if p["fwd"] == "lds" else p["fwd"]


def chain_of(fwd, chol):
    run, never = {BUILD, CHOL, SYRK}, set()
    (run if chol == "panels" else never).update((CHOL_SOLVE, CHOL_SYRK))
    (run if fwd == "ksplit" else never).add(KSPLIT)
    (never if fwd == "ksplit" else run).add(LDS)
    (run if fwd == "grouped" else never).add(GEMM)
    return run, never


# --------------------------------------------------------------------------------------------------- scenes, oracles, engines
_SCENES = {}


def scene(case, n_frames=None):
    """The rendered sequences of a case (a Pair without engine), shared by every case of the same camera, map sizes and length."""
    key = (case.cam, tuple(case.counts), len(case.schedule))
    if key not in _SCENES:
        _SCENES[key] = Pair(max(case.counts), len(case.schedule), batch=case.batch, cam=synth.default_camera(*case.cam),
                            feature_counts=case.counts, make_engine=False)
    return _SCENES[key]


def fresh_oracles(pr):
    """One new OracleSLAM per sequence of the scene, with the features' prior covariance of the engine."""
    out = []
    for b in range(pr.B):
        spec = pr.specs[b]
        o = oa.OracleSLAM(pr.cam, pr.params["delta_t"], max(spec.feat_y.shape[0], 1))
        o.set_state(spec.xv0, spec.Pxx0)
        for i in range(spec.feat_y.shape[0]):
            o.add_known_feature(spec.feat_y[i], spec.poses[0], pr.templates[b][i])
            o.set_feature_Pyy(i, np.eye(3) * FEATURE_SIGMA ** 2)
        out.append(o)
    return out


def make_engine(case, pr, monkeypatch):
    """The case's engine on the scene's sequences; the TEST library and its environment switches only where the case has some,
    and the environment only around sl2_create."""
    lib = None
    if case.env:
        from scenelib2_amd import _lib
        lib = _lib.load_testing()
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    pr.params = synth.default_params(case.n_select)
    try:
        return pr.make_engine_for(0, case.batch, case.max_features, feature_sigma=FEATURE_SIGMA, lib=lib)
    finally:
        for k in case.env:
            monkeypatch.delenv(k, raising=False)


def oracle_frame(case, pr, oracles, k, truth_of=()):
    """Frame k of the case through the oracles' seams.  Returns {b: truth} for b in truth_of, each with the oracle's own
    posterior (x_oracle, P_oracle: after KalmanFilterUpdate, before normalise_state), and [m of every sequence] (None: paused)."""
    truths, ms = {}, []
    for b, o in enumerate(oracles):
        if b not in case.active(k):
            ms.append(None)
            continue
        if k in case.delete:
            assert o.delete_feature(case.delete[k])
        o.kalman_filter_predict()
        o.auto_select_n_features(case.n_of(k))
        if o.num_selected:
            o.make_measurements(pr.frames[b][k])
        m = o.measurement_size if o.num_selected else 0
        ms.append(m)
        if b in truth_of:
            truths[b] = tr.posterior_truth_of_oracle(o) if m else None
        if m:                                              # GoOneStep: no update, no normalisation without a measurement
            o.kalman_filter_update()
            if b in truth_of:
                truths[b].update(x_oracle=o.total_state(), P_oracle=o.total_covariance())
            o.normalise_state()
        o.delete_bad_features()
    return truths, ms


def check_targets(case, ms_by_frame):
    """ms_by_frame[k][b] = m of sequence b on frame k (None: paused): does the run hit everything the case exists for?"""
    seen = {m for ms in ms_by_frame for m in ms if m is not None}
    live = {m: (m + 31) // 32 for m in seen}
    assert case.m <= seen, (case, sorted(case.m - seen), sorted(seen))
    assert case.blocks <= set(live.values()), (case, sorted(live.values()))
    for nb, residues in case.residues32.items():
        got = {m % 32 for m in seen if live[m] == nb}
        assert residues <= got, (case, nb, sorted(residues - got))
    assert case.residues16 <= {m % 16 for m in seen if m}, (case, sorted(seen))
    if case.shrinks:
        assert any(a is not None and b is not None and b < a for k in range(1, len(ms_by_frame))
                   for a, b in zip(ms_by_frame[k - 1], ms_by_frame[k])), (case, ms_by_frame)
        assert any(a is not None and b is not None and b > a for k in range(1, len(ms_by_frame))
                   for a, b in zip(ms_by_frame[k - 1], ms_by_frame[k])) or len(ms_by_frame) == 2, (case, ms_by_frame)
    for k, want in (case.m_by_frame or {}).items():
        assert list(ms_by_frame[k]) == want, (case, k, ms_by_frame[k])


def report(case, who, k, b, t, rP, rx):
    """One line per posterior compared with the truth: deviation / bound at C_BOUND, printed before anything is asserted."""
    print("ekf-edge-ratio group=%s case=%s who=%s frame=%d seq=%d m=%d cond=%.3g P=%.3g x=%.3g" % (
        case.group, case.name, who, k, b, t["m"], t["cond"], rP, rx))
