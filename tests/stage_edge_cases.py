"""Case builders for the stages on either side of the search: feature prediction (visibility_test), selection
(auto_select_n_features) and the end of the step (delete_bad_features) - maps whose features sit ON the edges those stages
branch at.  Pure numpy and the CPU oracle: nothing here needs a GPU (the helpers that step a slam_helpers.Pair also step its
engine when it was made with one).  tests/test_stage_edge_cases_host.py shows on the oracle
alone that every case is what it claims to be; tests/test_gpu_stage_edges.py holds the engine to the oracle on them.

Geometry: the camera starts at r = (0, 0, -0.6), q = (1, 0, 0, 0), looking along +z at the textured plane z = 0 (synth.py).  A
feature is placed analytically on a chosen pixel of the PREDICTED pose (the pose after KalmanFilterPredict, which is the motion
model applied to xv0: oracle_api.motion_model), by the camera's own Unproject formula, the way
test_visibility_edge_follows_the_sequence_s_own_principal_point places its fifth feature."""
import numpy as np

import oracle_api as oa
from scenelib2_amd import synth

DT = 1.0 / 30.0
XV0 = np.array([0.0, 0.0, -0.6, 1.0, 0.0, 0.0, 0.0, 0.03, -0.02, 0.01, 0.02, -0.01, 0.015])
TEX_EXTENT, TEX_ORIGIN = 2.0, (0.0, 0.0)
_TEX = []


def texture():
    if not _TEX:
        _TEX.append(synth.make_texture())
    return _TEX[0]


def default_Pxx():
    P = np.zeros((13, 13))
    P[0, 0] = P[1, 1] = P[2, 2] = 0.0004
    return P


def predicted_pose(xv0=XV0, dt=DT):
    """xp after KalmanFilterPredict: the first seven entries of the motion model's f(xv0)."""
    return oa.motion_model(xv0, dt)[0][:7].copy()


def rotation(q):
    return oa.quat_ops(q, q)[2]


def ray_of_pixel(cam, u, v):
    """Camera::Unproject (camera.cpp:133-154): the ray of image point (u, v) in the camera frame, z = 1."""
    c0, c1 = u - cam["u0"], v - cam["v0"]
    factor = np.sqrt(1 - 2 * cam["kd1"] * (c0 * c0 + c1 * c1))
    return np.array([(c0 / factor) / -cam["fku"], (c1 / factor) / -cam["fkv"], 1.0])


def point_on_pixel(cam, xp, u, v, depth=None):
    """The world point that the camera at pose xp sees at (u, v): on the plane z = 0 (depth=None) or `depth` along the ray."""
    d = rotation(xp[3:7]) @ ray_of_pixel(cam, u, v)
    t = -xp[2] / d[2] if depth is None else depth
    return xp[:3] + t * d


def turned(a, axis, theta):
    """Unit vector a turned by theta about a unit axis perpendicular to it (Rodrigues)."""
    return a * np.cos(theta) + np.cross(axis, a) * np.sin(theta)


class Case:
    """One sequence: initial state, known features (with their prior covariances) and what the stage calls are given."""

    def __init__(self, name, cam, n_select, capacity, y, xp_org, xv0=XV0, Pxx0=None, Pyy=None, templates=None, predict=True,
                 frame=None, meta=None):
        self.name, self.cam, self.n_select, self.capacity = name, dict(cam), int(n_select), int(capacity)
        self.y, self.xp_org = np.asarray(y, np.float64).reshape(-1, 3), np.asarray(xp_org, np.float64).reshape(-1, 7)
        self.N = self.y.shape[0]
        self.xv0 = np.asarray(xv0, np.float64)
        self.Pxx0 = default_Pxx() if Pxx0 is None else np.asarray(Pxx0, np.float64)
        self.Pyy = np.zeros((self.N, 3, 3)) if Pyy is None else np.asarray(Pyy, np.float64).reshape(self.N, 3, 3)
        self.templates = np.zeros((self.N, 11, 11), np.uint8) if templates is None else np.asarray(templates, np.uint8)
        self.predict = predict          # False: the selection runs on the state as set (no process noise in Pxx)
        self.frame = frame              # the image of the predicted pose, for the cases that run whole steps
        self.params = synth.default_params(max(self.n_select, 1), DT)
        self.meta = meta or {}

    def oracle(self, n_select=None):
        o = oa.OracleSLAM(self.cam, DT, self.n_select if n_select is None else n_select)
        o.set_state(self.xv0, self.Pxx0)
        for i in range(self.N):
            o.add_known_feature(self.y[i], self.xp_org[i], self.templates[i])
            if self.Pyy[i].any():
                o.set_feature_Pyy(i, self.Pyy[i])
        return o

    def run_seams(self, o, n=None):
        """kalman_filter_predict (unless the case says not to) and auto_select_n_features on an oracle of this case."""
        if self.predict:
            o.kalman_filter_predict()
        return o.auto_select_n_features(self.n_select if n is None else n)

    def vis_codes(self, o):
        """visibility_test's code of every feature at the pose oracle `o` holds now (the predicted one after run_seams)."""
        xp = o.get_state()[0][:7]
        return [oa.measurement_model(self.cam, xp, self.y[i], self.xp_org[i])["vis"] for i in range(self.N)]


# --------------------------------------------------------------------------------------------------------------- 1: visibility
BORDER = 20.0                  # kImageSearchBoundary (full_feature_model.cpp:51)
PIXEL_MARGIN = 0.05            # the members of a border pair sit this far on either side of the bound: 0.1 px apart
RATIO_MARGIN = 1e-6            # relative distance of a length-ratio pair from 2 and 1/2
ANGLE_MARGIN = 1e-6            # radians either side of 45 degrees
# (FP64 evaluates h to ~1e-12 px and the ratio / angle to ~1e-15: the margins are nine and more decades above that, so the
#  oracle's arithmetic decides every pair - the host test is the proof - and the device's, which may differ in the last bits, too)


def visibility_scene(cam):
    """Every way visibility_test can fail, alone, next to a twin that passes: a pair either side of each of the four image borders
    (bits 1 and 2), a feature behind the camera (16), pairs either side of length ratio 2 and 1/2 (4) and of 45 degrees between the
    current and the original viewing ray (8), and five ordinary features.  Everything except the feature behind the camera lies
    on the textured plane, with its template cut from the image of the predicted pose, so that a whole step measures the
    visible ones."""
    W, H = cam["width"], cam["height"]
    xp = predicted_pose()
    here = XV0[:7].copy()
    um, vm = W / 2.0 + 3.0, H / 2.0 - 2.0
    names, ys, xos, pairs = [], [], [], []

    def add(name, y, xo):
        names.append(name)
        ys.append(np.asarray(y, np.float64))
        xos.append(np.asarray(xo, np.float64))
        return len(names) - 1

    def far_pose(y, w, dist):
        return np.concatenate([y - w * dist, [1.0, 0.0, 0.0, 0.0]])

    ordinary = [(0.31 * W, 0.33 * H), (0.62 * W, 0.38 * H), (0.5 * W, 0.52 * H), (0.37 * W, 0.71 * H), (0.72 * W, 0.67 * H)]
    add("ordinary0", point_on_pixel(cam, xp, *ordinary[0]), here)
    for tag, bit, inside, outside in (("left", 1, (BORDER + PIXEL_MARGIN, vm), (BORDER - PIXEL_MARGIN, vm)),
                                      ("right", 1, (W - 1 - BORDER - PIXEL_MARGIN, vm + 9), (W - 1 - BORDER + PIXEL_MARGIN, vm + 9)),
                                      ("top", 2, (um, BORDER + PIXEL_MARGIN), (um, BORDER - PIXEL_MARGIN)),
                                      ("bottom", 2, (um - 11, H - 1 - BORDER - PIXEL_MARGIN), (um - 11, H - 1 - BORDER + PIXEL_MARGIN))):
        a = add(tag + "_in", point_on_pixel(cam, xp, *inside), here)
        b = add(tag + "_out", point_on_pixel(cam, xp, *outside), here)
        pairs.append((a, b, bit))
    add("ordinary1", point_on_pixel(cam, xp, *ordinary[1]), here)
    behind = add("behind", xp[:3] + rotation(xp[3:7]) @ np.array([0.02, 0.01, -0.5]), here)      # z = -0.5 in the camera frame
    add("ordinary2", point_on_pixel(cam, xp, *ordinary[2]), here)
    # length ratio |y - r| / |y - r_org| either side of 2 and of 1/2: r_org on a ray 0.01 rad off the current one (so that the
    # angle test sees a plain small angle, not acos of 1 +- one bit)
    spots = [(0.42 * W, 0.45 * H), (0.58 * W, 0.60 * H), (0.45 * W, 0.30 * H)]
    for tag, spot, target in (("ratio2", spots[0], 2.0), ("ratiohalf", spots[1], 0.5)):
        y = point_on_pixel(cam, xp, *spot)
        d = y - xp[:3]
        mod = np.sqrt(d @ d)
        axis = np.cross(d / mod, [0.0, 1.0, 0.0])
        w = turned(d / mod, axis / np.sqrt(axis @ axis), 0.01)
        # ratio = mod / mod_o: inside (1, 2) for the first pair's visible member, inside (1/2, 1) for the second's
        inner = target * (1 - RATIO_MARGIN) if target > 1 else target * (1 + RATIO_MARGIN)
        outer = target * (1 + RATIO_MARGIN) if target > 1 else target * (1 - RATIO_MARGIN)
        a = add(tag + "_in", y, far_pose(y, w, mod / inner))
        b = add(tag + "_out", y + np.array([1e-4, 0.0, 0.0]), far_pose(y + np.array([1e-4, 0.0, 0.0]), w, mod / outer))
        pairs.append((a, b, 4))
    add("ordinary3", point_on_pixel(cam, xp, *ordinary[3]), here)
    y = point_on_pixel(cam, xp, *spots[2])
    d = y - xp[:3]
    mod = np.sqrt(d @ d)
    axis = np.cross(d / mod, [0.0, 1.0, 0.0])
    axis /= np.sqrt(axis @ axis)
    a = add("angle_in", y, far_pose(y, turned(d / mod, axis, np.pi / 4 - ANGLE_MARGIN), mod))
    y2 = y + np.array([0.0, 1e-4, 0.0])
    d2 = y2 - xp[:3]
    mod2 = np.sqrt(d2 @ d2)
    axis2 = np.cross(d2 / mod2, [0.0, 1.0, 0.0])
    axis2 /= np.sqrt(axis2 @ axis2)
    b = add("angle_out", y2, far_pose(y2, turned(d2 / mod2, axis2, np.pi / 4 + ANGLE_MARGIN), mod2))
    pairs.append((a, b, 8))
    add("ordinary4", point_on_pixel(cam, xp, *ordinary[4]), here)

    frame = synth.render_host(cam, texture(), TEX_EXTENT, TEX_ORIGIN, xp[None])[0]
    n = len(names)
    templates = np.zeros((n, 11, 11), np.uint8)
    for i in range(n):
        h = oa.measurement_model(cam, xp, ys[i], xos[i])["h"]
        u, v = int(np.clip(round(h[0]), 5, W - 6)), int(np.clip(round(h[1]), 5, H - 6))
        templates[i] = frame[v - 5:v + 6, u - 5:u + 6]
    return Case("visibility_%dx%d" % (W, H), cam, 8, n + 3, np.stack(ys), np.stack(xos), templates=templates, frame=frame,
                meta=dict(names=names, pairs=pairs, behind=behind))


def on_the_bound_scene():
    """Predicted measurements EXACTLY on the upper bounds width - 21 and height - 21: visible, because the tests are strict
    (`h > bound`).  The pairs above sit a twentieth of a pixel off their bounds and cannot tell `>` from `>=`; these can.  Exact by
    construction: no distortion, fku = 137 and fkv = 94 with (u0, v0) = (162, 125), q = (1, 0, 0, 0) exactly (the selection runs
    on the state as set: a predict would turn q), features at (-1, 0, 1) / 2 and (0, -1, 1) / 2 in the camera frame - every
    product and quotient on the way to h = (299, 125) and (162, 219) is exact in binary floating point."""
    cam = dict(width=320, height=240, fku=137.0, fkv=94.0, u0=162.0, v0=125.0, kd1=0.0, sd=1)
    xv0 = np.array([0.0, 0.0, -0.5, 1.0, 0.0, 0.0, 0.0, 0.03, -0.02, 0.01, 0.02, -0.01, 0.015])
    y = np.array([[-0.5, 0.0, 0.0], [0.0, -0.5, 0.0], [0.125, 0.0625, 0.0], [-0.5, -0.5, 0.0]])
    xo = np.tile(np.concatenate([[0.0, 0.015625, -0.5], [1.0, 0.0, 0.0, 0.0]]), (4, 1))
    return Case("on_the_bound", cam, 4, 6, y, xo, xv0=xv0, predict=False,
                meta=dict(expect_h=[(299.0, 125.0), (162.0, 219.0), None, (299.0, 219.0)]))


# ------------------------------------------------------------------------------------------------- 2: ranks, ties, rank split
RANK_SIZES = [(63, 80), (64, 64), (65, 100), (127, 127), (128, 160), (129, 129), (192, 200), (193, 193), (256, 300), (257, 257)]
SELECT_THREADS = 256           # the block size of k_select (sl2_frontend.hip: launch_select)


def rank_split(ns, threads=SELECT_THREADS):
    """(P, slice boundaries) of select_body's rank count for a map of ns slots: P = threads / roundup(ns, 64) clamped to 1..4
    groups of threads, group `part` counting the slots part * ns / P .. (part + 1) * ns / P."""
    G = (ns + 63) // 64 * 64
    P = max(1, min(4, threads // G))
    return P, [part * ns // P for part in range(1, P)]


def _tie_layout(ns):
    """Slots of the tie groups of a rank map: pairs that straddle every slice boundary of the rank split, a triple with a member
    in as many different slices as there are, and (beyond the split: one group of threads, several features per thread from 257
    slots on) pairs across slots 63 | 64 and 255 | 256 or the map's last two."""
    P, bounds = rank_split(ns)
    if P == 4:
        pairs = [(b - 1, b) for b in bounds]
        triple = (bounds[0] - 3, bounds[1] + 2, bounds[2] + 3)
    elif P == 2:
        pairs = [(bounds[0] - 1, bounds[0])]
        triple = (bounds[0] - 4, bounds[0] + 3, ns - 2)
    else:
        last = min(256, ns - 1)
        pairs = [(63, 64), (last - 1, last)]
        triple = (3, ns // 2 + 5, ns - 4)
    return P, bounds, pairs, triple


def rank_map(ns, capacity):
    """ns live features of one sequence whose selection order is NOT list order (distinct positive Pyy, scattered), with tie
    groups - exact duplicates: same y, xp_org and Pyy, hence bit-identical S and score - placed across the slice boundaries of
    k_select's rank split, one tie pair that straddles the cut n_select makes, and invisible features in between (behind the
    left image border), one of which duplicates a tied feature's position under another xp_org (it fails the length ratio)."""
    cam = synth.default_camera()
    W, H = cam["width"], cam["height"]
    rng = np.random.default_rng(4200 + ns)
    xp = predicted_pose()
    here = XV0[:7].copy()
    P, bounds, pairs, triple = _tie_layout(ns)
    groups = [tuple(p) for p in pairs] + [tuple(triple)]
    taken = set(s for g in groups for s in g)
    assert len(taken) == sum(len(g) for g in groups) and min(taken) >= 0 and max(taken) < ns

    def free_from(s):
        while s in taken:
            s += 1
        assert s < ns
        taken.add(s)
        return s

    cut = (free_from(ns // 3), free_from(2 * ns // 3 + 1))            # the pair the cut falls into
    groups.append(cut)
    dup_invisible = free_from(ns // 2 - 7)                             # same y as triple[0], another xp_org
    invisible = [dup_invisible] + [free_from(s) for s in range(5, ns - 1, 9)]
    y, xo, Pyy = np.zeros((ns, 3)), np.tile(here, (ns, 1)), np.zeros((ns, 3, 3))
    sig = 0.002 + 0.00004 * rng.permutation(ns)                        # distinct prior sigmas, in no order
    sig[list(cut)] = 0.002 + 0.00004 * (ns // 2) + 0.00002             # the cut pair: a middling score of its own
    for i in range(ns):
        u, v = rng.uniform(45, W - 46), rng.uniform(45, H - 46)
        if i in invisible:
            u = 8.0
        y[i] = point_on_pixel(cam, xp, u, v, depth=rng.uniform(0.45, 0.9))
        Pyy[i] = np.eye(3) * sig[i] ** 2
    for g in groups:
        for m in g[1:]:
            y[m], xo[m], Pyy[m] = y[g[0]], xo[g[0]], Pyy[g[0]]
    y[dup_invisible] = y[triple[0]]
    xo[dup_invisible] = np.concatenate([y[triple[0]] - 0.3 * (y[triple[0]] - xp[:3]), [1.0, 0.0, 0.0, 0.0]])   # ratio 1 / 0.3
    case = Case("ranks_%d_of_%d" % (ns, capacity), cam, ns, capacity, y, xo, Pyy=Pyy,
                meta=dict(P=P, bounds=bounds, groups=groups, cut=cut, invisible=sorted(invisible), dup_invisible=dup_invisible,
                          dup_of=triple[0]))
    # n_select: the cut falls between the members of the cut pair, i.e. directly behind the first one in the oracle's order
    o = case.oracle(ns)
    case.run_seams(o, ns)
    order = list(o.selected_labels())
    case.n_select = order.index(cut[0]) + 1
    case.params = synth.default_params(case.n_select, DT)
    case.meta["full_order"] = order
    return case


def all_equal_map(n=40, capacity=48, n_select=12):
    """Every feature a duplicate of the first: one tie group of n.  The selection is the first n_select slots in order."""
    cam = synth.default_camera()
    xp = predicted_pose()
    y = point_on_pixel(cam, xp, 150.0, 110.0, depth=0.7)
    return Case("all_equal", cam, n_select, capacity, np.tile(y, (n, 1)), np.tile(XV0[:7], (n, 1)),
                Pyy=np.tile(np.eye(3) * 0.003 ** 2, (n, 1, 1)))


def zero_score_map():
    """Scores that are exactly 0.0: a camera with sd = 0 (R = 0), a vehicle covariance of zero and - so that no process noise
    enters Pxx - the selection on the state as set, without a predict.  S is then dh_by_dy Pyy dh_by_dy^T alone: positive for the
    features with a prior covariance, 0.0 for those without.  The reference stops selecting at the first zero score
    (monoslam.cpp:241-249)."""
    cam = dict(synth.default_camera(), sd=0)
    rng = np.random.default_rng(77)
    xp = XV0[:7]
    n = 20
    positive = [1, 2, 5, 8, 11, 12, 16, 19]
    y, Pyy = np.zeros((n, 3)), np.zeros((n, 3, 3))
    for i in range(n):
        y[i] = point_on_pixel(cam, xp, rng.uniform(45, 270), rng.uniform(45, 190), depth=rng.uniform(0.45, 0.9))
    for k, i in enumerate(positive):
        Pyy[i] = np.eye(3) * (0.002 + 0.0003 * ((k * 5) % 8)) ** 2
    return Case("zero_scores", cam, 16, 24, y, np.tile(XV0[:7], (n, 1)), Pxx0=np.zeros((13, 13)), Pyy=Pyy, predict=False,
                meta=dict(positive=positive, zero=[i for i in range(n) if i not in positive]))


def nan_score_map():
    """Scores that are all NaN: an angular velocity of exactly zero (Q10: the motion model's Jacobian divides by |omega|), so the
    predict turns Pxx, and with it every S, into NaN while the pose stays finite.  `score > other` is then false for every pair:
    the reference's insertion keeps list order; visibility is decided as usual.  Every fourth feature is behind the border."""
    cam = synth.default_camera()
    xv0 = XV0.copy()
    xv0[10:13] = 0.0
    rng = np.random.default_rng(11)
    xp = predicted_pose(xv0)
    n = 18
    invisible = [i for i in range(n) if i % 4 == 2]
    y = np.stack([point_on_pixel(cam, xp, 7.0 if i in invisible else rng.uniform(45, 270), rng.uniform(45, 190),
                                 depth=rng.uniform(0.45, 0.9)) for i in range(n)])
    Pyy = np.stack([np.eye(3) * (0.002 + 0.0002 * ((7 * i) % n)) ** 2 for i in range(n)])
    return Case("nan_scores", cam, 9, 20, y, np.tile(xv0[:7], (n, 1)), xv0=xv0, Pyy=Pyy, meta=dict(invisible=invisible, nan=True))


def none_visible_map(n=12, capacity=16):
    """Every feature behind the left image border: nothing is visible, nothing is selected."""
    cam = synth.default_camera()
    xp = predicted_pose()
    y = np.stack([point_on_pixel(cam, xp, 6.0, 40.0 + 12 * i, depth=0.6) for i in range(n)])
    frame = synth.render_host(cam, texture(), TEX_EXTENT, TEX_ORIGIN, xp[None])[0]
    return Case("none_visible", cam, 8, capacity, y, np.tile(XV0[:7], (n, 1)), frame=frame)


# ---------------------------------------------------------------------------------------------------------- 3: the deletion walk
def reference_walk(labels, scheduled):
    """delete_bad_features' list walk (monoslam.cpp:661-703, Q27) in plain Python: a scheduled element is erased and the element
    that follows it is not examined in this pass.  Returns the labels erased."""
    lst, gone, i = list(labels), [], 0
    while i < len(lst):
        if lst[i] in scheduled:
            gone.append(lst.pop(i))
        i += 1
    return gone


MIN_ATTEMPTS, FRACTION = 10, 0.5          # synth.default_params: minimum_attempted_measurements_of_feature, successful_match_fraction
GO = (12, 3)                              # a measured feature's counters: below the fraction whatever the next match does (13, 3 or 4)
# counters of the EXTRA features (behind the left border: never selected, so their counters stand as set when the walk reads them)
AT_MINIMUM = (MIN_ATTEMPTS, 4)            # attempted == minimum, 4 / 10 < 0.5: goes
BELOW_MINIMUM = (MIN_ATTEMPTS - 1, 0)     # one attempt short: stays
AT_FRACTION = (MIN_ATTEMPTS, 5)           # 5 / 10 == 0.5 exactly (the division is exact): stays, the comparison is a strict <
EXTRAS = 4


def deletion_plan(kind):
    """What a deletion case does: `base` features of a synthetic sequence plus EXTRAS invisible ones at the end of the list;
    `first` = labels retired in step 1 (the inactive slots of step 2's runs); `counters` = label -> (attempted, successful) set
    before step 2.  Runs of scheduled features of every length 1..5, at slot 0, at the last feature, with a retired slot inside
    and directly in front, two runs one unscheduled feature apart; and the three counter edges."""
    if kind == "ten":                      # runs [0 1 2], [4], [8 9]; the three counter edges on 6, 7, 8
        base, first = 6, []
        counters = {0: GO, 1: GO, 2: GO, 4: GO, 6: AT_FRACTION, 7: BELOW_MINIMUM, 8: AT_MINIMUM, 9: AT_MINIMUM}
        cam, n_select, sigma = synth.default_camera(), 6, 0.004
    elif kind == "ten_holes":              # run [0 (1) 2] with a retired slot inside, run [5] with one directly in front
        base, first = 6, [1, 4]
        counters = {0: GO, 2: GO, 5: GO, 6: AT_FRACTION, 7: BELOW_MINIMUM, 8: AT_MINIMUM, 9: AT_MINIMUM}
        cam, n_select, sigma = synth.default_camera(), 6, 0.004
    elif kind == "130":                    # every run length; a run over slots 124 .. 129: across thread 127 | slot 128 of k_finalize
        base, first = 126, [11, 20]
        runs = [[0, 1], [3], [10, 12, 13], [21, 22], [30, 31, 32, 33], [40, 41, 42, 43, 44], [50, 51], [53, 54, 55], [124, 125]]
        counters = {lab: GO for r in runs for lab in r}
        counters.update({126: AT_MINIMUM, 127: AT_MINIMUM, 128: AT_MINIMUM, 129: AT_MINIMUM})
        cam, n_select, sigma = synth.default_camera(), 126, 0.004
    elif kind == "257":                    # 784 state columns > 13 + 6 * 128: the strip leaves the registers; run over 254 .. 256
        base, first = 253, []
        counters = {0: GO, 100: GO, 101: GO, 102: GO, 253: AT_FRACTION, 254: AT_MINIMUM, 255: AT_MINIMUM, 256: AT_MINIMUM}
        cam, n_select, sigma = synth.default_camera(640, 480), 40, 0.003
    else:
        raise KeyError(kind)
    n = base + EXTRAS
    after_first = [lab for lab in range(n) if lab not in first]

    def scheduled(lab):            # at the time the walk reads the counters
        a, s = counters[lab]
        if counters[lab] == GO:    # a measured feature: one more attempt by then, matched or not
            return a + 1 >= MIN_ATTEMPTS and (s + 1) / (a + 1) < FRACTION
        return a >= MIN_ATTEMPTS and s / a < FRACTION

    sched = {lab for lab in counters if scheduled(lab)}
    gone2 = reference_walk(after_first, sched)
    left = [lab for lab in after_first if lab not in gone2]
    gone3 = reference_walk(left, sched - set(gone2))
    return dict(kind=kind, base=base, n=n, first=first, counters=counters, cam=cam, n_select=n_select, sigma=sigma,
                scheduled=sorted(sched), gone2=sorted(gone2), gone3=sorted(gone3), frames=4)


def deletion_pair(plan, make_engine):
    """slam_helpers.Pair of the plan's base features with the EXTRAS added to the oracle and (if made) the engine: points behind
    the left image border of the first pose, on the plane, blank templates."""
    from slam_helpers import Pair
    pr = Pair(plan["base"], plan["frames"], batch=1, cam=plan["cam"], n_select=plan["n_select"], max_features=plan["n"],
              feature_sigma=plan["sigma"], make_engine=make_engine)
    add_extras(pr, EXTRAS, plan["sigma"])
    return pr


def extra_features(pr, count, first=0):
    cam, pose0 = pr.cam, pr.specs[0].poses[0]
    H = cam["height"]
    y = np.stack([point_on_pixel(cam, pose0, 6.0, 0.25 * H + 0.1 * H * (first + j)) for j in range(count)])
    return y, np.tile(pose0, (count, 1)), np.zeros((count, 11, 11), np.uint8)


def add_extras(pr, count, sigma, first=0):
    """`count` known features that no frame of the sequence ever sees (6 px from the left edge), appended to the map of the
    Pair's oracle and engine alike."""
    y, xo, tpl = extra_features(pr, count, first)
    o = pr.oracles[0]
    n0 = o.num_features
    for j in range(count):
        o.add_known_feature(y[j], xo[j], tpl[j])
        if sigma > 0.0:
            o.set_feature_Pyy(n0 + j, np.eye(3) * sigma ** 2)
    if pr.engine is not None:
        assert len(pr.engine.features(0)) == n0
        pr.engine.add_known_features(y[None], xo[None], tpl[None])
        if sigma > 0.0:           # (sl2_set_feature_covariances addresses the first n features of the list: before the first step only)
            pr.engine.set_feature_covariances(np.tile(np.eye(3) * sigma ** 2, (1, n0 + count, 1, 1)))


def oracle_index(o, label):
    """Index in feature_list_ of the feature with this label (the oracle's counter hook takes the index)."""
    for i in range(o.num_features):
        if o.feature(i)["label"] == label:
            return i
    raise KeyError(label)


def oracle_labels(o):
    return [o.feature(i)["label"] for i in range(o.num_features)]


# ------------------------------------------------------------------------------- 4: a partial feature inside a scheduled run
def step(pr, k, enable_mapping=False):
    """One GoOneStep of the Pair's single oracle and, if it has one, of its engine, on frame k."""
    pr.oracles[0].go_one_step(pr.frames[0][k], False, enable_mapping)
    if pr.engine is not None:
        pr.engine.go_one_step(pr.frame_batch(k), False, enable_mapping)


def set_counters(pr, counters):
    """label -> (attempted, successful) on the oracle (which addresses by list index) and the engine (by label)."""
    o = pr.oracles[0]
    for lab, (a, s) in sorted(counters.items()):
        o.set_feature_counters(oracle_index(o, lab), a, s)
        if pr.engine is not None:
            pr.engine.set_feature_counters(0, lab, a, s)


PARTIAL_BASE = 6


def partial_run_pair(mirror, make_engine, fusion=True):
    """The list [0 .. 4, A, P, C] (mirror: [0 .. 4, A, P, C, D]): six known features stepped once, then a feature initialised by
    hand at the image centre - P, partially initialised: label 6, six states - then one (mirror: two) more known features behind
    the left image border.  A = label 5 and C = label 7 (mirror: D = label 8) are scheduled for deletion; returns the Pair, with
    the step that decides still to come (frame 1)."""
    from slam_helpers import Pair
    pr = Pair(PARTIAL_BASE, 4, batch=1, n_select=PARTIAL_BASE, max_features=12, make_engine=make_engine)
    if pr.engine is not None and not fusion:
        pr.engine.set_step_fusion(False)
    step(pr, 0)
    cam = pr.cam
    u, v = cam["width"] // 2, cam["height"] // 2
    pr.oracles[0].initialise_feature(pr.frames[0][0], u, v)
    if pr.engine is not None:
        assert list(pr.engine.initialise_feature(pr.frame_batch(0), [[u, v]])) == [True]
    add_extras(pr, 2 if mirror else 1, 0.0)
    set_counters(pr, {PARTIAL_BASE - 1: GO, (PARTIAL_BASE + 2 if mirror else PARTIAL_BASE + 1): AT_MINIMUM})
    return pr
