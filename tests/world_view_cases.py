"""The world view and picking: a NumPy restatement of the rules of include/scenelib2_amd.h ("the world view and picking"),
written from the header's text - it calls nothing of the library - and the cases the host and the GPU tests share.

* world_sigma, glyph_edge, glyph_segments, axes_segments, feature_items - the arithmetic in Python floats (IEEE doubles, no
  contraction), operation by operation in the header's order; the projection, the conic, the 3-D segment rule and the rounding
  are rectified_cases'.
* world_list  - the list builder over a sequence's public state (engine or oracle), with the extents.
* look_at     - the view from eye, target and up, by plain linear algebra (the check of sl2_view_look_at, not a restatement).
* pick / covers_window / pick_cases - the pick rule over a coverage computed by DRAWING the item alone (the caller supplies the
  drawing function), and the lists it is checked on.
"""
import numpy as np

import overlay_cases as oc
import rectified_cases as rc

TRAJECTORY, FEATURES, UNCERTAINTIES, CAMERA, AXES, ALL = 1, 2, 4, 8, 16, 31
GREY, WHITE = (150, 150, 150), (255, 255, 255)
BOX_LO, BOX_HI = (-0.032, -0.034, -0.012), (0.026, 0.020, 0.012)
LENS_HALF, LENS_Z = 0.012, -0.017
VIEW = np.dtype([("r", np.float64, (3,)), ("q", np.float64, (4,)), ("fku", np.float64), ("fkv", np.float64), ("u0", np.float64),
                 ("v0", np.float64)])


def world_item_bound(max_features, partial_slots):
    return 3 * max_features + partial_slots + 999 + 19


def make_view(r, q, cam):
    v = np.zeros((), VIEW)
    v["r"], v["q"] = r, q
    for k in ("fku", "fkv", "u0", "v0"):
        v[k] = cam[k]
    return v


def _cam(view):
    return dict(fku=float(view["fku"]), fkv=float(view["fkv"]), u0=float(view["u0"]), v0=float(view["v0"]))


def _pose(view):
    return [float(v) for v in view["r"]] + [float(v) for v in view["q"]]


def into_view(view, Y):
    """X = RRW (Y - r) of the view: zeroedyi's expressions."""
    return rc.zeroed_jac(_pose(view), Y)[0]


def world_sigma(Jy, Pyy):
    Pyy = [[float(v) for v in row] for row in Pyy]
    Cm = [[rc._dot(3, lambda k: Jy[i][k] * Pyy[k][c]) for c in range(3)] for i in range(3)]
    return [[rc._dot(3, lambda c: Cm[i][c] * Jy[j][c]) for j in range(3)] for i in range(3)]


def world_segment(view, A, B, rounded=None):
    return rc.scene_segment(_cam(view), into_view(view, A), into_view(view, B), rounded)


def glyph_edge(e):
    """The two ends of glyph edge e in the glyph's frame: the header's edge order."""
    if e < 12:
        axis, k = e // 4, e % 4
        bits = {0: (0, k & 1, k >> 1), 1: (k & 1, 0, k >> 1), 2: (k & 1, k >> 1, 0)}[axis]
        a = [BOX_HI[i] if bits[i] else BOX_LO[i] for i in range(3)]
        b = list(a)
        b[axis] = BOX_HI[axis]
        return a, b
    h = LENS_HALF
    corners = [(-h, -h), (h, -h), (h, h), (-h, h)]
    k = e - 12
    return list(corners[k]) + [LENS_Z], list(corners[(k + 1) % 4]) + [LENS_Z]


def glyph_world(xv, g):
    """W = r + R(qWO) g, qWO = (-qy, -qz, qw, qx), no normalisation."""
    xv = [float(v) for v in xv]
    R = rc._quat_to_rot([-xv[5], -xv[6], xv[3], xv[4]])
    return [xv[i] + rc._dot(3, lambda k: R[i * 3 + k] * g[k]) for i in range(3)]


def glyph_segments(view, xv, rounded=None):
    """[(edge, four coordinates)] of the edges that are drawn."""
    out = []
    for e in range(16):
        a, b = glyph_edge(e)
        c = world_segment(view, glyph_world(xv, a), glyph_world(xv, b), rounded)
        if c is not None:
            out.append((e, c))
    return out


def extend(ext, p):
    for k in range(3):
        v = float(p[k])
        if v < ext[2 * k]:
            ext[2 * k] = v
        if v > ext[2 * k + 1]:
            ext[2 * k + 1] = v


def axes_segments(view, ext, rounded=None):
    out = []
    for k in range(3):
        A, B = [0.0] * 3, [0.0] * 3
        A[k], B[k] = ext[2 * k], ext[2 * k + 1]
        c = world_segment(view, A, B, rounded)
        if c is not None:
            out.append((k, c))
    return out


def feature_items(view, y, Pyy, layers, rgb, label, rounded=None):
    """The marker (two RECTs) and the RING of a fully initialised feature."""
    cam = _cam(view)
    items = []
    m, _, Jy = rc.zeroed_jac(_pose(view), y)
    if (layers & FEATURES) and m[2] >= rc.NEAR:
        p = rc.project(cam, m)
        if rounded is not None:
            rounded += list(p)
        c = (rc.c_round(p[0]), rc.c_round(p[1]))
        if None not in c:
            items.append(oc.rect(c[0] - 1, c[1] - 1, c[0] + 1, c[1] + 1, rgb))
            items.append(oc.rect(c[0], c[1], c[0], c[1], rgb))
            items[-1]["label"] = items[-2]["label"] = label
    if layers & UNCERTAINTIES:
        got = rc.conic(cam, m, world_sigma(Jy, Pyy))
        if got is not None:
            if rounded is not None:
                rounded += list(got[0])
            c = (rc.c_round(got[0][0]), rc.c_round(got[0][1]))
            if None not in c:
                items.append(oc.ring(c[0], c[1], *got[1], rgb=rgb, label=label))
    return items


def world_list(state, view, layers, marked=-1):
    """The world's draw list of one sequence from its public state.  state: x (total state), P (total covariance), feats
    (feature_list_ order: dicts label, full, selected, success, size), traj [n][3] (oldest first).  Returns (items, rounded,
    extents): rounded = every unrounded coordinate that went through the rounding."""
    x, P = np.asarray(state["x"], np.float64), np.asarray(state["P"], np.float64)
    xv = [float(v) for v in x[:7]]
    items, rounded = [], []
    if layers & CAMERA:
        items += [rc.segment(*c, rgb=GREY, label=-1) for _, c in glyph_segments(view, xv, rounded)]
    if layers & TRAJECTORY:
        traj = [list(t) for t in state["traj"]]
        for a, b in zip(traj[:-1], traj[1:]):
            c = world_segment(view, a, b, rounded)
            if c is not None:
                items.append(rc.segment(*c, rgb=oc.YELLOW, label=-1))
    ext = [0.0] * 6
    extend(ext, xv)
    pos = 13
    for f in state["feats"]:
        at, pos = pos, pos + f["size"]
        mark = f["label"] == marked
        if f["full"]:
            if layers & FEATURES:
                extend(ext, x[at:at + 3])
            items += feature_items(view, x[at:at + 3], P[at:at + 3, at:at + 3], layers, rc._colour(mark, f["selected"], f["success"]),
                                   f["label"], rounded)
        elif layers & FEATURES:
            a = [float(v) for v in x[at:at + 3]]
            b = [a[k] + rc.RAY * float(x[at + 3 + k]) for k in range(3)]
            c = world_segment(view, a, b, rounded)
            if c is not None:
                items.append(rc.segment(*c, rgb=rc._colour(mark, False, False), label=f["label"]))
    if layers & AXES:
        items += [rc.segment(*c, rgb=WHITE, label=-1) for _, c in axes_segments(view, ext, rounded)]
    return oc.items_array(items), rounded, np.array(ext)


# ---- the views

SHIPPED = dict(rc.SHIPPED)
REFERENCE_EYE, REFERENCE_TARGET, REFERENCE_UP = (0.0, 0.18, -1.4), (0.0, 0.13, 0.0), (0.0, 1.0, 0.0)


def look_at(eye, target, up, cam):
    """The view by linear algebra: the rows of RRW are x = up x z normalised, y = z x x, z = (target - eye) normalised; the
    quaternion of RWR = RRW^T from the square roots of its diagonal sums (not the library's branches)."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], axis=1)          # RWR: columns x, y, z
    q = 0.5 * np.sqrt(np.maximum(0.0, [1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2],
                                       1 - R[0, 0] - R[1, 1] + R[2, 2]]))
    q[1:] = np.copysign(q[1:], [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])          # (views with q[0] > 0 only)
    q /= np.linalg.norm(q)
    return make_view(eye, q, cam)


def fixed_views(cam=None):
    """name -> view, the fixed views of the tests: the reference example's; one from the side and above; one INSIDE the map - the
    test scenes' features lie in the plane z = 0, their cameras near z = -0.6 - looking sideways along it (features behind it, rays across
    its near plane); one turned away from everything."""
    cam = dict(SHIPPED) if cam is None else cam
    return dict(reference=look_at(REFERENCE_EYE, REFERENCE_TARGET, REFERENCE_UP, cam),
                side=look_at((1.3, 0.7, -0.45), (0.02, 0.05, 0.35), (0.0, 1.0, 0.0), cam),
                inside=look_at((0.003, 0.081, -0.052), (0.6, 0.1, -0.3), (0.1, 1.0, 0.0), dict(cam, fku=171.3, fkv=168.9)),
                away=look_at((0.0, 0.0, -3.0), (0.0, 0.0, -9.0), (0.0, 1.0, 0.0), cam))


# ---- the cases of the stand-alone program: (view, xv [7], y [3], Pyy [3][3])

def math_cases(n=48, seed=23):
    """Views and features at every depth: in front, ellipsoids that straddle the view plane (no ring) and ones wholly behind it;
    a view quaternion slightly off the sphere now and then (nothing normalises it)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        if k % 6 == 0:
            q *= 1.0 + 1e-3 * rng.normal()
        r = rng.normal(scale=0.5, size=3)
        cam = dict(SHIPPED) if k % 2 else dict(fku=210.5, fkv=190.25, u0=150.3, v0=131.7)
        view = make_view(r, q, cam)
        R = np.array(rc._quat_to_rot(rc._quat_inverse([float(v) for v in q]))).reshape(3, 3)
        depth = (0.6, 2.5, 0.05, 0.011, -0.4, -0.05)[k % 6]
        m = np.array([rng.uniform(-0.3, 0.3) * abs(depth), rng.uniform(-0.2, 0.2) * abs(depth), depth])
        y = r + R.T @ m
        G = rng.normal(size=(3, 3)) * (0.01, 0.05, 0.2)[k % 3]
        xq = rng.normal(size=4)
        xv = np.concatenate([y + rng.normal(scale=0.2, size=3), xq / np.linalg.norm(xq)])          # a camera near the feature: its glyph
        out.append((view, xv, y, G @ G.T))
    return out


# ---- picking

def window(w, h, x, y):
    if not (0 <= x < w and 0 <= y < h):
        return None
    return max(x - 3, 0), max(y - 3, 0), min(x + 3, w - 1), min(y + 3, h - 1)


def coverage(draw, it, w, h, patches=None):
    """The pixels the item covers, found by DRAWING it alone: a pixel is covered iff it comes out the same over an all-0 and an
    all-255 frame.  draw(frame, items, patches) -> [h][w][3].  (A PATCH covers its 13 x 13 square by this test too: the template
    and the frame round it are both independent of the frame.)"""
    one = oc.items_array([it])
    lo, hi = draw(np.zeros((h, w), np.uint8), one, patches), draw(np.full((h, w), 255, np.uint8), one, patches)
    return (lo == hi).all(axis=2)


def pick(draw, items, w, h, x, y, patches=None):
    """(label, index) by the header's rule, over coverage()."""
    win = window(w, h, x, y)
    if win is None:
        return -1, -1
    x0, y0, x1, y1 = win
    for k in range(len(items) - 1, -1, -1):
        if int(items[k]["label"]) < 0:
            continue
        if coverage(draw, items[k], w, h, patches)[y0:y1 + 1, x0:x1 + 1].any():
            return int(items[k]["label"]), k
    return -1, -1


def _lab(it, label):
    it = it.copy()
    it["label"] = label
    return it


def pick_cases():
    """(name, (w, h), items, npatches, [(x, y) clicks]).  needs_device_list: a host-resident batch refuses the list (unknown
    kind, patch index outside the array), as sl2_draw_items_batch does."""
    w, h = 70, 37
    P = 5
    out = []
    add = lambda name, items, clicks, npatches=0, refused=False: out.append(dict(name=name, size=(w, h), items=oc.items_array(items), npatches=npatches,
                                                                                 clicks=clicks, refused_on_host=refused))
    two = [_lab(oc.rect(10, 10, 30, 25), 4), _lab(oc.rect(20, 5, 40, 20), 9)]
    add("later_of_two_wins", two, [(20, 10), (30, 20), (10, 17), (40, 12), (25, 15), (0, 0), (33, 25), (34, 25)])
    add("later_of_two_wins_reversed", two[::-1], [(20, 10), (30, 20), (25, 15)])
    add("unlabelled_on_top_does_not_hide", [_lab(oc.rect(10, 10, 30, 25), 4), oc.rect(9, 9, 31, 26), rc.segment(0, 10, 69, 10), _lab(oc.circle(20, 17, 9), -1)],
        [(10, 10), (20, 10), (31, 26), (36, 10)])
    big = _lab(oc.circle(35, 18, 14), 7)
    add("inside_a_large_ring", [big], [(35, 18), (35, 8), (35, 7), (35, 4), (45, 18), (46, 18), (49, 18), (52, 18), (53, 18), (25, 9)])
    seg = rc.segment(4, 4, 12, 8, oc.RED, label=2)          # half ties at x = 5, 7, 9, 11
    add("segment_ties", [seg], [(x, y) for x in (1, 5, 8, 9, 15, 16) for y in (0, 1, 2, 5, 9, 11, 12)])
    add("segment_ties_reversed", [rc.segment(12, 8, 4, 4, oc.RED, label=2)], [(x, y) for x in (1, 5, 8, 9, 15, 16) for y in (0, 1, 2, 5, 9, 11, 12)])
    add("steep_segment", [rc.segment(30, 36, 33, 2, oc.BLUE, label=11)], [(27, 30), (26, 30), (34, 30), (35, 30), (36, 2), (37, 2), (33, 0)])
    edge = [_lab(oc.rect(0, 0, 2, 2), 1), _lab(oc.rect(67, 34, 69, 36), 2), _lab(oc.rect(-9, 14, -4, 20), 3), _lab(oc.rect(70, 0, 75, 5), 5)]
    add("window_partly_off", edge, [(0, 0), (5, 5), (6, 6), (69, 36), (64, 31), (63, 31), (0, 17), (69, 3), (3, 36), (69, 0)])
    add("click_off_the_image", edge, [(-1, 0), (0, -1), (70, 5), (5, 37), (-3, -3), (72, 2), (-2 ** 31, 2 ** 31 - 1), (2 ** 31 - 1, -2 ** 31)])
    bad = [_lab(oc.ring(20, 18, 1.0, 0.0, 1.0, -4.0), 1), _lab(oc.ring(20, 18, 1.0, 3.0, 1.0, 25.0), 2), _lab(oc.ring(20, 18, float("nan"), 0.0, 1.0, 25.0), 3),
           _lab(oc.ring(20, 18, 0.0, 0.0, 1.0, 25.0), 4), _lab(oc.rect(25, 20, 15, 10), 5), _lab(oc.ring(2 ** 21, 18, 1.0, 0.0, 1.0, 25.0), 6)]
    add("items_that_draw_nothing", bad, [(20, 18), (25, 18), (20, 13)])
    add("items_that_draw_nothing_over_one_that_does", [_lab(oc.circle(20, 18, 5), 8)] + bad, [(20, 18), (25, 18), (20, 13), (29, 18)])
    kinds = []
    for kind in (0, 4, 6, -1):
        b = _lab(oc.rect(5, 5, 30, 30), 3)
        b["kind"] = kind
        kinds.append(b)
    add("unknown_kinds", [_lab(oc.rect(5, 5, 30, 30), 12)] + kinds, [(5, 5), (20, 20)], refused=True)
    patches = [oc.patch(20, 15, 2, label=6), oc.patch(40, 15, P, label=7), oc.patch(55, 15, -1, label=8), oc.patch(30, 28, P - 1, label=9)]
    add("patches_and_indices_outside", patches, [(20, 15), (29, 15), (30, 15), (40, 15), (55, 15), (30, 28), (30, 18), (30, 19), (23, 24), (24, 25)],
        npatches=P, refused=True)
    add("patch_square_is_covered_whole", [oc.patch(20, 15, 2, label=6)], [(20, 15), (29, 24), (30, 25), (11, 6), (10, 5), (23, 12)], npatches=P)
    add("no_patches_at_all", [oc.patch(20, 15, 0, label=6), _lab(oc.rect(18, 13, 22, 17), 2)], [(20, 15)], npatches=0, refused=True)
    rng = np.random.default_rng(5)
    for count in (0, 1, 63, 64, 65, 130):
        items = []
        for k in range(count):
            x0, y0 = int(rng.integers(-5, w)), int(rng.integers(-5, h))
            kind = k % 3
            label = -1 if k % 7 == 3 else k % 50
            if kind == 0:
                it = _lab(oc.rect(x0, y0, x0 + int(rng.integers(0, 9)), y0 + int(rng.integers(0, 7))), label)
            elif kind == 1:
                it = rc.segment(x0, y0, x0 + int(rng.integers(-12, 13)), y0 + int(rng.integers(-12, 13)), oc.RED, label=label)
            else:
                it = _lab(oc.ellipse(x0, y0, float(rng.uniform(1, 6)), float(rng.uniform(1, 4)), float(rng.uniform(0, 180))), label)
            items.append(it)
        clicks = [(int(rng.integers(0, w)), int(rng.integers(0, h))) for _ in range(6)]
        if count >= 64:          # the last item, and the one that starts the second round of lanes, under a click of their own
            clicks += [(max(0, min(w - 1, int(items[-1]["a"][0]))), max(0, min(h - 1, int(items[-1]["a"][1])))),
                       (max(0, min(w - 1, int(items[63]["a"][0]))), max(0, min(h - 1, int(items[63]["a"][1]))))]
        add("count_%d" % count, items, clicks)
    return out


PICK_CASES = pick_cases()


# ---- a map of two rounds of lanes: 70 known features (64 + 6) with random positive definite Pyy, never stepped

def large_map(n=70, seed=19):
    """What the GPU test puts into an engine (xv, Pxx, y, Pyy) and the public state that engine then shows (x, P, feats, traj)."""
    rng = np.random.default_rng(seed)
    xv = np.zeros(13)
    xv[0:3] = (0.021, 0.013, -0.11)
    xv[3] = 1.0
    Pxx = 1e-4 * np.eye(13)
    y = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.4, 0.4, n), rng.uniform(0.3, 1.6, n)], axis=1)
    G = rng.normal(size=(n, 3, 3)) * rng.uniform(0.004, 0.03, n)[:, None, None]
    Pyy = G @ np.transpose(G, (0, 2, 1)) + 1e-8 * np.eye(3)
    x = np.concatenate([xv, y.reshape(-1)])
    P = np.zeros((x.size, x.size))
    P[:13, :13] = Pxx
    for k in range(n):
        P[13 + 3 * k:16 + 3 * k, 13 + 3 * k:16 + 3 * k] = Pyy[k]
    feats = [dict(label=k, full=True, selected=False, success=False, size=3) for k in range(n)]
    return dict(xv=xv, Pxx=Pxx, y=y, Pyy=Pyy, x=x, P=P, feats=feats, traj=np.zeros((0, 3)))
