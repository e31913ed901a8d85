"""The rectified view: a NumPy restatement of the rules of include/scenelib2_amd.h ("the rectified view"), written from the
header's text - it calls nothing of the library - and the cases the host and the GPU tests share.

* segment_mask / reference   - SL2_ITEM_SEGMENT in Python integers (unbounded, // floors); the other kinds are overlay_cases'.
* rectify                    - the undistorted frame in float64 and int64, expression by expression in the header's order.
* zeroed_jac, sigma, conic, scene_segment, scene_list - the 3-D scene in Python floats, operation by operation in the header's
  order, and the list builder over a sequence's public state (engine or oracle).
"""
import numpy as np

import overlay_cases as oc

SEGMENT = 5
SIZES = oc.SIZES
FAR = oc.FAR
SHIPPED_KD1 = 9e-06


def segment(x0, y0, x1, y1, rgb=oc.YELLOW, label=-1):
    it = np.zeros((), oc.ITEM)
    it["kind"], it["label"], it["patch"], it["rgb"] = SEGMENT, label, -1, rgb
    it["a"] = (x0, y0, x1, y1)
    return it


def segment_pixels(a):
    """Every (x, y) the rule covers, unclipped, as a generator bounded by the caller's range of the major coordinate."""
    x0, y0, x1, y1 = (max(-FAR, min(FAR, int(v))) for v in a)
    dx, dy = x1 - x0, y1 - y0
    xmajor = abs(dx) >= abs(dy)
    if not xmajor:
        x0, y0, x1, y1 = y0, x0, y1, x1
    if x1 < x0:
        x0, y0, x1, y1 = x1, y1, x0, y0
    return xmajor, x0, y0, x1, y1


def segment_mask(a, w, h):
    mask = np.zeros((h, w), bool)
    xmajor, m0, n0, m1, n1 = segment_pixels(a)
    D, d = m1 - m0, n1 - n0
    lim_major, lim_minor = (w, h) if xmajor else (h, w)
    for m in range(max(m0, 0), min(m1, lim_major - 1) + 1):
        n = n0 if D == 0 else n0 + (2 * (m - m0) * d + D) // (2 * D)
        if 0 <= n < lim_minor:
            if xmajor:
                mask[n, m] = True
            else:
                mask[m, n] = True
    return mask


def half_ties(a):
    """The major coordinates at which the rule rounds an exact half: where a segment and its reverse may differ."""
    xmajor, m0, n0, m1, n1 = segment_pixels(a)
    D, d = m1 - m0, n1 - n0
    return xmajor, [m for m in range(m0, m1 + 1) if D and (2 * (m - m0) * d + D) % (2 * D) == 0]


def reference(frame, items, patches=None):
    f = np.asarray(frame, np.uint8)
    h, w = f.shape
    out = np.repeat(f[:, :, None], 3, axis=2).copy()
    for it in items:
        if int(it["kind"]) == SEGMENT:
            out[segment_mask(it["a"], w, h)] = it["rgb"]
        else:
            mask, colour = oc.covers(it, w, h, patches)
            out[mask] = colour[mask]
    return out


def rectify(frame, u0, v0, kd1):
    f = np.asarray(frame, np.uint8)
    h, w = f.shape
    u0, v0, kd1 = np.float64(u0), np.float64(v0), np.float64(kd1)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        cx = xs.astype(np.float64) - u0
        cy = ys.astype(np.float64) - v0
        r2 = cx * cx + cy * cy
        fac = np.float64(1.0) + (np.float64(2.0) * kd1) * r2
        ok = fac > 0
        s = np.sqrt(np.where(ok, fac, 1.0))
        sx = cx / s + u0
        sy = cy / s + v0
        ok &= np.isfinite(sx) & np.isfinite(sy) & (np.abs(sx) <= 2.0 ** 20) & (np.abs(sy) <= 2.0 ** 20)
        X = np.floor(np.where(ok, sx, 0.0) * 32.0 + 0.5).astype(np.int64)
        Y = np.floor(np.where(ok, sy, 0.0) * 32.0 + 0.5).astype(np.int64)
    ix, fx, iy, fy = X >> 5, X & 31, Y >> 5, Y & 31

    def tap(x, y):
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        return np.where(inside, f[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64), 0)

    val = ((32 - fx) * (32 - fy) * tap(ix, iy) + fx * (32 - fy) * tap(ix + 1, iy) + (32 - fx) * fy * tap(ix, iy + 1)
           + fx * fy * tap(ix + 1, iy + 1) + 512) >> 10
    return np.where(ok, val, 0).astype(np.uint8)


# ---- the segment cases: (name, (width, height), items, patches)

def segment_cases():
    out = []
    for w, h in SIZES:
        mx, my = w // 2, h // 2
        P = oc.patches_of(5, 121 if w == 70 else 128, seed=w)
        add = lambda name, items, patches=None: out.append(("%s_%dx%d" % (name, w, h), (w, h), list(items), patches))
        octants = [(11, 4), (4, 11), (-4, 11), (-11, 4), (-11, -4), (-4, -11), (4, -11), (11, -4)]
        for k, (dx, dy) in enumerate(octants):
            add("seg_octant_%d" % k, [segment(mx, my, mx + dx, my + dy, oc.RED)])
            add("seg_octant_%d_reversed" % k, [segment(mx + dx, my + dy, mx, my, oc.RED)])
        add("seg_all_octants", [segment(mx, my, mx + dx, my + dy, oc.GREEN if k % 2 else oc.BLUE) for k, (dx, dy) in enumerate(octants)])
        add("seg_horizontal", [segment(3, 5, 40, 5, oc.RED), segment(50, 9, 8, 9, oc.BLUE)])
        add("seg_vertical", [segment(7, 1, 7, h - 2, oc.RED), segment(20, h - 1, 20, 0, oc.BLUE)])
        add("seg_diagonals", [segment(2, 2, 14, 14, oc.RED), segment(30, 13, 18, 1, oc.BLUE), segment(40, 2, 52, 14), segment(40, 14, 52, 2, oc.GREEN)])
        add("seg_single_pixel", [segment(mx, my, mx, my, oc.GREEN), segment(0, 0, 0, 0, oc.RED), segment(w - 1, h - 1, w - 1, h - 1, oc.BLUE),
                                 segment(w, h, w, h), segment(-1, 0, -1, 0)])
        add("seg_half_ties", [segment(4, 4, 12, 8, oc.RED), segment(12, 10, 4, 6, oc.BLUE), segment(30, 1, 32, 9), segment(36, 9, 34, 1, oc.GREEN),
                              segment(44, 12, 50, 9, oc.RED), segment(58, 9, 52, 12, oc.BLUE)])
        add("seg_across_tile_edges", [segment(50, 3, 69, 30, oc.RED), segment(60, 16, 68, 16, oc.BLUE), segment(64, 2, 64, 30, oc.GREEN),
                                      segment(69, 15, 58, 17)])
        add("seg_one_end_off", [segment(mx, my, w + 25, my + 6, oc.RED), segment(-30, -9, mx, my - 3, oc.BLUE), segment(mx, h + 40, mx + 5, 3, oc.GREEN),
                                segment(10, 10, 10, -500)])
        add("seg_both_ends_off", [segment(-20, 5, w + 20, h - 4, oc.RED), segment(mx - 3, -50, mx + 9, h + 50, oc.BLUE), segment(-5, -5, -50, -9),
                                  segment(w + 3, 0, w + 3, h), segment(-40, h + 10, w + 40, h + 12), segment(-9, 20, 20, -9, oc.GREEN),
                                  segment(-32767, -32767, 32767, 32767), segment(32767, -3000, -32767, 3100, oc.GREEN)])
        add("seg_beyond_far", [segment(-2 ** 30, my, 2 ** 30, my, oc.RED), segment(mx, -2 ** 31, mx, 2 ** 31 - 1, oc.BLUE),
                               segment(-FAR - 7, -FAR - 7, FAR + 9, FAR + 9, oc.GREEN), segment(2 ** 31 - 1, 3, -2 ** 31, h - 3),
                               segment(-FAR, 0, FAR, h - 1, oc.RED), segment(FAR + 1, FAR + 1, 2 ** 30, 2 ** 30)])
        ringed = [oc.circle(mx, my, min(my - 2, 8), oc.RED), segment(mx - 14, my - 3, mx + 14, my + 4, oc.GREEN)]
        add("seg_over_ring", ringed)
        add("seg_under_ring", ringed[::-1])
        add("seg_with_patch_and_rect", [segment(0, 0, w - 1, h - 1, oc.RED), oc.patch(mx, my, 2, oc.BLUE), oc.rect(mx - 9, my - 4, mx + 9, my + 4),
                                        segment(0, h - 1, w - 1, 0, oc.BLUE)], P)
        weird = []
        for kind in (0, 4, -1, 2 ** 31 - 1):
            b = segment(2, 2, 30, 9, oc.GREEN).copy()
            b["kind"] = kind
            weird.append(b)
        add("seg_other_kinds_draw_nothing", weird + [segment(1, 1, 4, 1, oc.BLUE)])
        rng = np.random.default_rng(w * 77 + h)
        many = []
        for _ in range(600 if w == 70 else 90):
            rgb = tuple(int(v) for v in rng.integers(0, 256, 3))
            x0, y0 = int(rng.integers(-15, w + 15)), int(rng.integers(-15, h + 15))
            many.append(segment(x0, y0, x0 + int(rng.integers(-40, 41)), y0 + int(rng.integers(-40, 41)), rgb))
            if rng.integers(0, 4) == 0:
                many.append(oc.ellipse(x0, y0, float(rng.uniform(0.6, 9)), float(rng.uniform(0.6, 6)), float(rng.uniform(0, 180)), rgb))
        add("seg_many", many)
    return out


SEGMENT_CASES = segment_cases()


# ---- the remap cases: (name, (width, height), (u0, v0), kd1)

def remap_cases():
    out = []
    for w, h in SIZES:
        centres = dict(inside=(w / 2.0 - 0.5, h / 2.0 + 0.25), border=(0.0, h - 1.0), nondyadic=(162.3, 125.7))
        # f <= 0 where r2 >= -1 / (2 kd1): with the corners at r2 of about (w / 2)^2 + (h / 2)^2 from a centre inside
        corner_r2 = (w / 2.0) ** 2 + (h / 2.0) ** 2
        kds = dict(zero=0.0, shipped=SHIPPED_KD1, strong=2e-4, negative=-6e-5, corners_lost=-1.0 / (2.0 * 0.6 * corner_r2))
        for cn, (u0, v0) in centres.items():
            for kn, kd1 in kds.items():
                out.append(("remap_%s_%s_%dx%d" % (cn, kn, w, h), (w, h), (u0, v0), kd1))
    return out


REMAP_CASES = remap_cases()


def remap_frame(w, h, seed=0):
    """A textured frame without zeros, so that the border (0) shows where it is sampled."""
    rng = np.random.default_rng(300 + seed)
    return rng.integers(1, 256, (h, w), dtype=np.uint8)


# ---- the 3-D scene (include/scenelib2_amd.h, "THE SCENE'S DRAW LIST OF A SEQUENCE"), in Python floats: IEEE doubles, no
# contraction, every expression in the header's order - so that a list built here equals the library's to the bit.

TRAJECTORY, FEATURES, UNCERTAINTIES = 1, 2, 4
NEAR, RAY, GUARD = 0.01, 10.0, 32767.0
RING, RECT = oc.RING, oc.RECT


def scene_item_bound(max_features, partial_slots):
    return 3 * max_features + partial_slots + 999


def _quat_inverse(q):
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    return [q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2] if n2 > 0.0 else [0.0] * 4


def _quat_to_rot(q):
    w, x, y, z = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)]


def _dot(n, f):
    acc = 0.0
    for k in range(n):
        acc += f(k)
    return acc


def zeroed_jac(xp, y):
    """m = RRW (y - r), Jx = dzeroedyi_by_dxp [3][7], Jy = RRW [3][3] (full_feature_model.cpp:67-101)."""
    xp, y = [float(v) for v in xp], [float(v) for v in y]
    d = [y[0] - xp[0], y[1] - xp[1], y[2] - xp[2]]
    q = _quat_inverse(xp[3:7])
    R = _quat_to_rot(q)
    m = [_dot(3, lambda k: R[i * 3 + k] * d[k]) for i in range(3)]
    Jx = [[0.0] * 7 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            Jx[i][j] = R[i * 3 + j] * -1.0
    w, x, yy, z = q
    t = [[2 * w, -2 * z, 2 * yy, 2 * z, 2 * w, -2 * x, -2 * yy, 2 * x, 2 * w],
         [2 * x, 2 * yy, 2 * z, 2 * yy, -2 * x, -2 * w, 2 * z, 2 * w, -2 * x],
         [-2 * yy, 2 * x, 2 * w, 2 * x, 2 * yy, 2 * z, -2 * w, 2 * z, -2 * yy],
         [-2 * z, -2 * w, 2 * x, 2 * w, -2 * z, 2 * yy, 2 * x, 2 * yy, 2 * z]]
    for k in range(4):
        sgn = 1.0 if k == 0 else -1.0
        for i in range(3):
            Jx[i][3 + k] = _dot(3, lambda c: t[k][i * 3 + c] * d[c]) * sgn
    return m, Jx, [R[0:3], R[3:6], R[6:9]]


def sigma(Jx, Jy, Pxx, Pxy, Pyy):
    """Pzeroedyigraphics in the header's summation order; Pxx [7][7], Pxy [7][3], Pyy [3][3]."""
    Pxx, Pxy, Pyy = ([[float(v) for v in row] for row in M] for M in (Pxx, Pxy, Pyy))
    A = [[_dot(7, lambda k: Jx[i][k] * Pxx[k][c]) for c in range(7)] for i in range(3)]
    B = [[_dot(7, lambda k: Jx[i][k] * Pxy[k][c]) for c in range(3)] for i in range(3)]
    Cm = [[_dot(3, lambda k: Jy[i][k] * Pyy[k][c]) for c in range(3)] for i in range(3)]
    T3 = [[_dot(3, lambda c: B[i][c] * Jy[j][c]) for j in range(3)] for i in range(3)]
    S = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            t1 = _dot(7, lambda c: A[i][c] * Jx[j][c])
            t4 = _dot(3, lambda c: Cm[i][c] * Jy[j][c])
            S[i][j] = ((t1 + T3[j][i]) + T3[i][j]) + t4
    return S


def conic(cam, m, S):
    """None where d <= 0 or m[2] <= 0, else ((unrounded centre), (A, B, C, rhs))."""
    fku, fkv, u0, v0 = (float(cam[k]) for k in ("fku", "fkv", "u0", "v0"))
    m = [float(v) for v in m]
    D00, D01, D02 = m[0] * m[0] - 9.0 * S[0][0], m[0] * m[1] - 9.0 * S[0][1], m[0] * m[2] - 9.0 * S[0][2]
    D11, D12, d = m[1] * m[1] - 9.0 * S[1][1], m[1] * m[2] - 9.0 * S[1][2], m[2] * m[2] - 9.0 * S[2][2]
    if not (d > 0.0 and m[2] > 0.0):
        return None
    cn0, cn1 = D02 / d, D12 / d
    En00, En01, En11 = cn0 * cn0 - D00 / d, cn0 * cn1 - D01 / d, cn1 * cn1 - D11 / d
    E00, E01, E11 = (fku * En00) * fku, (fku * En01) * fkv, (fkv * En11) * fkv
    return (u0 - fku * cn0, v0 - fkv * cn1), (E11, -2.0 * E01, E00, E00 * E11 - E01 * E01)


def c_round(v):
    """int(v + 0.5) by C truncation, or None where the item is omitted."""
    if not np.isfinite(v) or not -40000.0 < v < 40000.0:
        return None
    c = int(v + 0.5)
    return c if -32767 <= c <= 32767 else None


def project(cam, X):
    return float(cam["u0"]) - float(cam["fku"]) * X[0] / X[2], float(cam["v0"]) - float(cam["fkv"]) * X[1] / X[2]


def scene_segment(cam, a, b, rounded=None):
    """The four rounded coordinates of the 3-D segment a .. b, or None where it is omitted."""
    a, b = [float(v) for v in a], [float(v) for v in b]
    a_behind, b_behind = not a[2] >= NEAR, not b[2] >= NEAR
    if a_behind and b_behind:
        return None
    if a_behind or b_behind:
        t = (NEAR - a[2]) / (b[2] - a[2])
        c = [a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), NEAR]
        if a_behind:
            a = c
        else:
            b = c
    with np.errstate(all="ignore"):
        p, r = project(cam, a), project(cam, b)
    if not all(np.isfinite(v) for v in p + r):
        return None
    dx, dy = r[0] - p[0], r[1] - p[1]
    t0, t1 = 0.0, 1.0
    for pk, qk in ((-dx, p[0] + GUARD), (dx, GUARD - p[0]), (-dy, p[1] + GUARD), (dy, GUARD - p[1])):
        if pk == 0.0:
            if qk < 0.0:
                return None
            continue
        t = qk / pk
        if pk < 0.0:
            if t > t1:
                return None
            t0 = max(t0, t)
        else:
            if t < t0:
                return None
            t1 = min(t1, t)
    ends = [p[0] + t0 * dx, p[1] + t0 * dy, p[0] + t1 * dx, p[1] + t1 * dy]
    if rounded is not None:
        rounded += ends
    out = [c_round(v) for v in ends]
    return None if None in out else out


def _colour(marked, selected, matched):
    return oc.GREEN if marked else oc.RED if selected and matched else oc.BLUE if selected else oc.YELLOW


def scene_list(view, layers, marked=-1):
    """The scene's draw list of one sequence from its public state.  view: cam (dict), x (total state), P (total covariance),
    feats (feature_list_ order: dicts label, full, selected, success, size), traj [n][3] (oldest first).  Returns (items,
    rounded): rounded = every unrounded coordinate that went through the rounding."""
    cam, x, P = view["cam"], np.asarray(view["x"], np.float64), np.asarray(view["P"], np.float64)
    xp = [float(v) for v in x[:7]]
    xq = [0.0, 0.0, 0.0] + xp[3:7]
    items, rounded = [], []
    if layers & TRAJECTORY:
        cf = [zeroed_jac(xp, t)[0] for t in view["traj"]]
        for a, b in zip(cf[:-1], cf[1:]):
            c = scene_segment(cam, a, b, rounded)
            if c is not None:
                items.append(segment(*c, rgb=oc.YELLOW, label=-1))
    pos = 13
    for f in view["feats"]:
        at, pos = pos, pos + f["size"]
        mark = f["label"] == marked
        if f["full"]:
            rgb = _colour(mark, f["selected"], f["success"])
            m, Jx, Jy = zeroed_jac(xp, x[at:at + 3])
            if (layers & FEATURES) and m[2] >= NEAR:
                p = project(cam, m)
                rounded += list(p)
                c = (c_round(p[0]), c_round(p[1]))
                if None not in c:
                    items.append(oc.rect(c[0] - 1, c[1] - 1, c[0] + 1, c[1] + 1, rgb))
                    items.append(oc.rect(c[0], c[1], c[0], c[1], rgb))
                    items[-1]["label"] = items[-2]["label"] = f["label"]
            if layers & UNCERTAINTIES:
                S = sigma(Jx, Jy, P[0:7, 0:7], P[0:7, at:at + 3], P[at:at + 3, at:at + 3])
                got = conic(cam, m, S)
                if got is not None:
                    rounded += list(got[0])
                    c = (c_round(got[0][0]), c_round(got[0][1]))
                    if None not in c:
                        items.append(oc.ring(c[0], c[1], *got[1], rgb=rgb, label=f["label"]))
        elif layers & FEATURES:
            a = zeroed_jac(xp, x[at:at + 3])[0]
            hh = zeroed_jac(xq, x[at + 3:at + 6])[0]
            c = scene_segment(cam, a, [a[k] + RAY * hh[k] for k in range(3)], rounded)
            if c is not None:
                items.append(segment(*c, rgb=_colour(mark, False, False), label=f["label"]))
    return oc.items_array(items), rounded


def skipped_fields(rounded):
    """How many of the rounded coordinates lie within 1e-6 of a half-integer (where another rounding of the arithmetic could
    give the neighbouring pixel)."""
    v = np.asarray(rounded, np.float64)
    v = v[np.isfinite(v)]
    return int((np.abs(v - np.floor(v) - 0.5) <= 1e-6).sum())


# ---- the scene cases of the stand-alone program: random poses, features and joint covariances; 3-D segments at every edge

SHIPPED = dict(fku=195.0, fkv=195.0, u0=162.0, v0=125.0)


def scene_math_cases(n=60, seed=11):
    """(cam, xp [7], y [3], Pxx [7][7], Pxy [7][3], Pyy [3][3]): the joint covariance positive semi-definite; features in front
    of the camera, near its plane (d <= 0: no ring) and behind it."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        if k % 5 == 0:
            q *= 1.0 + 1e-3 * rng.normal()          # (the model does not normalise: a quaternion slightly off the sphere)
        r = rng.normal(scale=0.3, size=3)
        xp = np.concatenate([r, q])
        R = np.array(_quat_to_rot(_quat_inverse([float(v) for v in q]))).reshape(3, 3)
        depth = (0.6, 2.5, 0.05, 0.011, -0.4)[k % 5]
        m = np.array([rng.uniform(-0.3, 0.3) * abs(depth), rng.uniform(-0.2, 0.2) * abs(depth), depth])
        y = r + R.T @ m          # RRW (y - r) = m for a unit quaternion
        G = rng.normal(size=(10, 10)) * np.concatenate([np.full(3, 0.02), np.full(4, 0.01), np.full(3, (0.01, 0.05, 0.2)[k % 3])])[:, None]
        J = G @ G.T
        cam = dict(SHIPPED) if k % 2 else dict(fku=210.5, fkv=190.25, u0=150.3, v0=131.7)
        out.append((cam, xp, y, J[:7, :7].copy(), J[:7, 7:].copy(), J[7:, 7:].copy()))
    return out


def segment3d_cases():
    """(cam, a [3], b [3]): in front, crossing the near plane either way, behind, touching it, beyond the guard square on every
    side, parallel to its edges, degenerate, not finite."""
    c = dict(SHIPPED)
    big = 400.0          # X / Z of 400 projects 78 000 pixels out: beyond the guard square
    pts = [([0.1, 0.05, 0.6], [-0.2, 0.1, 1.5]), ([0.1, 0.05, 0.6], [0.3, -0.1, -0.5]), ([0.3, -0.1, -0.5], [0.1, 0.05, 0.6]),
           ([0.0, 0.0, -1.0], [0.2, 0.2, -0.02]), ([0.1, 0.1, 0.01], [0.2, 0.0, 0.5]), ([0.1, 0.1, 0.0099999], [0.2, 0.0, 0.5]),
           ([0.1, 0.1, 0.01], [0.2, 0.3, 0.01]), ([0.0, 0.0, 0.5], [0.0, 0.0, 0.5]), ([0.0, 0.0, 0.5], [0.0, 0.0, 5.0]),
           ([big, 0.0, 1.0], [-big, 0.1, 1.0]), ([0.0, big, 1.0], [0.1, -big, 1.0]), ([big, big, 1.0], [2 * big, 2 * big, 1.0]),
           ([-big, 0.2, 1.0], [-2 * big, 0.1, 1.0]), ([0.0, -big, 1.0], [0.0, -3 * big, 1.0]), ([big, 0.0, 1.0], [0.0, big, 1.0]),
           ([big, 0.5, 1.0], [big, -0.5, 1.0]), ([0.5, 0.0, 1.0], [big, 0.0, 1.0]), ([0.0, 0.3, 1.0], [0.0, -big, 1.0]),
           ([0.1, 0.1, 0.2], [0.1, 0.1, -0.2]), ([1e300, 0.0, 1.0], [0.0, 0.0, 1.0]), ([float("nan"), 0.0, 1.0], [0.0, 0.0, 1.0]),
           ([0.0, 0.0, float("inf")], [0.1, 0.0, 1.0]), ([0.0, 0.0, float("nan")], [0.0, 0.0, float("nan")]),
           ([167.5 / 195.0, 0.0, 1.0], [0.0, 124.5 / 195.0, 1.0])]
    rng = np.random.default_rng(3)
    for _ in range(40):
        pts.append((list(rng.normal(scale=(2.0, 2.0, 1.0))), list(rng.normal(scale=(2.0, 2.0, 1.0)))))
    return [(c, a, b) for a, b in pts]
