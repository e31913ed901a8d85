"""Annotated frames: a NumPy restatement of the pixel rules of include/scenelib2_amd.h ("annotated frames", THE PIXEL RULES),
written from the header's text - it calls nothing of the library - and the list of raster cases the host and the GPU tests share.

reference(frame, items, patches) paints item after item over the replicated grey frame: the LAST item that covers a pixel wins.
"""
import itertools

import numpy as np

ITEM = np.dtype([("kind", np.int32), ("label", np.int32), ("a", np.int32, (4,)), ("patch", np.int32),
                 ("rgb", np.uint8, (3,)), ("pad", np.uint8), ("q", np.float64, (4,))])
RING, PATCH, RECT = 1, 2, 3
GREEN, RED, BLUE, YELLOW = (0, 255, 0), (255, 0, 0), (0, 0, 255), (255, 255, 0)
SIZES = ((70, 37), (64, 16))      # row bytes 210 (no multiple of 4) with remainders on both tile axes; exactly one 64 x 16 tile
FAR = 1 << 20                      # beyond: a ring or patch centre draws nothing, a rectangle's corner counts as this


def ring(cx, cy, A, B, C, rhs, rgb=YELLOW, label=0):
    it = np.zeros((), ITEM)
    it["kind"], it["label"], it["patch"], it["rgb"] = RING, label, -1, rgb
    it["a"][:2] = (cx, cy)
    it["q"] = (A, B, C, rhs)
    return it


def circle(cx, cy, r, rgb=YELLOW):
    return ring(cx, cy, 1.0, 0.0, 1.0, float(r) * float(r), rgb)


def ellipse(cx, cy, a, b, deg, rgb=YELLOW, scale=1.0):
    """Semi-axes a, b, the first turned by deg degrees: x^T R diag(1/a^2, 1/b^2) R^T x < 1, times `scale`."""
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    A = c * c / (a * a) + s * s / (b * b)
    B = 2.0 * c * s * (1.0 / (a * a) - 1.0 / (b * b))
    C = s * s / (a * a) + c * c / (b * b)
    return ring(cx, cy, A * scale, B * scale, C * scale, scale, rgb)


def patch(cx, cy, index, rgb=RED, label=0):
    it = np.zeros((), ITEM)
    it["kind"], it["label"], it["patch"], it["rgb"] = PATCH, label, index, rgb
    it["a"][:2] = (cx, cy)
    return it


def rect(x0, y0, x1, y1, rgb=GREEN):
    it = np.zeros((), ITEM)
    it["kind"], it["label"], it["patch"], it["rgb"] = RECT, -1, -1, rgb
    it["a"] = (x0, y0, x1, y1)
    return it


def items_array(items):
    out = np.zeros(len(items), ITEM)
    for k, it in enumerate(items):
        out[k] = it
    return out


# ---- the rules

def _inside(A, B, C, rhs, du, dv):
    with np.errstate(all="ignore"):
        return ((A * du) * du + (B * du) * dv) + (C * dv) * dv < rhs


def ring_valid(q):
    A, B, C, rhs = (np.float64(v) for v in q)
    if not np.isfinite([A, B, C, rhs]).all():
        return False
    with np.errstate(all="ignore"):
        return bool(A > 0 and C > 0 and (np.float64(4.0) * A) * C - B * B > 0 and rhs > 0)


def covers(it, w, h, patches):
    """(mask [h][w] of the pixels the item covers, colour [h][w][3] there)."""
    mask = np.zeros((h, w), bool)
    colour = np.zeros((h, w, 3), np.uint8)
    colour[:] = it["rgb"]
    kind = int(it["kind"])
    a = [int(v) for v in it["a"]]
    ys, xs = np.mgrid[0:h, 0:w]
    if kind == RING:
        if not ring_valid(it["q"]) or abs(a[0]) > FAR or abs(a[1]) > FAR:
            return mask, colour
        A, B, C, rhs = (np.float64(v) for v in it["q"])
        du, dv = (xs - a[0]).astype(np.float64), (ys - a[1]).astype(np.float64)
        ins = lambda ddu, ddv: _inside(A, B, C, rhs, du + ddu, dv + ddv)
        mask = ins(0, 0) & ~(ins(-1, 0) & ins(1, 0) & ins(0, -1) & ins(0, 1))
    elif kind == PATCH:
        npatches = 0 if patches is None else len(patches)
        if not 0 <= int(it["patch"]) < npatches or abs(a[0]) > FAR or abs(a[1]) > FAR:
            return mask, colour
        p = np.asarray(patches[int(it["patch"])]).reshape(-1)[:121]
        du, dv = xs - a[0], ys - a[1]
        inner = (np.abs(du) <= 5) & (np.abs(dv) <= 5)
        frame = np.maximum(np.abs(du), np.abs(dv)) == 6
        g = p[np.clip((dv + 5) * 11 + du + 5, 0, 120)]
        colour[inner] = np.repeat(g[inner][:, None], 3, axis=1)
        mask = inner | frame
    elif kind == RECT:
        x0, y0, x1, y1 = (max(-FAR, min(FAR, v)) for v in a)
        if x0 > x1 or y0 > y1:
            return mask, colour
        box = (xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1)
        mask = box & ((xs == x0) | (xs == x1) | (ys == y0) | (ys == y1))
    return mask, colour


def reference(frame, items, patches=None):
    f = np.asarray(frame, np.uint8)
    h, w = f.shape
    out = np.repeat(f[:, :, None], 3, axis=2).copy()
    for it in items:
        mask, colour = covers(it, w, h, patches)
        out[mask] = colour[mask]
    return out


# ---- the particle counter (graphictool.cpp:716-733), as the reference runs it and as the header states it

def particles_drawn_reference(n):
    step, counter, drawn = max(n // 10, 1), 1, []
    for k in range(n):
        if counter != step:
            counter += 1
        else:
            counter = 1
            drawn.append(k)
    return drawn


def particles_drawn(n):
    step = max(n // 10, 1)
    return [k for k in range(n) if (k + 1) % step == 0]


# ---- the cases: (name, (width, height), items, patches)

def frame_of(w, h, seed=0):
    rng = np.random.default_rng(100 + seed)
    return rng.integers(0, 256, (h, w), dtype=np.uint8)


def patches_of(n, stride=121, seed=0):
    rng = np.random.default_rng(200 + seed)
    return rng.integers(0, 256, (n, stride), dtype=np.uint8)


def _random_items(rng, n, w, h, npatches):
    out = []
    for _ in range(n):
        k = int(rng.integers(0, 3))
        cx, cy = int(rng.integers(-10, w + 10)), int(rng.integers(-10, h + 10))
        rgb = tuple(int(v) for v in rng.integers(0, 256, 3))
        if k == 0:
            out.append(ellipse(cx, cy, float(rng.uniform(0.6, 14)), float(rng.uniform(0.6, 9)), float(rng.uniform(0, 180)), rgb))
        elif k == 1:
            out.append(patch(cx, cy, int(rng.integers(0, npatches)), rgb))
        else:
            out.append(rect(cx, cy, cx + int(rng.integers(-2, 25)), cy + int(rng.integers(-2, 12)), rgb))
    return out


def cases():
    out = []
    nan, inf = float("nan"), float("inf")
    for w, h in SIZES:
        mx, my = w // 2, h // 2
        P = patches_of(5, 121 if w == 70 else 128, seed=w)
        add = lambda name, items, patches=None: out.append(("%s_%dx%d" % (name, w, h), (w, h), list(items), patches))
        add("empty", [])
        add("ring_interior", [circle(mx - 5, my, min(my - 2, 8), RED)])
        for name, (cx, cy) in dict(left=(2, my), right=(w - 3, my), top=(mx, 1), bottom=(mx, h - 2)).items():
            add("ring_clipped_" + name, [circle(cx, cy, 6, BLUE)])
        add("ring_centre_off_image", [circle(-5, -4, 12), circle(w + 9, h + 3, 14, RED), circle(mx, -20, 26, GREEN)])
        add("ring_larger_than_image", [circle(mx, my, 0.97 * float(np.hypot(mx, my)), RED), circle(mx, my, 200.0)])
        add("ring_one_pixel", [ring(mx, my, 1.0, 0.0, 1.0, 0.5, GREEN), ring(0, 0, 1.0, 0.0, 1.0, 1.0, RED), ring(w - 1, h - 1, 2.0, 0.0, 3.0, 1.5, BLUE)])
        for deg in (30, 77, 135, 0, 90):
            add("ring_eccentric_%d" % deg, [ellipse(mx, my, 25.0, 0.5, deg, RED), ellipse(mx + 3, my - 2, 500.0, 10.0, deg, BLUE, scale=4e6)])
        add("ring_nearly_degenerate", [ring(mx, my, 1.0, -1.9999999, 1.0, 4.0, RED), ring(mx, my, 1.0, 2.0 - 1e-15, 1.0, 2.0, BLUE),
                                       ring(mx, my, 1e-12, 0.0, 1e-12, 1.0, GREEN), ring(mx, my, 1e300, 0.0, 1e300, 1e299, YELLOW),
                                       ring(mx, my, 1e-300, 0.0, 1e-300, 1e-298, RED)])
        bad = [ring(mx, my, 1.0, 0.0, 1.0, 0.0), ring(mx, my, 1.0, 0.0, 1.0, -1.0), ring(mx, my, 0.0, 0.0, 1.0, 9.0),
               ring(mx, my, -1.0, 0.0, 1.0, 9.0), ring(mx, my, 1.0, 0.0, 0.0, 9.0), ring(mx, my, 1.0, 0.0, -2.0, 9.0),
               ring(mx, my, 1.0, 2.0, 1.0, 9.0), ring(mx, my, 1.0, -3.0, 1.0, 9.0)]
        for k in range(4):
            for v in (nan, inf, -inf):
                q = [1.0, 0.0, 1.0, 9.0]
                q[k] = v
                bad.append(ring(mx, my, *q))
        bad += [ring(FAR + 1, my, 1.0, 0.0, 1.0, 4e12), ring(mx, -FAR - 1, 1.0, 0.0, 1.0, 4e12), ring(2 ** 31 - 1, -2 ** 31, 1.0, 0.0, 1.0, 1e30)]
        add("ring_invalid_forms", bad)
        add("ring_far_centres", [ring(32767, my, 1.0, 0.0, 1.0, (32767.0 - mx) ** 2, RED), ring(mx, -32767, 1.0, 0.0, 1.0, (32767.0 + my) ** 2, BLUE),
                                 ring(FAR, my, 1.0, 0.0, 1.0, (float(FAR) - 3.0) ** 2, GREEN)])
        add("ring_across_tile_edges", [circle(64, 16, 6, RED), circle(63, 15, 3, BLUE), ellipse(64, 16, 20.0, 2.0, 20, GREEN)])
        add("patch_corners", [patch(0, 0, 0), patch(w - 1, h - 1, 1, BLUE), patch(w - 1, 0, 2, GREEN), patch(0, h - 1, 3, YELLOW)], P)
        add("patch_half_off", [patch(-3, my, 0), patch(w + 2, my - 3, 1, BLUE), patch(mx, -6, 2, GREEN), patch(mx + 14, h + 5, 3, YELLOW),
                               patch(-6, -6, 4, RED), patch(-7, -7, 4, RED), patch(mx, h + 6, 4, BLUE)], P)
        add("patch_interior", [patch(mx, my, 4, GREEN), patch(mx + 9, my + 2, 0, RED)], P)
        add("rect_forms", [rect(9, 7, 3, 12, RED), rect(3, 12, 9, 7, RED), rect(5, 5, 5, 5, BLUE), rect(0, 0, w - 1, h - 1, GREEN),
                           rect(-10, -10, w + 10, h + 10, RED), rect(-5, 3, 20, h + 20, YELLOW), rect(12, 2, 12, 9, RED), rect(14, 4, 30, 4, BLUE),
                           rect(-2 ** 30, 6, 2 ** 30, 8, BLUE), rect(40, -2 ** 31, 44, 2 ** 31 - 1, RED), rect(2 ** 30, 0, -2 ** 30, 5, RED)])
        trio = [circle(mx, my, 6, RED), patch(mx + 3, my + 1, 2, BLUE), rect(mx - 4, my - 5, mx + 8, my + 3, GREEN)]
        for n, order in enumerate(itertools.permutations(range(3))):
            add("painter_order_%d" % n, [trio[k] for k in order], P)
        weird = []
        for kind in (0, 4, -1, 2 ** 31 - 1):
            for it in (circle(mx, my, 5, RED), patch(mx, my, 1, BLUE), rect(2, 2, 9, 9, GREEN)):
                b = it.copy()
                b["kind"] = kind
                weird.append(b)
        add("bad_kind", weird + [rect(1, 1, 4, 4, BLUE)], P)
        add("bad_patch_index", [patch(mx, my, -1), patch(mx, my, 5), patch(mx, my, 2 ** 31 - 1), patch(mx, my, -2 ** 31), patch(mx + 20, my, 4, GREEN)], P)
        add("patch_without_array", [patch(mx, my, 0), circle(mx, my, 4, RED)], None)
        rng = np.random.default_rng(w * 1000 + h)
        add("many_items", _random_items(rng, 300 if w == 70 else 70, w, h, 5), P)
        add("more_items_than_three_rounds", _random_items(rng, 700, w, h, 5), P) if w == 70 else None
    return out


CASES = cases()
