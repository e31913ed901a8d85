"""Shared by tests/test_frame_remap_host.py and tests/test_gpu_frame_remap.py: the lens remap's case table and NumPy restatements
of its two definitions (include/scenelib2_amd.h, "the lens remap" and "maps from calibrations"), written from the header's text;
they call nothing of the library.  The grey planes are those of frame_convert_cases.py and frame_convert_raw_cases.py."""
import numpy as np

import frame_convert_cases as fc
import frame_convert_raw_cases as rc

BORDER = -2 ** 31
FORMATS = tuple(fc.FORMATS) + tuple(rc.FORMATS)          # all twelve
BPP = {**fc.BPP, **rc.BPP}
OUT_SIZES = [(1, 1), (7, 5), (33, 17), (64, 8), (65, 9)]     # one quad and less, odd widths (scalar map loads), one band, a second band of one row
SRC_SIZES = [(2, 2), (3, 3), (47, 17), (4096, 6)]
# a source whose map entries need the two-word device form (18 + 15 bits), for two formats: the other sizes take the one-word form
WIDE_SIZE, WIDE_FORMATS = (4096, 512), (fc.GRAY8, rc.BAYER_GRBG8)
KINDS = ("identity", "shift", "random", "left_edge", "last_column", "border")
RADIAL1, BROWN, FISHEYE = 0, 1, 2


def pads_offsets(fmt):
    return (fc.PITCH_PADS, fc.OFFSETS) if fmt in fc.FORMATS else (rc.PITCH_PADS[fmt], rc.OFFSETS[fmt])


def source(width, height, fmt, pad=0, offset=0):
    return dict(width=width, height=height, pitch=width * BPP[fmt] + pad, format=fmt, offset=offset)


def source_bytes(s):
    return s["offset"] + (s["height"] - 1) * s["pitch"] + s["width"] * BPP[s["format"]]


def random_raw(s, seed):
    return np.random.default_rng(seed).integers(0, 256, source_bytes(s), dtype=np.uint8)


def grey_plane(s, raw):
    """The grey value of every source pixel, int32 [height][width], any of the twelve formats."""
    return (fc.grey_plane if s["format"] in fc.FORMATS else rc.grey_plane)(s, raw).astype(np.int32)


def make_map(kind, out_w, out_h, W, H, seed):
    """int32 [out_h][out_w][2] of one of KINDS for a W x H source."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:out_h, 0:out_w]
    if kind == "identity":
        X, Y = 32 * x, 32 * y
    elif kind == "shift":               # whole pixels, either sign: part of the output leaves the source
        X, Y = 32 * (x + int(rng.integers(-2, 3))), 32 * (y + int(rng.integers(-2, 3)))
    elif kind == "random":              # from two pixels outside to two pixels beyond the last row and column, a few far away
        X = rng.integers(-64, 32 * (W + 1) + 32, (out_h, out_w))
        Y = rng.integers(-64, 32 * (H + 1) + 32, (out_h, out_w))
        far = rng.random((out_h, out_w)) < 0.05
        X = np.where(far, rng.choice([-2 ** 31 + 1, 2 ** 31 - 1, -2 ** 25, 2 ** 25, 32 * W, -32], (out_h, out_w)), X)
        far = rng.random((out_h, out_w)) < 0.05
        Y = np.where(far, rng.choice([-2 ** 31, 2 ** 31 - 1, -2 ** 25, 2 ** 25, 32 * H, -32], (out_h, out_w)), Y)
    elif kind == "left_edge":           # ix = -1 with fx != 0 (and iy = -1 with fy != 0 in the first row): only the far taps are inside
        X = np.broadcast_to(-32 + rng.integers(1, 32, (out_h, 1)), (out_h, out_w)) + 0 * x
        Y = np.where(y == 0, -32 + int(rng.integers(1, 32)), rng.integers(0, 32 * H, (out_h, out_w)))
    elif kind == "last_column":         # ix = W - 1 with fx = 0, iy = H - 1 with fy = 0: no tap beyond the image is needed
        X = np.full((out_h, out_w), 32 * (W - 1)) + 0 * x
        Y = np.where(x % 2 == 0, 32 * (H - 1), rng.integers(0, 32 * H, (out_h, out_w)))
    else:
        X, Y = np.full((out_h, out_w), BORDER), rng.integers(-2 ** 31, 2 ** 31, (out_h, out_w))
    return np.stack([np.asarray(X, np.int64), np.asarray(Y, np.int64)], axis=-1).astype(np.int32)


def cases():
    """(out size, source size, format, kind, pitch pad, offset, seed): every format on every output and source size under every
    kind of map; a format walks through its (pitch pad, offset) pairs on its own count.  4:2:2 sources have even widths."""
    n, used = 0, {}
    for out in OUT_SIZES:
        for fmt in FORMATS:
            sizes = list(SRC_SIZES) + ([WIDE_SIZE] if fmt in WIDE_FORMATS else [])
            for sw, sh in sizes:
                if not fc.allowed(fmt, sw):
                    sw += 1
                for kind in KINDS:
                    if (sw, sh) == WIDE_SIZE and kind not in ("random", "last_column"):
                        continue
                    k = used.get(fmt, 0)
                    pads, offs = pads_offsets(fmt)
                    yield out, (sw, sh), fmt, kind, pads[k % len(pads)], offs[(k // len(pads)) % len(offs)], 7000 + n
                    used[fmt] = k + 1
                    n += 1


CASES = list(cases())


def case_inputs(case):
    """(source dict, raw, map) of a case."""
    (ow, oh), (sw, sh), fmt, kind, pad, off, seed = case
    s = source(sw, sh, fmt, pad, off)
    return s, random_raw(s, seed), make_map(kind, ow, oh, sw, sh, seed + 1)


def remap_grey(g, xy):
    """The pixel rule on a grey plane g int [H][W] and a map int32 [oh][ow][2]: uint8 [oh][ow]."""
    g = np.asarray(g).astype(np.int64)
    H, W = g.shape
    X, Y = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    border = X == BORDER
    fx, fy = X & 31, Y & 31
    ix, iy = (X - fx) // 32, (Y - fy) // 32

    def tap(tx, ty):
        inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        return np.where(inside, g[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)], 0)

    # (a neighbour whose weight is 0 is not read: its product is 0 either way)
    acc = (32 - fx) * (32 - fy) * tap(ix, iy) + fx * (32 - fy) * tap(ix + 1, iy) + (32 - fx) * fy * tap(ix, iy + 1) + fx * fy * tap(ix + 1, iy + 1)
    out = np.where(border, 0, (acc + 512) >> 10)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def reference(s, raw, xy):
    return remap_grey(grey_plane(s, raw), xy)


def lens(model, width, height, fx, fy, cx, cy, k=()):
    return dict(model=model, width=width, height=height, fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), k=[float(v) for v in k])


def camera(width, height, fku, fkv, u0, v0, kd1=0.0, sd=1):
    return dict(width=width, height=height, fku=float(fku), fkv=float(fkv), u0=float(u0), v0=float(v0), kd1=float(kd1), sd=sd)


def lens_positions(ln, target):
    """Section "maps from calibrations", line by line in FP64: (valid [h][w], 32 us + 0.5, 32 vs + 0.5) before the floor."""
    f64 = np.float64
    k = [f64(v) for v in list(ln["k"]) + [0.0] * (8 - len(ln["k"]))]
    fx, fy, lcx, lcy = f64(ln["fx"]), f64(ln["fy"]), f64(ln["cx"]), f64(ln["cy"])
    y, x = np.mgrid[0:target["height"], 0:target["width"]]
    with np.errstate(all="ignore"):
        cx, cy = x.astype(f64) - f64(target["u0"]), y.astype(f64) - f64(target["v0"])
        f = f64(1.0) - (f64(2.0) * f64(target["kd1"])) * (cx * cx + cy * cy)
        valid = f > 0
        s = np.sqrt(np.where(valid, f, 1.0))
        a, b = (cx / s) / f64(target["fku"]), (cy / s) / f64(target["fkv"])
        if ln["model"] == RADIAL1:
            px, py = fx * a, fy * b
            q = f64(1.0) + (f64(2.0) * k[0]) * (px * px + py * py)
            valid &= q > 0
            s = np.sqrt(np.where(q > 0, q, 1.0))
            us, vs = px / s + lcx, py / s + lcy
        elif ln["model"] == BROWN:
            r2 = a * a + b * b
            r4 = r2 * r2
            r6 = r4 * r2
            num = ((f64(1.0) + k[0] * r2) + k[1] * r4) + k[4] * r6
            den = ((f64(1.0) + k[5] * r2) + k[6] * r4) + k[7] * r6
            valid &= ~(den == 0)
            rad, ab = num / den, a * b
            xd = (a * rad + (f64(2.0) * k[2]) * ab) + k[3] * (r2 + f64(2.0) * (a * a))
            yd = (b * rad + k[2] * (r2 + f64(2.0) * (b * b))) + (f64(2.0) * k[3]) * ab
            us, vs = fx * xd + lcx, fy * yd + lcy
        else:
            r = np.sqrt(a * a + b * b)
            th = np.arctan(r)
            t2 = th * th
            t4 = t2 * t2
            t6 = t4 * t2
            t8 = t4 * t4
            thd = th * ((((f64(1.0) + k[0] * t2) + k[1] * t4) + k[2] * t6) + k[3] * t8)
            sc = thd / r
            us = np.where(r == 0, lcx, fx * (a * sc) + lcx)
            vs = np.where(r == 0, lcy, fy * (b * sc) + lcy)
        lim = f64(1048576.0)
        valid &= (us >= -lim) & (us <= lim) & (vs >= -lim) & (vs <= lim)        # (a NaN or an infinity fails a comparison)
        return valid, us * f64(32.0) + f64(0.5), vs * f64(32.0) + f64(0.5)


def lens_reference(ln, target):
    """int32 [h][w][2]: the map of the definition."""
    valid, tx, ty = lens_positions(ln, target)
    X = np.where(valid, np.floor(np.where(valid, tx, 0.0)), BORDER).astype(np.int64)
    Y = np.where(valid, np.floor(np.where(valid, ty, 0.0)), 0).astype(np.int64)
    return np.stack([X, Y], axis=-1).astype(np.int32)


# The calibrations of the map tests: (lens, target).  The targets are a pinhole and a kd1 > 0 camera whose f reaches 0 inside the
# image (border entries), off-centre, unequal focal lengths; the BROWN lens has all eight coefficients and both tangential terms.
LENS_CASES = {
    "radial1_to_pinhole": (lens(RADIAL1, 640, 480, 410.0, 405.0, 318.5, 243.25, [9e-7]), camera(320, 240, 200.0, 198.0, 161.5, 118.75)),
    "radial1_to_radial": (lens(RADIAL1, 640, 480, 410.0, 405.0, 318.5, 243.25, [9e-7]), camera(97, 53, 60.0, 61.0, 47.3, 25.9, 2e-4)),
    "radial1_negative": (lens(RADIAL1, 64, 48, 40.0, 41.0, 31.0, 23.0, [-4e-4]), camera(33, 17, 9.0, 8.0, 16.0, 8.0)),
    "brown_to_pinhole": (lens(BROWN, 1280, 960, 811.3, 809.9, 642.1, 477.6, [-0.28, 0.09, 1.1e-3, -7e-4, -0.012, 0.02, -0.01, 0.003]),
                         camera(320, 240, 205.0, 205.0, 160.2, 119.1)),
    "brown_to_radial": (lens(BROWN, 1280, 960, 811.3, 809.9, 642.1, 477.6, [-0.28, 0.09, 1.1e-3, -7e-4, -0.012, 0.02, -0.01, 0.003]),
                        camera(161, 120, 100.0, 100.0, 80.0, 60.0, 6e-5)),
    "brown_zero_denominator": (lens(BROWN, 64, 48, 40.0, 40.0, 32.0, 24.0, [0, 0, 0, 0, 0, -1.0, 0, 0]), camera(33, 17, 4.0, 4.0, 16.0, 8.0)),
    "fisheye_to_pinhole": (lens(FISHEYE, 1280, 960, 420.7, 421.3, 639.4, 481.2, [-0.021, 0.0043, -0.0017, 0.0002]),
                           camera(320, 240, 140.0, 140.0, 159.5, 119.5)),
    "fisheye_to_radial": (lens(FISHEYE, 1280, 960, 420.7, 421.3, 639.4, 481.2, [-0.021, 0.0043, -0.0017, 0.0002]),
                          camera(320, 240, 140.0, 140.0, 160.0, 120.0, 9e-6)),       # integer centre: r == 0 at (160, 120)
}
