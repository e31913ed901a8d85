"""Shared by tests/test_frame_convert_host.py and tests/test_gpu_frame_convert.py: the shapes, the packing of a raw buffer, and a
NumPy restatement of the conversion's definition (include/scenelib2_amd.h, "raw camera frames") that calls nothing of the library."""
import numpy as np

GRAY8, RGB24, BGR24, UYVY, YUYV = range(5)
FORMATS = (GRAY8, RGB24, BGR24, UYVY, YUYV)
BPP = {GRAY8: 1, RGB24: 3, BGR24: 3, UYVY: 2, YUYV: 2}
OUT_SIZES = [(320, 240), (33, 17), (7, 5), (1, 1)]
# (961, 3): downscale by three with a remainder; (4096, 2): one band of source rows, at the width cap
SRC_SIZES = [(1, 1), (2, 2), (5, 3), (31, 17), (320, 240), (321, 241), (322, 242), (160, 120), (640, 480), (961, 3), (4096, 2)]
PITCH_PADS = (0, 1, 13)
OFFSETS = (0, 1, 7)


def allowed(fmt, width):
    return not (fmt in (UYVY, YUYV) and width % 2)


def source(width, height, fmt, pad=0, offset=0):
    return dict(width=width, height=height, pitch=width * BPP[fmt] + pad, format=fmt, offset=offset)


def source_bytes(s):
    return s["offset"] + (s["height"] - 1) * s["pitch"] + s["width"] * BPP[s["format"]]


def random_raw(s, seed):
    """A raw buffer of exactly the bytes the source reaches, every byte random (the pitch padding and the lead-in too)."""
    return np.random.default_rng(seed).integers(0, 256, source_bytes(s), dtype=np.uint8)


def rows_of(s, raw):
    """[height][row bytes] view of the source's rows."""
    rb = s["width"] * BPP[s["format"]]
    idx = s["offset"] + np.arange(s["height"])[:, None] * s["pitch"] + np.arange(rb)[None, :]
    return np.asarray(raw)[idx]


def grey_plane(s, raw):
    """The grey value of every source pixel, int32 [height][width]."""
    r = rows_of(s, raw).astype(np.int32)
    f = s["format"]
    if f == GRAY8:
        return r
    if f in (RGB24, BGR24):
        c0, c1, c2 = r[:, 0::3], r[:, 1::3], r[:, 2::3]
        R, B = (c0, c2) if f == RGB24 else (c2, c0)
        return (4899 * R + 9617 * c1 + 1868 * B + 8192) >> 14
    return r[:, 1::2] if f == UYVY else r[:, 0::2]


def taps(S, D):
    """Index, second index, w0, w1 and the float fraction of every output position along an axis."""
    d = np.arange(D, dtype=np.float64)
    scale = np.float64(S) / np.float64(D)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    i = np.floor(f).astype(np.int32)
    f = (f - i.astype(np.float32)).astype(np.float32)
    lo = i < 0
    i[lo] = 0
    f[lo] = 0
    hi = i >= S - 1
    i[hi] = S - 1
    f[hi] = 0
    i1 = np.minimum(i + 1, S - 1)
    w1 = np.rint(f * np.float32(2048.0)).astype(np.int32)
    w0 = np.rint((np.float32(1.0) - f) * np.float32(2048.0)).astype(np.int32)
    return i, i1, w0, w1, f


def reference(s, raw, out_w, out_h):
    """The definition, in 32-bit integers: uint8 [out_h][out_w]."""
    g = grey_plane(s, raw).astype(np.int32)
    x0, x1, a0, a1, _ = taps(s["width"], out_w)
    y0, y1, b0, b1, _ = taps(s["height"], out_h)
    H = g[:, x0] * a0[None, :] + g[:, x1] * a1[None, :]
    out = (((b0[:, None] * (H[y0] >> 4)) >> 16) + ((b1[:, None] * (H[y1] >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def exact_bilinear(s, raw, out_w, out_h):
    """Bilinear interpolation of the grey plane with the same fractions, in float64."""
    g = grey_plane(s, raw).astype(np.float64)
    x0, x1, _, _, fx = taps(s["width"], out_w)
    y0, y1, _, _, fy = taps(s["height"], out_h)
    fx = fx.astype(np.float64)[None, :]
    fy = fy.astype(np.float64)[:, None]
    top = g[y0][:, x0] * (1 - fx) + g[y0][:, x1] * fx
    bot = g[y1][:, x0] * (1 - fx) + g[y1][:, x1] * fx
    return top * (1 - fy) + bot * fy


def pack_grey(grey, fmt, pad=0, offset=0, seed=0):
    """A raw buffer whose grey plane is `grey` (uint8 [h][w]) wherever the format can say so exactly: GRAY8 and the two 4:2:2
    formats carry it as is (chroma random); RGB24 / BGR24 get R = G = B = grey, which the 14-bit coefficients map back to
    grey.  Returns (source dict, raw)."""
    h, w = grey.shape
    s = source(w, h, fmt, pad, offset)
    raw = random_raw(s, seed)
    rb = w * BPP[fmt]
    idx = s["offset"] + np.arange(h)[:, None] * s["pitch"] + np.arange(rb)[None, :]
    if fmt == GRAY8:
        raw[idx] = grey
    elif fmt in (RGB24, BGR24):
        raw[idx] = np.repeat(grey, 3, axis=1)
    else:
        raw[idx[:, (1 if fmt == UYVY else 0)::2]] = grey
    return s, raw
