"""Shared by tests/test_frame_convert_area_host.py and tests/test_gpu_frame_convert_area.py: the shapes of the area filter's tests
and a NumPy restatement of SL2_RESIZE_AREA's definition (include/scenelib2_amd.h, "raw camera frames") that calls nothing of
the library: int64 weight matrices, Wy @ g @ Wx.T, then the rounding."""
import functools

import numpy as np

import frame_convert_cases as fc
from frame_convert_cases import source, random_raw, grey_plane, pack_grey  # noqa: F401

LINEAR, AREA = 0, 1

# (source size, output size): single pixels, odd ratios, the identity, the HD cameras, one pixel more than the output per axis
# and two, the width cap (586 taps on x in the last one)
SHAPES = [((1, 1), (1, 1)), ((2, 2), (1, 1)), ((5, 3), (1, 1)), ((31, 17), (7, 5)), ((33, 17), (33, 17)), ((640, 480), (320, 240)),
          ((1280, 960), (320, 240)), ((1920, 1080), (320, 240)), ((1920, 1080), (33, 17)), ((961, 241), (320, 240)),
          ((321, 241), (320, 240)), ((322, 242), (320, 240)), ((4096, 18), (33, 17)), ((4096, 2), (7, 1))]
SMALL_SHAPES = [sd for sd in SHAPES if sd[0][0] * sd[0][1] <= 31 * 17 or sd[0] == (33, 17)]


@functools.lru_cache(maxsize=None)
def weights(S, D):
    """int64 [D][S]: w(d, i) = min((i + 1) D, (d + 1) S) - max(i D, d S) on the taps of d, 0 elsewhere."""
    assert S >= D >= 1
    d = np.arange(D, dtype=np.int64)[:, None]
    i = np.arange(S, dtype=np.int64)[None, :]
    w = np.minimum((i + 1) * D, (d + 1) * S) - np.maximum(i * D, d * S)
    w = np.maximum(w, 0)
    first, last = (d * S) // D, ((d + 1) * S - 1) // D
    assert ((w > 0) == ((i >= first) & (i <= last))).all()                    # the taps are exactly the overlapping pixels
    assert w.max() <= D and (w.sum(axis=1) == S).all() and (w.sum(axis=0) == D).all()
    return w


def accumulate(g, out_w, out_h):
    """acc[dy][dx] = sum_y sum_x wy wx g, int64 (exact: below 2^34 at the caps)."""
    g = np.asarray(g).astype(np.int64)
    wy, wx = weights(g.shape[0], out_h), weights(g.shape[1], out_w)
    if g.size <= 1 << 20:
        return wy @ g @ wx.T
    # NumPy's integer matrix product takes a second per HD source and many on a 17-megapixel one.  The same product in float64 is as exact:
    # every partial sum is an integer of at most 255 Sx Sy < 2^34, far below 2^53, so no addition or product ever rounds.
    assert 255 * g.size < 1 << 53
    acc = wy.astype(np.float64) @ g.astype(np.float64) @ wx.T.astype(np.float64)
    out = acc.astype(np.int64)
    assert (out == acc).all()
    return out


def round_mean(acc, n):
    out = (2 * acc + n) // (2 * n)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def reference(s, raw, out_w, out_h):
    """The definition: uint8 [out_h][out_w]."""
    g = grey_plane(s, raw)
    return round_mean(accumulate(g, out_w, out_h), g.shape[0] * g.shape[1])


def kron_accumulate(g, out_w, out_h):
    """The same sums by brute force: every source pixel cut into Dy x Dx cells, every output the sum of its Sy x Sx cells."""
    g = np.asarray(g).astype(np.int64)
    sy, sx = g.shape
    fine = np.kron(g, np.ones((out_h, out_w), np.int64))
    return fine.reshape(out_h, sy, out_w, sx).sum(axis=(1, 3))


def cases():
    """(source size, output size, format, pitch pad, offset, seed): every format the width allows on every shape; every format
    walks through the nine (pitch pad, offset) pairs on its own count."""
    n, used = 0, dict.fromkeys(fc.FORMATS, 0)
    for (sw, sh), (ow, oh) in SHAPES:
        for fmt in fc.FORMATS:
            if fc.allowed(fmt, sw):
                k = used[fmt]
                yield (sw, sh), (ow, oh), fmt, fc.PITCH_PADS[k % 3], fc.OFFSETS[(k // 3) % 3], 2000 + n
                used[fmt] += 1
                n += 1
    for fmt in fc.FORMATS:          # the 4:2:2 formats meet eight even widths: their ninth pair on the smallest even shape
        while used[fmt] < 9:
            k = used[fmt]
            yield (2, 2), (1, 1), fmt, fc.PITCH_PADS[k % 3], fc.OFFSETS[(k // 3) % 3], 2000 + n
            used[fmt] += 1
            n += 1


def stripes(width, height, pattern):
    """A grey frame whose columns repeat `pattern`."""
    row = np.resize(np.asarray(pattern, np.uint8), width)
    return np.repeat(row[None, :], height, axis=0)
