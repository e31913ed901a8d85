"""Shared by tests/test_frame_convert_raw_host.py and tests/test_gpu_frame_convert_raw.py: the machine-vision formats (deep grey in
16-bit words, Bayer mosaics), the shapes at which their staging can go wrong, and a NumPy restatement of their definition
(include/scenelib2_amd.h, "raw camera frames") that calls nothing of the library.  The two resize filters are those of
frame_convert_cases.py and frame_convert_area_cases.py, applied to this file's grey plane."""
import numpy as np

import frame_convert_cases as fc
import frame_convert_area_cases as fa

LINEAR, AREA = 0, 1
GRAY10, GRAY12, GRAY16 = 16, 17, 18
BAYER_RGGB8, BAYER_GRBG8, BAYER_GBRG8, BAYER_BGGR8 = 24, 25, 26, 27
DEEP = {GRAY10: 10, GRAY12: 12, GRAY16: 16}
BAYER = {BAYER_RGGB8: "RGGB", BAYER_GRBG8: "GRBG", BAYER_GBRG8: "GBRG", BAYER_BGGR8: "BGGR"}
FORMATS = tuple(DEEP) + tuple(BAYER)
BPP = {f: 2 if f in DEEP else 1 for f in FORMATS}
# every head length class of a 16-byte load for Bayer; the even ones for 16-bit words
OFFSETS = {f: (0, 2, 14) if f in DEEP else (0, 1, 7, 15) for f in FORMATS}
PITCH_PADS = {f: (0, 2, 14) if f in DEEP else (0, 1, 13) for f in FORMATS}

# output size -> source sizes.  Every output size is one converter of the GPU test.  Source widths 2, 3, 15, 16, 17, 31, 33, 47,
# 1001 (sixteen staged rows fill the LDS: a Bayer pass of sixteen grey rows needs eighteen raw rows, two sub-passes) and 4096 (the
# cap); heights 2, 3, 9, 17; the identity, a 2 x, a 3 x and a non-integer reduction, enlargements (LINEAR only); out_h 8 and 9: a
# band's last row takes its Bayer halo from the next band's rows.
SHAPES = {
    (1, 1): [(2, 2), (3, 3), (2, 3), (3, 2), (17, 9)],
    (7, 5): [(7, 5), (14, 10), (21, 15), (15, 9), (16, 17), (31, 17), (2, 2), (4096, 6)],
    (33, 17): [(33, 17), (66, 34), (99, 51), (47, 17), (1001, 17), (15, 9), (3, 2), (4096, 6)],
    (16, 8): [(16, 8), (32, 16), (33, 17), (47, 17), (17, 9)],
    (11, 9): [(11, 9), (33, 27), (1001, 40), (31, 17), (16, 17)],
}


def cases():
    """(out size, source size, format, filter, pitch pad, offset, seed): every format under both filters on every shape the
    filter allows (AREA only reduces); every (format, filter) walks through its (pitch pad, offset) pairs on its own count."""
    n, used = 0, {}
    for out, srcs in SHAPES.items():
        for sw, sh in srcs:
            for fmt in FORMATS:
                for flt in (LINEAR, AREA):
                    if flt == AREA and (sw < out[0] or sh < out[1]):
                        continue
                    k = used.get((fmt, flt), 0)
                    pads, offs = PITCH_PADS[fmt], OFFSETS[fmt]
                    yield out, (sw, sh), fmt, flt, pads[k % len(pads)], offs[(k // len(pads)) % len(offs)], 3000 + n
                    used[(fmt, flt)] = k + 1
                    n += 1


CASES = list(cases())


def source(width, height, fmt, pad=0, offset=0):
    return dict(width=width, height=height, pitch=width * BPP[fmt] + pad, format=fmt, offset=offset)


def source_bytes(s):
    return s["offset"] + (s["height"] - 1) * s["pitch"] + s["width"] * BPP[s["format"]]


def random_raw(s, seed):
    """A raw buffer of exactly the bytes the source reaches, every byte random (the bits above N, the padding and the lead-in too)."""
    return np.random.default_rng(seed).integers(0, 256, source_bytes(s), dtype=np.uint8)


def rows_of(s, raw):
    rb = s["width"] * BPP[s["format"]]
    idx = s["offset"] + np.arange(s["height"])[:, None] * s["pitch"] + np.arange(rb)[None, :]
    return np.asarray(raw)[idx]


def bayer_letters(fmt, width, height):
    """The colour letter of every site: letter (y & 1) * 2 + (x & 1) of the pattern's name."""
    name = np.array(list(BAYER[fmt]))
    y, x = np.arange(height)[:, None], np.arange(width)[None, :]
    return name[(y & 1) * 2 + (x & 1)]


def bayer_quarters(fmt, p):
    """(R4, G4, B4) of every site of the mosaic p [h][w]: the table of the header, indices reflected about the edge pixel."""
    p = np.asarray(p).astype(np.int32)
    h, w = p.shape
    assert h >= 2 and w >= 2
    P = np.pad(p, 1, mode="reflect")
    c = P[1:-1, 1:-1]
    h2 = P[1:-1, :-2] + P[1:-1, 2:]
    v2 = P[:-2, 1:-1] + P[2:, 1:-1]
    cross4 = h2 + v2
    diag4 = P[:-2, :-2] + P[:-2, 2:] + P[2:, :-2] + P[2:, 2:]
    col = bayer_letters(fmt, w, h)
    beside = bayer_letters(fmt, w + 1, h)[:, 1:]          # the letter one column to the right: in a mosaic, also the one to the left
    red, blue = col == "R", col == "B"
    green_r, green_b = (col == "G") & (beside == "R"), (col == "G") & (beside == "B")
    assert (red.astype(int) + blue + green_r + green_b == 1).all()
    R4 = np.select([red, blue, green_r, green_b], [4 * c, diag4, 2 * h2, 2 * v2])
    G4 = np.select([red, blue, green_r, green_b], [cross4, cross4, 4 * c, 4 * c])
    B4 = np.select([red, blue, green_r, green_b], [diag4, 4 * c, 2 * v2, 2 * h2])
    return R4, G4, B4


def grey_plane(s, raw):
    """The grey value of every source pixel, int32 [height][width]."""
    r = rows_of(s, raw).astype(np.int32)
    f = s["format"]
    if f in DEEP:
        n = DEEP[f]
        v = r[:, 0::2] | (r[:, 1::2] << 8)
        return (v & ((1 << n) - 1)) >> (n - 8)
    R4, G4, B4 = bayer_quarters(f, r)
    return (4899 * R4 + 9617 * G4 + 1868 * B4 + 32768) >> 16


def resize(g, out_w, out_h, flt):
    """Either filter's definition on a grey plane: uint8 [out_h][out_w]."""
    g = np.asarray(g).astype(np.int32)
    if flt == AREA:
        return fa.round_mean(fa.accumulate(g, out_w, out_h), g.shape[0] * g.shape[1])
    x0, x1, a0, a1, _ = fc.taps(g.shape[1], out_w)
    y0, y1, b0, b1, _ = fc.taps(g.shape[0], out_h)
    H = g[:, x0] * a0[None, :] + g[:, x1] * a1[None, :]
    out = (((b0[:, None] * (H[y0] >> 4)) >> 16) + ((b1[:, None] * (H[y1] >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def reference(s, raw, out_w, out_h, flt):
    return resize(grey_plane(s, raw), out_w, out_h, flt)


def pack_mosaic(mosaic, fmt, pad=0, offset=0, seed=0):
    """A Bayer raw buffer whose bytes are `mosaic` (uint8 [h][w]), the padding and lead-in random.  Returns (source dict, raw)."""
    h, w = mosaic.shape
    s = source(w, h, fmt, pad, offset)
    raw = random_raw(s, seed)
    raw[s["offset"] + np.arange(h)[:, None] * s["pitch"] + np.arange(w)[None, :]] = mosaic
    return s, raw


def pack_words(words, fmt, pad=0, offset=0, seed=0):
    """A deep grey raw buffer whose 16-bit little-endian words are `words` (uint16 [h][w]).  Returns (source dict, raw)."""
    h, w = words.shape
    s = source(w, h, fmt, pad, offset)
    raw = random_raw(s, seed)
    idx = s["offset"] + np.arange(h)[:, None] * s["pitch"] + 2 * np.arange(w)[None, :]
    raw[idx] = (words & 255).astype(np.uint8)
    raw[idx + 1] = (words >> 8).astype(np.uint8)
    return s, raw


def flat_colour_mosaic(fmt, width, height, rgb):
    """The mosaic a flat colour (R, G, B) leaves on a sensor of this pattern."""
    col = bayer_letters(fmt, width, height)
    return np.select([col == "R", col == "G", col == "B"], [rgb[0], rgb[1], rgb[2]]).astype(np.uint8)
