"""Case table of the frame monitor and a NumPy restatement of its definitions, written from the text of include/scenelib2_amd.h
("the frame monitor"); it calls nothing of the library.  Shared by tests/test_frame_monitor_host.py and
tests/test_gpu_frame_monitor.py."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FLAT, DARK, BRIGHT, BLURRED, REPEATED, SKIPPED = 1, 2, 4, 8, 16, 32
GATE_FIELDS = ("min_range", "dark_bins", "max_dark_pixels", "bright_bins", "max_bright_pixels", "reject_repeated", "min_gradient_energy")


def band_rows():
    """Rows of a frame one workgroup of k_frame_stats covers: the implementation's constant, from the testing header."""
    text = open(os.path.join(ROOT, "include", "scenelib2_amd_testing.h")).read()
    return int(re.search(r"#define SL2_FRAME_MONITOR_BAND_ROWS (\d+)", text).group(1))


BAND = band_rows()
FIXED_SHAPES = [(1, 1), (2, 2), (3, 3), (8, 1), (1, 9), (7, 5), (16, 3), (17, 4), (33, 9), (64, 64), (321, 7), (320, 240)]
# a row band that ends one row before, at and one row after the image's last row: one band and two, narrow, odd and a multiple of 16
BAND_SHAPES = [(w, k * BAND + d) for w in (5, 16, 23) for k in (1, 2) for d in (-1, 0, 1)]
SHAPES = FIXED_SHAPES + BAND_SHAPES          # (width, height)
CONTENTS = ("random", "zeros", "white", "checker", "corners", "band_edges")
STRIDE_PADS = (0, 1, 3, 16)                  # seq_stride = n + pad
OFFSETS = (0, 1, 8)                          # of the base pointer, in bytes


def frame(shape, content, seed=0):
    """uint8 [height][width]"""
    w, h = shape
    if content == "random":
        return np.random.default_rng(1000 * w + h + seed).integers(0, 256, (h, w), dtype=np.uint8)
    if content == "zeros":
        return np.zeros((h, w), np.uint8)
    if content == "white":
        return np.full((h, w), 255, np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    if content == "checker":
        return (((x + y) & 1) * 255).astype(np.uint8)
    f = np.full((h, w), 16 + seed, np.uint8)
    if content == "corners":
        f[0, 0] = f[0, w - 1] = f[h - 1, 0] = f[h - 1, w - 1] = 250
        return f
    assert content == "band_edges"
    for r in range(BAND, h + 1, BAND):          # the last row of a band and the first of the next, at both ends and inside
        for yy in (r - 1, r):
            if yy < h:
                f[yy, 0] = 240; f[yy, w - 1] = 241; f[yy, w // 2] = 242
    f[h - 1, w // 2] = 243
    return f


CASES = [(s, c) for s in SHAPES for c in CONTENTS]


def mix64(z):
    z = np.asarray(z, np.uint64)
    z = z ^ (z >> np.uint64(30)); z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27)); z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def digest(flat):
    n = flat.size
    nw = (n + 7) // 8
    padded = np.zeros(nw * 8, np.uint8)
    padded[:n] = flat
    words = (padded.reshape(nw, 8).astype(np.uint64) << (np.uint64(8) * np.arange(8, dtype=np.uint64))[None, :]).sum(axis=1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        k1 = (np.arange(nw, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        return int(mix64(words ^ k1).sum(dtype=np.uint64))


def reference(f):
    """The record of frame f (uint8 [H][W]) as a dict of Python ints and a list."""
    f = np.asarray(f, np.uint8)
    H, W = f.shape
    g = f.astype(np.int64)
    grad = 0
    if W >= 3 and H >= 3:
        dx = g[1:-1, 2:] - g[1:-1, :-2]
        dy = g[2:, 1:-1] - g[:-2, 1:-1]
        grad = int((dx * dx + dy * dy).sum())
    return dict(sum=int(g.sum()), sum_sq=int((g * g).sum()), gradient_energy=grad, digest=digest(f.reshape(-1)),
                min=int(f.min()), max=int(f.max()), hist=[int(v) for v in np.bincount((f >> 4).reshape(-1), minlength=16)])


def as_dict(rec):
    """A FRAME_STATS_DTYPE scalar as the dict reference() makes."""
    return dict(sum=int(rec["sum"]), sum_sq=int(rec["sum_sq"]), gradient_energy=int(rec["gradient_energy"]), digest=int(rec["digest"]),
                min=int(rec["min"]), max=int(rec["max"]), hist=[int(v) for v in rec["hist"]])


def verdict(rec, gate, have_previous=False, previous_digest=0):
    """The gate's rules on a record dict; gate: a dict of GATE_FIELDS (missing = 0)."""
    g = {n: int(gate.get(n, 0)) for n in GATE_FIELDS}
    v = 0
    if g["min_range"] and rec["max"] - rec["min"] < g["min_range"]:
        v |= FLAT
    if g["dark_bins"] and sum(rec["hist"][:g["dark_bins"]]) > g["max_dark_pixels"]:
        v |= DARK
    if g["bright_bins"] and sum(rec["hist"][16 - g["bright_bins"]:]) > g["max_bright_pixels"]:
        v |= BRIGHT
    if g["min_gradient_energy"] and rec["gradient_energy"] < g["min_gradient_energy"]:
        v |= BLURRED
    if g["reject_repeated"] and have_previous and rec["digest"] == previous_digest:
        v |= REPEATED
    return v


def table_gate(shape):
    """A gate for the GPU table that some contents pass and others trip: flat under 8 levels of range, dark / bright when more than
    half the pixels lie in the two end bins, blurred under a gradient energy of 1000."""
    n = shape[0] * shape[1]
    return dict(min_range=8, dark_bins=2, max_dark_pixels=n // 2, bright_bins=2, max_bright_pixels=n // 2, reject_repeated=1,
                min_gradient_energy=1000)
