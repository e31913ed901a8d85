"""Annotated frames (include/scenelib2_amd.h, "annotated frames"): the reference's raw-image display,
GraphicTool::DrawRawAR, as a draw list per sequence and a rasteriser.

* ITEM_DTYPE / make_items - the 64-byte sl2_overlay_item as a NumPy structured dtype.
* draw_items        - sl2_draw_items_batch: `nimages` frames and lists rasterised on the device in one launch.
* draw_items_host   - sl2_draw_items_host: one image in plain C++ from the same source as the kernel (no GPU needed).
* Engine.overlay_items / Engine.draw_overlays (monoslam.py) - the lists of an engine's sequences, and list + draw in one call.

Nothing here rasterises: the pixel rules live in scenelib2_amd/csrc/sl2_overlay_dev.hpp.
"""
import numpy as np

from . import _lib
from ._lib import (SL2_ITEM_PATCH, SL2_ITEM_RECT, SL2_ITEM_RING, SL2_OVERLAY_ALL, SL2_OVERLAY_DESCRIPTORS,  # noqa: F401
                   SL2_OVERLAY_INITIALISATION, SL2_OVERLAY_SEARCH_REGIONS)

ITEM_DTYPE = _lib.OVERLAY_ITEM_DTYPE
GREEN, RED, BLUE, YELLOW = (0, 255, 0), (255, 0, 0), (0, 0, 255), (255, 255, 0)


def item_bound(max_features, partial_slots):
    """sl2_overlay_item_bound: the longest list of a sequence, 2 max_features + 19 partial_slots + 2."""
    return int(_lib.load().sl2_overlay_item_bound(int(max_features), int(partial_slots)))


def ring(cx, cy, A, B, C, rhs, rgb=YELLOW, label=-1):
    it = np.zeros((), ITEM_DTYPE)
    it["kind"], it["label"], it["patch"] = SL2_ITEM_RING, label, -1
    it["a"][:2] = (cx, cy)
    it["rgb"] = rgb
    it["q"] = (A, B, C, rhs)
    return it


def patch(cx, cy, index, rgb=YELLOW, label=-1):
    it = np.zeros((), ITEM_DTYPE)
    it["kind"], it["label"], it["patch"] = SL2_ITEM_PATCH, label, index
    it["a"][:2] = (cx, cy)
    it["rgb"] = rgb
    return it


def rect(x0, y0, x1, y1, rgb=GREEN, label=-1):
    it = np.zeros((), ITEM_DTYPE)
    it["kind"], it["label"], it["patch"] = SL2_ITEM_RECT, label, -1
    it["a"] = (x0, y0, x1, y1)
    it["rgb"] = rgb
    return it


def make_items(items):
    """A list of items (ring / patch / rect, or records of ITEM_DTYPE) as one contiguous array."""
    if isinstance(items, np.ndarray) and items.dtype == ITEM_DTYPE:
        return np.ascontiguousarray(items).reshape(-1)
    out = np.zeros(len(items), ITEM_DTYPE)
    for k, it in enumerate(items):
        out[k] = it
    return out


def _patches_arg(patches):
    """patches: None, or uint8 [npatches][stride >= 121] (an [n][11][11] array is taken as stride 121)."""
    if patches is None:
        return None, 0, 0, None
    p = np.ascontiguousarray(patches, dtype=np.uint8)
    p = p.reshape(p.shape[0], -1)
    return p.ctypes.data_as(_lib.vp), p.shape[1], p.shape[0], p


def draw_items_host(frame, items, patches=None):
    """One image on the host: frame uint8 [height][width] -> uint8 [height][width][3]."""
    L = _lib.load()
    f = np.ascontiguousarray(frame, dtype=np.uint8)
    h, w = f.shape
    it = make_items(items)
    pp, stride, n, keep = _patches_arg(patches)
    out = np.zeros((h, w, 3), np.uint8)
    _lib.check(L.sl2_draw_items_host(f.ctypes.data_as(_lib.vp), w, h, it.ctypes.data_as(_lib.vp) if it.size else None, it.size, pp, stride, n,
                                     out.ctypes.data_as(_lib.vp)), L)
    return out


def draw_items(frames, lists, patches=None, device=0, stream=None):
    """sl2_draw_items_batch with everything in host memory: frames uint8 [nimages][height][width], lists a list of nimages item
    lists (make_items), patches as for draw_items_host.  Returns uint8 [nimages][height][width][3].  Waits for the device."""
    L = _lib.load()
    f = np.ascontiguousarray(frames, dtype=np.uint8)
    n, h, w = f.shape
    arrs = [make_items(l) for l in lists]
    assert len(arrs) == n
    stride = max([a.size for a in arrs] + [1])
    items = np.zeros((n, stride), ITEM_DTYPE)
    counts = np.zeros(n, np.int32)
    for i, a in enumerate(arrs):
        items[i, :a.size] = a
        counts[i] = a.size
    pp, pstride, npatches, keep = _patches_arg(patches)
    out = np.zeros((n, h, w, 3), np.uint8)
    _lib.check(L.sl2_draw_items_batch(int(device), _lib.vp(stream) if stream else None, f.ctypes.data_as(_lib.vp), 0, n, w, h, w * h,
                                      items.ctypes.data_as(_lib.vp), stride, counts.ctypes.data_as(_lib.vp), 0, pp, pstride, npatches,
                                      out.ctypes.data_as(_lib.vp), 3 * w * h, 0), L)
    return out


def write_ppm(path, rgb):
    """An RGB24 image [height][width][3] as a binary PPM."""
    a = np.ascontiguousarray(rgb, dtype=np.uint8)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (a.shape[1], a.shape[0]))
        f.write(a.tobytes())
