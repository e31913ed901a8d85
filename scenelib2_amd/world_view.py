"""The world view and picking (include/scenelib2_amd.h, "the world view and picking"): the reference's
main pane, GraphicTool::Draw3dScene - the map, the trajectory and the camera from a free virtual camera - and
GraphicTool::Picker, which feature lies under a click.

* look_at / view     - an sl2_view record (VIEW_DTYPE): from eye, target and up (sl2_view_look_at), or from a pose as given.
* REFERENCE_EYE ...  - the reference example's view (ModelViewLookAt(0, 0.18, -1.4, 0, 0.13, 0, AxisY)).
* pick_items         - sl2_pick_items_batch over host lists: (label, item index) per image; waits for the device.
* pick_items_host    - sl2_pick_items_host: one image in plain C++ from the same source as the kernel (no GPU needed).
* Engine.world_items / Engine.draw_world / Engine.draw_world_device (monoslam.py) - the lists (SL2_WORLD_* layers) with the
  maps' extents, and fill + list + draw in one call; item_bound below is the longest list.

Nothing here projects or rasterises: the arithmetic lives in scenelib2_amd/csrc/sl2_world_view_dev.hpp.
"""
import numpy as np

from . import _lib
from ._lib import (SL2_WORLD_ALL, SL2_WORLD_AXES, SL2_WORLD_CAMERA, SL2_WORLD_FEATURES, SL2_WORLD_TRAJECTORY,  # noqa: F401
                   SL2_WORLD_UNCERTAINTIES, VIEW_DTYPE)
from .overlay import ITEM_DTYPE, make_items

REFERENCE_EYE, REFERENCE_TARGET, REFERENCE_UP = (0.0, 0.18, -1.4), (0.0, 0.13, 0.0), (0.0, 1.0, 0.0)


def item_bound(max_features, partial_slots):
    """sl2_world_item_bound: the longest world list of a sequence, 3 max_features + partial_slots + 999 + 19."""
    return int(_lib.load().sl2_world_item_bound(int(max_features), int(partial_slots)))


def view(r, q, fku, fkv, u0, v0):
    """A view from a pose as given: r the position, q = qWR (w, x, y, z), used without normalisation."""
    v = np.zeros((), VIEW_DTYPE)
    v["r"], v["q"] = r, q
    v["fku"], v["fkv"], v["u0"], v["v0"] = fku, fkv, u0, v0
    return v


def look_at(eye, target, up, fku, fkv, u0, v0):
    """sl2_view_look_at: the view at `eye` looking at `target`, `up` towards the image's top."""
    L = _lib.load()
    e, t, u = (np.ascontiguousarray(a, dtype=np.float64).reshape(3) for a in (eye, target, up))
    out = np.zeros(1, VIEW_DTYPE)
    _lib.check(L.sl2_view_look_at(_lib.dp(e), _lib.dp(t), _lib.dp(u), float(fku), float(fkv), float(u0), float(v0),
                                  out.ctypes.data_as(_lib.vp)), L)
    return out[0]


def reference_view(cam):
    """The reference example's view with the camera's own intrinsics (cam: fku, fkv, u0, v0)."""
    return look_at(REFERENCE_EYE, REFERENCE_TARGET, REFERENCE_UP, cam["fku"], cam["fkv"], cam["u0"], cam["v0"])


def pick_items_host(width, height, items, x, y, npatches=0):
    """One image on the host: (label, item index) of the last labelled item that covers a pixel of the 7 x 7 window centred on
    (x, y), or (-1, -1)."""
    L = _lib.load()
    it = make_items(items)
    out = np.zeros(2, np.int32)
    _lib.check(L.sl2_pick_items_host(int(width), int(height), it.ctypes.data_as(_lib.vp) if it.size else None, it.size, int(npatches),
                                     int(x), int(y), out.ctypes.data_as(_lib.vp)), L)
    return int(out[0]), int(out[1])


def pick_items(width, height, lists, clicks, npatches=0, device=0, stream=None):
    """sl2_pick_items_batch with everything in host memory: lists a list of nimages item lists, clicks [nimages][2] (x, y).
    Returns int32 [nimages][2]: label and item index, or (-1, -1).  Waits for the device."""
    L = _lib.load()
    arrs = [make_items(l) for l in lists]
    n = len(arrs)
    stride = max([a.size for a in arrs] + [1])
    items = np.zeros((n, stride), ITEM_DTYPE)
    counts = np.zeros(n, np.int32)
    for i, a in enumerate(arrs):
        items[i, :a.size] = a
        counts[i] = a.size
    c = np.ascontiguousarray(clicks, dtype=np.int32).reshape(n, 2)
    out = np.zeros((n, 2), np.int32)
    _lib.check(L.sl2_pick_items_batch(int(device), _lib.vp(stream) if stream else None, n, int(width), int(height),
                                      items.ctypes.data_as(_lib.vp), stride, counts.ctypes.data_as(_lib.vp), int(npatches),
                                      c.ctypes.data_as(_lib.vp), out.ctypes.data_as(_lib.vp), 0), L)
    return out
