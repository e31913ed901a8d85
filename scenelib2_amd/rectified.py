"""The rectified view (include/scenelib2_amd.h, "the rectified view"): the reference's display of the map,
GraphicTool::DrawRectifiedAR - the line primitive of the rasteriser, the camera frame with the lens distortion removed, and
the 3-D scene as a draw list.

* segment             - an SL2_ITEM_SEGMENT record for overlay.draw_items / overlay.draw_items_host.
* rectify_frame_host  - sl2_rectify_frame_host: one image in plain C++ from the same source as the kernel (no GPU needed).
* Engine.rectify_frames / Engine.rectify_frames_device (monoslam.py) - a range of sequences, each with its own camera, in one launch.
* Engine.scene_items / Engine.draw_rectified / Engine.draw_rectified_device - the scene lists (SL2_SCENE_* layers), and
  rectify + list + draw in one call; item_bound below is the longest list.

Nothing here warps or rasterises: the pixel rules live in scenelib2_amd/csrc/sl2_rectify_dev.hpp and sl2_overlay_dev.hpp.
"""
import numpy as np

from . import _lib
from ._lib import (SL2_ITEM_SEGMENT, SL2_SCENE_ALL, SL2_SCENE_FEATURES, SL2_SCENE_TRAJECTORY,  # noqa: F401
                   SL2_SCENE_UNCERTAINTIES)
from .overlay import ITEM_DTYPE, YELLOW


def item_bound(max_features, partial_slots):
    """sl2_scene_item_bound: the longest scene list of a sequence, 3 max_features + partial_slots + 999."""
    return int(_lib.load().sl2_scene_item_bound(int(max_features), int(partial_slots)))


def segment(x0, y0, x1, y1, rgb=YELLOW, label=-1):
    it = np.zeros((), ITEM_DTYPE)
    it["kind"], it["label"], it["patch"] = SL2_ITEM_SEGMENT, label, -1
    it["a"] = (x0, y0, x1, y1)
    it["rgb"] = rgb
    return it


def rectify_frame_host(frame, u0, v0, kd1):
    """One image on the host: frame uint8 [height][width] -> uint8 [height][width], the view of a pinhole camera with the same
    principal point (u0, v0); kd1 is the radial distortion coefficient of the camera that took the frame."""
    L = _lib.load()
    f = np.ascontiguousarray(frame, dtype=np.uint8)
    h, w = f.shape
    out = np.zeros((h, w), np.uint8)
    _lib.check(L.sl2_rectify_frame_host(f.ctypes.data_as(_lib.vp), w, h, float(u0), float(v0), float(kd1), out.ctypes.data_as(_lib.vp)), L)
    return out
