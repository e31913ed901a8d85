"""Raw camera frames -> the engine's grey images (include/scenelib2_amd.h, "raw camera frames").

The reference's UsbCamGrabber reduces whatever the camera delivers to 8-bit grey and resizes it to the filter's image size
before GoOneStep sees it.  FrameConverter does that for a whole batch in one launch on the device: every sequence has its own
source size, row pitch and pixel format.  convert_frame_host is the same arithmetic for one sequence on the host, and
scale_camera the calibration that goes with the resized image.  A camera whose lens the filter's model does not describe
follows a per-pixel map instead (lens_map, pinhole_camera, FrameConverter.set_map / set_remaps, remap_frame_host).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import SL2_PIX_BGR24, SL2_PIX_GRAY8, SL2_PIX_RGB24, SL2_PIX_UYVY, SL2_PIX_YUYV  # noqa: F401
from ._lib import SL2_PIX_GRAY10, SL2_PIX_GRAY12, SL2_PIX_GRAY16  # noqa: F401
from ._lib import SL2_PIX_BAYER_BGGR8, SL2_PIX_BAYER_GBRG8, SL2_PIX_BAYER_GRBG8, SL2_PIX_BAYER_RGGB8  # noqa: F401

FORMATS = {"gray8": SL2_PIX_GRAY8, "rgb24": SL2_PIX_RGB24, "bgr24": SL2_PIX_BGR24, "uyvy": SL2_PIX_UYVY, "yuyv": SL2_PIX_YUYV,
           "gray10": SL2_PIX_GRAY10, "gray12": SL2_PIX_GRAY12, "gray16": SL2_PIX_GRAY16,
           "bayer_rggb8": SL2_PIX_BAYER_RGGB8, "bayer_grbg8": SL2_PIX_BAYER_GRBG8, "bayer_gbrg8": SL2_PIX_BAYER_GBRG8,
           "bayer_bggr8": SL2_PIX_BAYER_BGGR8}
FILTERS = {"linear": _lib.SL2_RESIZE_LINEAR, "area": _lib.SL2_RESIZE_AREA}
BYTES_PER_PIXEL = {SL2_PIX_GRAY8: 1, SL2_PIX_RGB24: 3, SL2_PIX_BGR24: 3, SL2_PIX_UYVY: 2, SL2_PIX_YUYV: 2,
                   SL2_PIX_GRAY10: 2, SL2_PIX_GRAY12: 2, SL2_PIX_GRAY16: 2,
                   SL2_PIX_BAYER_RGGB8: 1, SL2_PIX_BAYER_GRBG8: 1, SL2_PIX_BAYER_GBRG8: 1, SL2_PIX_BAYER_BGGR8: 1}


def _format(f):
    return FORMATS[f.lower()] if isinstance(f, str) else int(f)


def _filter(f):
    return FILTERS[f.lower()] if isinstance(f, str) else int(f)


def make_source(src):
    """dict(width, height, format[, pitch, offset]) -> sl2_frame_source; pitch defaults to the bytes of a row, offset to 0."""
    if isinstance(src, _lib.sl2_frame_source):
        return src
    fmt = _format(src["format"])
    pitch = src.get("pitch")
    if pitch is None:
        pitch = int(src["width"]) * BYTES_PER_PIXEL.get(fmt, 1)
    return _lib.sl2_frame_source(int(src["width"]), int(src["height"]), int(pitch), fmt, int(src.get("offset", 0)))


def source_bytes(src):
    """Bytes of the raw buffer a source reaches: offset + (height - 1) * pitch + the bytes of a row."""
    s = make_source(src)
    return s.offset + (s.height - 1) * s.pitch + s.width * BYTES_PER_PIXEL[s.format]


class FrameConverter:
    """nseq sequences' raw frames -> [nseq][out_height][out_width] grey on the device, one launch per call."""

    def __init__(self, device, nseq, out_width, out_height, lib=None):
        self.L = lib or _lib.load()
        self.device, self.nseq = int(device), int(nseq)
        self.out_width, self.out_height = int(out_width), int(out_height)
        self.frame_bytes = self.out_width * self.out_height
        h = _lib.vp()
        _lib.check(self.L.sl2_converter_create(self.device, self.nseq, self.out_width, self.out_height, C.byref(h)), self.L)
        self.h = h

    def set_sources(self, sources, seq0=0):
        """sources: a list of dicts (make_source) or sl2_frame_source, for sequences seq0 ...  A setup call: it may wait."""
        arr = (_lib.sl2_frame_source * len(sources))(*[make_source(s) for s in sources])
        _lib.check(self.L.sl2_converter_set_sources(self.h, int(seq0), len(sources), arr), self.L)

    def get_sources(self, seq0=0, nseq=None):
        nseq = self.nseq - seq0 if nseq is None else int(nseq)
        arr = (_lib.sl2_frame_source * nseq)()
        _lib.check(self.L.sl2_converter_get_sources(self.h, int(seq0), nseq, arr), self.L)
        return [dict(width=s.width, height=s.height, pitch=s.pitch, format=s.format, offset=s.offset) for s in arr]

    def set_filters(self, filters, seq0=0):
        """filters: "linear" / "area" (or SL2_RESIZE_*) for sequences seq0 ...; one value stands for a list of one.  A setup call
        like set_sources, before or after it.  "area", the exact box average, only reduces: a smaller source is refused."""
        if isinstance(filters, (str, int)):
            filters = [filters]
        arr = (C.c_int32 * len(filters))(*[_filter(f) for f in filters])
        _lib.check(self.L.sl2_converter_set_filters(self.h, int(seq0), len(filters), arr), self.L)

    def get_filters(self, seq0=0, nseq=None):
        nseq = self.nseq - seq0 if nseq is None else int(nseq)
        arr = (C.c_int32 * nseq)()
        _lib.check(self.L.sl2_converter_get_filters(self.h, int(seq0), nseq, arr), self.L)
        return list(arr)

    def set_map(self, slot, src_width=0, src_height=0, xy=None):
        """Fill or replace map slot `slot` (0 .. nseq - 1) with xy: int32 [out_height][out_width][2], positions in the grey plane
        of a src_width x src_height source in 1/32 pixel, SL2_REMAP_BORDER in X for no source (lens_map builds one from a
        calibration).  xy=None empties the slot.  A setup call: it may wait; xy is consumed before it returns."""
        if xy is None:
            _lib.check(self.L.sl2_converter_set_map(self.h, int(slot), int(src_width), int(src_height), None), self.L)
            return
        a = np.ascontiguousarray(xy, dtype=np.int32)
        assert a.shape == (self.out_height, self.out_width, 2), a.shape
        _lib.check(self.L.sl2_converter_set_map(self.h, int(slot), int(src_width), int(src_height), _lib.ip(a)), self.L)

    def set_remaps(self, slots, seq0=0):
        """The map slot of sequences seq0 ..., -1 (or None) for none; one value stands for a list of one.  A sequence with a map
        ignores its resize filter, which acts again once its slot is -1.  A setup call like set_sources."""
        if slots is None or isinstance(slots, int):
            slots = [slots]
        arr = (C.c_int32 * len(slots))(*[-1 if s is None else int(s) for s in slots])
        _lib.check(self.L.sl2_converter_set_remaps(self.h, int(seq0), len(slots), arr), self.L)

    def get_remaps(self, seq0=0, nseq=None):
        nseq = self.nseq - seq0 if nseq is None else int(nseq)
        arr = (C.c_int32 * nseq)()
        _lib.check(self.L.sl2_converter_get_remaps(self.h, int(seq0), nseq, arr), self.L)
        return list(arr)

    def convert(self, raw, d_frames, seq_stride=0, stream=None, raw_bytes=None):
        """raw: a uint8 array in host memory (copied to the converter's staging buffer on `stream`; keep it alive and
        unchanged until the stream has passed the copy), or a (device pointer, bytes) pair.  d_frames: a device pointer
        (or a DeviceBuffer) of nseq * seq_stride bytes; seq_stride defaults to out_width * out_height.  Asynchronous."""
        stride = int(seq_stride) if seq_stride else self.frame_bytes
        dst = d_frames.ptr if isinstance(d_frames, _lib.DeviceBuffer) else int(d_frames)
        st = _lib.vp(stream) if stream else None
        if isinstance(raw, tuple):
            ptr, n = raw
            _lib.check(self.L.sl2_convert_frames(self.h, st, _lib.vp(int(ptr)), int(n), 1, _lib.vp(dst), stride), self.L)
            return None
        a = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1)
        n = a.size if raw_bytes is None else int(raw_bytes)
        assert n <= a.size
        _lib.check(self.L.sl2_convert_frames(self.h, st, a.ctypes.data_as(_lib.vp), n, 0, _lib.vp(dst), stride), self.L)
        return a

    def close(self):
        if getattr(self, "h", None):
            self.L.sl2_converter_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def convert_frame_host(src, raw, out_width, out_height, raw_bytes=None, filter="linear"):
    """One sequence on the host (no GPU needed): uint8 [out_height][out_width].  filter: "linear" or "area" (FILTERS)."""
    L = _lib.load()
    a = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1)
    n = a.size if raw_bytes is None else int(raw_bytes)
    out = np.zeros((int(out_height), int(out_width)), np.uint8)
    s = make_source(src)
    f = _filter(filter)
    if f == _lib.SL2_RESIZE_LINEAR:
        _lib.check(L.sl2_convert_frame_host(C.byref(s), a.ctypes.data_as(_lib.vp), n, int(out_width), int(out_height), _lib.u8p(out)), L)
    else:
        _lib.check(L.sl2_convert_frame_host_filtered(C.byref(s), f, a.ctypes.data_as(_lib.vp), n, int(out_width), int(out_height),
                                                     _lib.u8p(out)), L)
    return out


LENS_MODELS = {"radial1": _lib.SL2_LENS_RADIAL1, "brown": _lib.SL2_LENS_BROWN, "fisheye": _lib.SL2_LENS_FISHEYE}
SL2_REMAP_BORDER = _lib.SL2_REMAP_BORDER


def _camera_dict(c):
    return dict(width=c.width, height=c.height, fku=c.fku, fkv=c.fkv, u0=c.u0, v0=c.v0, kd1=c.kd1, sd=c.sd)


def make_lens(lens):
    """dict(model, width, height, fx, fy, cx, cy[, k]) -> sl2_lens; model: "radial1" (k = [kd1]), "brown" (OpenCV's k1 k2 p1 p2 k3
    k4 k5 k6) or "fisheye" (k1 .. k4), or SL2_LENS_*; missing coefficients are 0."""
    if isinstance(lens, _lib.sl2_lens):
        return lens
    m = lens["model"]
    k = [float(v) for v in lens.get("k", ())]
    assert len(k) <= 8
    return _lib.sl2_lens(LENS_MODELS[m.lower()] if isinstance(m, str) else int(m), int(lens["width"]), int(lens["height"]),
                         float(lens["fx"]), float(lens["fy"]), float(lens["cx"]), float(lens["cy"]), (C.c_double * 8)(*(k + [0.0] * (8 - len(k)))))


def remap_frame_host(src, xy, raw, raw_bytes=None):
    """One sequence through the map xy (int32 [out_height][out_width][2], for a source of src's size) on the host (no GPU
    needed): uint8 [out_height][out_width]."""
    L = _lib.load()
    a = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1)
    n = a.size if raw_bytes is None else int(raw_bytes)
    m = np.ascontiguousarray(xy, dtype=np.int32)
    assert m.ndim == 3 and m.shape[2] == 2, m.shape
    out = np.zeros(m.shape[:2], np.uint8)
    s = make_source(src)
    _lib.check(L.sl2_remap_frame_host(C.byref(s), _lib.ip(m), a.ctypes.data_as(_lib.vp), n, m.shape[1], m.shape[0], _lib.u8p(out)), L)
    return out


def lens_map(lens, target):
    """The map that reads an image the camera `target` (a dict as for Engine: the calibration the engine runs with, its width and
    height the output size) would have seen out of the image of `lens` (make_lens): int32 [height][width][2].  Host only."""
    L = _lib.load()
    ln, cam = make_lens(lens), _lib.make_camera(target)
    xy = np.zeros((max(cam.height, 0), max(cam.width, 0), 2), np.int32)
    _lib.check(L.sl2_lens_map_host(C.byref(ln), C.byref(cam), _lib.ip(xy)), L)
    return xy


def pinhole_camera(lens, out_width, out_height, sd=1):
    """The pinhole target (kd1 = 0) that sees the lens's image plane resized to out_width x out_height, as a camera dict."""
    L = _lib.load()
    ln = make_lens(lens)
    out = _lib.sl2_camera()
    _lib.check(L.sl2_lens_pinhole_camera(C.byref(ln), int(out_width), int(out_height), int(sd), C.byref(out)), L)
    return _camera_dict(out)


def scale_camera(cam, out_width, out_height):
    """The calibration of the image resized to out_width x out_height, from the source image's (cam: a dict as for Engine;
    its width / height are the source size).  A resize that changes the aspect ratio is refused."""
    L = _lib.load()
    src = _lib.make_camera(cam)
    out = _lib.sl2_camera()
    _lib.check(L.sl2_scale_camera(C.byref(src), int(out_width), int(out_height), C.byref(out)), L)
    return dict(width=out.width, height=out.height, fku=out.fku, fkv=out.fkv, u0=out.u0, v0=out.v0, kd1=out.kd1, sd=out.sd)
