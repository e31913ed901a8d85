"""The frame monitor (include/scenelib2_amd.h, "the frame monitor"): exact integer statistics of every
sequence's engine-size grey frame and a per-sequence gate, on the device, in front of the step.

FrameMonitor.examine writes a record, a verdict word and an `active` byte per sequence; the active bytes are what
Engine.set_active(ptr, on_device=True) takes, so a camera that repeated its buffer or delivered a black frame sits the step out
without a host round trip.  frame_stats_host and frame_verdict_host are the same arithmetic for one frame on the host.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FRAME_STATS_DTYPE  # noqa: F401
from ._lib import SL2_FRAME_BLURRED, SL2_FRAME_BRIGHT, SL2_FRAME_DARK, SL2_FRAME_FLAT, SL2_FRAME_REPEATED, SL2_FRAME_SKIPPED  # noqa: F401

VERDICT_BITS = {"flat": SL2_FRAME_FLAT, "dark": SL2_FRAME_DARK, "bright": SL2_FRAME_BRIGHT, "blurred": SL2_FRAME_BLURRED,
                "repeated": SL2_FRAME_REPEATED, "skipped": SL2_FRAME_SKIPPED}
GATE_FIELDS = ("min_range", "dark_bins", "max_dark_pixels", "bright_bins", "max_bright_pixels", "reject_repeated",
               "min_gradient_energy")


def make_gate(gate=None, **kw):
    """dict or keywords of GATE_FIELDS -> sl2_frame_gate; what is missing is 0 (off)."""
    if isinstance(gate, _lib.sl2_frame_gate):
        return gate
    d = dict(gate or {}, **kw)
    unknown = set(d) - set(GATE_FIELDS)
    if unknown:
        raise ValueError("unknown gate fields: %s" % sorted(unknown))
    return _lib.sl2_frame_gate(*[int(d.get(n, 0)) for n in GATE_FIELDS])


def gate_dict(g):
    return {n: int(getattr(g, n)) for n in GATE_FIELDS}


def verdict_names(v):
    """The names of the bits of a verdict word."""
    return [n for n, b in VERDICT_BITS.items() if int(v) & b]


def _ptr(p):
    if p is None:
        return None
    return _lib.vp(p.ptr if isinstance(p, _lib.DeviceBuffer) else int(p))


class FrameMonitor:
    """`batch` sequences of width x height grey frames: two launches per examine call."""

    def __init__(self, device, batch, width, height, lib=None):
        self.L = lib or _lib.load()
        self.device, self.batch, self.width, self.height = int(device), int(batch), int(width), int(height)
        self.frame_bytes = self.width * self.height
        h = _lib.vp()
        _lib.check(self.L.sl2_frame_monitor_create(self.device, self.batch, self.width, self.height, C.byref(h)), self.L)
        self.h = h

    def set_gates(self, gates, seq0=0):
        """gates: a list of dicts (make_gate) or sl2_frame_gate for sequences seq0 ...; one dict stands for a list of one.
        Takes effect for the next examine call; never waits."""
        if isinstance(gates, (dict, _lib.sl2_frame_gate)):
            gates = [gates]
        arr = (_lib.sl2_frame_gate * len(gates))(*[make_gate(g) for g in gates])
        _lib.check(self.L.sl2_frame_monitor_set_gates(self.h, int(seq0), len(gates), arr), self.L)

    def get_gates(self, seq0=0, nseq=None):
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        arr = (_lib.sl2_frame_gate * nseq)()
        _lib.check(self.L.sl2_frame_monitor_get_gates(self.h, int(seq0), nseq, arr), self.L)
        return [gate_dict(g) for g in arr]

    def reset(self, seq0=0, nseq=None):
        """Forget the previous digests of the range: the next examined frame of such a sequence is not "repeated"."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        _lib.check(self.L.sl2_frame_monitor_reset(self.h, int(seq0), nseq), self.L)

    def examine(self, d_frames, seq_stride=0, base_active=None, stats_out=None, verdict_out=None, active_out=None, stream=None):
        """d_frames and the four optional arrays are device pointers (or DeviceBuffers): base_active [batch] bytes, stats_out
        [batch] records of FRAME_STATS_DTYPE, verdict_out [batch] uint32, active_out [batch] bytes.  Asynchronous on `stream`."""
        stride = int(seq_stride) if seq_stride else self.frame_bytes
        _lib.check(self.L.sl2_examine_frames(self.h, _lib.vp(stream) if stream else None, _ptr(d_frames), stride, _ptr(base_active),
                                             _ptr(stats_out), _ptr(verdict_out), _ptr(active_out)), self.L)

    def read(self, seq0=0, nseq=None):
        """(records as a FRAME_STATS_DTYPE array, verdicts as uint32) of the last examination.  Synchronises."""
        nseq = self.batch - seq0 if nseq is None else int(nseq)
        stats = np.zeros(nseq, FRAME_STATS_DTYPE)
        verdicts = np.zeros(nseq, np.uint32)
        _lib.check(self.L.sl2_frame_monitor_read(self.h, int(seq0), nseq, stats.ctypes.data_as(_lib.vp), verdicts.ctypes.data_as(_lib.vp)), self.L)
        return stats, verdicts

    def close(self):
        if getattr(self, "h", None):
            self.L.sl2_frame_monitor_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def frame_stats_host(frame, width=None, height=None):
    """The record of one frame on the host (no GPU needed), as a FRAME_STATS_DTYPE scalar.  frame: uint8 [height][width], or
    any uint8 array of at least width * height bytes with the size given."""
    L = _lib.load()
    a = np.ascontiguousarray(frame, dtype=np.uint8)
    if width is None:
        height, width = a.shape
    assert a.size >= int(width) * int(height)
    s = _lib.sl2_frame_stats()
    _lib.check(L.sl2_frame_stats_host(a.ctypes.data_as(_lib.vp), int(width), int(height), C.byref(s)), L)
    return np.frombuffer(bytes(s), FRAME_STATS_DTYPE)[0]


def _stats_struct(stats):
    if isinstance(stats, _lib.sl2_frame_stats):
        return stats
    return _lib.sl2_frame_stats.from_buffer_copy(np.asarray(stats, FRAME_STATS_DTYPE).tobytes())


def frame_verdict_host(stats, gate, have_previous=False, previous_digest=0):
    """The verdict word of a record (frame_stats_host, FrameMonitor.read) under a gate (make_gate)."""
    L = _lib.load()
    s, g = _stats_struct(stats), make_gate(gate)
    v = L.sl2_frame_verdict_host(C.byref(s), C.byref(g), 1 if have_previous else 0, int(previous_digest))
    if v == 0xFFFFFFFF:
        raise _lib.Sl2Error(_lib.SL2_ERR_INVALID, L.sl2_last_error().decode("utf-8", "replace"))
    return int(v)
