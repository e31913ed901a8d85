"""k_raw_linear and k_raw_area on the GPU: every case of frame_convert_raw_cases.py - the deep grey and Bayer formats under both
filters at every head length class, pitch and edge shape - byte for byte against the host forms (which
tests/test_frame_convert_raw_host.py holds to the definition), from a device and from a host raw buffer; the bytes around the
outputs; old and new formats in one call; the sources' round trip and the refusals.  A converter has ONE output size, so the
table goes through one converter per output size (five), each holding all its cases as the sequences of one batch: one
sl2_convert_frames call checks them all.
The converter exposes no launch counters: that a batch without a new format launches what it launched before is read from the
code (the two new launches are guarded by their lists being non-empty) and left to the timing against the parent's library."""
import numpy as np
import pytest

import frame_convert_cases as fc
import frame_convert_raw_cases as rc
from frame_convert_raw_cases import AREA, LINEAR

from scenelib2_amd import _lib, convert

pytestmark = pytest.mark.gpu

FILTER_NAME = {LINEAR: "linear", AREA: "area"}
LEAD = 16          # poison in front of the raw buffer on the device: a multiple of 16 keeps every case's head length class


def _layout(specs, seed):
    """(width, height, format, pitch pad, offset) sources one after the other, each from a 16-byte boundary plus its own offset,
    in one raw buffer of exactly the bytes they reach, every byte random."""
    srcs, total = [], 0
    for w, h, fmt, pad, off in specs:
        bpp = rc.BPP[fmt] if fmt in rc.BPP else fc.BPP[fmt]
        base = (total + 15) & ~15
        s = dict(width=w, height=h, pitch=w * bpp + pad, format=fmt, offset=base + off)
        total = s["offset"] + (h - 1) * s["pitch"] + w * bpp
        srcs.append(s)
    return srcs, np.random.default_rng(seed).integers(0, 256, total, dtype=np.uint8)


@pytest.fixture(scope="module")
def table():
    """out size -> (sources, filters, raw, what the host forms give [n][out_h * out_w]), computed once."""
    t = {}
    for out in rc.SHAPES:
        mine = [c for c in rc.CASES if c[0] == out]
        srcs, raw = _layout([(c[1][0], c[1][1], c[2], c[4], c[5]) for c in mine], 40 + out[0])
        filters = [c[3] for c in mine]
        want = np.stack([convert.convert_frame_host(s, raw, out[0], out[1], filter=FILTER_NAME[f]).reshape(-1) for s, f in zip(srcs, filters)])
        want.setflags(write=False)
        t[out] = (srcs, filters, raw, want)
    return t


class _Dev:
    """[poison | raw | poison] in one device block and an output block prefilled with 0xA5."""

    def __init__(self, raw, nseq, stride, tail=256, poison=4096):
        self.n, self.nseq, self.stride, self.tail = raw.size, nseq, stride, tail
        self.src = _lib.DeviceBuffer(LEAD + raw.size + poison)
        self.src.upload(np.concatenate([np.full(LEAD, 0xEE, np.uint8), raw, np.full(poison, 0xFF, np.uint8)]))
        self.out = _lib.DeviceBuffer(nseq * stride + tail)
        self.fill()

    def fill(self):
        self.out.upload(np.full(self.nseq * self.stride + self.tail, 0xA5, np.uint8))

    @property
    def raw(self):
        return (self.src.ptr + LEAD, self.n)

    def result(self, frame_bytes):
        """(frames [nseq][frame_bytes], everything else) of the output block."""
        a = self.out.download((self.nseq * self.stride + self.tail,), np.uint8)
        body = a[:self.nseq * self.stride].reshape(self.nseq, self.stride)
        return body[:, :frame_bytes], np.concatenate([body[:, frame_bytes:].reshape(-1), a[self.nseq * self.stride:]])

    def free(self):
        self.src.free()
        self.out.free()


def _assert_frames(frames, want, srcs, filters):
    for i in range(len(srcs)):
        diff = np.flatnonzero(frames[i] != want[i])
        assert diff.size == 0, "sequence %d (%s, filter %d): %d bytes differ, first at %d" % (i, srcs[i], filters[i], diff.size, diff[0])


@pytest.mark.parametrize("raw_on_device", [1, 0])
@pytest.mark.parametrize("out", list(rc.SHAPES))
def test_whole_table_equals_the_host_form_and_touches_nothing_else(table, out, raw_on_device):
    ow, oh = out
    srcs, filters, raw, want = table[out]
    n = len(srcs)
    stride = ow * oh + 37
    d = _Dev(raw, n, stride)
    cv = convert.FrameConverter(0, n, ow, oh)
    try:
        cv.set_sources(srcs)
        cv.set_filters(filters)
        keep = cv.convert(d.raw if raw_on_device else raw, d.out, seq_stride=stride)
        frames, rest = d.result(ow * oh)
        del keep
        _assert_frames(frames, want, srcs, filters)
        # the 37 bytes behind every sequence and the 256 behind the last one are as they were; the poisoned neighbours of the raw
        # buffer (0xEE in front, 0xFF behind) reached no output: the host form never saw them
        assert rest.size == n * 37 + 256 and (rest == 0xA5).all()
    finally:
        cv.close()
        d.free()


def test_old_and_new_formats_share_a_call_and_the_old_ones_keep_their_bytes():
    ow, oh = 33, 17
    old = [(640, 480, fc.UYVY, 0, 1, LINEAR), (47, 17, fc.RGB24, 1, 0, AREA), (31, 17, fc.GRAY8, 13, 7, LINEAR), (66, 34, fc.YUYV, 0, 0, AREA),
           (99, 51, fc.BGR24, 1, 1, LINEAR)]
    new = [(640, 480, rc.BAYER_RGGB8, 0, 1, LINEAR), (1280, 960, rc.BAYER_GRBG8, 13, 15, AREA), (1280, 960, rc.GRAY12, 2, 14, AREA),
           (47, 17, rc.GRAY10, 0, 2, LINEAR), (99, 51, rc.BAYER_BGGR8, 1, 7, AREA), (31, 17, rc.GRAY16, 14, 0, LINEAR),
           (1001, 40, rc.BAYER_GBRG8, 0, 0, LINEAR)]
    mixed = [old[0], new[0], new[1], old[1], old[2], new[2], new[3], old[3], new[4], new[5], old[4], new[6]]
    srcs, raw = _layout([m[:5] for m in mixed], 77)
    filters = [m[5] for m in mixed]
    n = len(mixed)
    want = np.stack([convert.convert_frame_host(s, raw, ow, oh, filter=FILTER_NAME[f]).reshape(-1) for s, f in zip(srcs, filters)])
    is_old = [m in old for m in mixed]
    d = _Dev(raw, n, ow * oh + 5)
    d_old = _Dev(raw, len(old), ow * oh, tail=0)
    cv = convert.FrameConverter(0, n, ow, oh)
    cv_old = convert.FrameConverter(0, len(old), ow, oh)
    try:
        cv.set_filters(filters)
        cv.set_sources(srcs)
        cv.convert(d.raw, d.out, seq_stride=ow * oh + 5)
        frames, rest = d.result(ow * oh)
        _assert_frames(frames, want, srcs, filters)
        assert (rest == 0xA5).all()
        # a converter that holds only the old-format sequences gives them the same bytes
        cv_old.set_sources([s for s, o in zip(srcs, is_old) if o])
        cv_old.set_filters([f for f, o in zip(filters, is_old) if o])
        cv_old.convert(d_old.raw, d_old.out)
        assert np.array_equal(d_old.result(ow * oh)[0], frames[np.array(is_old)])
        # a sequence changes family and filter in place: the lists follow
        cv.set_filters([LINEAR], seq0=2)
        cv.set_sources([srcs[1]], seq0=0)
        d.fill()
        cv.convert(d.raw, d.out, seq_stride=ow * oh + 5)
        again = d.result(ow * oh)[0]
        assert np.array_equal(again[0], want[1]) and np.array_equal(again[3:], want[3:]) and np.array_equal(again[1], want[1])
        assert np.array_equal(again[2], convert.convert_frame_host(srcs[2], raw, ow, oh).reshape(-1))
    finally:
        cv.close()
        cv_old.close()
        d.free()
        d_old.free()


def test_sources_round_trip_and_refusals_name_the_sequence_and_change_nothing():
    ow, oh = 16, 8
    specs = [(33, 17, rc.BAYER_GRBG8, 1, 15), (47, 17, rc.GRAY12, 2, 14), (16, 8, rc.BAYER_BGGR8, 0, 0), (17, 9, rc.GRAY16, 14, 2),
             (32, 16, rc.GRAY10, 0, 0), (33, 17, rc.BAYER_GBRG8, 13, 7), (17, 9, rc.BAYER_RGGB8, 0, 1)]
    srcs, raw = _layout(specs, 78)
    filters = [AREA, LINEAR, AREA, AREA, LINEAR, LINEAR, AREA]
    n = len(srcs)
    want = np.stack([convert.convert_frame_host(s, raw, ow, oh, filter=FILTER_NAME[f]).reshape(-1) for s, f in zip(srcs, filters)])
    d = _Dev(raw, n, ow * oh, tail=0)
    cv = convert.FrameConverter(0, n, ow, oh)

    def key(s):
        return (s["width"], s["height"], s["pitch"], s["format"], s["offset"])

    def refused(fn, *texts):
        with pytest.raises(_lib.Sl2Error) as ei:
            fn()
        assert ei.value.code == _lib.SL2_ERR_INVALID and all(t in str(ei.value) for t in texts), str(ei.value)
        assert cv.get_filters() == filters and [key(g) for g in cv.get_sources()] == [key(s) for s in srcs]
        d.fill()
        cv.convert(d.raw, d.out)
        assert np.array_equal(d.result(ow * oh)[0], want)

    try:
        cv.set_sources(srcs)
        cv.set_filters(filters)
        assert [key(g) for g in cv.get_sources()] == [key(s) for s in srcs]
        assert {g["format"] for g in cv.get_sources()} == set(rc.FORMATS)
        refused(lambda: cv.set_sources([srcs[0], rc.source(1, 9, rc.BAYER_RGGB8)], seq0=4), "sequence 5", "Bayer")
        refused(lambda: cv.set_sources([rc.source(16, 1, rc.BAYER_GBRG8)], seq0=1), "sequence 1", "Bayer")
        refused(lambda: cv.set_sources([rc.source(16, 8, rc.GRAY12, pad=1)], seq0=3), "sequence 3", "odd offset or pitch")
        refused(lambda: cv.set_sources([rc.source(16, 8, rc.GRAY16, offset=7)], seq0=6), "sequence 6", "odd offset or pitch")
        for fmt in (5, 9, 15, 19, 23, 28):
            refused(lambda: cv.set_sources([dict(rc.source(16, 8, rc.GRAY16), format=fmt)], seq0=2), "sequence 2", "unknown pixel format")
        refused(lambda: cv.set_sources([rc.source(15, 9, rc.BAYER_RGGB8)], seq0=0), "sequence 0", "only reduces")      # AREA, narrower
        refused(lambda: cv.set_sources([rc.source(16, 7, rc.GRAY10)], seq0=3), "sequence 3", "only reduces")           # AREA, lower
        cv.set_sources([rc.source(16, 7, rc.GRAY10)], seq0=4)                                                          # LINEAR takes it
    finally:
        cv.close()
        d.free()


def test_reach_and_an_odd_device_address_are_refused_before_anything_is_queued():
    ow, oh = 7, 5
    srcs, raw = _layout([(15, 9, rc.BAYER_RGGB8, 1, 1), (15, 9, rc.GRAY12, 2, 2)], 79)
    d = _Dev(raw, 2, ow * oh, tail=0)
    cv = convert.FrameConverter(0, 2, ow, oh)
    try:
        cv.set_sources(srcs)
        with pytest.raises(_lib.Sl2Error) as ei:
            cv.convert((d.raw[0], raw.size - 1), d.out)                      # the last source ends one byte past the buffer
        assert ei.value.code == _lib.SL2_ERR_INVALID and "sequence 1" in str(ei.value)
        with pytest.raises(_lib.Sl2Error) as ei:
            cv.convert((d.raw[0] - 1, raw.size + 1), d.out)                  # 16-bit words at odd addresses
        assert ei.value.code == _lib.SL2_ERR_INVALID and "sequence 1" in str(ei.value) and "odd address" in str(ei.value)
        assert (d.result(ow * oh)[0] == 0xA5).all()                          # nothing ran
        cv.convert(d.raw, d.out)
        want = np.stack([convert.convert_frame_host(s, raw, ow, oh).reshape(-1) for s in srcs])
        assert np.array_equal(d.result(ow * oh)[0], want)
    finally:
        cv.close()
        d.free()
