"""k_convert_area on the GPU: SL2_RESIZE_AREA and SL2_RESIZE_LINEAR sequences of every source size, pitch, offset and pixel format
in one call, byte for byte against sl2_convert_frame_host_filtered (which tests/test_frame_convert_area_host.py holds to the
definition); the bytes around the outputs and the raw buffer; the 64-bit accumulator; host and device raw buffers; a queued
conversion keeping its filters; the refusals; and the Python adapter stepping on area-reduced frames."""
import ctypes as C

import numpy as np
import pytest

import frame_convert_cases as fc
import frame_convert_area_cases as fa

from scenelib2_amd import _lib, convert

pytestmark = pytest.mark.gpu

LIN, AREA = fa.LINEAR, fa.AREA
# (width, height, format, pitch padding, bytes skipped in front, filter)
MIXED = [(1, 1, fc.GRAY8, 0, 0, LIN), (2, 2, fc.UYVY, 0, 0, LIN), (5, 3, fc.RGB24, 0, 0, LIN), (31, 17, fc.GRAY8, 0, 0, LIN),
         (640, 480, fc.UYVY, 0, 1, AREA), (961, 18, fc.RGB24, 1, 0, AREA), (4096, 18, fc.YUYV, 13, 7, AREA),
         (321, 241, fc.BGR24, 1, 1, AREA), (33, 17, fc.GRAY8, 0, 7, AREA), (1920, 1080, fc.YUYV, 0, 0, AREA),
         (160, 120, fc.BGR24, 13, 0, AREA)]
TWIN_OF = 4          # the first AREA sequence: a twelfth sequence names its bytes under LINEAR
SIX = [(640, 480, fc.UYVY, 0, 0, AREA), (1280, 960, fc.GRAY8, 0, 0, AREA), (1920, 1080, fc.YUYV, 0, 0, AREA),
       (961, 241, fc.RGB24, 0, 0, AREA), (321, 241, fc.BGR24, 0, 3, AREA), (320, 240, fc.GRAY8, 32, 0, AREA)]
STRIPES = 1          # SIX[1] carries the period-4 column pattern


def _layout(specs, seed, twin_of=None):
    """The sources one after the other in one raw buffer of exactly the bytes they reach, every byte random."""
    srcs, filters, total = [], [], 0
    for w, h, fmt, pad, gap, flt in specs:
        s = fc.source(w, h, fmt, pad, total + gap)
        total = fc.source_bytes(s)
        srcs.append(s)
        filters.append(flt)
    if twin_of is not None:
        srcs.append(dict(srcs[twin_of]))
        filters.append(LIN)
    raw = np.random.default_rng(seed).integers(0, 256, total, dtype=np.uint8)
    return srcs, filters, raw


def _host(srcs, filters, raw, ow, oh):
    return np.stack([convert.convert_frame_host(s, raw, ow, oh, filter=f) for s, f in zip(srcs, filters)])


class _Dev:
    """[lead | raw | poison] in one device block and an output block prefilled with 0xA5."""

    def __init__(self, raw, nseq, stride, lead=3, tail=256, poison=4096):
        self.lead, self.n, self.nseq, self.stride, self.tail = lead, raw.size, nseq, stride, tail
        self.src = _lib.DeviceBuffer(lead + raw.size + poison)
        self.src.upload(np.concatenate([np.full(lead, 0xEE, np.uint8), raw, np.full(poison, 0xFF, np.uint8)]))
        self.out = _lib.DeviceBuffer(nseq * stride + tail)
        self.out.upload(np.full(nseq * stride + tail, 0xA5, np.uint8))

    @property
    def raw(self):
        return (self.src.ptr + self.lead, self.n)

    def result(self, frame_bytes):
        """(frames [nseq][frame_bytes], everything else) of the output block."""
        a = self.out.download((self.nseq * self.stride + self.tail,), np.uint8)
        body = a[:self.nseq * self.stride].reshape(self.nseq, self.stride)
        return body[:, :frame_bytes], np.concatenate([body[:, frame_bytes:].reshape(-1), a[self.nseq * self.stride:]])

    def free(self):
        self.src.free()
        self.out.free()


def _assert_frames(frames, want, srcs):
    for i in range(len(srcs)):
        diff = np.flatnonzero(frames[i] != want[i].reshape(-1))
        assert diff.size == 0, "sequence %d (%s): %d bytes differ, first at %d" % (i, srcs[i], diff.size, diff[0])


@pytest.mark.parametrize("which", ["twelve-to-33x17", "six-to-320x240"])
def test_mixed_launch_equals_the_host_form_and_touches_nothing_else(which):
    twelve = which == "twelve-to-33x17"
    ow, oh = (33, 17) if twelve else (320, 240)
    srcs, filters, raw = _layout(MIXED if twelve else SIX, 21, twin_of=TWIN_OF if twelve else None)
    if not twelve:          # the aliasing anchor: columns 0, 255, 255, 0 across the 1280-wide grey frame
        s = srcs[STRIPES]
        raw[s["offset"]:s["offset"] + 1280 * 960] = fa.stripes(1280, 960, (0, 255, 255, 0)).reshape(-1)
    n = len(srcs)
    assert n == (12 if twelve else 6)
    want = _host(srcs, filters, raw, ow, oh)
    stride = ow * oh + 64
    d = _Dev(raw, n, stride)
    cv = convert.FrameConverter(0, n, ow, oh)
    try:
        assert cv.get_filters() == [LIN] * n          # the default, before any source is set
        cv.set_filters(filters[:5])                   # some before their sources, the rest after
        cv.set_sources(srcs)
        cv.set_filters(filters[5:], seq0=5)
        assert cv.get_filters() == filters and cv.get_filters(seq0=2, nseq=3) == filters[2:5]
        cv.convert(d.raw, d.out, seq_stride=stride)
        frames, rest = d.result(ow * oh)
        _assert_frames(frames, want, srcs)
        # the 64 bytes behind every sequence and the 256 behind the last one are as they were; the poisoned neighbours of the
        # raw buffer (0xEE in front, 0xFF behind) reached no output: the host form never saw them
        assert rest.size == n * 64 + 256 and (rest == 0xA5).all()
        if twelve:
            assert not np.array_equal(frames[TWIN_OF], frames[n - 1])          # the same bytes under the other filter
        else:
            assert (frames[STRIPES] == 128).all()
    finally:
        cv.close()
        d.free()


@pytest.mark.parametrize("fill", ["white", "random"])
def test_wide_accumulator(fill):
    """4096 x 4200 grey: 255 Sx Sy is over 2^32, the sequence takes the 64-bit accumulators."""
    sw, sh = 4096, 4200
    s = fc.source(sw, sh, fc.GRAY8)
    raw = np.full(sw * sh, 255, np.uint8) if fill == "white" else fc.random_raw(s, 31)
    d_raw = _lib.DeviceBuffer(raw.size)
    d_raw.upload(raw)
    try:
        for ow, oh in ((7, 5), (320, 240)):
            want = convert.convert_frame_host(s, raw, ow, oh, filter="area")
            if fill == "white":
                assert (want == 255).all()
            d_out = _lib.DeviceBuffer(ow * oh + 64)
            d_out.upload(np.full(ow * oh + 64, 0xA5, np.uint8))
            cv = convert.FrameConverter(0, 1, ow, oh)
            try:
                cv.set_sources([s])
                cv.set_filters("area")
                cv.convert((d_raw.ptr, raw.size), d_out)
                got = d_out.download((ow * oh + 64,), np.uint8)
                assert np.array_equal(got[:ow * oh], want.reshape(-1)), (ow, oh)
                assert (got[ow * oh:] == 0xA5).all()
            finally:
                cv.close()
                d_out.free()
    finally:
        d_raw.free()


def test_host_raw_equals_device_raw_for_an_area_batch():
    ow, oh = 33, 17
    srcs, filters, raw = _layout(MIXED[2:9], 22)
    n = len(srcs)
    want = _host(srcs, filters, raw, ow, oh).reshape(n, -1)
    d = _Dev(raw, n, ow * oh, tail=0)
    cv = convert.FrameConverter(0, n, ow, oh)
    try:
        cv.set_sources(srcs)
        cv.set_filters(filters)
        cv.convert(d.raw, d.out)
        on_device = d.result(ow * oh)[0].copy()
        d.out.upload(np.zeros(n * ow * oh, np.uint8))
        keep = cv.convert(raw, d.out)                        # host memory: staged on the stream
        from_host = d.result(ow * oh)[0].copy()
        del keep
        assert np.array_equal(on_device, want) and np.array_equal(from_host, want)
    finally:
        cv.close()
        d.free()


def test_a_queued_conversion_keeps_its_filters():
    ow, oh = 33, 17
    srcs, _, raw = _layout(MIXED[4:10], 23)
    n = len(srcs)
    first = _host(srcs, [LIN] * n, raw, ow, oh).reshape(n, -1)
    second = _host(srcs, [AREA] * n, raw, ow, oh).reshape(n, -1)
    assert not np.array_equal(first[0], second[0])
    d1, d2 = _Dev(raw, n, ow * oh, tail=0), _lib.DeviceBuffer(n * ow * oh)
    cv = convert.FrameConverter(0, n, ow, oh)
    try:
        cv.set_sources(srcs)
        cv.convert(d1.raw, d1.out)
        cv.set_filters([AREA] * n)                           # queued behind nothing the caller waited for
        cv.convert(d1.raw, d2)
        assert np.array_equal(d1.result(ow * oh)[0], first)
        assert np.array_equal(d2.download((n, ow * oh), np.uint8), second)
    finally:
        cv.close()
        d1.free()
        d2.free()


def test_refusals_happen_on_the_host_name_the_sequence_and_change_nothing():
    ow, oh = 33, 17
    specs = [MIXED[3], MIXED[5], MIXED[8], MIXED[10]]          # 31 x 17 (narrower than the output), 961 x 18, 33 x 17, 160 x 120
    srcs, _, raw = _layout(specs, 24)
    filters = [LIN, AREA, AREA, LIN]
    want = _host(srcs, filters, raw, ow, oh).reshape(4, -1)
    d = _Dev(raw, 4, ow * oh, tail=0)
    cv = convert.FrameConverter(0, 4, ow, oh)
    L = _lib.load()

    def refused(fn, text):
        with pytest.raises(_lib.Sl2Error) as ei:
            fn()
        assert ei.value.code == _lib.SL2_ERR_INVALID and text in str(ei.value), str(ei.value)
        # nothing changed: the filters, the sources, and what a conversion gives
        assert cv.get_filters() == filters
        assert [(g["width"], g["height"], g["pitch"], g["format"], g["offset"]) for g in cv.get_sources()] == \
            [(s["width"], s["height"], s["pitch"], s["format"], s["offset"]) for s in srcs]
        d.out.upload(np.full(4 * ow * oh, 0xA5, np.uint8))
        cv.convert(d.raw, d.out)
        assert np.array_equal(d.result(ow * oh)[0], want)

    try:
        cv.set_sources(srcs)
        cv.set_filters(filters)
        refused(lambda: cv.set_filters([LIN, LIN, 2]), "sequence 2")                      # an unknown id: the two before it stay too
        refused(lambda: cv.set_filters([-1], seq0=3), "sequence 3")
        refused(lambda: cv.set_filters([LIN, AREA], seq0=3), "sequence")                  # a range past the converter
        refused(lambda: cv.set_filters([AREA], seq0=-1), "sequence")
        refused(lambda: cv.set_filters([LIN, LIN, LIN, LIN, LIN]), "sequence")
        refused(lambda: cv.set_filters([AREA, LIN, LIN, AREA]), "sequence 0")             # 31 wide: narrower than 33
        refused(lambda: cv.set_sources([dict(srcs[0])], seq0=1), "sequence 1")            # the same source under a sequence that is AREA
        refused(lambda: cv.set_sources([fc.source(40, 16, fc.GRAY8, 0, 0)], seq0=2), "sequence 2")      # lower than 17
        refused(lambda: cv.set_sources([srcs[3], fc.source(32, 17, fc.GRAY8, 0, 0)], seq0=0), "sequence 1")
        assert L.sl2_converter_set_filters(cv.h, 0, 1, None) == _lib.SL2_ERR_INVALID
        assert L.sl2_converter_get_filters(cv.h, 0, 1, None) == _lib.SL2_ERR_INVALID
        one = (C.c_int32 * 1)(AREA)
        assert L.sl2_converter_set_filters(None, 0, 1, one) == _lib.SL2_ERR_INVALID
        assert L.sl2_converter_get_filters(cv.h, 3, 2, (C.c_int32 * 2)()) == _lib.SL2_ERR_INVALID
        refused(lambda: _lib.check(L.sl2_converter_set_filters(cv.h, 4, 1, one), L), "sequence 4")
        cv.set_filters([LIN], seq0=1)                                                     # and a linear sequence takes the small source
        cv.set_sources([dict(srcs[0])], seq0=1)
    finally:
        cv.close()
        d.free()


def test_python_adapter_steps_on_area_reduced_frames():
    """MonoSLAM.SetFrameSource(1280, 960, 1280, "gray8") + SetFrameFilter("area"): every 320 x 240 synthetic frame enlarged by
    np.kron to 4 x 4 blocks.  The box average of a block is its pixel, so GoOneStepRaw steps on exactly the frames GoOneStep is
    given, and both filters end in the same state to the digit."""
    from scenelib2_amd import MonoSLAM
    from slam_helpers import Pair
    pr = Pair(12, 3, batch=1, make_engine=False)
    spec = pr.specs[0]
    slams = []
    for _ in range(2):
        m = MonoSLAM(max_features=12).InitFromValues(pr.cam, pr.params, spec.xv0, spec.Pxx0)
        for i in range(spec.feat_y.shape[0]):
            m.AddNewKnownFeature(spec.feat_y[i], spec.poses[0], pr.templates[0][i])
        slams.append(m)
    raw_slam, ref_slam = slams
    w, h = pr.cam["width"], pr.cam["height"]
    assert (w, h) == (320, 240)
    raw_slam.SetFrameFilter("area")                              # before the source ...
    raw_slam.SetFrameSource(1280, 960, 1280, "gray8")
    raw_slam.SetFrameFilter("linear")
    raw_slam.SetFrameFilter("area")                              # ... and after it
    assert raw_slam._converter.get_filters() == [AREA]
    with pytest.raises(ValueError):
        raw_slam.SetFrameFilter("cubic")
    with pytest.raises(_lib.Sl2Error):
        raw_slam.SetFrameSource(160, 120, 160, "gray8")          # area only reduces
    for k in range(3):
        big = np.kron(pr.frames[0][k], np.ones((4, 4), np.uint8))
        assert big.shape == (960, 1280)
        assert np.array_equal(convert.convert_frame_host(fc.source(1280, 960, fc.GRAY8), big, w, h, filter="area"), pr.frames[0][k])
        assert raw_slam.GoOneStepRaw(big) is True
        ref_slam.GoOneStep(pr.frames[0][k])
        xa, Pa = raw_slam._engine.get_vehicle_state()
        xb, Pb = ref_slam._engine.get_vehicle_state()
        assert np.isfinite(xa).all() and np.array_equal(xa, xb) and np.array_equal(Pa, Pb), k
