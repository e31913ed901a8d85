"""k_convert_frames on the GPU: sequences of every source size, pitch, offset and pixel format in one launch, byte for byte against
sl2_convert_frame_host (which tests/test_frame_convert_host.py holds to the definition); the bytes around the outputs and the raw
buffer; host and device raw buffers; new sources between calls; and a batch stepped on device-converted frames."""
import numpy as np
import pytest

import frame_convert_cases as fc

from scenelib2_amd import _lib, convert

pytestmark = pytest.mark.gpu

# (width, height, format, pitch padding, bytes skipped in front): every format, aligned and unaligned rows
MIXED = [(640, 480, fc.UYVY, 0, 1), (961, 3, fc.RGB24, 1, 0), (4096, 2, fc.YUYV, 13, 7), (321, 241, fc.BGR24, 1, 1),
         (1, 1, fc.GRAY8, 0, 7), (2, 2, fc.UYVY, 13, 0), (5, 3, fc.RGB24, 0, 1), (31, 17, fc.GRAY8, 13, 7),
         (322, 242, fc.YUYV, 1, 0), (160, 120, fc.BGR24, 13, 1), (320, 240, fc.GRAY8, 0, 0)]
SIX = [(640, 480, fc.UYVY, 0, 0), (960, 720, fc.RGB24, 0, 0), (321, 241, fc.BGR24, 0, 3), (160, 120, fc.GRAY8, 0, 1),
       (4096, 2, fc.YUYV, 0, 0), (320, 240, fc.GRAY8, 32, 0)]


def _layout(specs, seed, twin_of_first=False):
    """The sources one after the other in one raw buffer of exactly the bytes they reach, every byte random."""
    srcs, total = [], 0
    for w, h, fmt, pad, gap in specs:
        s = fc.source(w, h, fmt, pad, total + gap)
        total = fc.source_bytes(s)
        srcs.append(s)
    if twin_of_first:
        srcs.append(dict(srcs[0]))          # a second sequence that names the first one's bytes
    raw = np.random.default_rng(seed).integers(0, 256, total, dtype=np.uint8)
    return srcs, raw


def _host(srcs, raw, ow, oh):
    return np.stack([convert.convert_frame_host(s, raw, ow, oh) for s in srcs])


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


@pytest.mark.parametrize("specs,ow,oh,twin", [(MIXED, 33, 17, True), (SIX, 320, 240, False)], ids=["twelve-to-33x17", "six-to-320x240"])
def test_mixed_launch_equals_the_host_form_and_touches_nothing_else(specs, ow, oh, twin):
    srcs, raw = _layout(specs, 11, twin_of_first=twin)
    n = len(srcs)
    assert n == (12 if twin else 6)
    want = _host(srcs, raw, ow, oh)
    stride = ow * oh + 64
    d = _Dev(raw, n, stride)
    cv = convert.FrameConverter(0, n, ow, oh)
    try:
        cv.set_sources(srcs)
        got_src = cv.get_sources()
        assert [(g["width"], g["height"], g["pitch"], g["format"], g["offset"]) for g in got_src] == \
            [(s["width"], s["height"], s["pitch"], s["format"], s["offset"]) for s in srcs]
        cv.convert(d.raw, d.out, seq_stride=stride)
        frames, rest = d.result(ow * oh)
        for i in range(n):
            diff = np.flatnonzero(frames[i] != want[i].reshape(-1))
            assert diff.size == 0, "sequence %d (%s): %d bytes differ, first at %d" % (i, srcs[i], diff.size, diff[0])
        # the 64 bytes behind every sequence and the 256 behind the last one are as they were; the poisoned neighbours of the
        # raw buffer (0xEE in front, 0xFF behind) reached no output: the host form never saw them
        assert rest.size == n * 64 + 256 and (rest == 0xA5).all()
        if twin:
            assert np.array_equal(frames[0], frames[n - 1])
    finally:
        cv.close()
        d.free()


def test_host_raw_equals_device_raw_and_the_staging_buffer_grows():
    ow, oh = 33, 17
    srcs, raw = _layout(MIXED[3:8], 12)
    n = len(srcs)
    want = _host(srcs, raw, ow, oh).reshape(n, -1)
    d = _Dev(raw, n, ow * oh, tail=0)
    cv = convert.FrameConverter(0, n, ow, oh)
    try:
        cv.set_sources(srcs)
        cv.convert(d.raw, d.out)
        on_device = d.result(ow * oh)[0].copy()
        d.out.upload(np.zeros(n * ow * oh, np.uint8))
        keep = cv.convert(raw, d.out)                        # host memory: staged on the stream
        from_host = d.result(ow * oh)[0].copy()
        assert np.array_equal(on_device, want) and np.array_equal(from_host, want)
        bigger = np.concatenate([raw, np.full(100000, 0x5A, np.uint8)])      # a larger raw buffer: the staging buffer grows
        d.out.upload(np.zeros(n * ow * oh, np.uint8))
        keep = cv.convert(bigger, d.out)
        assert np.array_equal(d.result(ow * oh)[0], want)
        d.out.upload(np.zeros(n * ow * oh, np.uint8))
        keep = cv.convert(raw, d.out)                        # and a smaller one again fits what is there
        assert np.array_equal(d.result(ow * oh)[0], want)
        del keep
    finally:
        cv.close()
        d.free()


def test_set_sources_between_calls_leaves_the_queued_conversion_its_tables():
    ow, oh = 33, 17
    srcs, raw = _layout(MIXED[3:10], 13)
    n = len(srcs)
    # three sequences then read OTHER sequences' bytes as something else: sizes that stay inside the same raw buffer
    later = [dict(s) for s in srcs]
    later[0] = dict(srcs[6], format=fc.RGB24)                               # 160 x 120: BGR24 -> RGB24
    later[2] = fc.source(14, 16, fc.UYVY, 0, srcs[4]["offset"] + 1)         # inside the 31 x 17 grey source, on its 44-byte pitch
    later[2]["pitch"] = 44
    later[5] = fc.source(107, 241, fc.BGR24, 0, srcs[0]["offset"])          # a third of the 321-pixel rows
    later[5]["pitch"] = srcs[0]["pitch"]
    first, second = _host(srcs, raw, ow, oh).reshape(n, -1), _host(later, raw, ow, oh).reshape(n, -1)
    assert not np.array_equal(first[0], second[0]) and not np.array_equal(first[5], second[5])
    d1, d2 = _Dev(raw, n, ow * oh, tail=0), _lib.DeviceBuffer(n * ow * oh)
    cv = convert.FrameConverter(0, n, ow, oh)
    try:
        cv.set_sources(srcs)
        cv.convert(d1.raw, d1.out)
        cv.set_sources([later[0]], seq0=0)                   # queued behind nothing the caller waited for
        cv.set_sources([later[2]], seq0=2)
        cv.set_sources([later[5]], seq0=5)
        cv.convert(d1.raw, d2)
        assert np.array_equal(d1.result(ow * oh)[0], first)
        assert np.array_equal(d2.download((n, ow * oh), np.uint8), second)
    finally:
        cv.close()
        d1.free()
        d2.free()


def test_refusals_happen_on_the_host_and_name_the_sequence():
    ow, oh = 33, 17
    srcs, raw = _layout(MIXED[4:8], 14)
    d = _Dev(raw, 4, ow * oh, tail=0)
    cv = convert.FrameConverter(0, 4, ow, oh)
    L = _lib.load()

    def refused(fn, text):
        with pytest.raises(_lib.Sl2Error) as ei:
            fn()
        assert ei.value.code == _lib.SL2_ERR_INVALID and text in str(ei.value), str(ei.value)

    try:
        cv.set_sources(srcs[:3])
        refused(lambda: cv.convert(d.raw, d.out), "sequence 3")                               # never set
        refused(lambda: cv.get_sources(), "sequence 3")
        refused(lambda: cv.set_sources([dict(srcs[3], pitch=30)], seq0=3), "sequence 3")      # 31 grey pixels need 31 bytes
        refused(lambda: cv.set_sources([dict(srcs[3], format=9)], seq0=3), "sequence 3")
        refused(lambda: cv.set_sources([dict(srcs[1], width=3)], seq0=1), "sequence 1")       # odd width, 4:2:2
        refused(lambda: cv.set_sources([dict(srcs[3], width=4097, pitch=5000)], seq0=3), "sequence 3")
        refused(lambda: cv.set_sources([dict(srcs[3], height=0)], seq0=3), "sequence 3")
        cv.set_sources(srcs[3:], seq0=3)
        refused(lambda: cv.convert((d.raw[0], raw.size - 1), d.out), "sequence 3")            # one byte short: the last source
        refused(lambda: cv.convert(d.raw, d.out, seq_stride=ow * oh - 1), "seq_stride")
        cv.convert(d.raw, d.out)                                                              # the exact size passes
        assert np.array_equal(d.result(ow * oh)[0], _host(srcs, raw, ow, oh).reshape(4, -1))
        assert L.sl2_converter_create(0, 0, ow, oh, None) == _lib.SL2_ERR_INVALID
    finally:
        cv.close()
        d.free()


def _replicate(frame, k):
    return np.repeat(np.repeat(frame, k, axis=0), k, axis=1)


def test_stepping_on_device_converted_frames_equals_stepping_on_host_converted_ones():
    """Batch 3, 12 features, 5 steps: a 640 x 480 UYVY, a 960 x 720 RGB24 and a padded native grey camera.  The step reads the
    same bytes either way, so state, covariance and selection agree bit for bit."""
    from slam_helpers import Pair
    pr = Pair(12, 5, batch=3)
    dev_eng, host_eng = pr.engine, pr.make_engine_for(0, 3, 12)
    w, h = pr.cam["width"], pr.cam["height"]
    fb = w * h
    cv = convert.FrameConverter(0, 3, w, h)
    d_frames = _lib.DeviceBuffer(3 * fb)
    try:
        for k in range(5):
            parts = [fc.pack_grey(_replicate(pr.frames[0][k], 2), fc.UYVY, seed=k),
                     fc.pack_grey(_replicate(pr.frames[1][k], 3), fc.RGB24, seed=k),
                     fc.pack_grey(pr.frames[2][k], fc.GRAY8, pad=32, seed=k)]
            srcs, total = [], 0
            for s, r in parts:
                srcs.append(dict(s, offset=total))
                total += r.size
            raw = np.concatenate([r for _, r in parts])
            if k == 0:
                cv.set_sources(srcs)
            keep = cv.convert(raw, d_frames, stream=dev_eng.stream)
            dev_eng.go_one_step(d_frames.ptr, on_device=True)
            dev_eng.synchronize()
            del keep
            host_frames = _host(srcs, raw, w, h)
            if k == 0:          # a 2x and a 3x pixel replication resize back to the frame itself: these filters do track
                assert np.array_equal(host_frames, pr.frame_batch(k))
            host_eng.go_one_step(host_frames)
        xa, Pa = dev_eng.get_vehicle_state()
        xb, Pb = host_eng.get_vehicle_state()
        assert np.isfinite(xa).all() and np.array_equal(xa, xb) and np.array_equal(Pa, Pb)
        for b in range(3):
            assert np.array_equal(dev_eng.total_state(b), host_eng.total_state(b))
            assert np.array_equal(dev_eng.total_covariance(b), host_eng.total_covariance(b))
            sa, ca = dev_eng.selection(b)
            sb, cb = host_eng.selection(b)
            assert list(sa) == list(sb) and ca == cb and ca["measurement_size"] > 0
    finally:
        cv.close()
        d_frames.free()
        host_eng.close()


def test_python_adapter_steps_on_raw_frames():
    """MonoSLAM.SetFrameSource + GoOneStepRaw (a 640 x 480 UYVY camera, then the same camera switched to 960 x 720 BGR24) against
    GoOneStep on the host-converted frame."""
    from scenelib2_amd import MonoSLAM
    from slam_helpers import Pair
    pr = Pair(12, 4, batch=1, make_engine=False)
    spec = pr.specs[0]
    slams = []
    for _ in range(2):
        m = MonoSLAM(max_features=12).InitFromValues(pr.cam, pr.params, spec.xv0, spec.Pxx0)
        for i in range(spec.feat_y.shape[0]):
            m.AddNewKnownFeature(spec.feat_y[i], spec.poses[0], pr.templates[0][i])
        slams.append(m)
    raw_slam, ref_slam = slams
    with pytest.raises(RuntimeError):
        raw_slam.GoOneStepRaw(np.zeros(16, np.uint8))          # no source yet
    for k in range(4):
        if k == 0:
            raw_slam.SetFrameSource(640, 480, 1280, "uyvy")
        if k == 2:
            raw_slam.SetFrameSource(960, 720, 2880 + 5, convert.SL2_PIX_BGR24)
        s, raw = (fc.pack_grey(_replicate(pr.frames[0][k], 2), fc.UYVY, seed=k) if k < 2 else
                  fc.pack_grey(_replicate(pr.frames[0][k], 3), fc.BGR24, pad=5, seed=k))
        assert raw_slam.GoOneStepRaw(raw) is True
        frame = convert.convert_frame_host(s, raw, pr.cam["width"], pr.cam["height"])
        assert np.array_equal(frame, pr.frames[0][k])
        ref_slam.GoOneStep(frame)
        xa, Pa = raw_slam._engine.get_vehicle_state()
        xb, Pb = ref_slam._engine.get_vehicle_state()
        assert np.isfinite(xa).all() and np.array_equal(xa, xb) and np.array_equal(Pa, Pb), k
