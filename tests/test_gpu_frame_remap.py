"""k_convert_remap on the GPU: every case of frame_remap_cases.py - all twelve formats, every pitch and offset class, the edge
maps, both device forms of a map - byte for byte against the host form (which tests/test_frame_remap_host.py holds to the
definition), from a device and from a host raw buffer; the bytes around the outputs; mapped and unmapped sequences of every
kernel family in one call; replacing a map; taking it away again; the refusals of the device setters; the example.  A converter has ONE
output size, so the table goes through one converter per output size (five), each holding all its cases as the sequences of
one batch, every sequence with a map slot of its own: one sl2_convert_frames call checks them all."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import frame_convert_cases as fc
import frame_convert_raw_cases as rc
import frame_remap_cases as rm
from frame_convert_raw_cases import AREA, LINEAR

from scenelib2_amd import _lib, convert

pytestmark = pytest.mark.gpu

LEAD = 16          # poison in front of the raw buffer on the device: a multiple of 16 keeps every case's head length class


def _layout(specs, seed):
    """(width, height, format, pitch pad, offset) sources one after the other, each from a 16-byte boundary plus its own offset,
    in one raw buffer of exactly the bytes they reach, every byte random."""
    srcs, total = [], 0
    for w, h, fmt, pad, off in specs:
        base = (total + 15) & ~15
        s = dict(width=w, height=h, pitch=w * rm.BPP[fmt] + pad, format=fmt, offset=base + off)
        total = rm.source_bytes(s)
        srcs.append(s)
    return srcs, np.random.default_rng(seed).integers(0, 256, total, dtype=np.uint8)


@pytest.fixture(scope="module")
def table():
    """out size -> (sources, maps, raw, what the host form gives [n][out_h * out_w]), computed once."""
    t = {}
    for out in rm.OUT_SIZES:
        mine = [c for c in rm.CASES if c[0] == out]
        srcs, raw = _layout([(c[1][0], c[1][1], c[2], c[4], c[5]) for c in mine], 50 + out[0])
        maps = [rm.make_map(c[3], out[0], out[1], c[1][0], c[1][1], c[6] + 1) for c in mine]          # case_inputs' maps
        want = np.stack([convert.remap_frame_host(s, m, raw).reshape(-1) for s, m in zip(srcs, maps)])
        want.setflags(write=False)
        t[out] = (srcs, maps, raw, want)
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


def _assert_frames(frames, want, what):
    for i in range(len(want)):
        diff = np.flatnonzero(frames[i] != want[i])
        assert diff.size == 0, "sequence %d (%s): %d bytes differ, first at %d" % (i, what[i], diff.size, diff[0])


@pytest.mark.parametrize("raw_on_device", [1, 0])
@pytest.mark.parametrize("out", rm.OUT_SIZES)
def test_whole_table_equals_the_host_form_and_touches_nothing_else(table, out, raw_on_device):
    ow, oh = out
    srcs, maps, raw, want = table[out]
    n = len(srcs)
    stride = ow * oh + 37
    d = _Dev(raw, n, stride)
    cv = convert.FrameConverter(0, n, ow, oh)
    try:
        assert cv.get_remaps() == [-1] * n
        cv.set_sources(srcs)
        for i, (s, m) in enumerate(zip(srcs, maps)):
            cv.set_map(i, s["width"], s["height"], m)
        cv.set_remaps(list(range(n)))
        assert cv.get_remaps() == list(range(n))
        keep = cv.convert(d.raw if raw_on_device else raw, d.out, seq_stride=stride)
        frames, rest = d.result(ow * oh)
        del keep
        _assert_frames(frames, want, srcs)
        # the 37 bytes behind every sequence and the 256 behind the last one are as they were; the poisoned neighbours of the raw
        # buffer (0xEE in front, 0xFF behind) reached no output: the host form never saw them
        assert rest.size == n * 37 + 256 and (rest == 0xA5).all()
    finally:
        cv.close()
        d.free()


def _filtered(s, raw, ow, oh, flt):
    return convert.convert_frame_host(s, raw, ow, oh, filter="area" if flt == AREA else "linear").reshape(-1)


def test_mixed_batch_replaced_map_and_the_way_back_to_the_filter():
    """One call with a mapped GRAY8, a mapped Bayer and a mapped GRAY12 sequence, unmapped LINEAR, AREA and raw-format ones, and
    two sequences of different formats on one slot; the unmapped ones keep the bytes of a converter that has no maps at all;
    replacing a slot's map changes the next call only; set_remaps(-1) brings the filter's bytes back."""
    ow, oh = 64, 48
    W, H = 130, 100
    #        w, h, format, pad, offset, filter, slot
    specs = [(W, H, fc.GRAY8, 1, 7, LINEAR, 0),               # mapped GRAY8
             (W, H, fc.RGB24, 0, 1, LINEAR, -1),              # unmapped LINEAR
             (W, H, rc.BAYER_GRBG8, 13, 15, AREA, 1),         # mapped Bayer: its AREA filter is ignored
             (200, 150, fc.UYVY, 0, 0, AREA, -1),             # unmapped AREA
             (W, H, rc.GRAY12, 2, 14, LINEAR, 2),             # mapped GRAY12
             (97, 61, rc.BAYER_RGGB8, 1, 1, LINEAR, -1),      # unmapped raw format, LINEAR
             (W, H, fc.YUYV, 1, 0, LINEAR, 3),                # two formats ...
             (W, H, rc.BAYER_BGGR8, 0, 7, LINEAR, 3),         # ... on one slot
             (140, 99, rc.GRAY16, 0, 2, AREA, -1)]            # unmapped raw format, AREA
    srcs, raw = _layout([sp[:5] for sp in specs], 91)
    filters, slots = [sp[5] for sp in specs], [sp[6] for sp in specs]
    n = len(specs)
    target = rm.camera(ow, oh, 40.0, 40.0, 31.5, 23.5, 4e-4)          # f <= 0 in the corners: border entries
    maps = [convert.lens_map(rm.lens(rm.BROWN, W, H, 70.0, 71.0, 64.0, 50.0, [-0.2, 0.05, 1e-3, -1e-3, 0.0]), target),
            rm.make_map("random", ow, oh, W, H, 5),
            convert.lens_map(rm.lens(rm.FISHEYE, W, H, 45.0, 45.0, 64.5, 49.5, [-0.02, 0.004]), target),
            rm.make_map("shift", ow, oh, W, H, 6)]
    other = convert.lens_map(rm.lens(rm.RADIAL1, W, H, 80.0, 80.0, 60.0, 52.0, [2e-5]), target)
    assert (maps[0][..., 0] == rm.BORDER).any() and not np.array_equal(maps[0], other)

    def expected(slot_maps, sl):
        return np.stack([convert.remap_frame_host(s, slot_maps[k], raw).reshape(-1) if k >= 0 else _filtered(s, raw, ow, oh, f)
                         for s, f, k in zip(srcs, filters, sl)])

    want = expected(maps, slots)
    plain = expected(maps, [-1] * n)
    unmapped = np.array([k < 0 for k in slots])
    assert all(not np.array_equal(want[i], plain[i]) for i in range(n) if slots[i] >= 0)
    stride = ow * oh + 5
    d = _Dev(raw, n, stride)
    d_plain = _Dev(raw, n, ow * oh, tail=0)
    cv = convert.FrameConverter(0, n, ow, oh)
    cv_plain = convert.FrameConverter(0, n, ow, oh)
    try:
        for k, m in enumerate(maps):
            cv.set_map(k, W, H, m)
        cv.set_filters(filters)
        cv.set_remaps(slots)                     # before the sources: the sizes are checked when those arrive
        cv.set_sources(srcs)
        assert cv.get_remaps() == slots and cv.get_filters() == filters
        cv.convert(d.raw, d.out, seq_stride=stride)
        frames, rest = d.result(ow * oh)
        _assert_frames(frames, want, specs)
        assert (rest == 0xA5).all()
        # a converter that has no maps at all gives the unmapped sequences the same bytes
        cv_plain.set_sources(srcs)
        cv_plain.set_filters(filters)
        cv_plain.convert(d_plain.raw, d_plain.out)
        got_plain = d_plain.result(ow * oh)[0]
        _assert_frames(got_plain, plain, specs)
        assert np.array_equal(got_plain[unmapped], frames[unmapped])
        # slot 0 replaced between two calls, the first of them still queued: that call keeps its map, the next has the new one
        d.fill()
        cv.convert(d.raw, d.out, seq_stride=stride)
        cv.set_map(0, W, H, other)
        assert np.array_equal(d.result(ow * oh)[0], want)
        d.fill()
        cv.convert(d.raw, d.out, seq_stride=stride)
        _assert_frames(d.result(ow * oh)[0], expected([other] + maps[1:], slots), specs)
        # from a host raw buffer
        d.fill()
        keep = cv.convert(raw, d.out, seq_stride=stride)
        _assert_frames(d.result(ow * oh)[0], expected([other] + maps[1:], slots), specs)
        del keep
        # -1 brings the filter's bytes back (AREA for sequence 2), and the emptied slot can be filled again
        cv.set_remaps([-1, -1, -1], seq0=0)
        cv.set_remaps(-1, seq0=4)
        assert cv.get_remaps() == [-1, -1, -1, -1, -1, -1, 3, 3, -1] and cv.get_filters() == filters
        cv.set_map(0)
        d.fill()
        cv.convert(d.raw, d.out, seq_stride=stride)
        back = d.result(ow * oh)[0]
        _assert_frames(back, expected(maps, [-1, -1, -1, -1, -1, -1, 3, 3, -1]), specs)
        assert np.array_equal(back[:6], plain[:6]) and np.array_equal(back[8], plain[8])
        cv.set_remaps([-1, -1], seq0=6)
        d.fill()
        cv.convert(d.raw, d.out, seq_stride=stride)
        assert np.array_equal(d.result(ow * oh)[0], plain)
    finally:
        cv.close()
        cv_plain.close()
        d.free()
        d_plain.free()


def test_device_setters_refuse_with_the_sequence_named_and_change_nothing():
    ow, oh = 16, 8
    specs = [(33, 17, fc.GRAY8, 1, 1), (33, 17, rc.BAYER_GBRG8, 0, 7), (47, 17, fc.BGR24, 13, 0), (33, 17, rc.GRAY10, 2, 2)]
    srcs, raw = _layout(specs, 92)
    n = len(srcs)
    m33, m47 = rm.make_map("random", ow, oh, 33, 17, 1), rm.make_map("random", ow, oh, 47, 17, 2)
    slots = [0, 0, 1, -1]
    want = np.stack([convert.remap_frame_host(srcs[0], m33, raw).reshape(-1), convert.remap_frame_host(srcs[1], m33, raw).reshape(-1),
                     convert.remap_frame_host(srcs[2], m47, raw).reshape(-1), _filtered(srcs[3], raw, ow, oh, LINEAR)])
    d = _Dev(raw, n, ow * oh, tail=0)
    cv = convert.FrameConverter(0, n, ow, oh)

    def refused(fn, *texts):
        with pytest.raises(_lib.Sl2Error) as ei:
            fn()
        assert ei.value.code == _lib.SL2_ERR_INVALID and all(t in str(ei.value) for t in texts), str(ei.value)
        assert cv.get_remaps() == slots and [g["width"] for g in cv.get_sources()] == [s["width"] for s in srcs]
        d.fill()
        cv.convert(d.raw, d.out)
        assert np.array_equal(d.result(ow * oh)[0], want)

    try:
        cv.set_sources(srcs)
        cv.set_map(0, 33, 17, m33)
        cv.set_map(1, 47, 17, m47)
        cv.set_remaps(slots)
        refused(lambda: cv.set_remaps([1, 2], seq0=2), "sl2_converter_set_remaps", "sequence 3", "empty")                 # an empty slot
        refused(lambda: cv.set_remaps([1], seq0=3), "sequence 3", "another size")                                          # the map's size
        refused(lambda: cv.set_remaps([-1, 0], seq0=1), "sequence 2", "another size")                                      # nothing of the range changed
        refused(lambda: cv.set_remaps([4], seq0=0), "sequence 0", "slot outside")
        refused(lambda: cv.set_remaps([-2], seq0=0), "sequence 0", "slot outside")
        refused(lambda: cv.set_remaps([0], seq0=4), "outside the converter")
        refused(lambda: cv.set_sources([rm.source(47, 17, fc.GRAY8)], seq0=1), "sl2_converter_set_sources", "sequence 1", "another source size")
        refused(lambda: cv.set_sources([srcs[3], rm.source(33, 18, fc.GRAY8)], seq0=1), "sequence 2", "another source size")
        refused(lambda: cv.set_map(0), "sl2_converter_set_map", "sequence 0", "emptied")                                  # a slot in use
        refused(lambda: cv.set_map(1, 47, 18, m47), "sequence 2", "size would change")
        refused(lambda: cv.set_map(4, 33, 17, m33), "slot outside")
        refused(lambda: cv.set_map(-1, 33, 17, m33), "slot outside")
        for w, h in ((0, 17), (33, 0), (4097, 17), (33, 16385)):
            refused(lambda: cv.set_map(3, w, h, m33), "source size")
        cv.set_map(3, 4096, 16384, m33)                                   # the caps themselves pass; an unused slot may be anything ...
        cv.set_map(3)                                                     # ... and may be emptied, twice
        cv.set_map(3)
        cv.set_map(1, 47, 17, m33)                                        # the same size: a slot in use may be replaced
        cv.set_sources([dict(srcs[0], format=fc.GRAY8)], seq0=0)          # a source of the map's size is accepted
        d.fill()
        cv.convert(d.raw, d.out)
        got = d.result(ow * oh)[0]
        assert np.array_equal(got[2], convert.remap_frame_host(srcs[2], m33, raw).reshape(-1)) and np.array_equal(got[[0, 1, 3]], want[[0, 1, 3]])
    finally:
        cv.close()
        d.free()


EXAMPLE_LINE = re.compile(r"^sequence (\d)  source (\d+)x(\d+) (\S+)  map (\S+)  fku (\S+) fkv (\S+) u0 (\S+) v0 (\S+) kd1 (\S+) sd (\d+)  "
                          r"position error (\S+) m  visible (\d+)  selected (\d+)  measured (\d+)  flags (\d+)")


def test_lens_remap_example_builds_runs_and_every_sequence_keeps_measuring():
    """examples/lens_remap_monoslam.cpp end to end: a 640 x 480 camera under a strongly distorting RADIAL1 lens, remapped into a
    pinhole and into a mild-kd1 target, beside a control rendered directly under each target at 320 x 240.  A demonstration: the
    test checks that it builds, runs and prints finite numbers, that the printed calibrations are sl2_lens_pinhole_camera's (and
    the mild-kd1 variant), that no status flag is set and that every sequence keeps measuring.  The position errors are printed
    side by side; no bound is set on them."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "lens_remap_monoslam")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(root, "examples")])
    out = subprocess.run([exe, "--steps", "12"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    rows = {}
    for line in out.stdout.split("\n"):
        m = EXAMPLE_LINE.match(line)
        if m:
            rows[int(m.group(1))] = m.groups()
    assert sorted(rows) == [0, 1, 2, 3], out.stdout
    assert "lens RADIAL1 640x480 fx 390.000000 fy 390.000000 cx 324.000000 cy 250.000000 k0 2.000000e-06" in out.stdout
    pin = convert.pinhole_camera(rm.lens(rm.RADIAL1, 640, 480, 390.0, 390.0, 324.0, 250.0, [2e-6]), 320, 240, sd=1)
    assert (pin["fku"], pin["fkv"], pin["u0"], pin["v0"], pin["kd1"]) == (195.0, 195.0, 161.75, 124.75, 0.0)
    expect = {0: (640, 480, "PINHOLE", 0.0), 1: (640, 480, "RADIAL", 3e-6), 2: (320, 240, "NONE", 0.0), 3: (320, 240, "NONE", 3e-6)}
    for seq, g in rows.items():
        w, h, name, kd1 = expect[seq]
        assert (int(g[1]), int(g[2]), g[3], g[4]) == (w, h, "GRAY8", name)
        got = [float(v) for v in g[5:10]]
        assert all(math.isfinite(v) for v in got + [float(g[11])]), g
        for v, key in zip(got, ("fku", "fkv", "u0", "v0")):
            assert abs(v - pin[key]) <= 1e-6, (seq, key, v)      # (%.6f)
        assert abs(got[4] - kd1) <= 1e-12 and int(g[10]) == 1
        assert int(g[15]) == 0 and int(g[14]) >= 1, g              # no status flag; at least one feature measured in the last step


def test_python_adapter_steps_on_remapped_frames_under_the_target_camera():
    """MonoSLAM.SetLens(lens, target) + SetFrameSource + GoOneStepRaw against a second MonoSLAM given SetCameraParameters(target)
    and the frames sl2_remap_frame_host makes of the same bytes: the same state to the digit, and the camera is the target."""
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
    ln = rm.lens(rm.BROWN, 2 * w, 2 * h, 2 * pr.cam["fku"], 2 * pr.cam["fkv"], 2 * pr.cam["u0"] + 0.5, 2 * pr.cam["v0"] + 0.5, [-0.03, 0.004, 2e-4, -1e-4])
    target = dict(pr.cam, kd1=pr.cam["kd1"] * 0.5, sd=pr.cam["sd"])
    with pytest.raises(ValueError):
        raw_slam.SetLens(ln, dict(target, width=w + 1))
    raw_slam.SetLens(ln, target)                                 # before the source ...
    raw_slam.SetFrameSource(2 * w, 2 * h, 2 * w + 3, "gray8")
    with pytest.raises(_lib.Sl2Error):
        raw_slam.SetFrameSource(w, h, w, "gray8")                # not the lens's size
    raw_slam.SetLens(ln, target)                                 # ... and after it
    assert raw_slam._converter.get_remaps() == [0] and raw_slam.camera_["kd1"] == target["kd1"]
    assert raw_slam._engine.get_cameras()[0]["kd1"] == target["kd1"]
    ref_slam.SetCameraParameters(w, h, target["fku"], target["fkv"], target["u0"], target["v0"], target["kd1"], target["sd"])
    xy = convert.lens_map(ln, target)
    s = dict(width=2 * w, height=2 * h, pitch=2 * w + 3, format=fc.GRAY8, offset=0)
    for k in range(3):
        big = np.zeros((2 * h, 2 * w + 3), np.uint8)
        big[:, :2 * w] = np.kron(pr.frames[0][k], np.ones((2, 2), np.uint8))
        raw = big.reshape(-1)[:rm.source_bytes(s)]
        assert raw_slam.GoOneStepRaw(raw) is True
        ref_slam.GoOneStep(convert.remap_frame_host(s, xy, raw))
        xa, Pa = raw_slam._engine.get_vehicle_state()
        xb, Pb = ref_slam._engine.get_vehicle_state()
        assert np.isfinite(xa).all() and np.array_equal(xa, xb) and np.array_equal(Pa, Pb), k
