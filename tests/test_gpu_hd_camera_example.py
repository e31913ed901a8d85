"""examples/hd_camera_monoslam.cpp end to end on a GPU: a 1280 x 960 UYVY and a 1920 x 1440 RGB24 camera, each in the batch once
under SL2_RESIZE_LINEAR and once under SL2_RESIZE_AREA, beside one control rendered directly at 320 x 240.  A demonstration: the
test checks that it builds, runs and prints finite numbers, that the printed calibrations are sl2_scale_camera's, that no status
flag is set and that every converted sequence keeps measuring.  The position errors are printed side by side; no bound is set on
them or on which filter wins.

Measured on an MI355X (--steps 12), position error in metres, LINEAR | AREA (the control, rendered at 320 x 240: 0.002220):
1280 x 960 UYVY 0.002333 | 0.002342; 1920 x 1440 RGB24 0.002333 | 0.002362 (all five sequences: 12 visible, 10 selected, 20
measured, no status flag)."""
import math
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^sequence (\d)  source (\d+)x(\d+) (\S+)  filter (\S+)  fku (\S+) fkv (\S+) u0 (\S+) v0 (\S+) kd1 (\S+) sd (\d+)  "
                  r"position error (\S+) m  visible (\d+)  selected (\d+)  measured (\d+)  flags (\d+)")
ENGINE_CAM = dict(width=320, height=240, fku=195.0, fkv=195.0, u0=162.0, v0=125.0, kd1=9e-06, sd=1)


def _source_camera(width, height):
    k = width / ENGINE_CAM["width"]
    return dict(width=width, height=height, fku=ENGINE_CAM["fku"] * k, fkv=ENGINE_CAM["fkv"] * k, u0=(ENGINE_CAM["u0"] + 0.5) * k - 0.5,
                v0=(ENGINE_CAM["v0"] + 0.5) * k - 0.5, kd1=ENGINE_CAM["kd1"] / (k * k), sd=1)


def test_hd_camera_example_builds_runs_and_every_sequence_keeps_measuring():
    from scenelib2_amd import convert
    exe = os.path.join(ROOT, "examples", "hd_camera_monoslam")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    out = subprocess.run([exe, "--steps", "12"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    rows = {}
    for line in out.stdout.split("\n"):
        m = LINE.match(line)
        if m:
            rows[int(m.group(1))] = m.groups()
    assert sorted(rows) == [0, 1, 2, 3, 4], out.stdout
    expect = {0: (1280, 960, "UYVY", "LINEAR"), 1: (1280, 960, "UYVY", "AREA"), 2: (1920, 1440, "RGB24", "LINEAR"),
              3: (1920, 1440, "RGB24", "AREA"), 4: (320, 240, "GRAY8", "NONE")}
    for seq, g in rows.items():
        w, h, name, flt = expect[seq]
        assert (int(g[1]), int(g[2]), g[3], g[4]) == (w, h, name, flt)
        want = convert.scale_camera(_source_camera(w, h), 320, 240)
        got = [float(v) for v in g[5:10]]
        assert all(math.isfinite(v) for v in got + [float(g[11])]), g
        for v, key in zip(got, ("fku", "fkv", "u0", "v0")):
            assert abs(v - want[key]) <= 1e-6 and abs(v - ENGINE_CAM[key]) <= 1e-6, (seq, key, v)      # (%.6f)
        assert abs(got[4] - want["kd1"]) <= 1e-12 and int(g[10]) == want["sd"] == 1
        assert int(g[15]) == 0 and int(g[14]) >= 1, g              # no status flag; at least one feature measured in the last step
        print("sequence %d (%dx%d %s, %s): position error %s m, visible %s selected %s measured %s" % (seq, w, h, name, flt, g[11], g[12], g[13], g[14]))
