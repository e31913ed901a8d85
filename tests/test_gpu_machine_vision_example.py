"""examples/machine_vision_monoslam.cpp end to end on a GPU: a 640 x 480 BAYER_RGGB8 camera under SL2_RESIZE_LINEAR, a 1280 x 960
BAYER_GRBG8 and a 1280 x 960 GRAY12 camera under SL2_RESIZE_AREA, beside one control rendered directly at 320 x 240.  A
demonstration: the test checks that it builds, runs and prints finite numbers, that the printed calibrations are
sl2_scale_camera's, that no status flag is set and that every sequence keeps measuring.  No bound is set on the position errors.

Measured on an MI355X (--steps 12), position error in metres (the control, rendered at 320 x 240: 0.002220): 640 x 480
BAYER_RGGB8 LINEAR 0.002342; 1280 x 960 BAYER_GRBG8 AREA 0.002342; 1280 x 960 GRAY12 AREA 0.002342 (all four sequences: 12 visible,
10 selected, 20 measured, no status flag)."""
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


def test_machine_vision_example_builds_runs_and_every_sequence_keeps_measuring():
    from scenelib2_amd import convert
    exe = os.path.join(ROOT, "examples", "machine_vision_monoslam")
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
    assert sorted(rows) == [0, 1, 2, 3], out.stdout
    expect = {0: (640, 480, "BAYER_RGGB8", "LINEAR"), 1: (1280, 960, "BAYER_GRBG8", "AREA"), 2: (1280, 960, "GRAY12", "AREA"),
              3: (320, 240, "GRAY8", "NONE")}
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
