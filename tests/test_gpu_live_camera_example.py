"""examples/live_camera_monoslam.cpp end to end on a GPU: a 640 x 480 UYVY, a 960 x 720 RGB24 and a padded native grey camera
converted in one launch per frame and stepped as one batch, beside three unconverted controls.  A demonstration: the test checks
that it builds, runs and prints finite numbers, that the printed calibrations are sl2_scale_camera's, that the padded native
camera ends in exactly its control's state, and that the two resized cameras keep measuring.  Their position errors are printed
beside their controls' (the same views rendered directly at 320 x 240); no bound is set on them.

Measured on an MI355X (--steps 12), position error in metres, converted | rendered directly at 320 x 240:
640 x 480 UYVY 0.002362 | 0.002220; 960 x 720 RGB24 0.002220 | 0.002220 (all six sequences: 12 visible, 10 selected, 20 measured)."""
import math
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^camera (\d)  source (\d+)x(\d+) (\S+) pitch (\d+)  fku (\S+) fkv (\S+) u0 (\S+) v0 (\S+) kd1 (\S+) sd (\d+)  "
                  r"position error (\S+) m  control (\S+) m  visible (\d+)  selected (\d+)  measured (\d+)  flags (\d+)  "
                  r"control: visible (\d+)  selected (\d+)  measured (\d+)  flags (\d+)")
ENGINE_CAM = dict(width=320, height=240, fku=195.0, fkv=195.0, u0=162.0, v0=125.0, kd1=9e-06, sd=1)


def _source_camera(width, height):
    k = width / ENGINE_CAM["width"]
    return dict(width=width, height=height, fku=ENGINE_CAM["fku"] * k, fkv=ENGINE_CAM["fkv"] * k, u0=(ENGINE_CAM["u0"] + 0.5) * k - 0.5,
                v0=(ENGINE_CAM["v0"] + 0.5) * k - 0.5, kd1=ENGINE_CAM["kd1"] / (k * k), sd=1)


def test_live_camera_example_builds_runs_and_the_native_camera_equals_its_control():
    from scenelib2_amd import convert
    exe = os.path.join(ROOT, "examples", "live_camera_monoslam")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    out = subprocess.run([exe, "--steps", "12"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    rows, states = {}, {}
    for line in out.stdout.split("\n"):
        m = LINE.match(line)
        if m:
            rows[int(m.group(1))] = m.groups()
        if line.startswith("state "):
            states[int(line.split()[1])] = line.split()[2:]
    assert sorted(rows) == [0, 1, 2] and sorted(states) == [2, 3], out.stdout
    sources = {0: (640, 480, "UYVY", 1280), 1: (960, 720, "RGB24", 2880), 2: (320, 240, "GRAY8", 352)}
    for cam, g in rows.items():
        w, h, name, pitch = sources[cam]
        assert (int(g[1]), int(g[2]), g[3], int(g[4])) == (w, h, name, pitch)
        want = convert.scale_camera(_source_camera(w, h), 320, 240)
        got = [float(v) for v in g[5:10]]
        assert all(math.isfinite(v) for v in got + [float(g[11]), float(g[12])]), g
        for v, key in zip(got, ("fku", "fkv", "u0", "v0")):
            assert abs(v - want[key]) <= 1e-6 and abs(v - ENGINE_CAM[key]) <= 1e-6, (cam, key, v)      # (%.6f)
        assert abs(got[4] - want["kd1"]) <= 1e-12 and int(g[10]) == want["sd"] == 1
        assert int(g[16]) == 0 and int(g[15]) >= 1, g              # no status flag; at least one feature measured in the last step
        print("camera %d (%dx%d %s): position error %s m converted, %s m for its control" % (cam, w, h, name, g[11], g[12]))
    # the native camera with the padded pitch against the unconverted control fed the same grey frames: the same state, to the digit
    assert len(states[2]) == 13 and states[2] == states[3], (states[2], states[3])
    assert all(math.isfinite(float(v)) for v in states[2])
    g = rows[2]
    assert g[11] == g[12] and g[13:17] == g[17:21]
    assert float(g[11]) < 0.01 and int(g[13]) == 12 and int(g[14]) == 10      # and it tracks, like the mixed-camera example's cameras
