"""examples/mixed_camera_monoslam.cpp end to end on a GPU: three synthetic cameras of one image size and three calibrations in one
batch of three, each fed frames rendered for its own camera.  A demonstration: the test checks that it builds, runs and prints
finite numbers, that sl2_get_cameras reports each sequence's own calibration and that every camera keeps tracking."""
import math
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^camera (\d)  fku (\S+) fkv (\S+) u0 (\S+) v0 (\S+) kd1 (\S+) sd (\d+)  r = \( *(\S+) +(\S+) +(\S+)\)  "
                  r"position error (\S+) m  visible (\d+)  selected (\d+)")


def test_mixed_camera_example_builds_runs_and_prints_finite_numbers():
    exe = os.path.join(ROOT, "examples", "mixed_camera_monoslam")
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
    assert sorted(rows) == [0, 1, 2], out.stdout
    want = {0: (195.0, 195.0, 162.0, 125.0, 9e-06, 1), 1: (195 * 1.07, 195 * 0.94, 171.5, 118.75, 1.8e-05, 1),
            2: (195 * 0.9, 195.0, 162.0, 125.0, 0.0, 2)}
    for cam, g in rows.items():
        assert all(math.isfinite(float(v)) for v in g[1:6] + g[7:11]), g
        fku, fkv, u0, v0, kd1, sd = want[cam]
        assert abs(float(g[1]) - fku) < 1e-3 and abs(float(g[2]) - fkv) < 1e-3 and abs(float(g[3]) - u0) < 1e-3
        assert abs(float(g[4]) - v0) < 1e-3 and abs(float(g[5]) - kd1) < 1e-8 and int(g[6]) == sd
        assert float(g[10]) < 0.01, g                    # each filter is within a centimetre of the pose its last frame was rendered from
        assert int(g[11]) == 12 and int(g[12]) == 10, g  # all twelve features visible, ten selected
