"""examples/mixed_rate_monoslam.cpp end to end on a GPU: a 30 fps and a 15 fps synthetic camera in one batch of two, the slow one
paused every other engine step and given dt = 1/15 with sl2_set_delta_t.  A demonstration: the test checks that it builds, runs
and prints finite numbers, and that each filter predicted over its own camera's interval."""
import math
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^camera (\d)  dt (\S+)  last predict over (\S+)  frames +(\d+)  r = \( *(\S+) +(\S+) +(\S+)\)  position error (\S+) m  "
                  r"visible (\d+)  selected (\d+)")


def test_mixed_rate_example_builds_runs_and_prints_finite_numbers():
    exe = os.path.join(ROOT, "examples", "mixed_rate_monoslam")
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
    assert sorted(rows) == [0, 1], out.stdout
    for cam, frames, dt in ((0, 12, 1.0 / 30.0), (1, 6, 1.0 / 15.0)):
        g = rows[cam]
        assert all(math.isfinite(float(v)) for v in g[1:3] + g[4:8]), g
        assert int(g[3]) == frames
        assert abs(float(g[1]) - dt) < 1e-6 and abs(float(g[2]) - dt) < 1e-6       # each predicted over its own interval
