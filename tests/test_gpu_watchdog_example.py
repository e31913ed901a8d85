"""examples/watchdog_monoslam.cpp end to end on a GPU: four sequences replay one recording, one of them is handed another
recording's frames from step 8 on, and the loop - which reads sl2_get_step_stats for the whole batch after every step - resets
the sequence that matched nothing three steps in a row and replays its own recording.  Wrong frames are ordinary input: the
filter finds no match in them, nothing more."""
import os
import re
import subprocess

import pytest

from mapping_helpers import make_mapping_sequence
from test_gpu_headless_example import _write_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = re.compile(r"^step +(\d+) seq (\d)  own step +(\d+)  matched +(\d+) / +(\d+)  dof +(\d+)  nis +(\S+)  log det S +(\S+)  worst label +(-?\d+)")


def test_watchdog_example_resets_the_sequence_that_lost_its_map(tmp_path):
    exe = os.path.join(ROOT, "examples", "watchdog_monoslam")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    steps, victim, start, patience = 20, 2, 8, 3
    cam, params, spec, frames, templates = make_mapping_sequence(n_frames=steps)
    good, other = tmp_path / "good", tmp_path / "other"
    good.mkdir()
    other.mkdir()
    cfg, fd = _write_scene(str(good), cam, params, spec, frames, templates)
    cam2, params2, spec2, frames2, templates2 = make_mapping_sequence(seed=11, n_frames=steps)
    _, wrong = _write_scene(str(other), cam2, params2, spec2, frames2, templates2)
    out = subprocess.run([exe, "--cfg", cfg, "--frames", fd, "--wrong", wrong, "--victim", str(victim), "--from", str(start),
                          "--patience", str(patience)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    rows = {}
    for line in out.stdout.split("\n"):
        m = STEP.match(line)
        if m:
            k, s, own, matched, selected, dof = (int(v) for v in m.groups()[:6])
            rows[(k, s)] = dict(own=own, matched=matched, selected=selected, dof=dof, nis=float(m.group(7)), label=int(m.group(9)),
                                rest=line.split("own step")[1])
    assert len(rows) == 4 * steps
    resets = re.findall(r"^step +(\d+) seq (\d)  RESET", out.stdout, flags=re.M)
    assert resets == [(str(start + patience - 1), str(victim))], resets
    reset_at = start + patience - 1
    for k in range(steps):
        for s in (0, 1, 3):                                       # the neighbours: one recording, one line each, never disturbed
            r = rows[(k, s)]
            assert r["own"] == k + 1 and r["matched"] > 0 and r["dof"] == 2 * r["matched"] and r["nis"] > 0 and r["label"] >= 0
            assert r["rest"] == rows[(k, 0)]["rest"]
        v = rows[(k, victim)]
        if k < start:
            assert v["rest"] == rows[(k, 0)]["rest"]
        elif k <= reset_at:                                       # the wrong feed: selected, searched, nothing matched
            assert v["own"] == k + 1 and v["matched"] == 0 and v["dof"] == 0 and v["label"] == -1 and v["selected"] > 0
        else:                                                     # its own recording from the start: what sequence 0 said then
            assert v["rest"] == rows[(k - reset_at - 1, 0)]["rest"]
    finals = re.findall(r"^final seq (\d)  own steps (\d+)  matched (\d+)  dof (\d+)  resets (\d+)", out.stdout, flags=re.M)
    assert [(int(a), int(b), int(e)) for a, b, c, d, e in finals] == [
        (s, steps - reset_at - 1 if s == victim else steps, 1 if s == victim else 0) for s in range(4)]
