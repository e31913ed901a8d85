"""examples/frame_gate_monoslam.cpp end to end on a GPU, and the Python adapter's SetFrameGate.  The example is a demonstration:
the test checks that it builds, runs and prints finite numbers, that the gate rejects exactly the five repeated and the three
black frames and nothing of the control, and that the control is the same with the gate and without it.  The position errors
are printed; no bound is set on them."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from scenelib2_amd import MonoSLAM, frame_monitor as M, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^camera (\d) \((.*?)\)  rejected (\d+)  position error with the gate (\S+) m \(worst on a good frame (\S+) m\)  "
                  r"without (\S+) m \(worst (\S+) m\)")


def test_frame_gate_example_builds_runs_and_rejects_the_bad_frames():
    exe = os.path.join(ROOT, "examples", "frame_gate_monoslam")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    out = subprocess.run([exe, "--steps", "20"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    print(out.stdout)
    rows = {int(m.group(1)): m.groups() for m in map(LINE.match, out.stdout.split("\n")) if m}
    assert sorted(rows) == [0, 1, 2], out.stdout
    assert [int(rows[c][2]) for c in range(3)] == [5, 3, 0]
    for g in rows.values():
        assert all(math.isfinite(float(v)) for v in g[3:7]), g
    assert rows[2][3] == rows[2][5] and rows[2][4] == rows[2][6]          # the control: the gate changes nothing
    steps = {int(m.group(1)): [int(v) for v in m.groups()[1:]] for m in re.finditer(r"step +(\d+)  verdicts +(\d+) +(\d+) +(\d+) \| (\d+) (\d+) (\d+)", out.stdout)}
    assert steps[7] == [0] * 6 and steps[13] == [0] * 6
    for k in range(8, 13):
        assert steps[k][0] == 16 and steps[k][2] == 0 and steps[k][3:] == [0, 0, 0], (k, steps[k])          # REPEATED
        assert (steps[k][1] != 0) == (k < 11) and (steps[k][1] & 2 if k < 11 else True)                    # DARK while black


def test_python_adapter_gate_on_host_and_device_frames():
    cam, params = synth.default_camera(), synth.default_params(6)
    spec, tpl, frames, _ = synth.make_sequence(cam, 8, 5, seq_index=0, tex=synth.make_texture())
    W, H = cam["width"], cam["height"]
    gate = dict(reject_repeated=1, dark_bins=1, max_dark_pixels=W * H // 2)

    def make():
        m = MonoSLAM(max_features=8).InitFromValues(cam, params, spec.xv0, spec.Pxx0)
        for i in range(spec.feat_y.shape[0]):
            m.AddNewKnownFeature(spec.feat_y[i], spec.poses[0], tpl[i])
        return m

    gated, plain = make(), make()
    assert gated.LastFrameVerdict() == 0
    gated.SetFrameGate(gate)
    feed = [frames[0], frames[1], frames[1], np.zeros_like(frames[0]), frames[2]]          # a repeat and a black frame
    want = [0, 0, M.SL2_FRAME_REPEATED, M.SL2_FRAME_DARK, 0]
    for f, v in zip(feed, want):          # host frames: the two host forms
        before = gated._engine.get_vehicle_state()[0]
        gated.GoOneStep(f)
        assert gated.LastFrameVerdict() == v
        if v:          # a rejected frame leaves the filter as it was
            assert np.array_equal(gated._engine.get_vehicle_state()[0], before)
        else:
            plain.GoOneStep(f)
            assert not np.array_equal(gated._engine.get_vehicle_state()[0], before)
    assert np.array_equal(gated._engine.get_vehicle_state()[0], plain._engine.get_vehicle_state()[0])          # good frames only, both
    # device frames: GoOneStepRaw through the converter (a grey source of the engine's size), the chain on the engine's stream
    gated, plain = make(), make()
    gated.SetFrameGate(gate, catch_up=False)
    for m in (gated, plain):
        m.SetFrameSource(W, H, W, "gray8")
    for f, v in zip(feed, want):
        gated.GoOneStepRaw(np.ascontiguousarray(f).reshape(-1))
        assert gated.LastFrameVerdict() == v
        if not v:
            plain.GoOneStepRaw(np.ascontiguousarray(f).reshape(-1))
    assert np.array_equal(gated._engine.get_vehicle_state()[0], plain._engine.get_vehicle_state()[0])
    assert list(gated._engine.active()) == [1]
