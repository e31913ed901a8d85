"""examples/publish_monoslam.cpp driven end to end on a GPU: after every frame ONE sl2_snapshot_batch(POSE + FEATURES +
SELECTION) for the whole batch and a digest line per sequence.  The lines must be those the same program builds from one
sl2_snapshot per sequence (--single: the full blob of each), frame by frame - positions, counts and the digest over xv_, Pxx_,
the feature records and the selection."""
import os
import re
import subprocess

import pytest

from mapping_helpers import make_mapping_sequence
from test_gpu_headless_example import _write_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mapping", [False, True])
def test_publish_example_prints_the_digest_of_per_sequence_snapshots(tmp_path, mapping):
    exe = os.path.join(ROOT, "examples", "publish_monoslam")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    n_frames = 12
    cam, params, spec, frames, templates = make_mapping_sequence(n_frames=n_frames)
    cfg, fd = _write_scene(str(tmp_path), cam, params, spec, frames, templates)
    runs = {}
    for mode in ("batch", "single"):
        cmd = [exe, "--cfg", cfg, "--frames", fd] + (["--mapping"] if mapping else []) + (["--single"] if mode == "single" else [])
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        runs[mode] = ([l for l in out.stdout.splitlines() if l.startswith("frame ")], int(out.stderr.split()[0]))
    lines, sent = runs["batch"]
    assert lines == runs["single"][0] and len(lines) == 4 * n_frames
    assert 0 < sent < runs["single"][1]                    # fewer bytes crossed the bus: three sections, not six
    rec = [re.match(r"frame +(\d+) seq (\d)  own steps +(\d+)  features +(\d+)  selected +(\d+)  partial (\d)  r (\S+) (\S+) (\S+)  digest ([0-9a-f]{16})$", l)
           for l in lines]
    assert all(rec)
    last = {int(m.group(2)): m for m in rec[-4:]}
    # camera s > 0 dropped every (s + 3)rd frame: its own step count says so, and its state is not camera 0's
    assert [int(last[s].group(3)) for s in range(4)] == [n_frames - (n_frames // (s + 3) if s else 0) for s in range(4)]
    assert all(int(last[s].group(4)) >= spec.n_features for s in range(4))
    assert len({last[s].group(10) for s in range(4)}) == 4
    if mapping:
        assert any(int(m.group(4)) > spec.n_features or int(m.group(6)) > 0 for m in rec)
