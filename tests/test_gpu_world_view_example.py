"""examples/world_view_monoslam.cpp driven end to end on a GPU: two sequences replay a recording, every frame's map is written
as a PPM seen through a view fitted to the map's extents, and after the last frame a click on a feature's marker picks that
feature, which is then deleted: it is gone from sl2_get_features afterwards."""
import os
import re
import subprocess

import numpy as np
import pytest

from mapping_helpers import make_mapping_sequence
from test_gpu_headless_example import _write_scene
from test_gpu_overlay_example import _read_ppm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_world_view_example_draws_the_map_and_deletes_the_picked_feature(tmp_path):
    exe = os.path.join(ROOT, "examples", "world_view_monoslam")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    n_frames = 12
    cam, params, spec, frames, templates = make_mapping_sequence(n_frames=n_frames)
    cfg, fd = _write_scene(str(tmp_path), cam, params, spec, frames, templates)
    out_dir = os.path.join(str(tmp_path), "world")
    os.makedirs(out_dir)
    run = subprocess.run([exe, "--cfg", cfg, "--frames", fd, "--out", out_dir, "--no-mapping"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    rec = [re.match(r"frame +(\d+) seq (\d)  items +(\d+)  glyph +(\d+)  trajectory +(\d+)  rays (\d)  markers +(\d+)  ellipsoids +(\d+)  axes (\d)  extents (.*)$", l)
           for l in run.stdout.splitlines() if l.startswith("frame ")]
    n_written = len(os.listdir(fd))
    assert all(rec) and len(rec) == 2 * n_written and {int(m.group(2)) for m in rec} == {0, 1}
    assert sorted(os.listdir(out_dir)) == sorted("seq%d_frame%03d.ppm" % (s, k) for s in range(2) for k in range(n_written))
    nums = np.array([[int(g) for g in m.groups()[:9]] for m in rec])
    # the fitted views hold the whole map: the glyph, the three axes and a marker and an outline for every feature
    assert (nums[:, 3] == 16).all() and (nums[:, 8] == 3).all() and (nums[:, 6] == spec.n_features).all() and (nums[:, 7] >= spec.n_features - 2).all()
    assert (nums[:, 2] == nums[:, 3] + nums[:, 4] + nums[:, 5] + 2 * nums[:, 6] + nums[:, 7] + nums[:, 8]).all()
    ext = np.array([[float(v) for v in m.group(10).split()] for m in rec])
    assert (ext[:, 0::2] <= 0).all() and (ext[:, 1::2] >= 0).all() and (ext[:, 1] - ext[:, 0] > 0.3).all()          # 0 is taken in; the map is decimetres wide
    colours = set()
    for m in rec[::5]:
        s, k = int(m.group(2)), int(m.group(1))
        img = _read_ppm(os.path.join(out_dir, "seq%d_frame%03d.ppm" % (s, k)))
        assert img.shape == (360, 480, 3)
        black = (img == 0).all(axis=2)
        assert black.mean() > 0.8 and not black.all()
        colours |= {tuple(c) for c in img[~black].reshape(-1, 3).tolist()}
    assert {(150, 150, 150), (255, 255, 255)} <= colours and colours & {(255, 0, 0), (0, 0, 255), (255, 255, 0)}
    picks = [re.match(r"pick seq (\d)  click (-?\d+) (-?\d+)  marker of label (-?\d+)  picked label (-?\d+) item (-?\d+)  deleted (\d)  still listed (\d)  features left (\d+)$", l)
             for l in run.stdout.splitlines() if l.startswith("pick ")]
    assert len(picks) == 2 and all(picks)
    for m in picks:
        seq, x, y, want, label, item, deleted, still, left = (int(g) for g in m.groups())
        assert 0 <= x < 480 and 0 <= y < 360 and want >= 0
        assert label >= 0 and item >= 0 and deleted == 1 and still == 0 and left == spec.n_features - 1          # the picked feature is gone
    assert any(int(m.group(4)) == int(m.group(5)) for m in picks)
