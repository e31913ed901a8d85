"""examples/rectified_monoslam.cpp driven end to end on a GPU: a mapping run of three sequences shown through three lens
distortions, written as PPM frames the way the reference's rectified display shows the map.  The frames are grey where nothing
was drawn, carry the display's colours, and the printed list counts show a marker and an ellipsoid outline per feature and the
ray of a feature being initialised."""
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


def test_rectified_example_writes_the_map_over_undistorted_frames(tmp_path):
    exe = os.path.join(ROOT, "examples", "rectified_monoslam")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    n_frames = 20
    cam, params, spec, frames, templates = make_mapping_sequence(n_frames=n_frames)
    cfg, fd = _write_scene(str(tmp_path), cam, params, spec, frames, templates)
    out_dir = os.path.join(str(tmp_path), "rectified")
    os.makedirs(out_dir)
    run = subprocess.run([exe, "--cfg", cfg, "--frames", fd, "--out", out_dir], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    rec = [re.match(r"frame +(\d+) seq (\d)  items +(\d+)  trajectory +(\d+)  rays (\d)  markers +(\d+)  ellipsoids +(\d+)  green (\d)  pixels moved +(\d+)$", l)
           for l in run.stdout.splitlines() if l.startswith("frame ")]
    n_written = len(os.listdir(fd))
    assert all(rec) and len(rec) == 3 * n_written and {int(m.group(2)) for m in rec} == {0, 1, 2}
    assert sorted(os.listdir(out_dir)) == sorted("seq%d_frame%03d.ppm" % (s, k) for s in range(3) for k in range(n_written))
    nums = np.array([[int(g) for g in m.groups()] for m in rec])
    # every fully initialised feature in front of the camera has a marker and an ellipsoid outline; the marked one is green (its
    # marker's two rectangles and its ring); a ray is listed while a feature is being initialised
    assert (nums[:, 5] >= spec.n_features - 2).all() and (nums[:, 6] >= spec.n_features - 2).all() and (nums[:, 7] == 3).mean() > 0.8
    assert (nums[:, 4] > 0).any(), "no ray of a partially initialised feature was listed"
    assert (nums[:, 2] == nums[:, 3] + nums[:, 4] + 2 * nums[:, 5] + nums[:, 6]).all()
    # the three lenses: the stronger the distortion the more pixels the warp moves; with the recording's own it moves some
    moved = [nums[nums[:, 1] == s, 8].mean() for s in range(3)]
    assert 0 < moved[0] < moved[2] < moved[1], moved
    colours = set()
    for m in rec[::5]:
        s, k = int(m.group(2)), int(m.group(1))
        img = _read_ppm(os.path.join(out_dir, "seq%d_frame%03d.ppm" % (s, k)))
        assert img.shape == (cam["height"], cam["width"], 3)
        grey = (img[:, :, 0] == img[:, :, 1]) & (img[:, :, 1] == img[:, :, 2])
        assert grey.mean() > 0.8 and not grey.all()
        colours |= {tuple(c) for c in img[~grey].reshape(-1, 3).tolist()}
    assert {(255, 0, 0), (0, 255, 0)} <= colours          # matched features red, the marked one green
