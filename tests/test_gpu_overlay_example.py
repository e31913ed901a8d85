"""examples/overlay_monoslam.cpp driven end to end on a GPU: a mapping run of four sequences that writes annotated PPM frames for
two of them; one camera's lens is covered now and then, so that matches fail.  The frames are the engine's grey frames where nothing
was drawn, carry the four colours of the display (red matched, blue failed, yellow unselected, green marked), and the
printed draw-list counts show a string of particle ellipses while a feature is being initialised."""
import os
import re
import subprocess

import numpy as np
import pytest

from mapping_helpers import make_mapping_sequence
from test_gpu_headless_example import _write_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read_ppm(path):
    raw = open(path, "rb").read()
    m = re.match(rb"P6\n(\d+) (\d+)\n255\n", raw)
    w, h = int(m.group(1)), int(m.group(2))
    return np.frombuffer(raw, np.uint8, 3 * w * h, m.end()).reshape(h, w, 3)


def test_overlay_example_writes_annotated_frames(tmp_path):
    exe = os.path.join(ROOT, "examples", "overlay_monoslam")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    n_frames = 16
    cam, params, spec, frames, templates = make_mapping_sequence(n_frames=n_frames)
    cfg, fd = _write_scene(str(tmp_path), cam, params, spec, frames, templates)
    out_dir = os.path.join(str(tmp_path), "annotated")
    os.makedirs(out_dir)
    run = subprocess.run([exe, "--cfg", cfg, "--frames", fd, "--out", out_dir], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    rec = [re.match(r"frame +(\d+) seq (\d)  items +(\d+)  rings +(\d+)  patches +(\d+)  boxes (\d)  red +(\d+)  blue +(\d+)  yellow +(\d+)  green +(\d+)$", l)
           for l in run.stdout.splitlines() if l.startswith("frame ")]
    n_written = len(os.listdir(fd))
    assert all(rec) and len(rec) == 2 * n_written and {int(m.group(2)) for m in rec} == {1, 2}
    assert sorted(os.listdir(out_dir)) == sorted("seq%d_frame%03d.ppm" % (s, k) for s in (1, 2) for k in range(n_written))
    nums = np.array([[int(g) for g in m.groups()] for m in rec])
    # every frame shows every live feature's template; red matches and the green marked feature appear; while a feature is being
    # initialised a string of yellow particle ellipses is listed (more rings than a dozen features could have)
    assert (nums[:, 4] >= spec.n_features).all() and (nums[:, 6] > 0).any() and (nums[:, 9] > 0).all() and (nums[:, 8] > 0).any()
    assert (nums[:, 3] >= nums[:, 4] + 5).any(), "no string of particle ellipses was listed"
    colours = set()
    for m in rec:
        s, k = int(m.group(2)), int(m.group(1))
        img = _read_ppm(os.path.join(out_dir, "seq%d_frame%03d.ppm" % (s, k)))
        assert img.shape == (cam["height"], cam["width"], 3)
        grey = (img[:, :, 0] == img[:, :, 1]) & (img[:, :, 1] == img[:, :, 2])
        assert grey.mean() > 0.8 and not grey.all()
        colours |= {tuple(c) for c in img[~grey].reshape(-1, 3).tolist()}
    assert {(255, 0, 0), (0, 255, 0), (255, 255, 0), (0, 0, 255)} <= colours          # the four colours of the display
    # blue = a selected feature whose search failed: camera 2 on the frames its lens is covered (every sixth): nothing is red there
    covered = np.array([int(m.group(2)) == 2 and int(m.group(1)) > 0 and int(m.group(1)) % 6 == 0 for m in rec])
    assert covered.sum() == 2 and (nums[covered, 7] > 0).all() and (nums[covered, 6] == 0).all()
    assert (nums[:, 7] > 0).any()
