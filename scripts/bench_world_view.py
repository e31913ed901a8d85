#!/usr/bin/env python3
"""Speed of the world view and of picking (k_world_list, k_overlay_draw, k_pick_items), written to profiles/world_view_bench.json.

    python scripts/bench_world_view.py [--out FILE]

Two shapes, built as scripts/bench_snapshot_batch.py builds them: the headline (1024 sequences x 100 features, 320 x 240) and the
--mapping shape of bench.py (1024 x 12 known features in 32 slots, feature initialisation on).  For nseq in 8, 64, 1024, all
through one shared view fitted to the first map's extents, 320 x 240 images:

  list       sl2_world_items with views, lists, counts and extents in device memory (one launch), timed to its completion;
  draw       sl2_draw_world with views and output in device memory (a fill and two launches), timed to its completion;
  draw_host  the same with the RGB images returned to pageable host memory (one wait, one copy of 3 bytes a pixel);
  pick       sl2_pick_items_batch over the device lists, one click per sequence, everything in device memory (one launch);
  rectified  sl2_draw_rectified of the same commit, device form, beside them for scale.

A sample is a host clock around REPS calls that end in a wait for the device; SAMPLES samples after a warm-up (first use allocates
the staging); medians, with min and max.  Every step runs under a time limit of its own: an alarm with the default disposition,
which ends the process even where it waits inside the runtime.  The lists' lengths are recorded.  No target was fixed in
advance; the JSON says what was measured."""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np
import torch          # before scenelib2_amd: one HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_overlay import commit  # noqa: E402
from bench_snapshot_batch import SHAPES, build_engine, stats  # noqa: E402
from scenelib2_amd import _lib, overlay, world_view  # noqa: E402

NSEQ = (8, 64, 1024)
SAMPLES, REPS = 7, 10
W, H = 320, 240
STEP_LIMIT_S = 60


def sample(call, wait):
    signal.alarm(STEP_LIMIT_S)
    try:
        call(); wait(); call(); wait()
        out = []
        for _ in range(SAMPLES):
            t0 = time.perf_counter()
            for _ in range(REPS):
                call()
            wait()
            out.append((time.perf_counter() - t0) * 1e3 / REPS)
    finally:
        signal.alarm(0)
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_view_bench.json"))
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("bench_world_view: no HIP device (there is no CPU fallback)")
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    px = W * H
    runs = []
    for shape_name in ("headline", "mapping"):
        shape = SHAPES[shape_name]
        eng, keep = build_engine(shape)
        L, B = eng.L, shape["batch"]
        vp = _lib.vp
        d_frames = keep[3]
        frames_ptr = d_frames.ptr + shape["steps"] * B * px          # the frames of the last step taken
        cam = eng.get_cameras(0, 1)[0]
        ref = world_view.reference_view(cam)
        _, ext = eng.world_items(ref, 0, 1)
        ex = ext[0]
        centre = [(ex[0] + ex[1]) / 2, (ex[2] + ex[3]) / 2, (ex[4] + ex[5]) / 2]
        size = max(0.2, ex[1] - ex[0], ex[3] - ex[2], ex[5] - ex[4])
        view = world_view.look_at([centre[0] + 0.3 * size, centre[1] + 0.5 * size, centre[2] - 1.8 * size], centre, (0.0, 1.0, 0.0),
                                  cam["fku"], cam["fkv"], W / 2.0, H / 2.0)
        lists, _ = eng.world_items(view, 0, B)
        counts = np.array([l.size for l in lists])
        kinds = np.concatenate([l["kind"] for l in lists])
        stride = eng.world_item_bound()
        varr = np.ascontiguousarray(view).reshape(1)
        clicks = np.zeros((B, 2), np.int32)
        for i, l in enumerate(lists):          # a click on the last marker of every list
            m = l[(l["kind"] == 3) & (l["a"][:, 0] == l["a"][:, 2])]
            clicks[i] = (m[-1]["a"][0], m[-1]["a"][1]) if m.size else (W // 2, H // 2)
        d_view, d_items, d_counts = _lib.DeviceBuffer(varr.nbytes), _lib.DeviceBuffer(64 * stride * B), _lib.DeviceBuffer(4 * B)
        d_ext, d_clicks, d_picked = _lib.DeviceBuffer(48 * B), _lib.DeviceBuffer(8 * B), _lib.DeviceBuffer(8 * B)
        d_out = _lib.DeviceBuffer(3 * px * B)
        d_view.upload(varr)
        d_clicks.upload(clicks)
        host = np.zeros((B, 3 * px), np.uint8)                       # (pages touched once: the copy must not pay for page faults)
        stream = eng.stream
        for n in NSEQ:
            def list_call():
                _lib.check(L.sl2_world_items(eng.h, 0, n, vp(d_view.ptr), 1, 31, None, vp(d_items.ptr), stride, vp(d_counts.ptr), vp(d_ext.ptr), 1), L)
            def draw_call():
                _lib.check(L.sl2_draw_world(eng.h, 0, n, vp(d_view.ptr), 1, W, H, 0, 31, None, vp(d_out.ptr), 3 * px, 1), L)
            def host_call():
                _lib.check(L.sl2_draw_world(eng.h, 0, n, varr.ctypes.data_as(vp), 1, W, H, 0, 31, None, host.ctypes.data_as(vp), 3 * px, 0), L)
            def pick_call():
                _lib.check(L.sl2_pick_items_batch(0, vp(stream) if stream else None, n, W, H, vp(d_items.ptr), stride, vp(d_counts.ptr), 0,
                                                  vp(d_clicks.ptr), vp(d_picked.ptr), 1), L)
            def rect_call():
                _lib.check(L.sl2_draw_rectified(eng.h, 0, n, vp(frames_ptr), px, 1, 7, None, vp(d_out.ptr), 3 * px, 1), L)
            rect = sample(rect_call, eng.synchronize)
            lst = sample(list_call, eng.synchronize)
            pick = sample(pick_call, eng.synchronize)
            drw = sample(draw_call, eng.synchronize)
            hst = sample(host_call, lambda: None)
            runs.append(dict(shape=shape_name, nseq=n, width=W, height=H,
                             items_per_sequence=dict(mean=float(counts[:n].mean()), max=int(counts[:n].max())),
                             world_items_device=lst, draw_world_device=drw, draw_world_host=hst, pick_items_device=pick,
                             draw_rectified_device=rect, host_GBps_of_rgb=3 * px * n / hst["median_ms"] / 1e6))
            print("%s nseq %d: list %.4f ms, draw device %.4f ms, host %.4f ms, pick %.4f ms; draw_rectified %.4f ms" % (
                shape_name, n, lst["median_ms"], drw["median_ms"], hst["median_ms"], pick["median_ms"], rect["median_ms"]), flush=True)
        # the results are right before their time is worth anything: the device form against the host form and against the host
        # rasteriser of the device's list, and the picks against the host form
        eng.synchronize()
        got = d_out.download((B, H, W, 3), np.uint8)
        assert np.array_equal(got, host.reshape(B, H, W, 3)) and (got[:, :, :, 0] != got[:, :, :, 2]).any()
        assert np.array_equal(got[0], overlay.draw_items_host(np.zeros((H, W), np.uint8), lists[0], None))
        picked = d_picked.download((B, 2), np.int32)
        for i in (0, 1, B - 1):
            assert tuple(picked[i]) == world_view.pick_items_host(W, H, lists[i], int(clicks[i, 0]), int(clicks[i, 1]))
        runs[-1]["item_kinds_whole_batch"] = dict(rings=int((kinds == 1).sum()), rects=int((kinds == 3).sum()), segments=int((kinds == 5).sum()))
        runs[-1]["picked_a_feature"] = int((picked[:, 0] >= 0).sum())
        eng.close()
        for d in [d_view, d_items, d_counts, d_ext, d_clicks, d_picked, d_out] + list(keep):
            d.free()
        torch.cuda.empty_cache()
    res = dict(commit=commit(), device=torch.cuda.get_device_name(0), samples=SAMPLES, reps_per_sample=REPS, layers="all five", runs=runs,
               note="one shared view fitted to the first map's extents; sl2_draw_rectified of the same library beside the world view for scale "
                    "(it undistorts a frame per sequence in addition)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
