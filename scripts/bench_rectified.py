#!/usr/bin/env python3
"""Speed of the rectified view (k_rectify, k_scene_list, k_overlay_draw), written to profiles/rectified_bench.json.

    python scripts/bench_rectified.py [--out FILE]

Two shapes, built as scripts/bench_snapshot_batch.py builds them: the headline (1024 sequences x 100 features, 320 x 240) and the
--mapping shape of bench.py (1024 x 12 known features in 32 slots, feature initialisation on).  For nseq in 8, 64, 1024:

  rectify  sl2_rectify_frames with frames and output in device memory (one launch), timed to its completion;
  copy     a device-to-device copy in the same process that moves the same traffic: the warp reads 1 byte and writes 1 per pixel
           (its four taps share cache lines), so a copy of 1 byte a pixel (1 read + 1 written: 2 bytes a pixel in all);
  device   sl2_draw_rectified with frames and output in device memory (three launches), timed to its completion;
  host     the same with the RGB images returned to pageable host memory (one wait, one copy of 3 bytes a pixel).

A sample is a host clock around REPS calls that end in a wait for the device; SAMPLES samples after a warm-up (first use allocates
the staging); medians, with min and max.  Every step runs under a time limit of its own: an alarm with the default disposition, which ends the
process even where it waits inside the runtime.  The scene lists' lengths are recorded.  No target was fixed in advance; the
JSON says what was measured."""
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
from scenelib2_amd import _lib  # noqa: E402

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectified_bench.json"))
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("bench_rectified: no HIP device (there is no CPU fallback)")
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    px = W * H
    runs = []
    for shape_name in ("headline", "mapping"):
        shape = SHAPES[shape_name]
        eng, keep = build_engine(shape)
        L, B = eng.L, shape["batch"]
        d_frames = keep[3]
        frames_ptr = d_frames.ptr + shape["steps"] * B * px          # the frames of the last step taken
        lists = eng.scene_items(0, B)
        counts = np.array([l.size for l in lists])
        kinds = np.concatenate([l["kind"] for l in lists])
        d_grey = _lib.DeviceBuffer(px * B)
        d_out = _lib.DeviceBuffer(3 * px * B)
        host = np.zeros((B, 3 * px), np.uint8)                       # (pages touched once: the copy must not pay for page faults)
        a = torch.empty(px * B, dtype=torch.uint8, device="cuda")
        b = torch.empty(px * B, dtype=torch.uint8, device="cuda")
        for n in NSEQ:
            def rect_call():
                _lib.check(L.sl2_rectify_frames(eng.h, 0, n, _lib.vp(frames_ptr), px, 1, _lib.vp(d_grey.ptr), px, 1), L)
            def copy_call():
                b[:px * n].copy_(a[:px * n], non_blocking=True)
            def dev_call():
                _lib.check(L.sl2_draw_rectified(eng.h, 0, n, _lib.vp(frames_ptr), px, 1, 7, None, _lib.vp(d_out.ptr), 3 * px, 1), L)
            def host_call():
                _lib.check(L.sl2_draw_rectified(eng.h, 0, n, _lib.vp(frames_ptr), px, 1, 7, None, host.ctypes.data_as(_lib.vp), 3 * px, 0), L)
            rect = sample(rect_call, eng.synchronize)
            cpy = sample(copy_call, torch.cuda.synchronize)
            dev = sample(dev_call, eng.synchronize)
            hst = sample(host_call, lambda: None)
            traffic = 2 * px * n
            runs.append(dict(shape=shape_name, nseq=n, width=W, height=H, rectify_traffic_bytes=traffic,
                             items_per_sequence=dict(mean=float(counts[:n].mean()), max=int(counts[:n].max())),
                             rectify=rect, copy_same_traffic=cpy, draw_rectified_device=dev, draw_rectified_host=hst,
                             rectify_over_copy=rect["median_ms"] / cpy["median_ms"],
                             rectify_GBps=traffic / rect["median_ms"] / 1e6, copy_GBps=traffic / cpy["median_ms"] / 1e6,
                             rectify_Gpixel_per_s=px * n / rect["median_ms"] / 1e6,
                             host_GBps_of_rgb=3 * px * n / hst["median_ms"] / 1e6))
            print("%s nseq %d: rectify %.4f ms, copy %.4f ms, draw device %.4f ms, host %.4f ms" % (
                shape_name, n, rect["median_ms"], cpy["median_ms"], dev["median_ms"], hst["median_ms"]), flush=True)
        # the images are right before their time is worth anything: the device form against the host form, colour in them, and
        # the warp against the host form of one image
        eng.synchronize()
        got = d_out.download((B, H, W, 3), np.uint8)
        assert np.array_equal(got, host.reshape(B, H, W, 3)) and (got[:, :, :, 0] != got[:, :, :, 2]).any()
        from scenelib2_amd import rectified
        cam = eng.get_cameras(0, 1)[0]
        first = d_frames.download((H, W), np.uint8, offset=shape["steps"] * B * px)
        assert np.array_equal(d_grey.download((H, W), np.uint8), rectified.rectify_frame_host(first, cam["u0"], cam["v0"], cam["kd1"]))
        runs[-1]["item_kinds_whole_batch"] = dict(rings=int((kinds == 1).sum()), rects=int((kinds == 3).sum()), segments=int((kinds == 5).sum()))
        eng.close()
        for d in [d_out, d_grey] + list(keep):
            d.free()
        del a, b
        torch.cuda.empty_cache()
    res = dict(commit=commit(), device=torch.cuda.get_device_name(0), samples=SAMPLES, reps_per_sample=REPS, layers="all three", runs=runs,
               note="copy_same_traffic moves 1 byte a pixel device to device: 1 read + 1 written, the warp's own.  Below 256 MiB (nseq 8 and "
                    "64) both can live in the Infinity Cache between repeats, and both are bound by launch and wait, not by bytes.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
