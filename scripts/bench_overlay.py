#!/usr/bin/env python3
"""Speed of sl2_draw_overlays (k_overlay_list + k_overlay_draw), written to profiles/overlay_bench.json.

    python scripts/bench_overlay.py [--out FILE]

Two shapes, built as scripts/bench_snapshot_batch.py builds them: the headline (1024 sequences x 100 features, 320 x 240) and the
--mapping shape of bench.py (1024 x 12 known features in 32 slots, feature initialisation on).  For nseq in 8, 64, 1024:

  device   sl2_draw_overlays with frames and output in device memory (two launches), timed to its completion;
  host     the same with the RGB images returned to pageable host memory (one wait, one copy of 3 bytes a pixel);
  copy     a device-to-device copy in the same process that moves the same traffic: the rasteriser reads 1 byte and writes 3 per
           pixel, so a copy of 2 bytes a pixel (2 read + 2 written).

A sample is a host clock around REPS calls that end in a wait for the device; SAMPLES samples after a warm-up (first use allocates
the staging); medians, with min and max.  The draw lists' lengths are recorded: the rasteriser's work beyond the pixel traffic is
items x tiles they meet.  No target was fixed in advance; the JSON says what was measured."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch          # before scenelib2_amd: one HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_snapshot_batch import SHAPES, build_engine, stats  # noqa: E402
from scenelib2_amd import _lib  # noqa: E402

NSEQ = (8, 64, 1024)
SAMPLES, REPS = 7, 10
W, H = 320, 240


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        p = os.path.join(ROOT, ".build_git")
        return open(p).read().strip() if os.path.exists(p) else "unknown"


def sample(call, wait):
    call(); wait(); call(); wait()
    out = []
    for _ in range(SAMPLES):
        t0 = time.perf_counter()
        for _ in range(REPS):
            call()
        wait()
        out.append((time.perf_counter() - t0) * 1e3 / REPS)
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_bench.json"))
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("bench_overlay: no HIP device (there is no CPU fallback)")
    px = W * H
    runs = []
    for shape_name in ("headline", "mapping"):
        shape = SHAPES[shape_name]
        eng, keep = build_engine(shape)
        L, B = eng.L, shape["batch"]
        d_frames = keep[3]
        frames_ptr = d_frames.ptr + shape["steps"] * B * px          # the frames of the last step taken
        lists = eng.overlay_items(0, B)
        counts = np.array([l.size for l in lists])
        kinds = np.concatenate([l["kind"] for l in lists])
        d_out = _lib.DeviceBuffer(3 * px * B)
        host = np.zeros((B, 3 * px), np.uint8)                       # (pages touched once: the copy must not pay for page faults)
        a = torch.empty(2 * px * B, dtype=torch.uint8, device="cuda")
        b = torch.empty(2 * px * B, dtype=torch.uint8, device="cuda")
        for n in NSEQ:
            def dev_call():
                _lib.check(L.sl2_draw_overlays(eng.h, 0, n, _lib.vp(frames_ptr), px, 1, 7, None, _lib.vp(d_out.ptr), 3 * px, 1), L)
            def host_call():
                _lib.check(L.sl2_draw_overlays(eng.h, 0, n, _lib.vp(frames_ptr), px, 1, 7, None, host.ctypes.data_as(_lib.vp), 3 * px, 0), L)
            def copy_call():
                b[:2 * px * n].copy_(a[:2 * px * n], non_blocking=True)
            dev = sample(dev_call, eng.synchronize)
            hst = sample(host_call, lambda: None)
            cpy = sample(copy_call, torch.cuda.synchronize)
            traffic = 4 * px * n
            runs.append(dict(shape=shape_name, nseq=n, width=W, height=H, pixel_traffic_bytes=traffic,
                             items_per_sequence=dict(mean=float(counts[:n].mean()), max=int(counts[:n].max())),
                             device=dev, host=hst, copy_same_traffic=cpy,
                             device_over_copy=dev["median_ms"] / cpy["median_ms"], host_over_copy=hst["median_ms"] / cpy["median_ms"],
                             device_GBps=traffic / dev["median_ms"] / 1e6, copy_GBps=traffic / cpy["median_ms"] / 1e6,
                             host_GBps_of_rgb=3 * px * n / hst["median_ms"] / 1e6))
        # the images are right before their time is worth anything: the device form against the host form, and colour in them
        eng.synchronize()
        got = d_out.download((B, H, W, 3), np.uint8)
        assert np.array_equal(got, host.reshape(B, H, W, 3)) and (got[:, :, :, 0] != got[:, :, :, 2]).any()
        runs[-1]["item_kinds_whole_batch"] = dict(rings=int((kinds == 1).sum()), patches=int((kinds == 2).sum()), boxes=int((kinds == 3).sum()))
        eng.close()
        d_out.free()
        for d in keep:
            d.free()
        del a, b
        torch.cuda.empty_cache()
    res = dict(commit=commit(), device=torch.cuda.get_device_name(0), samples=SAMPLES, reps_per_sample=REPS, layers="all three", runs=runs,
               note="copy_same_traffic moves 2 bytes a pixel device to device: 2 read + 2 written, the rasteriser's 1 + 3.  Below 256 MiB "
                    "(nseq 8 and 64) both can live in the Infinity Cache between repeats, and both are bound by launch and wait, not by bytes.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
