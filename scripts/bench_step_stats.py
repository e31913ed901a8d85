#!/usr/bin/env python
"""Cost of sl2_get_step_stats, written to profiles/step_stats_bench.json: at 1024 sequences x 100 features and at 1 x 12.

Every sequence of the batch is the same synthetic sequence (tiled), stepped twice so that an update with every feature matched
is what the query describes.  Per shape, after a warm-up, median of --reps:
  device form   device events on the engine's stream around the call (the launch of k_step_stats, nothing else);
  host form     wall clock around the call (launch, one stream synchronisation, the copy out of the pinned buffer);
  yardstick     wall clock of one sl2_get_selection call per sequence - what the same counts cost before;
  the step      device events around one sl2_go_one_step with device-resident frames, for scale.

    python scripts/bench_step_stats.py [--reps 25] [--out profiles/step_stats_bench.json]
"""
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
from scenelib2_amd import Engine, _lib, synth  # noqa: E402


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        p = os.path.join(ROOT, ".build_git")
        return open(p).read().strip() if os.path.exists(p) else "unknown"


def median(v):
    return float(np.median(np.asarray(v)))


def one_shape(B, N, reps, warmup):
    cam = synth.default_camera(320, 240)
    params = synth.default_params(N)
    spec, tpl, frames, _ = synth.make_sequence(cam, N, 4, tex=synth.make_texture())
    stream = torch.cuda.Stream()
    eng = Engine(cam, params, B, N, stream=stream.cuda_stream)
    eng.set_vehicle_state(np.tile(spec.xv0, (B, 1)), np.tile(spec.Pxx0, (B, 1, 1)))
    eng.add_known_features(np.tile(spec.feat_y, (B, 1, 1)), np.tile(spec.poses[0], (B, N, 1)), np.tile(tpl, (B, 1, 1, 1)))
    fb = cam["width"] * cam["height"]
    dev = [torch.from_numpy(np.tile(frames[k].reshape(1, fb), (B, 1))).cuda() for k in range(4)]
    for k in range(2):
        eng.go_one_step(dev[k].data_ptr(), on_device=True, seq_stride=fb)
    out = torch.empty(B * 96, dtype=torch.uint8, device="cuda")
    eng.synchronize()

    def events(fn):
        ms = []
        for i in range(warmup + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            if i >= warmup:
                ms.append(a.elapsed_time(b))
        return ms

    def wall(fn):
        ms = []
        for i in range(warmup + reps):
            eng.synchronize()
            t0 = time.perf_counter()
            fn()
            if i >= warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    dev_ms = events(lambda: eng.step_stats_device(out.data_ptr()))
    host_ms = wall(lambda: eng.step_stats())
    labels = np.zeros(N, dtype=np.int32)
    counters = np.zeros(3, dtype=np.int32)

    def selections():
        for s in range(B):
            eng.L.sl2_get_selection(eng.h, s, _lib.ip(labels), N, _lib.ip(counters))

    sel_ms = wall(selections)
    step_ms = events(lambda: eng.go_one_step(dev[2 + (len(dev_ms) & 1)].data_ptr(), on_device=True, seq_stride=fb))
    rec = eng.step_stats()
    res = dict(batch=B, features=N, dof=[int(rec["dof"].min()), int(rec["dof"].max())], reps=reps,
               step_stats_device_form_ms=median(dev_ms), step_stats_host_form_ms=median(host_ms),
               get_selection_per_sequence_calls=B, get_selection_all_sequences_ms=median(sel_ms),
               go_one_step_ms=median(step_ms),
               spread_ms=dict(device_form=[min(dev_ms), max(dev_ms)], host_form=[min(host_ms), max(host_ms)],
                              get_selection=[min(sel_ms), max(sel_ms)], go_one_step=[min(step_ms), max(step_ms)]))
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_stats_bench.json"))
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("bench_step_stats: no HIP device (there is no CPU fallback)")
    res = dict(commit=commit(), device=torch.cuda.get_device_name(0),
               note="device form: device events; host form and sl2_get_selection: wall clock around calls that end in a synchronisation",
               shapes=[one_shape(1024, 100, args.reps, args.warmup), one_shape(1, 12, args.reps, args.warmup)])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
