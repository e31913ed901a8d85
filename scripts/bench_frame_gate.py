#!/usr/bin/env python
"""Speed of the frame monitor's examine chain (k_frame_stats + k_frame_gate), written to profiles/frame_gate_bench.json.

Part 1, per shape - 8, 64 and 1024 sequences of 320 x 240 and 1024 sequences of 640 x 480, random frames in device memory -
timed with device events on one stream, after a warm-up, median, least and greatest of --reps calls:
  (a) sl2_examine_frames with every output (two launches),
  (b) hipMemcpyAsync device-to-device of the same bytes in the same process: the yardstick, there being no earlier build.  The copy
      reads AND writes those bytes: twice the traffic of the statistics kernel, which only reads them.
Both walk a ring of frame buffers that together exceed 640 MB (at most 16 of them), one buffer a call, so that at the large batches
no call finds its frames in the 256 MiB Infinity Cache from the call before: the figures are rates from memory, for the chain and
for the copy alike.  (The copy's destination is one buffer.)
The records are checked against sl2_frame_stats_host on a few sequences first.

Part 2 (skipped with --no-step): the headline step (bench.py's workload: 1024 sequences of 320 x 240 with 100 features) with the
gate chain in front of it - examine on the engine's stream, then sl2_set_active_sequences in device form - against the step
without it, every frame passing, in interleaved rounds of one process.  The price of the feature: reported, not gated.

    python scripts/bench_frame_gate.py [--reps 30] [--out profiles/frame_gate_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch          # before scenelib2_amd: one HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scenelib2_amd import Engine, _lib, frame_monitor, synth  # noqa: E402

SHAPES = [(8, 320, 240), (64, 320, 240), (1024, 320, 240), (1024, 640, 480)]


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        p = os.path.join(ROOT, ".build_git")
        return open(p).read().strip() if os.path.exists(p) else "unknown"


def passing_gate(n):
    """Every rule on, with thresholds a textured frame passes: the whole gate is evaluated."""
    return dict(min_range=1, dark_bins=1, max_dark_pixels=n, bright_bins=1, max_bright_pixels=n, reject_repeated=1, min_gradient_energy=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=15, help="steps per arm per round of part 2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_gate_bench.json"))
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("bench_frame_gate: no HIP device (there is no CPU fallback)")
    stream = torch.cuda.Stream()
    med = lambda v: float(np.median(np.asarray(v)))

    def timed(fn):
        ms = []
        for i in range(args.warmup + args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                fn()
                b.record(stream)
            b.synchronize()
            if i >= args.warmup:
                ms.append(a.elapsed_time(b))
        return ms

    runs = []
    for B, w, h in SHAPES:
        n = w * h
        g = torch.Generator(device="cuda")
        g.manual_seed(B + w)
        nbuf = min(16, -(-640_000_000 // (B * n)))          # a ring that the Infinity Cache cannot hold
        ring = [torch.randint(0, 256, (B * n,), dtype=torch.uint8, device="cuda", generator=g) for _ in range(nbuf)]
        frames = ring[0]
        copy_to = torch.empty_like(frames)
        turn = [0]

        def next_frames():
            turn[0] = (turn[0] + 1) % nbuf
            return ring[turn[0]]
        stats = torch.empty(B * _lib.FRAME_STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        verdict = torch.empty(B, dtype=torch.int32, device="cuda")
        active = torch.empty(B, dtype=torch.uint8, device="cuda")
        mon = frame_monitor.FrameMonitor(0, B, w, h)
        mon.set_gates([dict(passing_gate(n), reject_repeated=0)] * B)
        go_on = lambda f: mon.examine(f.data_ptr(), n, None, stats.data_ptr(), verdict.data_ptr(), active.data_ptr(), stream=stream.cuda_stream)
        go = lambda: go_on(next_frames())
        go_on(frames)
        stream.synchronize()
        got = np.frombuffer(stats.cpu().numpy().tobytes(), _lib.FRAME_STATS_DTYPE)
        for s in (0, B // 2, B - 1):          # the bytes are right before their time is worth anything
            want = frame_monitor.frame_stats_host(frames[s * n:(s + 1) * n].cpu().numpy().reshape(h, w))
            assert got[s].tobytes() == want.tobytes(), (B, w, h, s)
        assert (verdict.cpu().numpy() == 0).all() and (active.cpu().numpy() == 1).all()

        def d2d():
            with torch.cuda.stream(stream):
                copy_to.copy_(next_frames(), non_blocking=True)

        ex_ms, cp_ms = timed(go), timed(d2d)
        runs.append(dict(batch=B, width=w, height=h, bytes_read=B * n, ring_buffers=nbuf, examine_ms=med(ex_ms), examine_read_TBps=B * n / med(ex_ms) / 1e9,
                         memcpy_d2d_ms=med(cp_ms), memcpy_traffic_TBps=2 * B * n / med(cp_ms) / 1e9,
                         examine_over_memcpy=med(ex_ms) / med(cp_ms),
                         spread_ms=dict(examine=[min(ex_ms), max(ex_ms)], memcpy_d2d=[min(cp_ms), max(cp_ms)])))
        print(json.dumps(runs[-1]), flush=True)
        mon.close()
        del frames, copy_to, ring
        torch.cuda.empty_cache()
    res = dict(commit=commit(), device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, runs=runs,
               note="the copy moves twice the bytes the statistics kernel reads; every call takes the next buffer of a ring of more than "
                    "640 MB (16 buffers at most: the two small batches, which are bound by their launches, stay cache-resident)")
    if not args.no_step:
        res["headline_step"] = headline(args, med)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, runs=len(runs), headline_step=res.get("headline_step"))))


def headline(args, med):
    """bench.py's workload, stepped with and without the gate chain in front, in interleaved rounds."""
    import time
    import bench
    B, N, W, H = 1024, 100, 320, 240
    fb = W * H
    warm = 10
    n_render = warm + 2 * args.rounds * args.steps
    cam, params = synth.default_camera(W, H), synth.default_params(N)
    tex = synth.make_texture()
    specs = bench.make_specs(cam, N, n_render, list(range(B)), {}, 1)
    d_tex = _lib.DeviceBuffer(tex.nbytes); d_tex.upload(tex)
    poses = np.ascontiguousarray(np.stack([s.poses for s in specs], axis=1))
    origins = np.ascontiguousarray(np.tile(np.stack([s.tex_origin for s in specs])[None], (n_render + 1, 1, 1)))
    d_pose = _lib.DeviceBuffer(poses.nbytes); d_pose.upload(poses)
    d_org = _lib.DeviceBuffer(origins.nbytes); d_org.upload(origins)
    d_frames = _lib.DeviceBuffer((n_render + 1) * B * fb)
    synth.render_device(cam, d_tex.ptr, tex.shape[0], specs[0].tex_extent, d_org.ptr, d_pose.ptr, (n_render + 1) * B, d_frames.ptr)
    torch.cuda.synchronize()
    frame0 = d_frames.download((B, H, W), np.uint8)
    templates = np.stack([synth.cut_templates(frame0[b], specs[b].feat_px) for b in range(B)])
    eng = Engine(cam, params, B, N)
    eng.set_vehicle_state(np.stack([s.xv0 for s in specs]), np.stack([s.Pxx0 for s in specs]))
    eng.add_known_features(np.stack([s.feat_y for s in specs]), np.stack([s.xp_org() for s in specs]), templates)
    eng.set_feature_covariances(np.tile(np.eye(3) * 0.005 ** 2, (B, N, 1, 1)))
    mon = frame_monitor.FrameMonitor(0, B, W, H)
    mon.set_gates([passing_gate(fb)] * B)
    d_active, d_verdict = _lib.DeviceBuffer(B), _lib.DeviceBuffer(4 * B)
    k = [0]

    def step(gated):
        ptr = d_frames.ptr + (k[0] + 1) * B * fb
        if gated:
            mon.examine(ptr, fb, None, None, d_verdict, d_active, stream=eng.stream)
            eng.set_active((d_active.ptr, B), on_device=True)
        eng.go_one_step(ptr, on_device=True, seq_stride=fb)
        k[0] += 1

    for _ in range(warm):
        step(False)
    eng.synchronize()
    plain, gated = [], []
    for _ in range(args.rounds):
        for arm, out in ((False, plain), (True, gated)):
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(arm)
            eng.synchronize()
            out.append((time.perf_counter() - t0) / args.steps * 1e3)
    assert (d_verdict.download((B,), np.uint32) == 0).all() and (eng.active() == 1).all()          # every frame passed
    return dict(batch=B, features=N, width=W, height=H, rounds=args.rounds, steps_per_arm_per_round=args.steps,
                step_ms=med(plain), step_with_gate_chain_ms=med(gated), price_ms=med(gated) - med(plain),
                price_over_step=med(gated) / med(plain) - 1.0,
                spread_ms=dict(step=[min(plain), max(plain)], step_with_gate_chain=[min(gated), max(gated)]))


if __name__ == "__main__":
    main()
