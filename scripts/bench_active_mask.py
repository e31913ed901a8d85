#!/usr/bin/env python
"""What a step costs under a mask of paused sequences (sl2_set_active_sequences) at BASELINE configs[2] (1024 sequences x 100
features), written to profiles/active_mask_bench.json.

One engine of 1024 sequences is warmed up and its sequences are saved to a device buffer (sl2_save_sequences).  Every mask then
starts from that same state and steps over the same frames: all active, a contiguous half paused, every second sequence paused,
one sequence active.  A second engine of 512 sequences (the first half of the batch) gives the other yardstick.  A step is timed
with device events on the engine's stream, median and min / max of --reps; a further pass with a bracket on every launch gives
the per-kernel times.  The XCD question (sl2_common.hpp: xcd_map puts sequence b on XCD b % 8, so the alternating mask idles
four XCDs in every kernel that uses it) is answered by alternating_minus_contiguous_ms against the spread of the two.
Also: host time of sl2_set_active_sequences per call (host and device form, 1 and 1024 sequences), and frames per second of
sl2_ingest_next_ragged against sl2_ingest_next on directories of equal length.

    python scripts/bench_active_mask.py [--batch 1024] [--features 100] [--reps 20] [--warmup 5] [--out profiles/active_mask_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch          # before scenelib2_amd: one HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (make_specs: the flagship workload's sequences)
from scenelib2_amd import Engine, _lib, ingest, sharding, synth  # noqa: E402


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        p = os.path.join(ROOT, ".build_git")
        return open(p).read().strip() if os.path.exists(p) else "unknown"


def stats(v):
    a = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "active_mask_bench.json"))
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("bench_active_mask: no HIP device (there is no CPU fallback)")
    B, N, W, H = args.batch, args.features, 320, 240
    K, Wm = args.reps, args.warmup
    n_render = Wm + 2 * K
    cam = synth.default_camera(W, H)
    params = synth.default_params(N)
    fb = W * H
    tex = synth.make_texture()
    specs = bench.make_specs(cam, N, n_render, sharding.global_sequence_ids(B, 1, 0), {}, 1)
    d_tex = _lib.DeviceBuffer(tex.nbytes, 0); d_tex.upload(tex)
    poses = np.ascontiguousarray(np.stack([s.poses for s in specs], axis=1))
    origins = np.ascontiguousarray(np.tile(np.stack([s.tex_origin for s in specs])[None], (n_render + 1, 1, 1)))
    d_pose = _lib.DeviceBuffer(poses.nbytes, 0); d_pose.upload(poses)
    d_org = _lib.DeviceBuffer(origins.nbytes, 0); d_org.upload(origins)
    d_frames = _lib.DeviceBuffer((n_render + 1) * B * fb, 0)
    synth.render_device(cam, d_tex.ptr, tex.shape[0], specs[0].tex_extent, d_org.ptr, d_pose.ptr, (n_render + 1) * B, d_frames.ptr, device=0)
    torch.cuda.synchronize()
    frame0 = d_frames.download((B, H, W), np.uint8)
    templates = np.stack([synth.cut_templates(frame0[b], specs[b].feat_px) for b in range(B)])
    stream = torch.cuda.Stream()

    def engine(nb):
        e = Engine(cam, params, nb, N, stream=stream.cuda_stream)
        e.set_vehicle_state(np.stack([s.xv0 for s in specs[:nb]]), np.stack([s.Pxx0 for s in specs[:nb]]))
        e.add_known_features(np.stack([s.feat_y for s in specs[:nb]]), np.stack([s.xp_org() for s in specs[:nb]]), templates[:nb])
        e.set_feature_covariances(np.tile(np.eye(3) * 0.005 ** 2, (nb, N, 1, 1)))
        return e

    def step(e, k):                          # frame k (0-based) = pose k + 1; an engine of nb sequences reads the first nb of the batch
        e.go_one_step(d_frames.ptr + (k + 1) * B * fb, on_device=True, seq_stride=fb)

    def timed_steps(e, k0):
        ms = []
        for k in range(k0, k0 + K):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            step(e, k)
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    def kernel_ms(e, k0):
        e.set_profiling(2)
        e.reset_kernel_times()
        for k in range(k0, k0 + K):
            step(e, k)
        e.synchronize()
        kt = e.kernel_times()
        e.set_profiling(0)
        return {k: round(v["total_ms"] / K, 5) for k, v in sorted(kt.items(), key=lambda q: -q[1]["total_ms"])}

    eng = engine(B)
    for k in range(Wm):
        step(eng, k)
    eng.synchronize()
    cap = eng.sequence_blob_capacity()
    state = torch.empty(B * cap, dtype=torch.uint8, device="cuda")
    eng.save_sequences_device(state.data_ptr(), cap)
    eng.synchronize()

    masks = {"all_active": np.ones(B, np.uint8),
             "contiguous_half_paused": (np.arange(B) < B // 2).astype(np.uint8),
             "every_second_paused": (np.arange(B) % 2 == 0).astype(np.uint8),
             "one_active": (np.arange(B) == 0).astype(np.uint8)}
    res = dict(commit=commit(), device=torch.cuda.get_device_name(0), batch=B, features=N, reps=K, warmup=Wm, masks={})
    order = ["all_active", "contiguous_half_paused", "every_second_paused", "one_active", "every_second_paused", "contiguous_half_paused",
             "all_active"]                                       # every mask but one twice, in mirrored order: drift shows as a difference of the two
    for name in order:
        eng.load_sequences_device(state.data_ptr(), cap)
        eng.set_active(masks[name])
        ms = timed_steps(eng, Wm)
        rec = res["masks"].setdefault(name, dict(active=int(masks[name].sum()), step_ms_runs=[]))
        rec["step_ms_runs"].append(stats(ms))
        if "kernels_ms_per_step" not in rec:
            eng.load_sequences_device(state.data_ptr(), cap)
            rec["kernels_ms_per_step"] = kernel_ms(eng, Wm)
            rec["work"] = eng.step_work()
    eng.set_active(masks["all_active"])

    # host time of the call itself, behind an idle stream (nothing to wait for either way)
    d_mask = _lib.DeviceBuffer(B, 0); d_mask.upload(masks["every_second_paused"])
    call = {}
    for nseq in (1, B):
        m = masks["every_second_paused"][:nseq].copy()
        for form in ("host", "device"):
            us = []
            for i in range(220):
                t0 = time.perf_counter()
                if form == "host":
                    eng.L.sl2_set_active_sequences(eng.h, 0, nseq, _lib.u8p(m), 0)
                else:
                    eng.L.sl2_set_active_sequences(eng.h, 0, nseq, _lib.C.cast(_lib.vp(d_mask.ptr), _lib.c_u8p), 1)
                us.append((time.perf_counter() - t0) * 1e6)
                if i % 20 == 19:
                    eng.synchronize()
            call["%s_form_%d_sequences_us" % (form, nseq)] = stats(us[20:])
    res["set_active_call"] = call
    eng.set_active(masks["all_active"])
    eng.close()

    half = engine(B // 2)
    for k in range(Wm):
        step(half, k)
    half.synchronize()
    res["all_active_%d" % (B // 2)] = dict(step_ms=stats(timed_steps(half, Wm)), kernels_ms_per_step=kernel_ms(half, Wm + K))
    half.close()

    med = lambda name: float(np.median([r["median"] for r in res["masks"][name]["step_ms_runs"]]))
    spread = lambda name: max(r["max"] for r in res["masks"][name]["step_ms_runs"]) - min(r["min"] for r in res["masks"][name]["step_ms_runs"])
    for name in res["masks"]:
        res["masks"][name]["step_ms_median"] = med(name)
    full, halfms = med("all_active"), res["all_active_%d" % (B // 2)]["step_ms"]["median"]
    c, a = med("contiguous_half_paused"), med("every_second_paused")
    res["summary"] = dict(all_active_1024_ms=full, all_active_512_ms=halfms, contiguous_half_paused_ms=c, every_second_paused_ms=a,
                          one_active_ms=med("one_active"), alternating_minus_contiguous_ms=a - c,
                          spread_contiguous_ms=spread("contiguous_half_paused"), spread_alternating_ms=spread("every_second_paused"),
                          alternating_slower_beyond_spread=bool(a - c > max(spread("contiguous_half_paused"), spread("every_second_paused"))),
                          half_paused_nearer_to=("512" if abs(c - halfms) < abs(c - full) else "1024"))

    # ragged ingest against the plain one on directories of equal length: the same code path
    with tempfile.TemporaryDirectory() as tmp:
        rng = np.random.default_rng(0)
        dirs, nfr = [], 60
        for s in range(4):
            d = os.path.join(tmp, "s%d" % s); os.makedirs(d); dirs.append(d)
            for k in range(nfr):
                ingest.write_pgm(os.path.join(d, "%05d.pgm" % k), rng.integers(0, 256, size=(H, W), dtype=np.uint8))
        fps = {}
        for kind in ("next", "next_ragged", "next", "next_ragged"):
            g = ingest.FrameIngest(dirs, W, H, depth=8)
            g.set_zero_copy(0)
            t0 = time.perf_counter()
            for k in range(nfr):
                g.next() if kind == "next" else g.next_ragged()
            torch.cuda.synchronize()
            fps.setdefault(kind, []).append(nfr / (time.perf_counter() - t0))
            g.close()
        res["ingest_frames_per_s"] = {k: [round(x, 1) for x in v] for k, v in fps.items()}

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["summary"]))
    print(json.dumps(res["set_active_call"]))
    print(json.dumps(res["ingest_frames_per_s"]))


if __name__ == "__main__":
    main()
