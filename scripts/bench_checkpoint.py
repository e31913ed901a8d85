#!/usr/bin/env python
"""Speed of sl2_save_sequences / sl2_load_sequences at BASELINE configs[2] (1024 sequences x 100 features), written to
profiles/checkpoint_bench.json.

Timed with device events on the engine's stream, after a warm-up, median of --reps:
  (a) save of all sequences into a device buffer (k_seq_pack, one launch),
  (b) load back from it (the whole call: header fetch + check on the host, k_seq_unpack) and k_seq_unpack alone (the engine's
      per-kernel brackets),
  (c) hipMemcpyAsync device-to-device of the same number of bytes in the same process - the yardstick.
Host destination (wall clock around calls that end in a synchronisation): save / load of 1 sequence and of all of them.

    python scripts/bench_checkpoint.py [--batch 1024] [--features 100] [--reps 25] [--out profiles/checkpoint_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--features", type=int, default=100)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint_bench.json"))
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("bench_checkpoint: no HIP device (there is no CPU fallback)")
    B, N = args.batch, args.features
    cam = synth.default_camera(320, 240)
    params = synth.default_params(N)
    stream = torch.cuda.Stream()
    eng = Engine(cam, params, B, N, stream=stream.cuda_stream)
    # a full map in every sequence: what is moved depends on the sizes, not on the values
    rng = np.random.default_rng(0)
    xv = np.zeros((B, 13)); xv[:, 3] = 1.0
    eng.set_vehicle_state(xv, np.tile(np.eye(13) * 1e-4, (B, 1, 1)))
    xp = np.zeros((B, N, 7)); xp[:, :, 3] = 1.0
    eng.add_known_features(rng.normal(size=(B, N, 3)), xp, rng.integers(0, 256, size=(B, N, 11, 11), dtype=np.uint8))
    eng.set_feature_covariances(np.tile(np.eye(3) * 1e-4, (B, N, 1, 1)))
    cap = eng.sequence_blob_capacity()
    buf = torch.empty(B * cap, dtype=torch.uint8, device="cuda")
    buf2 = torch.empty(B * cap, dtype=torch.uint8, device="cuda")
    eng.save_sequences_device(buf.data_ptr(), cap)
    eng.synchronize()
    blob_bytes = int(_lib.sl2_sequence_blob_header.from_buffer_copy(bytes(buf[:256].cpu().numpy())).bytes)
    total = blob_bytes * B

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

    def d2d():
        with torch.cuda.stream(stream):
            buf2[:total].copy_(buf[:total], non_blocking=True)

    save_ms = timed(lambda: eng.save_sequences_device(buf.data_ptr(), cap))
    load_ms = timed(lambda: eng.load_sequences_device(buf.data_ptr(), cap))
    copy_ms = timed(d2d)
    # the unpack kernel alone (the load call also fetches and checks the headers on the host while the stream idles)
    eng.set_profiling(2)
    eng.reset_kernel_times()
    for _ in range(args.reps):
        eng.load_sequences_device(buf.data_ptr(), cap)
        eng.save_sequences_device(buf.data_ptr(), cap)
    eng.synchronize()
    kt = eng.kernel_times()
    eng.set_profiling(0)
    kernel_ms = {k: v["total_ms"] / max(v["launches"], 1) for k, v in kt.items() if k in ("k_seq_pack", "k_seq_unpack")}

    def wall(fn, reps):
        out = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            eng.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    one = eng.save_sequences(0, 1)
    host = dict(save_1_ms=median(wall(lambda: eng.save_sequences(0, 1), 10)),
                load_1_ms=median(wall(lambda: eng.load_sequences(one, 0), 10)))
    t0 = time.perf_counter(); blobs = eng.save_sequences(); host["save_all_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter(); eng.load_sequences(blobs); host["load_all_ms"] = (time.perf_counter() - t0) * 1e3
    host["save_all_GBps"] = total / host["save_all_ms"] / 1e6
    host["load_all_GBps"] = total / host["load_all_ms"] / 1e6
    host["note"] = "wall clock, pageable numpy memory on the host side, Python packing of the blobs included"

    gbps = lambda ms: 2.0 * total / ms / 1e6          # read + write
    res = dict(commit=commit(), device=torch.cuda.get_device_name(0), batch=B, features=N, blob_bytes=blob_bytes,
               blob_capacity=cap, total_bytes=total, reps=args.reps,
               save_device_ms=median(save_ms), load_device_call_ms=median(load_ms), memcpy_d2d_ms=median(copy_ms),
               k_seq_pack_ms=kernel_ms.get("k_seq_pack"), k_seq_unpack_ms=kernel_ms.get("k_seq_unpack"),
               save_over_memcpy=median(save_ms) / median(copy_ms), load_call_over_memcpy=median(load_ms) / median(copy_ms),
               unpack_kernel_over_memcpy=(kernel_ms.get("k_seq_unpack") or float("nan")) / median(copy_ms),
               save_GBps_read_plus_write=gbps(median(save_ms)), memcpy_GBps_read_plus_write=gbps(median(copy_ms)),
               spread_ms=dict(save=[min(save_ms), max(save_ms)], load=[min(load_ms), max(load_ms)], memcpy=[min(copy_ms), max(copy_ms)]),
               host=host)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
