#!/usr/bin/env python3
"""Reading out a whole batch: a loop of sl2_snapshot calls against one sl2_snapshot_batch.  Writes profiles/snapshot_batch_bench.json.

    python scripts/bench_snapshot_batch.py --parent-lib PATH/libscenelib2_amd.so [--rounds 3] [--out FILE]

Two shapes: the headline (1024 sequences x 100 features, dense covariance) and the --mapping shape of bench.py (1024 x 12 known
features in 32 slots, feature initialisation on).  For nseq in 8, 64, 256, 1024:

  loop        nseq x sl2_snapshot (one launch and one wait each, the full blob into the engine's pinned buffer), on the PARENT
              commit's library (--parent-lib) and on this one;
  batch       one sl2_snapshot_batch: SL2_SNAP_ALL and FEATURES | SELECTION, host form (three launches, one wait, one copy of the
              packed bytes into pageable host memory) and device form (three launches, timed to their completion), with the
              bytes that were packed.

Every leg is a fresh child process (a library is chosen when it is loaded: SL2_LIB_PATH), parent and this alternating, `--rounds`
of each, so that both see the same device in the same minutes.  A child warms every call it times (first use allocates staging
and loads code objects), then takes SAMPLES samples of each; a sample is a host clock around calls that end in a wait for the
device - REPS calls for the batch forms, so that a sample is milliseconds, not microseconds.  Reported: the median of a child's
samples per round, and over the rounds min / max / spread.  The claim the numbers must carry: at every nseq >= 8 the batch call
(SL2_SNAP_ALL, host form - the like-for-like read-out) is faster than the parent's loop by more than the parent's run-to-run
spread.  No ratio is assumed; the JSON says what was measured."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NSEQ = (8, 64, 256, 1024)
SAMPLES, REPS = 7, 10
SHAPES = dict(headline=dict(batch=1024, features=100, slots=100, mapping=False, steps=8),
              mapping=dict(batch=1024, features=12, slots=32, mapping=True, steps=30))


def build_engine(shape):
    """bench.py's set-up at this shape: device-rendered frames, `steps` steps taken."""
    import numpy as np
    import bench
    from scenelib2_amd import Engine, _lib, synth
    B, N, W, H = shape["batch"], shape["features"], 320, 240
    n_render = shape["steps"]
    cam = synth.default_camera(W, H)
    params = synth.default_params(min(N, 10) if shape["mapping"] else N)
    spec_kw = dict(v_amp=np.array([0.3, 0.3, 0.03]), w_amp=0.03) if shape["mapping"] else {}
    tex = synth.make_texture()
    specs = bench.make_specs(cam, N, n_render, list(range(B)), spec_kw)
    fb = W * H
    d_tex = _lib.DeviceBuffer(tex.nbytes); d_tex.upload(tex)
    poses = np.ascontiguousarray(np.stack([s.poses for s in specs], axis=1))
    origins = np.ascontiguousarray(np.tile(np.stack([s.tex_origin for s in specs])[None], (n_render + 1, 1, 1)))
    d_pose = _lib.DeviceBuffer(poses.nbytes); d_pose.upload(poses)
    d_org = _lib.DeviceBuffer(origins.nbytes); d_org.upload(origins)
    d_frames = _lib.DeviceBuffer((n_render + 1) * B * fb)
    synth.render_device(cam, d_tex.ptr, tex.shape[0], specs[0].tex_extent, d_org.ptr, d_pose.ptr, (n_render + 1) * B, d_frames.ptr)
    _lib.check(_lib.load().sl2_dev_download(0, np.empty(1, np.uint8).ctypes.data_as(_lib.vp), _lib.vp(d_frames.ptr), 1))      # (waits for the render)
    frame0 = d_frames.download((B, H, W), np.uint8)
    templates = np.stack([synth.cut_templates(frame0[b], specs[b].feat_px) for b in range(B)])
    eng = Engine(cam, params, B, shape["slots"])
    eng.set_vehicle_state(np.stack([s.xv0 for s in specs]), np.stack([s.Pxx0 for s in specs]))
    eng.add_known_features(np.stack([s.feat_y for s in specs]), np.stack([s.xp_org() for s in specs]), templates)
    if not shape["mapping"]:
        eng.set_feature_covariances(np.tile(np.eye(3) * 0.005 ** 2, (B, N, 1, 1)))
    for k in range(shape["steps"]):
        eng.go_one_step(d_frames.ptr + (k + 1) * B * fb, on_device=True, seq_stride=fb, save_trajectory=True, enable_mapping=shape["mapping"])
    eng.synchronize()
    return eng, (d_tex, d_pose, d_org, d_frames)


def stats(samples):
    s = sorted(samples)
    return dict(median_ms=s[len(s) // 2], min_ms=s[0], max_ms=s[-1])


def child(shape_name):
    """One library (the one SL2_LIB_PATH names, else this tree's), one shape: a JSON line on stdout."""
    import ctypes as C
    import numpy as np
    from scenelib2_amd import _lib
    shape = SHAPES[shape_name]
    eng, keep = build_engine(shape)
    L = eng.L
    has_batch = hasattr(L, "sl2_snapshot_batch")
    out = dict(shape=shape_name, library=os.environ.get("SL2_LIB_PATH", "this"), has_batch=has_batch, loop={}, batch={})
    blob, nb = _lib.vp(), C.c_size_t(0)

    def loop(n):
        total = 0
        for s in range(n):
            _lib.check(L.sl2_snapshot(eng.h, s, 0, 0, C.byref(blob), C.byref(nb)), L)
            total += nb.value
        return total
    for n in NSEQ:
        loop(min(n, 64))                                                   # warm
        samples = []
        for _ in range(SAMPLES):
            t0 = time.perf_counter()
            nbytes = loop(n)
            samples.append((time.perf_counter() - t0) * 1e3)
        out["loop"][str(n)] = dict(stats(samples), bytes=nbytes, calls=n)
    if has_batch:
        FS = _lib.SL2_SNAP_FEATURES | _lib.SL2_SNAP_SELECTION
        for sec_name, sections in (("all", _lib.SL2_SNAP_ALL), ("features_selection", FS)):
            bound = eng.snapshot_bound(sections)
            host = np.empty(bound * max(NSEQ), dtype=np.uint8)
            host[:] = 0                                                    # (touch the pages once: the copy must not pay for page faults)
            offs = np.zeros(max(NSEQ) + 1, dtype=np.uint64)
            d_out, d_off = _lib.DeviceBuffer(bound * max(NSEQ)), _lib.DeviceBuffer(8 * (max(NSEQ) + 1))
            for n in NSEQ:
                def host_call():
                    _lib.check(L.sl2_snapshot_batch(eng.h, 0, n, sections, None, host.ctypes.data_as(_lib.vp), host.nbytes,
                                                    offs.ctypes.data_as(_lib.vp), 0), L)
                def dev_call():
                    _lib.check(L.sl2_snapshot_batch(eng.h, 0, n, sections, None, _lib.vp(d_out.ptr), d_out.nbytes, _lib.vp(d_off.ptr), 1), L)
                    eng.synchronize()
                for form, call in (("host", host_call), ("device", dev_call)):
                    call(); call()                                         # warm (staging, code objects)
                    samples = []
                    for _ in range(SAMPLES):
                        t0 = time.perf_counter()
                        for _ in range(REPS):
                            call()
                        samples.append((time.perf_counter() - t0) * 1e3 / REPS)
                    host_call()
                    rec = dict(stats(samples), bytes=int(offs[n]), calls_per_sample=REPS)
                    rec["gb_per_s"] = rec["bytes"] / (rec["median_ms"] * 1e-3) / 1e9
                    out["batch"]["%s/%s/%d" % (sec_name, form, n)] = rec
            d_out.free(); d_off.free()
    eng.close()
    print("SNAPBENCH " + json.dumps(out), flush=True)


def over_rounds(recs):
    meds = [r["median_ms"] for r in recs]
    return dict(round_medians_ms=meds, median_ms=sorted(meds)[len(meds) // 2], min_ms=min(r["min_ms"] for r in recs),
                max_ms=max(r["max_ms"] for r in recs), spread_of_round_medians_ms=max(meds) - min(meds), bytes=recs[0]["bytes"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libscenelib2_amd.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="headline,mapping")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_batch_bench.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("--parent-lib: the parent commit's libscenelib2_amd.so is needed for the loop it is compared with")
    runs = {}
    for shape in args.shapes.split(","):
        for rnd in range(args.rounds):
            for leg in ("parent", "this"):
                env = dict(os.environ)
                env.pop("SL2_LIB_PATH", None)
                if leg == "parent":
                    env["SL2_LIB_PATH"] = os.path.abspath(args.parent_lib)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape], env=env, capture_output=True, text=True, timeout=600)
                line = [l for l in p.stdout.splitlines() if l.startswith("SNAPBENCH ")]
                if p.returncode != 0 or not line:
                    sys.exit("child (%s, %s) failed with status %d:\n%s" % (shape, leg, p.returncode, p.stderr[-2000:]))
                runs.setdefault(shape, {}).setdefault(leg, []).append(json.loads(line[0][len("SNAPBENCH "):]))
                print("%s round %d %s done" % (shape, rnd, leg), flush=True)
    result = dict(note="times in ms; a loop sample = nseq sl2_snapshot calls, a batch sample = the mean of %d calls; %d samples a round, "
                  "%d rounds, parent and this alternating, a process each" % (REPS, SAMPLES, args.rounds), nseq=list(NSEQ), shapes={})
    for shape, legs in runs.items():
        assert not legs["parent"][0]["has_batch"] and legs["this"][0]["has_batch"]
        rec = dict(shape=SHAPES[shape], by_nseq={})
        for n in NSEQ:
            parent = over_rounds([r["loop"][str(n)] for r in legs["parent"]])
            this = over_rounds([r["loop"][str(n)] for r in legs["this"]])
            row = dict(parent_loop=parent, this_loop=this, batch={})
            for key in ("all/host", "all/device", "features_selection/host", "features_selection/device"):
                b = over_rounds([r["batch"]["%s/%d" % (key, n)] for r in legs["this"]])
                b["gb_per_s"] = b["bytes"] / (b["median_ms"] * 1e-3) / 1e9
                b["parent_loop_over_this"] = parent["median_ms"] / b["median_ms"]
                # the slowest batch sample against the fastest loop sample, and the gap against the parent's own spread
                b["faster_by_more_than_parent_spread"] = (parent["min_ms"] - b["max_ms"]) > (parent["max_ms"] - parent["min_ms"])
                row["batch"][key] = b
            rec["by_nseq"][str(n)] = row
        result["shapes"][shape] = rec
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    for shape, rec in result["shapes"].items():
        for n, row in rec["by_nseq"].items():
            print(shape, "nseq", n, "parent loop %.3f ms" % row["parent_loop"]["median_ms"], "this loop %.3f" % row["this_loop"]["median_ms"],
                  " ".join("%s %.3f ms (x%.1f, %.2f GB/s, %d B)" % (k, b["median_ms"], b["parent_loop_over_this"], b["gb_per_s"], b["bytes"])
                           for k, b in row["batch"].items()))


if __name__ == "__main__":
    main()
