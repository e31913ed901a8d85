#!/usr/bin/env python
"""Same-box A/B of the fused small-map step between two builds of libscenelib2_amd.so: the build in the tree and an older
one (--prev-lib: the library file of a checkout of the parent commit, built with the same Makefile).  The two are run
ALTERNATELY, --runs times each, a process per run:

  bench.py --mapping --gpus 1       the reference's default workload, 1024 sequences (ms_per_step; k_small_back is its update)
  bench.py --gpus 1                 the headline, 1024 x 100 features (ms_per_step; ten launches, k_search_score among them)
  examples/monoslam_adapter         one sequence, mapping on: the adapter's per-frame latency (frame_us_median)

and the medians are reported beside the older build's own run-to-run spread, which is the yardstick for "no slower".

    python scripts/ab_small_step.py --prev-lib ../parent/scenelib2_amd/libscenelib2_amd.so [--runs 5] [--out profiles/step_stats_ab.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def bench(extra, prev_lib):
    env = dict(os.environ)
    if prev_lib:
        env["SL2_LIB_PATH"] = prev_lib
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "100", "--warmup", "30"] + extra,
                         env=env, capture_output=True, text=True, timeout=600, check=True).stdout
    return json.loads([l for l in out.split("\n") if l.startswith("{")][-1])["ms_per_step"]


def adapter(cfg, fd, out, prev_lib):
    env = dict(os.environ)
    if prev_lib:          # the example finds the library through a RUNPATH, which LD_LIBRARY_PATH precedes
        env["LD_LIBRARY_PATH"] = os.path.dirname(prev_lib) + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    subprocess.run([os.path.join(ROOT, "examples", "monoslam_adapter"), "--cfg", cfg, "--frames", fd, "--latency", out, "--mapping"],
                   env=env, check=True, timeout=600, stdout=subprocess.DEVNULL)
    return json.load(open(out))["frame_us_median"]


def summary(prev, this):
    prev, this = np.asarray(prev), np.asarray(this)
    return dict(prev=prev.tolist(), this=this.tolist(), prev_median=float(np.median(prev)), this_median=float(np.median(this)),
                this_minus_prev=float(np.median(this) - np.median(prev)), prev_spread=float(prev.max() - prev.min()),
                within_prev_spread=bool(abs(np.median(this) - np.median(prev)) <= prev.max() - prev.min()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prev-lib", required=True)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_stats_ab.json"))
    args = ap.parse_args()
    prev_lib = os.path.abspath(args.prev_lib)
    assert os.path.exists(prev_lib), prev_lib
    from mapping_helpers import make_mapping_sequence
    from test_gpu_headless_example import _write_scene
    res = dict(note="alternating runs, a process each, one box, one session; prev = the parent commit's library; ms_per_step of bench.py "
                    "(--steps 100 --warmup 30), frame_us_median of examples/monoslam_adapter --latency --mapping (120 frames)")
    legs = {"bench_mapping_ms_per_step": ["--mapping"], "bench_headline_ms_per_step": []}
    for name, extra in legs.items():
        prev, this = [], []
        for _ in range(args.runs):
            prev.append(bench(extra, prev_lib))
            this.append(bench(extra, None))
        res[name] = summary(prev, this)
        print(name, json.dumps(res[name]), flush=True)
    with tempfile.TemporaryDirectory() as d:
        cam, params, spec, frames, tpl = make_mapping_sequence(n_frames=120)
        cfg, fd = _write_scene(d, cam, params, spec, frames, tpl)
        prev, this = [], []
        for _ in range(args.runs):
            prev.append(adapter(cfg, fd, os.path.join(d, "p.json"), prev_lib))
            this.append(adapter(cfg, fd, os.path.join(d, "t.json"), None))
        res["adapter_mapping_frame_us_median"] = summary(prev, this)
        print("adapter", json.dumps(res["adapter_mapping_frame_us_median"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
