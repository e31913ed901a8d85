#!/usr/bin/env python
"""Speed of sl2_convert_frames (k_convert_frames) for 1024 sequences to 320 x 240, written to profiles/frame_convert_bench.json.

Four sources, every sequence of a run the same: 640 x 480 UYVY, 640 x 480 RGB24, 960 x 720 RGB24 and the native grey copy.
Per source, timed with device events on one stream, after a warm-up, median of --reps launches:
  (a) the conversion (one launch; the raw frames are device memory),
  (b) hipMemcpyAsync device-to-device in the same process - the yardstick, there being no earlier build - of as many bytes as
      the kernel must touch (memcpy_touched: it reads AND writes that many, twice the kernel's traffic) and of half as many
      (memcpy_same_traffic: its reads plus writes equal the kernel's bytes).
"Must touch" is computed here from the shapes: the source rows that some row tap names, at the bytes of a row each, plus the
output.  Rates are those bytes over the time.  The result is checked against sl2_convert_frame_host on a few sequences first.

    python scripts/bench_frame_convert.py [--batch 1024] [--reps 30] [--out profiles/frame_convert_bench.json]

--filter area times k_convert_area (SL2_RESIZE_AREA) instead, from 640 x 480 UYVY, 1280 x 960 GRAY8, 1920 x 1080 YUYV and
960 x 720 RGB24, and writes profiles/frame_convert_area_bench.json.  The area filter reads every source byte, so bytes_read is the
whole source.  --linear-json / --linear-parent-json name the results of two --filter linear runs of the same session, this
commit's library and its parent's (SL2_LIB_PATH): they are recorded beside the area runs, with whether every convert_ms of this
commit lies inside the parent's spread_ms.

--filter raw times k_raw_linear and k_raw_area (the machine-vision formats) instead: 640 x 480 BAYER_RGGB8 under LINEAR, 1280 x 960
BAYER_RGGB8 and 1280 x 960 GRAY12 under AREA, and writes profiles/frame_convert_raw_bench.json.  Beside the flat copy, every source
is timed against a GRAY8 source of the same size under the same filter through the existing kernel, in the same run: it moves the
same bytes for Bayer and half the bytes for deep grey, so the difference is the demosaic or the narrowing itself.
--ab-out FILE with --linear-json / --linear-parent-json / --area-json / --area-parent-json (four runs of one session, this commit's
library and its parent's under both filters) writes only the comparison of the existing kernels to FILE and times nothing.

--filter remap times k_convert_remap (the lens remap) instead: 640 x 480 GRAY8, 640 x 480 BAYER_RGGB8 and 1280 x 960 GRAY8, each under
a BROWN and under a FISHEYE lens remapped into its sl2_lens_pinhole_camera target, with ONE map shared by all sequences and with a
map per sequence (the same calibration but for a sub-unit shift of the centre per sequence: as many slots, as many bytes), and writes
profiles/frame_convert_remap_bench.json.  Every run stands beside the same source through the existing LINEAR kernel in the same
run, and beside the flat copy.  "Must touch": the map entries (per slot), the 128-byte lines of the source that some tap names (a
Bayer tap names its 3 x 3 neighbourhood), the output.
--ab-out FILE --this-jsons A .. --parent-jsons P ..: results of this script (any of linear / area / raw) and saved bench.py lines,
several runs of this commit's library and of its parent's (SL2_LIB_PATH) from ONE session; per source the parent's run-to-run spread
(least and greatest of its runs' medians) and whether each of this commit's medians lies inside it.  Times nothing.
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
from scenelib2_amd import _lib, convert  # noqa: E402

SOURCES = [("640x480 UYVY", 640, 480, "uyvy"), ("640x480 RGB24", 640, 480, "rgb24"), ("960x720 RGB24", 960, 720, "rgb24"),
           ("320x240 GRAY8 (native copy)", 320, 240, "gray8")]
AREA_SOURCES = [("640x480 UYVY", 640, 480, "uyvy"), ("1280x960 GRAY8", 1280, 960, "gray8"), ("1920x1080 YUYV", 1920, 1080, "yuyv"),
                ("960x720 RGB24", 960, 720, "rgb24")]
RAW_SOURCES = [("640x480 BAYER_RGGB8", 640, 480, "bayer_rggb8", "linear"), ("1280x960 BAYER_RGGB8", 1280, 960, "bayer_rggb8", "area"),
               ("1280x960 GRAY12", 1280, 960, "gray12", "area")]
REMAP_SOURCES = [("640x480 GRAY8", 640, 480, "gray8"), ("640x480 BAYER_RGGB8", 640, 480, "bayer_rggb8"), ("1280x960 GRAY8", 1280, 960, "gray8")]


def remap_lens(model, w, h):
    """A calibration of the kind the model is used for, for a w x h camera (coefficients for a 640-wide image, focal lengths scaled)."""
    k = w / 640.0
    if model == "brown":
        return dict(model="brown", width=w, height=h, fx=400.0 * k, fy=400.0 * k, cx=319.5 * k, cy=239.5 * k, k=[-0.28, 0.09, 1.1e-3, -7e-4, -0.012])
    return dict(model="fisheye", width=w, height=h, fx=250.0 * k, fy=250.0 * k, cx=319.5 * k, cy=239.5 * k, k=[-0.021, 0.0043, -0.0017, 0.0002])


def remap_reach(xy, w, h, pitch, bpp, bayer):
    """(distinct source pixels some tap names, distinct 128-byte lines of the source they lie in) of one map: the definition's
    taps - (ix, iy), (ix + 1, iy) where fx != 0 ... inside the image -, for Bayer the 3 x 3 neighbourhood of each, reflected."""
    X, Y = xy[..., 0].astype(np.int64).ravel(), xy[..., 1].astype(np.int64).ravel()
    live = X != convert.SL2_REMAP_BORDER
    X, Y = X[live], Y[live]
    fx, fy = X & 31, Y & 31
    ix, iy = (X - fx) // 32, (Y - fy) // 32
    mask = np.zeros((h, w), bool)
    refl = lambda i, S: np.where(i < 0, -i, np.where(i >= S, 2 * (S - 1) - i, i))
    for dx, dy, use in ((0, 0, np.ones_like(fx, bool)), (1, 0, fx != 0), (0, 1, fy != 0), (1, 1, (fx != 0) & (fy != 0))):
        tx, ty = ix + dx, iy + dy
        ok = use & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
        tx, ty = tx[ok], ty[ok]
        if not bayer:
            mask[ty, tx] = True
            continue
        for ny in (-1, 0, 1):
            for nx in (-1, 0, 1):
                mask[refl(ty + ny, h), refl(tx + nx, w)] = True
    ys, xs = np.nonzero(mask)
    return int(mask.sum()), int(np.unique((ys * pitch + xs * bpp) // 128).size)


def ab_runs(this_jsons, parent_jsons):
    """Per (filter, source) - and the headline step of saved bench.py lines -: the medians of every run of either library, the parent's
    run-to-run spread, and whether each of this commit's medians lies inside it."""
    def collect(paths):
        got = {}
        for path in paths:
            d = json.load(open(path))
            if "runs" in d:
                for r in d["runs"]:
                    got.setdefault("%s %s: %s" % (d["filter"], r["filter"], r["source"]), []).append(r["convert_ms"])
            else:
                got.setdefault("headline step (bench.py ms_per_step)", []).append(d["ms_per_step"])
        return got
    this, parent = collect(this_jsons), collect(parent_jsons)
    rows = []
    for key in parent:
        lo, hi = min(parent[key]), max(parent[key])
        mine = this.get(key, [])
        rows.append(dict(what=key, parent_ms=parent[key], parent_spread_ms=[lo, hi], this_commit_ms=mine,
                         inside_parent_spread=[lo <= v <= hi for v in mine], at_most_parent_slowest=[v <= hi for v in mine],
                         this_median_over_parent_median=float(np.median(mine) / np.median(parent[key])) if mine else None))
    return dict(runs=rows, all_inside=all(all(r["inside_parent_spread"]) for r in rows), none_slower=all(all(r["at_most_parent_slowest"]) for r in rows))


STEP_MS = 1.45          # the headline step (README) the conversion sits in front of


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        p = os.path.join(ROOT, ".build_git")
        return open(p).read().strip() if os.path.exists(p) else "unknown"


def rows_read(src_h, out_h, halo=False):
    """Source rows that some row tap names (the definition of include/scenelib2_amd.h, in float32 like it); halo: and the rows
    above and below them, which a Bayer grey row needs."""
    d = np.arange(out_h, dtype=np.float64)
    f = ((d + 0.5) * (np.float64(src_h) / np.float64(out_h)) - 0.5).astype(np.float32)
    i = np.clip(np.floor(f).astype(np.int64), 0, src_h - 1)
    rows = np.unique(np.concatenate([i, np.minimum(i + 1, src_h - 1)]))
    if halo:
        rows = np.unique(np.clip(np.concatenate([rows - 1, rows, rows + 1]), 0, src_h - 1))
    return int(rows.size)


def unchanged(this_json, parent_json):
    """The runs of this commit's library beside those of its parent's: is every convert_ms inside the parent's spread?"""
    this, parent = json.load(open(this_json)), json.load(open(parent_json))
    pick = lambda r: dict(source=r["source"], convert_ms=r["convert_ms"], spread_ms=r["spread_ms"]["convert"],
                          convert_over_memcpy_same_traffic=r["convert_over_memcpy_same_traffic"])
    rows = [dict(this_commit=pick(a), parent=pick(b), inside_parent_spread=b["spread_ms"]["convert"][0] <= a["convert_ms"] <= b["spread_ms"]["convert"][1],
                 at_most_parent_slowest=a["convert_ms"] <= b["spread_ms"]["convert"][1])
            for a, b in zip(this["runs"], parent["runs"])]
    return dict(parent_library=parent.get("library"), runs=rows, all_inside=all(r["inside_parent_spread"] for r in rows),
                none_slower=all(r["at_most_parent_slowest"] for r in rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--filter", choices=("linear", "area", "raw", "remap"), default="linear")
    ap.add_argument("--this-jsons", nargs="*", default=None)
    ap.add_argument("--parent-jsons", nargs="*", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--linear-json", default=None)
    ap.add_argument("--linear-parent-json", default=None)
    ap.add_argument("--area-json", default=None)
    ap.add_argument("--area-parent-json", default=None)
    ap.add_argument("--ab-out", default=None)
    args = ap.parse_args()
    if args.ab_out and args.parent_jsons:
        res = dict(commit=commit(), **ab_runs(args.this_jsons or [], args.parent_jsons))
        with open(args.ab_out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res))
        return
    if args.ab_out:
        res = dict(commit=commit(), linear_unchanged=unchanged(args.linear_json, args.linear_parent_json),
                   area_unchanged=unchanged(args.area_json, args.area_parent_json))
        with open(args.ab_out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res))
        return
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", {"linear": "frame_convert_bench.json", "area": "frame_convert_area_bench.json",
                                                   "raw": "frame_convert_raw_bench.json", "remap": "frame_convert_remap_bench.json"}[args.filter])
    if _lib.device_count() < 1:
        raise SystemExit("bench_frame_convert: no HIP device (there is no CPU fallback)")
    B, ow, oh = args.batch, 320, 240
    stream = torch.cuda.Stream()
    out = torch.empty(B * ow * oh, dtype=torch.uint8, device="cuda")

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

    med = lambda v: float(np.median(np.asarray(v)))
    if args.filter == "remap":
        return bench_remap(args, B, ow, oh, stream, out, timed, med)
    runs = []
    todo = []
    for src in {"linear": SOURCES, "area": AREA_SOURCES, "raw": RAW_SOURCES}[args.filter]:
        todo.append(src if len(src) == 5 else src + (args.filter,))
        if args.filter == "raw":          # the yardstick through the existing kernel: GRAY8 of the same size under the same filter
            todo.append(("%dx%d GRAY8 (%s)" % (src[1], src[2], src[4]), src[1], src[2], "gray8", src[4]))
    for name, w, h, fmt, flt in todo:
        area = flt == "area"
        bpp = convert.BYTES_PER_PIXEL[convert.FORMATS[fmt]]
        frame = w * h * bpp
        g = torch.Generator(device="cuda")
        g.manual_seed(w * 31 + bpp)
        raw = torch.randint(0, 256, (B * frame,), dtype=torch.uint8, device="cuda", generator=g)
        cv = convert.FrameConverter(0, B, ow, oh)
        cv.set_sources([dict(width=w, height=h, format=fmt, offset=s * frame) for s in range(B)])
        if area:
            cv.set_filters(["area"] * B)
        go = lambda: cv.convert((raw.data_ptr(), raw.numel()), out.data_ptr(), stream=stream.cuda_stream)
        go()
        stream.synchronize()
        for s in (0, B // 2, B - 1):          # the bytes are right before their time is worth anything
            want = convert.convert_frame_host(dict(width=w, height=h, format=fmt), raw[s * frame:(s + 1) * frame].cpu().numpy(), ow, oh,
                                              **(dict(filter="area") if area else {}))
            assert np.array_equal(out[s * ow * oh:(s + 1) * ow * oh].cpu().numpy().reshape(oh, ow), want), (name, s)
        src_rows = h if area else rows_read(h, oh, halo=fmt.startswith("bayer"))          # the area filter reads every source byte
        read = B * src_rows * w * bpp
        touched = read + B * ow * oh
        conv_ms = timed(go)
        scratch_a = torch.empty(touched, dtype=torch.uint8, device="cuda")
        scratch_b = torch.empty(touched, dtype=torch.uint8, device="cuda")

        def d2d(n):
            def fn():
                with torch.cuda.stream(stream):
                    scratch_b[:n].copy_(scratch_a[:n], non_blocking=True)
            return fn

        full_ms, half_ms = timed(d2d(touched)), timed(d2d(touched // 2))
        runs.append(dict(source=name, filter=flt, raw_bytes=B * frame, bytes_read=read, bytes_written=B * ow * oh, bytes_touched=touched,
                         source_rows_read=src_rows, convert_ms=med(conv_ms), convert_TBps=touched / med(conv_ms) / 1e9,
                         memcpy_touched_ms=med(full_ms), memcpy_same_traffic_ms=med(half_ms),
                         memcpy_same_traffic_TBps=touched / med(half_ms) / 1e9,
                         convert_over_memcpy_same_traffic=med(conv_ms) / med(half_ms),
                         convert_over_memcpy_touched=med(conv_ms) / med(full_ms),
                         convert_over_step=med(conv_ms) / STEP_MS,
                         spread_ms=dict(convert=[min(conv_ms), max(conv_ms)], memcpy_same_traffic=[min(half_ms), max(half_ms)])))
        cv.close()
        del raw, scratch_a, scratch_b
        torch.cuda.empty_cache()
    res = dict(commit=commit(), library="another build (SL2_LIB_PATH)" if os.environ.get("SL2_LIB_PATH") else "this build", filter=args.filter,
               device=torch.cuda.get_device_name(0), batch=B, out_width=ow, out_height=oh, reps=args.reps,
               headline_step_ms=STEP_MS, runs=runs,
               note="bytes_touched below 256 MiB (the native copy) can live in the Infinity Cache between repeats: for the "
                    "conversion and for the copy alike")
    if args.filter == "raw":          # each new source over the GRAY8 source timed right after it
        res["over_gray8"] = [dict(source=a["source"], filter=a["filter"], convert_ms=a["convert_ms"], gray8_ms=b["convert_ms"],
                                  convert_over_gray8=a["convert_ms"] / b["convert_ms"],
                                  convert_over_memcpy_same_traffic=a["convert_over_memcpy_same_traffic"])
                             for a, b in zip(runs[0::2], runs[1::2])]
    if args.linear_json and args.linear_parent_json:
        res["linear_unchanged"] = unchanged(args.linear_json, args.linear_parent_json)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def bench_remap(args, B, ow, oh, stream, out, timed, med):
    runs = []
    for name, w, h, fmt in REMAP_SOURCES:
        bpp = convert.BYTES_PER_PIXEL[convert.FORMATS[fmt]]
        frame = w * h * bpp
        g = torch.Generator(device="cuda")
        g.manual_seed(w * 31 + bpp)
        raw = torch.randint(0, 256, (B * frame,), dtype=torch.uint8, device="cuda", generator=g)
        cv = convert.FrameConverter(0, B, ow, oh)
        cv.set_sources([dict(width=w, height=h, format=fmt, offset=s * frame) for s in range(B)])
        go = lambda: cv.convert((raw.data_ptr(), raw.numel()), out.data_ptr(), stream=stream.cuda_stream)
        go()
        stream.synchronize()
        linear_ms = timed(go)                      # the same source through the existing LINEAR kernel, in this run
        linear_rows = rows_read(h, oh, halo=fmt.startswith("bayer"))
        linear_touched = B * linear_rows * w * bpp + B * ow * oh
        for model in ("brown", "fisheye"):
            lens = remap_lens(model, w, h)
            target = convert.pinhole_camera(lens, ow, oh)
            base = convert.lens_map(lens, target)
            pixels, lines = remap_reach(base, w, h, w * bpp, bpp, fmt.startswith("bayer"))
            for arrangement in ("shared", "distinct"):
                nslots = 1 if arrangement == "shared" else B
                maps = []
                for k in range(nslots):          # a map per sequence: the same map moved by a unit (1/32 pixel) in X, in Y, in both or not at all
                    xy = base.copy()
                    if k:
                        xy[..., 0] = np.where(base[..., 0] == convert.SL2_REMAP_BORDER, base[..., 0], base[..., 0] + (k % 2))
                        xy[..., 1] = np.where(base[..., 0] == convert.SL2_REMAP_BORDER, base[..., 1], base[..., 1] + ((k // 2) % 2))
                    cv.set_map(k, w, h, xy)
                    if k < 4 or k == nslots - 1:
                        maps.append((k, xy))
                cv.set_remaps([s % nslots for s in range(B)])
                go()
                stream.synchronize()
                for k, xy in maps:          # the bytes are right before their time is worth anything
                    s = k if arrangement == "distinct" else (0, B // 2, B - 1)[k % 3]
                    want = convert.remap_frame_host(dict(width=w, height=h, format=fmt), xy, raw[s * frame:(s + 1) * frame].cpu().numpy())
                    assert np.array_equal(out[s * ow * oh:(s + 1) * ow * oh].cpu().numpy().reshape(oh, ow), want), (name, model, arrangement, s)
                entry = 4 if (32 * (w + 1) - 1).bit_length() + (32 * (h + 1) - 1).bit_length() <= 32 else 8
                map_bytes = nslots * ow * oh * entry
                read = B * lines * 128
                touched = map_bytes + read + B * ow * oh
                ms = timed(go)
                scratch_a = torch.empty(touched, dtype=torch.uint8, device="cuda")
                scratch_b = torch.empty(touched, dtype=torch.uint8, device="cuda")

                def d2d(n):
                    def fn():
                        with torch.cuda.stream(stream):
                            scratch_b[:n].copy_(scratch_a[:n], non_blocking=True)
                    return fn

                half_ms = timed(d2d(touched // 2))
                runs.append(dict(source=name, lens=model, maps=arrangement, map_slots=nslots, map_entry_bytes=entry, map_bytes=map_bytes,
                                 map_bytes_read_by_workgroups=B * ow * oh * entry, border_entries=int((base[..., 0] == convert.SL2_REMAP_BORDER).sum()),
                                 source_pixels_named=pixels, source_lines_128B=lines, bytes_read_source=read, source_bytes_named=B * pixels * bpp,
                                 raw_bytes=B * frame, bytes_written=B * ow * oh, bytes_touched=touched,
                                 remap_ms=med(ms), remap_TBps=touched / med(ms) / 1e9, linear_ms=med(linear_ms),
                                 linear_bytes_touched=linear_touched, remap_over_linear=med(ms) / med(linear_ms),
                                 memcpy_same_traffic_ms=med(half_ms), memcpy_same_traffic_TBps=touched / med(half_ms) / 1e9,
                                 remap_over_memcpy_same_traffic=med(ms) / med(half_ms), remap_over_step=med(ms) / STEP_MS,
                                 spread_ms=dict(remap=[min(ms), max(ms)], linear=[min(linear_ms), max(linear_ms)],
                                                memcpy_same_traffic=[min(half_ms), max(half_ms)])))
                print(json.dumps(runs[-1]), flush=True)
                del scratch_a, scratch_b
                cv.set_remaps([-1] * B)
                for k in range(nslots):
                    cv.set_map(k)
        cv.close()
        del raw
        torch.cuda.empty_cache()
    by = {(r["source"], r["lens"]): {} for r in runs}
    for r in runs:
        by[(r["source"], r["lens"])][r["maps"]] = r
    distinct_over_shared = [dict(source=s, lens=l, shared_ms=v["shared"]["remap_ms"], distinct_ms=v["distinct"]["remap_ms"],
                                 extra_ms=v["distinct"]["remap_ms"] - v["shared"]["remap_ms"],
                                 extra_map_bytes=v["distinct"]["map_bytes"] - v["shared"]["map_bytes"],
                                 extra_bytes_at_the_copy_rate_ms=(v["distinct"]["map_bytes"] - v["shared"]["map_bytes"]) /
                                 (v["distinct"]["memcpy_same_traffic_TBps"] * 1e9)) for (s, l), v in by.items()]
    res = dict(commit=commit(), library="another build (SL2_LIB_PATH)" if os.environ.get("SL2_LIB_PATH") else "this build", filter="remap",
               device=torch.cuda.get_device_name(0), batch=B, out_width=ow, out_height=oh, reps=args.reps, headline_step_ms=STEP_MS, runs=runs,
               distinct_over_shared=distinct_over_shared,
               note="bytes_touched = the map entries of every slot + 128-byte source lines that some tap names, per sequence + the output; "
                    "a shared map is read by every workgroup (map_bytes_read_by_workgroups) but from the cache")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(out=args.out, runs=len(runs))))


if __name__ == "__main__":
    main()
