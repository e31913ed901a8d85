// The undistorted frame (include/scenelib2_amd.h, "the rectified view"): the image half of
// GraphicTool::DrawRectifiedAR (graphic/graphictool.cpp:222-283, DrawFrame 799-836) for a range of sequences, exact per pixel
// where the reference stretches a 10 x 10 mesh.  One launch; no workgroup waits for another.  The pixel rule is
// sl2_rectify_dev.hpp's, shared with sl2_rectify_frame_host.  The scene half (DrawRectifiedAR's features, ellipsoids, rays and
// trajectory) is a draw list per sequence (k_scene_list) for the rasteriser of sl2_overlay.hip; sl2_draw_rectified chains the
// three launches on the engine's stream.
#include "sl2_display.hpp"
#include "sl2_drawlist_dev.hpp"
#include "sl2_rectify_dev.hpp"

namespace sl2 {

constexpr int kRectThreads = 256;
constexpr int kRectTileW = 64, kRectTileH = 16;      // a thread owns 4 consecutive pixels of a row: one dword of the output

// A workgroup per (image, tile of 64 x 16 output pixels).  The source is GATHERED THROUGH THE CACHES, not staged in LDS: the
// map is smooth and nearly the identity, so the four taps of the 64 x 16 pixels of a tile fall into a source window of about
// the tile's own size - some twenty 64-byte lines that the CU's vector cache holds after the first touch - while the window's
// extent depends on kd1 and the tile's place (it grows without bound for kd1 < 0 towards the corners), which a static LDS
// tile would have to bound and a fallback would have to catch.  The arithmetic is what costs: an FP64 square root and two FP64
// divisions a pixel.  The camera is the sequence's own, read from its line of seq_cam with a workgroup-uniform address.
struct RectifyArgs {
  const uint8_t* frames; size_t seq_stride;
  int seq0, width, height, tiles_x, tiles;
  uint8_t* out; size_t out_stride;
  int dword_out;      // every row of every output image starts on a 4-byte boundary: a thread's 4 bytes go out as one dword
};

__global__ void __launch_bounds__(kRectThreads) k_rectify(const SeqArrays S, const RectifyArgs A) {
  const int tid = threadIdx.x;
  const int img = blockIdx.x / A.tiles, tile = blockIdx.x % A.tiles;
  const int px = (tile % A.tiles_x) * kRectTileW + (tid & 15) * 4, py = (tile / A.tiles_x) * kRectTileH + (tid >> 4);
  if (py >= A.height || px >= A.width) return;
  const CameraParams cam = load_cam(S.seq_cam, A.seq0 + img, A.width, A.height);
  const uint8_t* __restrict__ src = A.frames + (size_t)img * A.seq_stride;
  uint8_t* o = A.out + (size_t)img * A.out_stride + (size_t)py * A.width + px;
  uint32_t v[4];
  for (int j = 0; j < 4; ++j) v[j] = px + j < A.width ? rectify_pixel(src, A.width, A.height, cam.u0, cam.v0, cam.kd1, px + j, py) : 0u;
  if (A.dword_out && px + 3 < A.width) {
    *reinterpret_cast<uint32_t*>(o) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);      // px is a multiple of 4
  } else {
    for (int j = 0; j < 4; ++j)
      if (px + j < A.width) o[j] = (uint8_t)v[j];
  }
}

// ---- the scene's draw list of sequence seq0 + i: one wavefront (sl2_drawlist_dev.hpp).  First the trajectory, then the features,
// a lane per slot, 64 slots a round (up to three items each, placed in slot order).
__global__ void __launch_bounds__(kListThreads) k_scene_list(const SeqArrays S, int seq0, int nseq, int N, int ld, int ppos, int kpart, int width,
                                                             int height, int layers, const int32_t* __restrict__ marked,
                                                             sl2_overlay_item* __restrict__ items, int item_stride, int32_t* __restrict__ counts) {
  SeqWave w;
  if (!seq_wave(S, seq0, nseq, N, ld, kpart, marked, &w)) return;
  const CameraParams cam = load_cam(S.seq_cam, w.seq, width, height);
  const double* xb = w.xb;
  const double* Pb = S.P + (size_t)w.seq * ld * ld;
  ListWriter list(items, w.i, item_stride, w.lane);
  double xp[7];
  for (int k = 0; k < 7; ++k) xp[k] = xb[k];
  if (layers & SL2_SCENE_TRAJECTORY)
    list_trajectory(list, S, w.seq, [&](const double* older, const double* newer, int* c) {
      double a[3], b[3];
      zeroedyi_only(xp, older, a);
      zeroedyi_only(xp, newer, b);
      return scene_segment(cam.fku, cam.fkv, cam.u0, cam.v0, a, b, c);
    });
  if (layers & (SL2_SCENE_FEATURES | SL2_SCENE_UNCERTAINTIES))
    for (int base = 0; base < w.ns; base += 64) {
      const int f = base + w.lane;
      const SlotClass s = classify_slot(S, w.o, f, w.ns);
      bool has_marker = false, has_ring = false, has_ray = false;
      int mx = 0, my = 0, rx = 0, ry = 0, ray[4] = {0, 0, 0, 0};
      double q[4] = {0.0, 0.0, 0.0, 0.0};
      if (s.full) {
        const int pos = 13 + 3 * f;
        double m[3];
        if (layers & SL2_SCENE_UNCERTAINTIES) {
          double Jx[21], Jy[9], Pxx7[49], Pxy7[21], Pyy[9], Sg[9], centre[2];
          scene_zeroed_jac(xp, xb + pos, m, Jx, Jy);
          for (int r = 0; r < 7; ++r) {
            for (int c = 0; c < 7; ++c) Pxx7[r * 7 + c] = Pb[(size_t)r * ld + c];
            for (int c = 0; c < 3; ++c) Pxy7[r * 3 + c] = Pb[(size_t)r * ld + pos + c];
          }
          for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Pyy[r * 3 + c] = Pb[(size_t)(pos + r) * ld + pos + c];
          scene_sigma(Jx, Jy, Pxx7, Pxy7, Pyy, Sg);
          has_ring = scene_conic(cam.fku, cam.fkv, cam.u0, cam.v0, m, Sg, centre, q) && overlay_round(centre[0], &rx) && overlay_round(centre[1], &ry);
        } else {
          zeroedyi_only(xp, xb + pos, m);
        }
        if ((layers & SL2_SCENE_FEATURES) && m[2] >= kSceneNear) {
          double p[2];
          scene_project(cam.fku, cam.fkv, cam.u0, cam.v0, m, p);
          has_marker = overlay_round(p[0], &mx) && overlay_round(p[1], &my);
        }
      } else if (s.part && (layers & SL2_SCENE_FEATURES)) {
        const int ks = partial_slot_of(w.psb, kpart, f);
        if (ks >= 0) {
          // the partial model's zeroed state (part_feature_model.cpp:80-146): RRW (r_i - r) and RRW hhat_i
          const double* y6 = xb + ppos + 6 * ks;
          const double xq[7] = {0.0, 0.0, 0.0, xp[3], xp[4], xp[5], xp[6]};
          double a[3], hh[3], b[3];
          zeroedyi_only(xp, y6, a);
          zeroedyi_only(xq, y6 + 3, hh);
          for (int k = 0; k < 3; ++k) b[k] = a[k] + kSceneRayLength * hh[k];
          has_ray = scene_segment(cam.fku, cam.fkv, cam.u0, cam.v0, a, b, ray);
        }
      }
      list_feature(list, s, w.mark, has_marker, mx, my, has_ring, rx, ry, q, has_ray, ray);
    }
  list.finish(counts, w.i);
}

// one launch of k_rectify: device frames in, device images out
static int launch_rectify(sl2_engine* e, int seq0, int nseq, const uint8_t* d_frames, size_t seq_stride, uint8_t* d_out, size_t out_stride) {
  const int W = e->cam.width, H = e->cam.height;
  RectifyArgs A;
  A.frames = d_frames; A.seq_stride = seq_stride;
  A.seq0 = seq0; A.width = W; A.height = H;
  A.tiles_x = (W + kRectTileW - 1) / kRectTileW;
  A.tiles = A.tiles_x * ((H + kRectTileH - 1) / kRectTileH);
  A.out = d_out; A.out_stride = out_stride;
  A.dword_out = (W % 4 == 0 && (uintptr_t)d_out % 4 == 0 && out_stride % 4 == 0) ? 1 : 0;
  // (the root's arrays on the engine's stream, like sl2_overlay_items: the groups' streams join it at the end of every stepping call)
  LaunchScope ls(e, "k_rectify");
  hipLaunchKernelGGL(k_rectify, dim3((unsigned)(nseq * A.tiles)), dim3(kRectThreads), 0, e->stream, seq_arrays(e), A);
  SL2_HIP(hipGetLastError());
  return SL2_OK;
}

static int launch_scene_list(sl2_engine* e, int seq0, int nseq, int layers, const ListStage& d) {
  LaunchScope ls(e, "k_scene_list");
  hipLaunchKernelGGL(k_scene_list, dim3((nseq + kListSeqs - 1) / kListSeqs), dim3(kListThreads), 0, e->stream, seq_arrays(e), seq0, nseq, e->N, e->ld,
                     e->ppos, e->kpart, e->cam.width, e->cam.height, layers, d.marked, d.items, d.stride, d.counts);
  SL2_HIP(hipGetLastError());
  return SL2_OK;
}

}  // namespace sl2

using namespace sl2;

extern "C" int sl2_rectify_frame_host(const uint8_t* frame, int width, int height, double u0, double v0, double kd1, uint8_t* out) {
  if (!frame || !out) { set_error("sl2_rectify_frame_host: null pointer"); return SL2_ERR_INVALID; }
  if (width < 1 || height < 1 || width > kRectifyMaxSide || height > kRectifyMaxSide) {
    set_error("sl2_rectify_frame_host: width or height outside 1 .. 32768");
    return SL2_ERR_INVALID;
  }
  if (!(u0 - u0 == 0.0 && v0 - v0 == 0.0 && kd1 - kd1 == 0.0)) { set_error("sl2_rectify_frame_host: u0, v0 or kd1 not finite"); return SL2_ERR_INVALID; }
  rectify_host_body(frame, width, height, u0, v0, kd1, out);
  return SL2_OK;
}

extern "C" int sl2_rectify_frames(sl2_engine* e, int seq0, int nseq, const uint8_t* frames, size_t seq_stride, int frames_on_device, uint8_t* out,
                                  size_t out_stride, int out_on_device) {
  const char* why = range_fault(e, seq0, nseq, 0, 0, nullptr);      // (no layers)
  const int W = e ? e->cam.width : 0, H = e ? e->cam.height : 0;
  if (!why && (!frames || !out)) why = "null frames or out";
  if (!why && seq_stride < (size_t)W * (size_t)H) why = "seq_stride below width * height";
  if (!why && out_stride < (size_t)W * (size_t)H) why = "out_stride below width * height";      // (one byte a pixel: not geometry_fault's rule)
  const long long tiles_x = (W + kRectTileW - 1) / kRectTileW, tiles = tiles_x * ((H + kRectTileH - 1) / kRectTileH);
  if (!why && (W > kRectifyMaxSide || H > kRectifyMaxSide || tiles * nseq > 0x7fffffffll)) why = "more tiles than one launch takes";
  if (why) { set_error(range_text("sl2_rectify_frames", "sequences", seq0, nseq, why)); return SL2_ERR_INVALID; }
  SL2_HIP(hipSetDevice(e->device));
  // image staging (shared with sl2_draw_overlays, which orders itself on the same stream): host frames on their way in
  // (packed), then host-bound images on their way out (packed)
  const size_t px = (size_t)W * H;
  const size_t in_bytes = frames_on_device ? 0 : ((px * (size_t)nseq + 255) & ~(size_t)255), out_bytes = out_on_device ? 0 : px * (size_t)nseq;
  { int _rc = grow_device(&e->ovl_images, &e->ovl_images_bytes, in_bytes + out_bytes); if (_rc != SL2_OK) return _rc; }
  const uint8_t* d_frames = frames;
  size_t d_seq_stride = seq_stride;
  if (!frames_on_device) {
    SL2_HIP(hipMemcpy2DAsync(e->ovl_images, px, frames, seq_stride, px, (size_t)nseq, hipMemcpyHostToDevice, e->stream));
    d_frames = (const uint8_t*)e->ovl_images; d_seq_stride = px;
    // The caller's frames may be pageable memory and may be reused the moment the call returns.  The host form waits at its end
    // anyway; with the output left on the device this is the one place the call waits: until the frames have been copied.
    if (out_on_device) SL2_HIP(hipStreamSynchronize(e->stream));
  }
  uint8_t* d_out = out_on_device ? out : (uint8_t*)e->ovl_images + in_bytes;
  { int _rc = launch_rectify(e, seq0, nseq, d_frames, d_seq_stride, d_out, out_on_device ? out_stride : px); if (_rc != SL2_OK) return _rc; }
  if (out_on_device) return SL2_OK;
  SL2_HIP(hipMemcpy2DAsync(out, out_stride, d_out, px, px, (size_t)nseq, hipMemcpyDeviceToHost, e->stream));
  SL2_HIP(hipStreamSynchronize(e->stream));
  return SL2_OK;
}

extern "C" size_t sl2_scene_item_bound(int max_features, int partial_slots) {
  if (max_features < 0 || partial_slots < 0) return 0;
  return 3 * (size_t)max_features + (size_t)partial_slots + (size_t)(kTrajCapacity - 1);
}

extern "C" int sl2_scene_items(sl2_engine* e, int seq0, int nseq, int layers, const int32_t* marked, sl2_overlay_item* items, int item_stride,
                               int32_t* counts, int on_device) {
  const char* why = range_fault(e, seq0, nseq, layers, SL2_SCENE_ALL, "layers with bits outside SL2_SCENE_ALL");
  return items_call("sl2_scene_items", e, seq0, nseq, why, sl2_scene_item_bound, "item_stride below sl2_scene_item_bound", nullptr, 0, marked, items,
                    item_stride, counts, nullptr, on_device, [&](const ListStage& d) { return launch_scene_list(e, seq0, nseq, layers, d); });
}

extern "C" int sl2_draw_rectified(sl2_engine* e, int seq0, int nseq, const uint8_t* frames, size_t seq_stride, int frames_on_device, int layers,
                                  const int32_t* marked, uint8_t* out, size_t out_stride, int out_on_device) {
  const char* why = range_fault(e, seq0, nseq, layers, SL2_SCENE_ALL, "layers with bits outside SL2_SCENE_ALL");
  if (!why && (!frames || !out)) why = "null frames or out";
  if (!why) why = geometry_fault(nseq, e->cam.width, e->cam.height, seq_stride, out_stride);
  if (why) { set_error(range_text("sl2_draw_rectified", "sequences", seq0, nseq, why)); return SL2_ERR_INVALID; }
  const int W = e->cam.width, H = e->cam.height;
  // the rasteriser draws over the rectified frames
  return draw_call(e, nseq, W, H, sl2_scene_item_bound(e->N, e->kpart), frames, seq_stride, frames_on_device, nullptr, 0, marked, nullptr, out, out_stride,
                   out_on_device,
                   [&](const uint8_t* d_frames, size_t d_seq_stride, uint8_t* d_grey) {
                     return launch_rectify(e, seq0, nseq, d_frames, d_seq_stride, d_grey, (size_t)W * H);
                   },
                   [&](const ListStage& d) { return launch_scene_list(e, seq0, nseq, layers, d); });
}
