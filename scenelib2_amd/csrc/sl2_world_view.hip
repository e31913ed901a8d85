// The world view and picking (include/scenelib2_amd.h, "the world view and picking"): the numerical half
// of GraphicTool::Draw3dScene (graphic/graphictool.cpp:113-175) and of GraphicTool::Picker (1475-1571) for a range of
// sequences.  k_world_list lists the map, the trajectory, the camera glyph and the axes as seen from a free camera, for the
// rasteriser of sl2_overlay.hip; k_pick_items answers which labelled item of any draw list covers a click's window.  The
// arithmetic is sl2_world_view_dev.hpp's, shared with sl2_pick_items_host.  No workgroup waits for another.
#include "sl2_display.hpp"
#include "sl2_drawlist_dev.hpp"
#include "sl2_rectify_dev.hpp"
#include "sl2_world_view_dev.hpp"

namespace sl2 {

static_assert(sizeof(sl2_view) == 88, "sl2_view is 88 bytes");

constexpr int kPickThreads = 256;
constexpr int kPickImages = kPickThreads / 64;      // images per workgroup of k_pick_items, a wavefront each

__device__ __forceinline__ double wave_min(double v) {
  for (int d = 32; d > 0; d >>= 1) { const double t = __shfl_xor(v, d); if (t < v) v = t; }
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
  for (int d = 32; d > 0; d >>= 1) { const double t = __shfl_xor(v, d); if (t > v) v = t; }
  return v;
}

// ---- the world's draw list of sequence seq0 + i: one wavefront (sl2_drawlist_dev.hpp).  The glyph's 16 edges, the trajectory's
// pairs and the three axes yield one item or none per lane; the features, a lane per slot, 64 slots a round, up to three, placed
// in slot order.  Every lane keeps the extents of the slots it saw; a wave min / max after the last round makes them the map's,
// before the axes are listed.
__global__ void __launch_bounds__(kListThreads) k_world_list(const SeqArrays S, int seq0, int nseq, int N, int ld, int ppos, int kpart,
                                                             const sl2_view* __restrict__ views, int nviews, int layers,
                                                             const int32_t* __restrict__ marked, sl2_overlay_item* __restrict__ items,
                                                             int item_stride, int32_t* __restrict__ counts, double* __restrict__ extents) {
  SeqWave w;
  if (!seq_wave(S, seq0, nseq, N, ld, kpart, marked, &w)) return;
  const int lane = w.lane;
  const sl2_view view = views[nviews == 1 ? 0 : w.i];
  const double* xb = w.xb;
  const double* Pb = S.P + (size_t)w.seq * ld * ld;
  ListWriter list(items, w.i, item_stride, lane);
  double xp[7], xv[7];
  world_view_pose(view, xp);
  for (int k = 0; k < 7; ++k) xv[k] = xb[k];
  if (layers & SL2_WORLD_CAMERA) {
    const uint8_t grey[3] = {150, 150, 150};
    int c[4] = {0, 0, 0, 0};
    const bool ok = lane < kWorldGlyphEdges && world_glyph_segment(view, xp, xv, lane, c);
    const int at = list.one(ok);
    if (ok) list.put(at, draw_item(SL2_ITEM_SEGMENT, -1, c[0], c[1], c[2], c[3], grey));
  }
  if (layers & SL2_WORLD_TRAJECTORY)
    list_trajectory(list, S, w.seq, [&](const double* older, const double* newer, int* c) { return world_segment(view, xp, older, newer, c); });
  // the extents: r of xv_ (every lane, the same), then the lane's own slots
  // (six named scalars, not an array: the axes pick theirs by lane, and an index known only at run time would put it in scratch)
  double xmin = 0.0, xmax = 0.0, ymin = 0.0, ymax = 0.0, zmin = 0.0, zmax = 0.0;
  world_extend(&xmin, &xmax, xv[0]); world_extend(&ymin, &ymax, xv[1]); world_extend(&zmin, &zmax, xv[2]);
  const bool list_features = (layers & (SL2_WORLD_FEATURES | SL2_WORLD_UNCERTAINTIES)) != 0;
  for (int base = 0; base < w.ns; base += 64) {
    const int f = base + lane;
    const SlotClass s = classify_slot(S, w.o, f, w.ns);
    bool has_marker = false, has_ring = false, has_ray = false;
    int mk[2] = {0, 0}, rc[2] = {0, 0}, ray[4] = {0, 0, 0, 0};
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    if (s.full) {
      const int pos = 13 + 3 * f;
      if (layers & SL2_WORLD_FEATURES) { world_extend(&xmin, &xmax, xb[pos]); world_extend(&ymin, &ymax, xb[pos + 1]); world_extend(&zmin, &zmax, xb[pos + 2]); }
      if (list_features) {
        const bool want_ring = (layers & SL2_WORLD_UNCERTAINTIES) != 0;
        double Pyy[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (want_ring)
          for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Pyy[r * 3 + c] = Pb[(size_t)(pos + r) * ld + pos + c];
        world_feature(view, xp, xb + pos, Pyy, (layers & SL2_WORLD_FEATURES) != 0, want_ring, &has_marker, mk, &has_ring, rc, q);
      }
    } else if (s.part && (layers & SL2_WORLD_FEATURES)) {
      const int ks = partial_slot_of(w.psb, kpart, f);
      if (ks >= 0) has_ray = world_ray(view, xp, xb + ppos + 6 * ks, ray);
    }
    if (!list_features) continue;                      // (wave-uniform: the round only fed the extents)
    list_feature(list, s, w.mark, has_marker, mk[0], mk[1], has_ring, rc[0], rc[1], q, has_ray, ray);
  }
  xmin = wave_min(xmin); xmax = wave_max(xmax);
  ymin = wave_min(ymin); ymax = wave_max(ymax);
  zmin = wave_min(zmin); zmax = wave_max(zmax);
  if (layers & SL2_WORLD_AXES) {
    const uint8_t white[3] = {255, 255, 255};
    int c[4] = {0, 0, 0, 0};
    const double lo = lane == 0 ? xmin : (lane == 1 ? ymin : zmin), hi = lane == 0 ? xmax : (lane == 1 ? ymax : zmax);
    const bool ok = lane < kWorldAxes && world_axis_segment(view, xp, lo, hi, lane, c);
    const int at = list.one(ok);
    if (ok) list.put(at, draw_item(SL2_ITEM_SEGMENT, -1, c[0], c[1], c[2], c[3], white));
  }
  list.finish(counts, w.i);
  if (lane == 0 && extents) {
    double* ex = extents + (size_t)w.i * 6;
    ex[0] = xmin; ex[1] = xmax; ex[2] = ymin; ex[3] = ymax; ex[4] = zmin; ex[5] = zmax;
  }
}

// ---- picking: a wavefront per image, lanes over the items, 64 a round; every lane keeps the largest index of its items that
// cover a pixel of the window, a wave max makes it the list's.  A count is clamped as in the rasteriser.
__global__ void __launch_bounds__(kPickThreads) k_pick_items(int nimages, int width, int height, const sl2_overlay_item* __restrict__ items,
                                                             int item_stride, const int32_t* __restrict__ counts, int npatches,
                                                             const int32_t* __restrict__ clicks, int32_t* __restrict__ picked) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * kPickImages + (threadIdx.x >> 6);
  if (i >= nimages) return;                            // (a whole wavefront)
  const int count = min(max(counts[i], 0), item_stride);
  const sl2_overlay_item* list = items + (size_t)i * item_stride;
  int x0 = 0, y0 = 0, x1 = -1, y1 = -1;
  const bool inside = pick_window(width, height, clicks[2 * i], clicks[2 * i + 1], &x0, &y0, &x1, &y1);   // wave-uniform
  int best = -1;
  if (inside)
    for (int base = 0; base < count; base += 64) {
      const int k = base + lane;
      if (k < count && pick_item_hits(list[k], npatches, x0, y0, x1, y1)) best = k;
    }
  for (int d = 32; d > 0; d >>= 1) best = max(best, __shfl_xor(best, d));
  if (lane != 0) return;
  picked[2 * i] = best >= 0 ? list[best].label : -1;
  picked[2 * i + 1] = best;
}

static int launch_world_list(sl2_engine* e, int seq0, int nseq, int nviews, int layers, const ListStage& d) {
  // (the root's arrays on the engine's stream, like sl2_scene_items: the groups' streams join it at the end of every stepping call)
  LaunchScope ls(e, "k_world_list");
  hipLaunchKernelGGL(k_world_list, dim3((nseq + kListSeqs - 1) / kListSeqs), dim3(kListThreads), 0, e->stream, seq_arrays(e), seq0, nseq, e->N, e->ld,
                     e->ppos, e->kpart, d.views, nviews, layers, d.marked, d.items, d.stride, d.counts, d.extents);
  SL2_HIP(hipGetLastError());
  return SL2_OK;
}

// why a range of sequences cannot be seen through these views (nullptr: it can)
static const char* world_range_fault(const sl2_engine* e, int seq0, int nseq, const sl2_view* views, int nviews, int layers) {
  const char* views_fault = !views ? "null views" : (nviews != 1 && nviews != nseq) ? "nviews is neither 1 nor nseq" : nullptr;
  return range_fault(e, seq0, nseq, layers, SL2_WORLD_ALL, "layers with bits outside SL2_WORLD_ALL", views_fault);
}

}  // namespace sl2

using namespace sl2;

extern "C" int sl2_view_look_at(const double eye[3], const double target[3], const double up[3], double fku, double fkv, double u0, double v0,
                                sl2_view* out) {
  if (!eye || !target || !up || !out) { set_error("sl2_view_look_at: null pointer"); return SL2_ERR_INVALID; }
  const double in[13] = {eye[0], eye[1], eye[2], target[0], target[1], target[2], up[0], up[1], up[2], fku, fkv, u0, v0};
  for (double d : in)
    if (!overlay_finite(d)) { set_error("sl2_view_look_at: a number that is not finite"); return SL2_ERR_INVALID; }
  double z[3] = {target[0] - eye[0], target[1] - eye[1], target[2] - eye[2]};
  const double zn = sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
  if (!(zn > 0.0) || !overlay_finite(zn)) { set_error("sl2_view_look_at: eye and target coincide"); return SL2_ERR_INVALID; }
  for (int k = 0; k < 3; ++k) z[k] /= zn;
  double x[3] = {up[1] * z[2] - up[2] * z[1], up[2] * z[0] - up[0] * z[2], up[0] * z[1] - up[1] * z[0]};
  const double xn = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]), un = sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2]);
  if (!(un > 0.0) || !overlay_finite(un) || !(xn > 1e-12 * un)) {
    set_error("sl2_view_look_at: up is zero or parallel to the viewing direction");
    return SL2_ERR_INVALID;
  }
  for (int k = 0; k < 3; ++k) x[k] /= xn;
  const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
  // RWR has the columns x, y, z; its quaternion by the branch with the largest pivot (Shepperd), then normalised
  const double m00 = x[0], m01 = y[0], m02 = z[0], m10 = x[1], m11 = y[1], m12 = z[1], m20 = x[2], m21 = y[2], m22 = z[2];
  const double tr = m00 + m11 + m22;
  double q[4];
  if (tr > 0.0) {
    const double s = sqrt(tr + 1.0) * 2.0;
    q[0] = 0.25 * s; q[1] = (m21 - m12) / s; q[2] = (m02 - m20) / s; q[3] = (m10 - m01) / s;
  } else if (m00 > m11 && m00 > m22) {
    const double s = sqrt(1.0 + m00 - m11 - m22) * 2.0;
    q[0] = (m21 - m12) / s; q[1] = 0.25 * s; q[2] = (m01 + m10) / s; q[3] = (m02 + m20) / s;
  } else if (m11 > m22) {
    const double s = sqrt(1.0 + m11 - m00 - m22) * 2.0;
    q[0] = (m02 - m20) / s; q[1] = (m01 + m10) / s; q[2] = 0.25 * s; q[3] = (m12 + m21) / s;
  } else {
    const double s = sqrt(1.0 + m22 - m00 - m11) * 2.0;
    q[0] = (m10 - m01) / s; q[1] = (m02 + m20) / s; q[2] = (m12 + m21) / s; q[3] = 0.25 * s;
  }
  const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double sgn = q[0] < 0.0 ? -1.0 : 1.0;
  for (int k = 0; k < 4; ++k) out->q[k] = sgn * (q[k] / qn);
  if (out->q[0] == 0.0) out->q[0] = 0.0;      // (no negative zero)
  for (int k = 0; k < 3; ++k) out->r[k] = eye[k];
  out->fku = fku; out->fkv = fkv; out->u0 = u0; out->v0 = v0;
  return SL2_OK;
}

extern "C" size_t sl2_world_item_bound(int max_features, int partial_slots) {
  if (max_features < 0 || partial_slots < 0) return 0;
  return 3 * (size_t)max_features + (size_t)partial_slots + (size_t)(kTrajCapacity - 1) + (size_t)(kWorldGlyphEdges + kWorldAxes);
}

extern "C" int sl2_world_items(sl2_engine* e, int seq0, int nseq, const sl2_view* views, int nviews, int layers, const int32_t* marked,
                               sl2_overlay_item* items, int item_stride, int32_t* counts, double* extents, int on_device) {
  const char* why = world_range_fault(e, seq0, nseq, views, nviews, layers);
  return items_call("sl2_world_items", e, seq0, nseq, why, sl2_world_item_bound, "item_stride below sl2_world_item_bound", views, nviews, marked, items,
                    item_stride, counts, extents, on_device, [&](const ListStage& d) { return launch_world_list(e, seq0, nseq, nviews, layers, d); });
}

extern "C" int sl2_draw_world(sl2_engine* e, int seq0, int nseq, const sl2_view* views, int nviews, int width, int height, int background,
                              int layers, const int32_t* marked, uint8_t* out, size_t out_stride, int out_on_device) {
  const char* why = world_range_fault(e, seq0, nseq, views, nviews, layers);
  if (!why && !out) why = "null out";
  if (!why && (background < 0 || background > 255)) why = "background outside 0 .. 255";
  if (!why && out_on_device && (uintptr_t)views % 8) why = "device views not 8-byte aligned";
  if (!why) why = geometry_fault(nseq, width, height, (size_t)(width > 0 ? width : 0) * (size_t)(height > 0 ? height : 0), out_stride);
  if (why) { set_error(range_text("sl2_draw_world", "sequences", seq0, nseq, why)); return SL2_ERR_INVALID; }
  if (!out_on_device) {
    const std::string bad = view_fault_text("sl2_draw_world", seq0, nseq, views, nviews);
    if (!bad.empty()) { set_error(bad); return SL2_ERR_INVALID; }
  }
  // the rasteriser draws over constant grey frames
  return draw_call(e, nseq, width, height, sl2_world_item_bound(e->N, e->kpart), nullptr, 0, 0, views, nviews, marked, nullptr, out, out_stride, out_on_device,
                   [&](const uint8_t*, size_t, uint8_t* d_grey) {
                     SL2_HIP(hipMemsetAsync(d_grey, background, (size_t)width * height * (size_t)nseq, e->stream));
                     return SL2_OK;
                   },
                   [&](const ListStage& d) { return launch_world_list(e, seq0, nseq, nviews, layers, d); });
}

extern "C" int sl2_pick_items_host(int width, int height, const sl2_overlay_item* items, int count, int npatches, int x, int y, int32_t picked[2]) {
  if (!picked || count < 0 || (count > 0 && !items) || npatches < 0) {
    set_error("sl2_pick_items_host: null pointer or negative count or npatches");
    return SL2_ERR_INVALID;
  }
  if (width < 1 || height < 1 || width > kOverlayMaxSide || height > kOverlayMaxSide) {
    set_error("sl2_pick_items_host: width or height outside 1 .. 32768");
    return SL2_ERR_INVALID;
  }
  pick_host_body(width, height, items, count, npatches, x, y, picked);
  return SL2_OK;
}

extern "C" int sl2_pick_items_batch(int device, void* stream, int nimages, int width, int height, const sl2_overlay_item* items, int item_stride,
                                    const int32_t* counts, int npatches, const int32_t* clicks, int32_t* picked, int on_device) {
  const char* why = nullptr;
  if (nimages < 1) why = "no images";
  else if (!items || !counts || !clicks || !picked) why = "null pointer";
  else if (item_stride < 0 || npatches < 0) why = "negative item_stride or npatches";
  else if (width < 1 || height < 1 || width > kOverlayMaxSide || height > kOverlayMaxSide) why = "width or height outside 1 .. 32768";
  else if (on_device && (uintptr_t)items % 8) why = "device items not 8-byte aligned";
  if (why) { set_error(range_text("sl2_pick_items_batch", "images", 0, nimages, why)); return SL2_ERR_INVALID; }
  if (!on_device)
    for (int i = 0; i < nimages; ++i) {
      const char* bad = (counts[i] < 0 || counts[i] > item_stride) ? "count negative or over item_stride" : nullptr;
      for (int k = 0; !bad && k < counts[i]; ++k) bad = overlay_item_fault(items[(size_t)i * item_stride + k], npatches);
      if (bad) {
        char buf[256];
        snprintf(buf, sizeof(buf), "sl2_pick_items_batch: image %d: %s", i, bad);
        set_error(buf);
        return SL2_ERR_INVALID;
      }
    }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device (the engine has no CPU fallback)"); return SL2_ERR_NO_DEVICE; }
  SL2_HIP(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((nimages + kPickImages - 1) / kPickImages));
  if (on_device) {
    hipLaunchKernelGGL(k_pick_items, grid, dim3(kPickThreads), 0, st, nimages, width, height, items, item_stride, counts, npatches, clicks, picked);
    SL2_HIP(hipGetLastError());
    return SL2_OK;
  }
  DeviceTemps tmp(st);
  void* d = nullptr;
  const size_t ib = sizeof(sl2_overlay_item) * (size_t)item_stride * (size_t)nimages, nb = sizeof(int32_t) * (size_t)nimages;
  if (tmp.alloc(&d, ib + 5 * nb)) { set_error("sl2_pick_items_batch: device allocation failed"); return SL2_ERR_HIP; }
  sl2_overlay_item* d_items = (sl2_overlay_item*)d;
  int32_t* d_counts = (int32_t*)((char*)d + ib);
  int32_t *d_clicks = d_counts + nimages, *d_picked = d_clicks + 2 * (size_t)nimages;
  if (ib) SL2_HIP(hipMemcpyAsync(d_items, items, ib, hipMemcpyHostToDevice, st));
  SL2_HIP(hipMemcpyAsync(d_counts, counts, nb, hipMemcpyHostToDevice, st));
  SL2_HIP(hipMemcpyAsync(d_clicks, clicks, 2 * nb, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_pick_items, grid, dim3(kPickThreads), 0, st, nimages, width, height, (const sl2_overlay_item*)d_items, item_stride,
                     (const int32_t*)d_counts, npatches, (const int32_t*)d_clicks, d_picked);
  SL2_HIP(hipGetLastError());
  SL2_HIP(hipMemcpyAsync(picked, d_picked, 2 * nb, hipMemcpyDeviceToHost, st));
  SL2_HIP(hipStreamSynchronize(st));
  return SL2_OK;
}
