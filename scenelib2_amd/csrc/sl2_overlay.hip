// Annotated frames (include/scenelib2_amd.h, "annotated frames"): the numerical half of
// GraphicTool::DrawRawAR (graphic/graphictool.cpp:285-364) for a range of sequences - a draw list per sequence (k_overlay_list)
// and a rasteriser (k_overlay_draw).  Two stream-ordered launches; no workgroup waits for another.  The pixel rules are
// sl2_overlay_dev.hpp's, shared with sl2_draw_items_host.  The plain functions of sl2_display.hpp, which the three views share,
// are defined here.
#include "sl2_display.hpp"
#include "sl2_drawlist_dev.hpp"

namespace sl2 {

static_assert(sizeof(sl2_overlay_item) == 64, "sl2_overlay_item is 64 bytes");
static_assert(sizeof(OverlayPrep) == 72, "OverlayPrep");

constexpr int kDrawThreads = 256;
constexpr int kTileW = 64, kTileH = 16;           // a thread owns 4 consecutive pixels of a row
constexpr int kDrawChunk = kDrawThreads;          // items culled and staged per round, one per thread: 18 KB of LDS
constexpr int kMaxParticlesDrawn = 19;            // what the reference's counter lets through at most

// ---- 1. the draw list of sequence seq0 + i: one wavefront (sl2_drawlist_dev.hpp), a lane per slot, 64 slots a round.  Every lane
// counts its slot's items, the writer places them in slot order, then every lane writes its own.
// patch_mode 0: an item's patch is i * N + the feature's index in feature_list_ order (the public list); 1: seq * N + slot, the
// index into the engine's own template array (sl2_draw_overlays).
__global__ void __launch_bounds__(kListThreads) k_overlay_list(const SeqArrays S, int seq0, int nseq, int N, int ld, int pcap, int kpart, int width,
                                                               int height, int layers, int patch_mode, const int32_t* __restrict__ marked,
                                                               sl2_overlay_item* __restrict__ items, int item_stride, int32_t* __restrict__ counts) {
  SeqWave q;
  if (!seq_wave(S, seq0, nseq, N, ld, kpart, marked, &q)) return;
  const int lane = q.lane, seq = q.seq, mark = q.mark;
  const size_t o = q.o;
  const double* xb = q.xb;
  const CameraParams cam = load_cam(S.seq_cam, seq, width, height);
  ListWriter w(items, q.i, item_stride, lane);
  double xp[7];
  for (int k = 0; k < 7; ++k) xp[k] = xb[k];
  int nlive = 0;                                       // wave-uniform: the live features of the rounds before
  for (int base = 0; base < q.ns; base += 64) {
    const int f = base + lane;
    const SlotClass s = classify_slot(S, o, f, q.ns);
    const int fl = s.fl, label = s.label;
    const bool part = s.part, full = s.full;
    const unsigned long long m_live = __ballot(part || full);
    const int li = nlive + __popcll(m_live & w.below);
    int c = 0;
    bool has_ring = false, has_patch = false;      // (two named records, not an array: an index known only at run time would put them in scratch)
    sl2_overlay_item it_ring = overlay_blank_item(SL2_ITEM_RING, label), it_patch = overlay_blank_item(SL2_ITEM_PATCH, label);
    // the partial slot whose label sits in feature slot f, and its drawn particles
    int np = 0, step = 1;
    const double* pp = nullptr;
    if (full) {
      double zeroed[3], hi[2], Hx[14], Hy[6], Rn;
      measurement_model(cam, xp, xb + 13 + 3 * f, zeroed, hi, Hx, Hy, &Rn);
      if (zeroed[2] > 0.0) {
        const bool sel = (fl & FF_SELECTED) != 0, ok = (fl & FF_SUCCESS) != 0;
        uint8_t rgb[3];
        overlay_colour(label == mark, sel, ok, rgb);
        int cx, cy;
        if ((layers & SL2_OVERLAY_SEARCH_REGIONS) && sel && overlay_round(S.f_h[(o + f) * 2], &cx) && overlay_round(S.f_h[(o + f) * 2 + 1], &cy)) {
          const double* Sf = S.f_S + (o + f) * 4;
          it_ring = draw_item(SL2_ITEM_RING, label, cx, cy, 0, 0, rgb);
          sl2_overlay_item& r = it_ring;
          r.q[0] = Sf[3]; r.q[1] = -(Sf[1] + Sf[2]); r.q[2] = Sf[0]; r.q[3] = 9.0 * (Sf[0] * Sf[3] - Sf[1] * Sf[2]);
          has_ring = true;
        }
        const double px = (sel && ok) ? S.f_z[(o + f) * 2] : hi[0], py = (sel && ok) ? S.f_z[(o + f) * 2 + 1] : hi[1];
        if ((layers & SL2_OVERLAY_DESCRIPTORS) && overlay_round(px, &cx) && overlay_round(py, &cy)) {
          it_patch = draw_item(SL2_ITEM_PATCH, label, cx, cy, 0, 0, rgb);
          it_patch.patch = patch_mode ? seq * N + f : q.i * N + li;
          has_patch = true;
        }
        c = (has_ring ? 1 : 0) + (has_patch ? 1 : 0);
      }
    } else if (part && (layers & SL2_OVERLAY_SEARCH_REGIONS)) {
      const int ks = partial_slot_of(q.psb, kpart, f);
      if (ks >= 0) {
        np = min(max(q.psb[ks * kPsInts + kPsNp], 0), pcap);
        step = overlay_particle_step(np);
        pp = S.particles + ((size_t)seq * kpart + ks) * pcap * kParticleDoubles;
        int cx, cy;
        for (int k = 0; k < np; ++k)
          if ((k + 1) % step == 0 && overlay_round(pp[(size_t)k * kParticleDoubles + 3], &cx) && overlay_round(pp[(size_t)k * kParticleDoubles + 4], &cy)) ++c;
        if (c > kMaxParticlesDrawn) c = kMaxParticlesDrawn;      // (cannot happen: n < 20 passes n, n >= 20 passes n / (n / 10) <= 19)
      }
    }
    int at = w.reserve(c);
    if (full) {
      if (has_ring) w.put(at++, it_ring);
      if (has_patch) w.put(at, it_patch);
    } else if (c > 0) {
      uint8_t rgb[3];
      overlay_colour(label == mark, false, false, rgb);
      int cx, cy, written = 0;
      for (int k = 0; k < np && written < c; ++k)
        if ((k + 1) % step == 0 && overlay_round(pp[(size_t)k * kParticleDoubles + 3], &cx) && overlay_round(pp[(size_t)k * kParticleDoubles + 4], &cy)) {
          const double* p = pp + (size_t)k * kParticleDoubles;
          sl2_overlay_item r = draw_item(SL2_ITEM_RING, label, cx, cy, 0, 0, rgb);
          r.q[0] = p[7]; r.q[1] = 2.0 * p[8]; r.q[2] = p[9]; r.q[3] = 9.0;
          w.put(at + written, r);
          ++written;
        }
    }
    nlive += __popcll(m_live);
  }
  if (lane == 0 && (layers & SL2_OVERLAY_INITIALISATION)) {      // the two boxes of the feature being initialised, behind the features
    const int* pi = S.part_i + (size_t)seq * kPartInts;
    const uint8_t green[3] = {0, 255, 0};
    if (pi[kPartCreated]) w.put(w.total++, draw_item(SL2_ITEM_RECT, -1, pi[kPartUU] - 6, pi[kPartVV] - 6, pi[kPartUU] + 6, pi[kPartVV] + 6, green));
    if (pi[kPartRegionValid])
      w.put(w.total++, draw_item(SL2_ITEM_RECT, -1, pi[kPartRegion], pi[kPartRegion + 1], pi[kPartRegion + 2], pi[kPartRegion + 3], green));
  }
  w.finish(counts, q.i);
}

// ---- 2. the rasteriser: a workgroup per (image, tile of 64 x 16 pixels), a thread per 4 consecutive pixels of a row.  The list
// is walked in rounds of kDrawChunk items: every thread prepares one, the items whose conservative box meets the TILE are staged
// in list order into LDS (so what a round skips is the same for the whole workgroup), then every thread walks the staged items
// for its pixels and keeps the last hit.  Later rounds overwrite earlier ones: painter's order.
struct DrawArgs {
  const uint8_t* frames; size_t seq_stride;
  int width, height, tiles_x, tiles;
  const sl2_overlay_item* items; int item_stride; const int32_t* counts;
  const uint8_t* patches; size_t patch_stride; int npatches;
  uint8_t* out; size_t out_stride;
  int dword_out;      // every row of every image starts on a 4-byte boundary: a thread's 12 bytes go out as three dwords
};

// (Eight waves a SIMD are asked for: with the SEGMENT kind the allocator took 66 registers without the bound, seven waves, and the
// kernel - bound by latency, not by bytes - ran 12-14 % slower at 1024 sequences; at 64 registers it parks 20 scalars in vector lanes.)
__global__ void __launch_bounds__(kDrawThreads, 8) k_overlay_draw(const DrawArgs A) {
  __shared__ OverlayPrep s_prep[kDrawChunk];
  __shared__ int s_wave[kDrawThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int img = blockIdx.x / A.tiles, tile = blockIdx.x % A.tiles;
  const int x0 = (tile % A.tiles_x) * kTileW, y0 = (tile / A.tiles_x) * kTileH;
  const int x1 = min(x0 + kTileW - 1, A.width - 1), y1 = min(y0 + kTileH - 1, A.height - 1);
  const int px = x0 + (tid & 15) * 4, py = y0 + (tid >> 4);
  const bool row_ok = py < A.height && px < A.width;
  const uint8_t* frame = A.frames + (size_t)img * A.seq_stride;
  uint32_t c[4];
  for (int j = 0; j < 4; ++j) {
    const uint32_t g = (row_ok && px + j < A.width) ? frame[(size_t)py * A.width + px + j] : 0u;
    c[j] = g | (g << 8) | (g << 16);
  }
  const int count = min(max(A.counts[img], 0), A.item_stride);
  const sl2_overlay_item* list = A.items + (size_t)img * A.item_stride;
  for (int base = 0; base < count; base += kDrawChunk) {
    const int k = base + tid;
    OverlayPrep p;
    bool keep = false;
    if (k < count) keep = overlay_prepare(list[k], A.npatches, &p) && overlay_box_meets(p, x0, y0, x1, y1);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave[wv] = __popcll(m);
    __syncthreads();
    int off = __popcll(m & ((1ull << lane) - 1ull)), n = 0;
    for (int w = 0; w < kDrawThreads / 64; ++w) { if (w < wv) off += s_wave[w]; n += s_wave[w]; }
    if (keep) s_prep[off] = p;
    __syncthreads();
    if (row_ok)
      for (int q = 0; q < n; ++q) {
        const OverlayPrep& P = s_prep[q];
        if (py < P.by0 || py > P.by1 || px > P.bx1 || px + 3 < P.bx0) continue;
        for (int j = 0; j < 4; ++j) {
          uint32_t h;
          if (px + j < A.width && overlay_hit(P, A.patches, A.patch_stride, px + j, py, &h)) c[j] = h;
        }
      }
    __syncthreads();      // (the next round overwrites s_prep and s_wave)
  }
  if (!row_ok) return;
  uint8_t* o = A.out + (size_t)img * A.out_stride + ((size_t)py * A.width + px) * 3;
  if (A.dword_out && px + 3 < A.width) {
    uint32_t* o4 = reinterpret_cast<uint32_t*>(o);      // px is a multiple of 4, so 3 px is one of 4 too
    o4[0] = c[0] | (c[1] << 24);
    o4[1] = (c[1] >> 8) | (c[2] << 16);
    o4[2] = (c[2] >> 16) | (c[3] << 8);
  } else {
    for (int j = 0; j < 4; ++j)
      if (px + j < A.width) { o[3 * j] = (uint8_t)c[j]; o[3 * j + 1] = (uint8_t)(c[j] >> 8); o[3 * j + 2] = (uint8_t)(c[j] >> 16); }
  }
}

static std::string at_text(const char* fn, const char* noun, int idx, const char* what) {
  char buf[256];
  snprintf(buf, sizeof(buf), "%s: %s %d: %s", fn, noun, idx, what);
  return buf;
}
std::string range_text(const char* fn, const char* noun, int first, int count, const char* what) {
  char buf[256];
  snprintf(buf, sizeof(buf), "%s: %s %d .. %d: %s", fn, noun, first, first + (count > 0 ? count : 1) - 1, what);
  return buf;
}
const char* range_fault(const sl2_engine* e, int seq0, int nseq, int layers, int all_layers, const char* layers_fault, const char* views_fault) {
  if (!e) return "null engine";
  if (nseq < 1) return "nseq below 1";
  if (seq0 < 0 || seq0 > e->B - nseq) return "outside the batch";
  if (views_fault) return views_fault;
  if (layers & ~all_layers) return layers_fault;
  return nullptr;
}
std::string view_fault_text(const char* fn, int seq0, int nseq, const sl2_view* views, int nviews) {
  for (int i = 0; i < nviews; ++i) {
    const sl2_view& v = views[i];
    const double all[11] = {v.r[0], v.r[1], v.r[2], v.q[0], v.q[1], v.q[2], v.q[3], v.fku, v.fkv, v.u0, v.v0};
    for (double d : all) {
      if (overlay_finite(d)) continue;
      char buf[256];
      if (nviews == 1) snprintf(buf, sizeof(buf), "%s: sequences %d .. %d: the view holds a number that is not finite", fn, seq0, seq0 + nseq - 1);
      else snprintf(buf, sizeof(buf), "%s: sequence %d: its view holds a number that is not finite", fn, seq0 + i);
      return buf;
    }
  }
  return std::string();
}

int launch_draw(hipStream_t stream, const uint8_t* d_frames, size_t seq_stride, int nimages, int width, int height,
                       const sl2_overlay_item* d_items, int item_stride, const int32_t* d_counts, const uint8_t* d_patches, size_t patch_stride,
                       int npatches, uint8_t* d_out, size_t out_stride) {
  DrawArgs A;
  A.frames = d_frames; A.seq_stride = seq_stride; A.width = width; A.height = height;
  A.tiles_x = (width + kTileW - 1) / kTileW;
  A.tiles = A.tiles_x * ((height + kTileH - 1) / kTileH);
  A.items = d_items; A.item_stride = item_stride; A.counts = d_counts;
  A.patches = d_patches; A.patch_stride = patch_stride; A.npatches = d_patches ? npatches : 0;
  A.out = d_out; A.out_stride = out_stride;
  A.dword_out = ((3 * (size_t)width) % 4 == 0 && (uintptr_t)d_out % 4 == 0 && out_stride % 4 == 0) ? 1 : 0;
  hipLaunchKernelGGL(k_overlay_draw, dim3((unsigned)(nimages * A.tiles)), dim3(kDrawThreads), 0, stream, A);
  SL2_HIP(hipGetLastError());
  return SL2_OK;
}

const char* geometry_fault(int nimages, int width, int height, size_t seq_stride, size_t out_stride) {
  if (nimages < 1) return "no images";
  if (width < 1 || height < 1 || width > kOverlayMaxSide || height > kOverlayMaxSide) return "width or height outside 1 .. 32768";
  if (seq_stride < (size_t)width * (size_t)height) return "seq_stride below width * height";
  if (out_stride < 3 * (size_t)width * (size_t)height) return "out_stride below 3 * width * height";
  const long long tiles = (long long)((width + kTileW - 1) / kTileW) * ((height + kTileH - 1) / kTileH);
  if (tiles * nimages > 0x7fffffffll) return "more tiles than one launch takes";
  return nullptr;
}

int grow_device(void** p, size_t* have, size_t need) {
  if (need <= *have) return SL2_OK;
  if (*p) { SL2_HIP(hipFree(*p)); *p = nullptr; *have = 0; }
  SL2_HIP(hipMalloc(p, need));
  *have = need;
  return SL2_OK;
}

static int launch_list(sl2_engine* e, int seq0, int nseq, int layers, int patch_mode, const ListStage& d) {
  // (the root's arrays on the engine's stream, like sl2_snapshot_batch: the groups' streams join it at the end of every stepping call)
  LaunchScope ls(e, "k_overlay_list");
  hipLaunchKernelGGL(k_overlay_list, dim3((nseq + kListSeqs - 1) / kListSeqs), dim3(kListThreads), 0, e->stream, seq_arrays(e), seq0, nseq, e->N, e->ld,
                     e->pcap, e->kpart, e->cam.width, e->cam.height, layers, patch_mode, d.marked, d.items, d.stride, d.counts);
  SL2_HIP(hipGetLastError());
  return SL2_OK;
}

int list_stage(sl2_engine* e, int nseq, int nviews, size_t stride, ListStage* st) {
  const size_t item_bytes = sizeof(sl2_overlay_item) * stride * (size_t)nseq, int_bytes = 2 * sizeof(int32_t) * (size_t)nseq;
  const size_t view_bytes = sizeof(sl2_view) * (size_t)nviews, ext_bytes = 6 * sizeof(double) * (size_t)nseq;
  { int _rc = grow_device(&e->ovl_lists, &e->ovl_lists_bytes, item_bytes + int_bytes + view_bytes + ext_bytes); if (_rc != SL2_OK) return _rc; }
  char* p = (char*)e->ovl_lists;
  st->items = (sl2_overlay_item*)p;
  st->stride = (int)stride;
  st->counts = (int32_t*)(p + item_bytes);
  st->marked = st->counts + nseq;
  st->views = (const sl2_view*)(p + item_bytes + int_bytes);      // (8-byte aligned: 64 stride nseq + 8 nseq)
  st->extents = (double*)(p + item_bytes + int_bytes + view_bytes);
  return SL2_OK;
}

int stage_inputs(sl2_engine* e, int nseq, const sl2_view* views, int nviews, const int32_t* marked, ListStage* st) {
  if (views) SL2_HIP(hipMemcpyAsync((void*)st->views, views, sizeof(sl2_view) * (size_t)nviews, hipMemcpyHostToDevice, e->stream));
  else st->views = nullptr;
  if (marked) SL2_HIP(hipMemcpyAsync((void*)st->marked, marked, sizeof(int32_t) * (size_t)nseq, hipMemcpyHostToDevice, e->stream));
  else st->marked = nullptr;
  return SL2_OK;
}

}  // namespace sl2

using namespace sl2;

extern "C" size_t sl2_overlay_item_bound(int max_features, int partial_slots) {
  if (max_features < 0 || partial_slots < 0) return 0;
  return 2 * (size_t)max_features + (size_t)kMaxParticlesDrawn * (size_t)partial_slots + 2;
}

extern "C" int sl2_draw_items_host(const uint8_t* frame, int width, int height, const sl2_overlay_item* items, int count, const uint8_t* patches,
                                   size_t patch_stride, int npatches, uint8_t* out) {
  if (!frame || !out || count < 0 || (count > 0 && !items) || npatches < 0 || (npatches > 0 && (!patches || patch_stride < SL2_PATCH_BYTES))) {
    set_error("sl2_draw_items_host: null pointer, negative count or patch_stride below 121");
    return SL2_ERR_INVALID;
  }
  if (width < 1 || height < 1 || width > kOverlayMaxSide || height > kOverlayMaxSide) {
    set_error("sl2_draw_items_host: width or height outside 1 .. 32768");
    return SL2_ERR_INVALID;
  }
  std::vector<OverlayPrep> prep((size_t)count + 1);
  overlay_draw_host_body(frame, width, height, items, count, patches, patch_stride, npatches, prep.data(), out);
  return SL2_OK;
}

extern "C" int sl2_overlay_items(sl2_engine* e, int seq0, int nseq, int layers, const int32_t* marked, sl2_overlay_item* items, int item_stride,
                                 int32_t* counts, int on_device) {
  const char* why = range_fault(e, seq0, nseq, layers, SL2_OVERLAY_ALL, "layers with bits outside SL2_OVERLAY_ALL");
  return items_call("sl2_overlay_items", e, seq0, nseq, why, sl2_overlay_item_bound, "item_stride below sl2_overlay_item_bound", nullptr, 0, marked, items,
                    item_stride, counts, nullptr, on_device, [&](const ListStage& d) { return launch_list(e, seq0, nseq, layers, 0, d); });
}

extern "C" int sl2_draw_overlays(sl2_engine* e, int seq0, int nseq, const uint8_t* frames, size_t seq_stride, int frames_on_device, int layers,
                                 const int32_t* marked, uint8_t* out, size_t out_stride, int out_on_device) {
  const char* why = range_fault(e, seq0, nseq, layers, SL2_OVERLAY_ALL, "layers with bits outside SL2_OVERLAY_ALL");
  if (!why && (!frames || !out)) why = "null frames or out";
  if (!why) why = geometry_fault(nseq, e->cam.width, e->cam.height, seq_stride, out_stride);
  if (why) { set_error(range_text("sl2_draw_overlays", "sequences", seq0, nseq, why)); return SL2_ERR_INVALID; }
  // the rasteriser draws over the caller's frames as they are, and reads the engine's own templates
  return draw_call(e, nseq, e->cam.width, e->cam.height, sl2_overlay_item_bound(e->N, e->kpart), frames, seq_stride, frames_on_device, nullptr, 0, marked,
                   e->patch, out, out_stride, out_on_device, nullptr, [&](const ListStage& d) { return launch_list(e, seq0, nseq, layers, 1, d); });
}

extern "C" int sl2_draw_items_batch(int device, void* stream, const uint8_t* frames, int frames_on_device, int nimages, int width, int height,
                                    size_t seq_stride, const sl2_overlay_item* items, int item_stride, const int32_t* counts, int items_on_device,
                                    const uint8_t* patches, size_t patch_stride, int npatches, uint8_t* out, size_t out_stride, int out_on_device) {
  if (!frames || !items || !counts || !out || item_stride < 0 || npatches < 0 || (npatches > 0 && (!patches || patch_stride < SL2_PATCH_BYTES)) ||
      (items_on_device && (uintptr_t)items % 8)) {
    set_error(range_text("sl2_draw_items_batch", "images", 0, nimages,
                         "null pointer, negative item_stride or npatches, patch_stride below 121, or device items not 8-byte aligned"));
    return SL2_ERR_INVALID;
  }
  if (const char* why = geometry_fault(nimages, width, height, seq_stride, out_stride)) {
    set_error(range_text("sl2_draw_items_batch", "images", 0, nimages, why));
    return SL2_ERR_INVALID;
  }
  if (!items_on_device)
    for (int i = 0; i < nimages; ++i) {
      if (counts[i] < 0 || counts[i] > item_stride) { set_error(at_text("sl2_draw_items_batch", "image", i, "count negative or over item_stride")); return SL2_ERR_INVALID; }
      for (int k = 0; k < counts[i]; ++k)
        if (const char* why = overlay_item_fault(items[(size_t)i * item_stride + k], npatches)) {
          set_error(at_text("sl2_draw_items_batch", "image", i, why));
          return SL2_ERR_INVALID;
        }
    }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device (the engine has no CPU fallback)"); return SL2_ERR_NO_DEVICE; }
  SL2_HIP(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  DeviceTemps tmp(st);
  const size_t px = (size_t)width * height;
  const uint8_t* d_frames = frames;
  size_t d_seq_stride = seq_stride;
  if (!frames_on_device) {
    void* d = nullptr;
    if (tmp.alloc(&d, px * (size_t)nimages)) { set_error("sl2_draw_items_batch: device allocation failed"); return SL2_ERR_HIP; }
    SL2_HIP(hipMemcpy2DAsync(d, px, frames, seq_stride, px, (size_t)nimages, hipMemcpyHostToDevice, st));
    d_frames = (const uint8_t*)d; d_seq_stride = px;
  }
  const sl2_overlay_item* d_items = items;
  const int32_t* d_counts = counts;
  const uint8_t* d_patches = patches;
  if (!items_on_device) {
    void *di = nullptr, *dc = nullptr, *dp = nullptr;
    const size_t ib = sizeof(sl2_overlay_item) * (size_t)item_stride * (size_t)nimages, pb = (size_t)npatches * patch_stride;
    if (tmp.alloc(&di, ib) || tmp.alloc(&dc, sizeof(int32_t) * (size_t)nimages) || tmp.alloc(&dp, pb)) {
      set_error("sl2_draw_items_batch: device allocation failed");
      return SL2_ERR_HIP;
    }
    if (ib) SL2_HIP(hipMemcpyAsync(di, items, ib, hipMemcpyHostToDevice, st));
    SL2_HIP(hipMemcpyAsync(dc, counts, sizeof(int32_t) * (size_t)nimages, hipMemcpyHostToDevice, st));
    // (the last entry of a host array need not be padded to the stride: 121 bytes of it are read)
    if (pb) SL2_HIP(hipMemcpyAsync(dp, patches, pb - patch_stride + SL2_PATCH_BYTES, hipMemcpyHostToDevice, st));
    d_items = (const sl2_overlay_item*)di; d_counts = (const int32_t*)dc; d_patches = npatches ? (const uint8_t*)dp : nullptr;
  }
  uint8_t* d_out = out;
  size_t d_out_stride = out_stride;
  if (!out_on_device) {
    void* d = nullptr;
    if (tmp.alloc(&d, 3 * px * (size_t)nimages)) { set_error("sl2_draw_items_batch: device allocation failed"); return SL2_ERR_HIP; }
    d_out = (uint8_t*)d; d_out_stride = 3 * px;
  }
  { int _rc = launch_draw(st, d_frames, d_seq_stride, nimages, width, height, d_items, item_stride, d_counts, d_patches, patch_stride, npatches, d_out, d_out_stride);
    if (_rc != SL2_OK) return _rc; }
  if (!out_on_device) {
    SL2_HIP(hipMemcpy2DAsync(out, out_stride, d_out, 3 * px, 3 * px, (size_t)nimages, hipMemcpyDeviceToHost, st));
    SL2_HIP(hipStreamSynchronize(st));
  }
  return SL2_OK;
}
