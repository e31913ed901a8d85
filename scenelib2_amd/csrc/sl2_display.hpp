// The host side of the three display views (DESIGN.md sections 8h-8j): annotated frames (sl2_overlay.hip), the rectified view
// (sl2_rectify.hip) and the world view with picking (sl2_world_view.hip).  Each view supplies a list kernel and, where it draws
// over frames of its own making, a producer of grey frames; the checks, the staging and the order of the launches are here.
// The plain functions are defined in sl2_overlay.hip.
#pragma once
#include <type_traits>

#include "sl2_common.hpp"

namespace sl2 {

// the rasteriser's launch (k_overlay_draw): device frames, lists and patches in, device images out
int launch_draw(hipStream_t stream, const uint8_t* d_frames, size_t seq_stride, int nimages, int width, int height, const sl2_overlay_item* d_items,
                int item_stride, const int32_t* d_counts, const uint8_t* d_patches, size_t patch_stride, int npatches, uint8_t* d_out, size_t out_stride);
// what every drawing call checks of its image geometry (nullptr: fine)
const char* geometry_fault(int nimages, int width, int height, size_t seq_stride, size_t out_stride);
// the text of a fault that every sequence or image of the call shares (a stride, the geometry, a pointer): the range is named
std::string range_text(const char* fn, const char* noun, int first, int count, const char* what);
// Why a range of sequences cannot be served (nullptr: it can).  layers_fault names the view's mask; views_fault is what the
// caller found wrong with its views, which ranks before the layers.
const char* range_fault(const sl2_engine* e, int seq0, int nseq, int layers, int all_layers, const char* layers_fault, const char* views_fault = nullptr);
// the refusal of host-resident views that hold a number that is not finite (empty: all are finite)
std::string view_fault_text(const char* fn, int seq0, int nseq, const sl2_view* views, int nviews);
int grow_device(void** p, size_t* have, size_t need);

// Device pointers of one call's lists: the caller's own, or the engine-owned staging (ovl_lists, grown on demand) laid out as
// items [nseq][stride], counts [nseq], marked [nseq], views [nviews], extents [nseq][6].  marked, views and extents may be null.
struct ListStage { sl2_overlay_item* items; int stride; int32_t* counts; const int32_t* marked; const sl2_view* views; double* extents; };
int list_stage(sl2_engine* e, int nseq, int nviews, size_t stride, ListStage* st);
// the caller's host-resident views and marked labels on their way into the staging; a null one stays null
int stage_inputs(sl2_engine* e, int nseq, const sl2_view* views, int nviews, const int32_t* marked, ListStage* st);

// device temporaries of whatever arrived in host memory, released on every exit path (after the stream has drained)
struct DeviceTemps {
  std::vector<void*> p;
  hipStream_t st;
  explicit DeviceTemps(hipStream_t s) : st(s) {}
  ~DeviceTemps() { if (!p.empty()) (void)hipStreamSynchronize(st); for (void* q : p) if (q) (void)hipFree(q); }
  int alloc(void** o, size_t bytes) {
    *o = nullptr;
    const hipError_t e = hipMalloc(o, bytes ? bytes : 1);
    if (e == hipSuccess) p.push_back(*o);
    return e == hipSuccess ? SL2_OK : SL2_ERR_HIP;
  }
};

// A sl2_*_items call.  `why` is the view's verdict on the range and the layers; bound is its sl2_*_item_bound.  launch(d) queues
// the view's list kernel on e->stream over the device pointers d.  Device form: one launch, no wait.  Host form: staged, and whole
// strides come back in one copy - the items behind a list's count are not part of it (whatever the staging held).
template <class Launch>
int items_call(const char* fn, sl2_engine* e, int seq0, int nseq, const char* why, size_t (*bound)(int, int), const char* stride_fault,
               const sl2_view* views, int nviews, const int32_t* marked, sl2_overlay_item* items, int item_stride, int32_t* counts, double* extents,
               int on_device, Launch launch) {
  if (!why && (!items || !counts)) why = "null items or counts";
  if (!why && on_device && ((uintptr_t)items % 8 || (uintptr_t)views % 8 || (uintptr_t)extents % 8))
    why = views ? "device items, views or extents not 8-byte aligned" : "device items not 8-byte aligned";
  if (!why && (item_stride < 0 || (size_t)item_stride < bound(e->N, e->kpart))) why = stride_fault;
  if (why) { set_error(range_text(fn, "sequences", seq0, nseq, why)); return SL2_ERR_INVALID; }
  if (views && !on_device) {
    const std::string bad = view_fault_text(fn, seq0, nseq, views, nviews);
    if (!bad.empty()) { set_error(bad); return SL2_ERR_INVALID; }
  }
  SL2_HIP(hipSetDevice(e->device));
  if (on_device) return launch(ListStage{items, item_stride, counts, marked, views, extents});
  ListStage st;
  { int _rc = list_stage(e, nseq, nviews, (size_t)item_stride, &st); if (_rc != SL2_OK) return _rc; }
  { int _rc = stage_inputs(e, nseq, views, nviews, marked, &st); if (_rc != SL2_OK) return _rc; }
  { int _rc = launch(st); if (_rc != SL2_OK) return _rc; }
  SL2_HIP(hipMemcpyAsync(counts, st.counts, sizeof(int32_t) * (size_t)nseq, hipMemcpyDeviceToHost, e->stream));
  SL2_HIP(hipMemcpyAsync(items, st.items, sizeof(sl2_overlay_item) * (size_t)item_stride * (size_t)nseq, hipMemcpyDeviceToHost, e->stream));
  if (extents) SL2_HIP(hipMemcpyAsync(extents, st.extents, 6 * sizeof(double) * (size_t)nseq, hipMemcpyDeviceToHost, e->stream));
  SL2_HIP(hipStreamSynchronize(e->stream));
  return SL2_OK;
}

// A sl2_draw_* call after its checks: W x H images of nseq sequences, lists of `stride` items.  The chain on e->stream:
// host frames in, host views and marked labels in, the grey frames, the lists, the rasteriser, host-bound images out.
// frames: the caller's grey frames, or null where the view makes its own.  grey: nullptr where the rasteriser draws over the
// caller's frames as they are, else grey(d_frames, d_seq_stride, d_grey) queues the producer of packed grey frames.  Views and
// marked labels live where the output lives.  launch(d) as in items_call; patches: the engine's templates, or null.
template <class Grey, class Launch>
int draw_call(sl2_engine* e, int nseq, int W, int H, size_t stride, const uint8_t* frames, size_t seq_stride, int frames_on_device,
              const sl2_view* views, int nviews, const int32_t* marked, const uint8_t* patches, uint8_t* out, size_t out_stride, int out_on_device,
              Grey grey, Launch launch) {
  constexpr bool own_grey = !std::is_same<Grey, std::nullptr_t>::value;
  SL2_HIP(hipSetDevice(e->device));
  const size_t px = (size_t)W * H, packed = (px * (size_t)nseq + 255) & ~(size_t)255;
  ListStage st;
  { int _rc = list_stage(e, nseq, nviews, stride, &st); if (_rc != SL2_OK) return _rc; }
  // image staging (ovl_images): host frames on their way in, the view's own grey frames (the rasteriser's frames), then
  // host-bound images on their way out - all packed
  const size_t in_bytes = (frames && !frames_on_device) ? packed : 0, grey_bytes = own_grey ? packed : 0;
  const size_t out_bytes = out_on_device ? 0 : 3 * px * (size_t)nseq;
  { int _rc = grow_device(&e->ovl_images, &e->ovl_images_bytes, in_bytes + grey_bytes + out_bytes); if (_rc != SL2_OK) return _rc; }
  const uint8_t* d_frames = frames;
  size_t d_seq_stride = seq_stride;
  if (in_bytes) {
    SL2_HIP(hipMemcpy2DAsync(e->ovl_images, px, frames, seq_stride, px, (size_t)nseq, hipMemcpyHostToDevice, e->stream));
    d_frames = (const uint8_t*)e->ovl_images; d_seq_stride = px;
    // The caller's frames may be pageable memory and may be reused the moment the call returns.  The host form waits at its end
    // anyway; with the output left on the device this is the one place the call waits: until the frames have been copied.
    if (out_on_device) SL2_HIP(hipStreamSynchronize(e->stream));
  }
  if (out_on_device) { st.views = views; st.marked = marked; }
  else { int _rc = stage_inputs(e, nseq, views, nviews, marked, &st); if (_rc != SL2_OK) return _rc; }
  st.extents = nullptr;
  if constexpr (own_grey) {
    uint8_t* d_grey = (uint8_t*)e->ovl_images + in_bytes;
    { int _rc = grey(d_frames, d_seq_stride, d_grey); if (_rc != SL2_OK) return _rc; }
    d_frames = d_grey; d_seq_stride = px;
  }
  { int _rc = launch(st); if (_rc != SL2_OK) return _rc; }
  uint8_t* d_out = out_on_device ? out : (uint8_t*)e->ovl_images + in_bytes + grey_bytes;
  const size_t d_out_stride = out_on_device ? out_stride : 3 * px;
  {
    LaunchScope ls(e, "k_overlay_draw");
    int _rc = launch_draw(e->stream, d_frames, d_seq_stride, nseq, W, H, st.items, st.stride, st.counts, patches, patches ? (size_t)kPatchStride : 0,
                          patches ? e->B * e->N : 0, d_out, d_out_stride);
    if (_rc != SL2_OK) return _rc;
  }
  if (out_on_device) return SL2_OK;
  SL2_HIP(hipMemcpy2DAsync(out, out_stride, d_out, 3 * px, 3 * px, (size_t)nseq, hipMemcpyDeviceToHost, e->stream));
  SL2_HIP(hipStreamSynchronize(e->stream));
  return SL2_OK;
}

}  // namespace sl2
