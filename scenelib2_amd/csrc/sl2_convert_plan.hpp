// Which kernel of the frame converter owns a sequence, and what sl2_convert_frames launches, decided ONCE (DESIGN.md section 8f,
// "routes"): the constants the converter's two units (sl2_convert.hip, sl2_convert_remap.hip) and its host code share, the route
// of a sequence with the bits that carry it to the device, and the plan - counts, list offsets and dynamic LDS of every launch.
// converter_upload makes the plan whenever a source, a filter or a remap changes; sl2_convert_frames walks it and decides nothing.
// Host-only arithmetic, no HIP: tests/convert_plan_host.cpp compiles this header alone.
#pragma once
#include <cstdint>
#include <vector>

#include "sl2_convert_dev.hpp"

namespace sl2 {

// ---- the constants (the kernels use them by name)
constexpr int kConvThreads = 256;
constexpr int kConvBandRows = 8;                              // output rows per workgroup
constexpr int kConvSlots = 2 * kConvBandRows;                 // source rows staged at once, at most
// LDS of the staged grey rows: four rows at the width cap (a staged row is shifted by up to 15 bytes so that its 16-byte
// stores are aligned: kConvertMaxWidth + 16 each), all sixteen of a band up to 1000 pixels.  16.1 KB: the registers, not the
// LDS, bound the workgroups a CU takes (eight: the launch bound holds the kernel to 64 registers; at 32 KB and four
// workgroups it was 1.2 to 1.45 times slower, a workgroup's life being a chain of dependent round trips to memory that only
// other workgroups hide).
constexpr int kConvLdsBytes = 4 * (kConvertMaxWidth + 16);
// Bayer: the grey of a listed row needs raw rows y - 1, y, y + 1, so the raw rows are staged first (as GRAY8 rows, in dynamic LDS
// sized by the widest Bayer source of the launch) and the grey rows are formed from them, LDS to LDS.  At most kRawSlots raw rows
// at once (sixteen consecutive grey rows and their halo) and kRawLdsBytes: four raw rows at the width cap, eighteen up to 880.
constexpr int kRawSlots = 18;
constexpr int kRawLdsBytes = 4 * (kConvertMaxWidth + 16);
// a staged row of w pixels: shifted by up to 15 bytes, and a multiple of 16
constexpr int conv_row_pad(int w) { return (w + 15 + 15) & ~15; }

// The device copy of a source carries its sequence's route in its format word (the host copy and the C ABI never see it): the
// filter, whether the format is a deep grey or Bayer one, whether the sequence follows a map
constexpr int kConvAreaBit = 0x100;
constexpr int kConvRawBit = 0x200;
constexpr int kConvRemapBit = 0x400;
constexpr int kConvFormatMask = 0xff;

// ---- the routes: one kernel each.  k_convert_frames walks every sequence and leaves those whose record has a bit set; the
// other four take the sequences of their list.
enum ConvRoute { kRouteNone = -1, kRouteLinear, kRouteArea, kRouteRawLinear, kRouteRawArea, kRouteRemap };
constexpr int kConvRoutes = 5;

// have: the sequence has a source.  A mapped sequence is k_convert_remap's whatever its format and filter.
inline ConvRoute convert_route(bool have, int filter, int format, int remap_slot) {
  if (!have) return kRouteNone;
  if (remap_slot >= 0) return kRouteRemap;
  const bool area = filter == SL2_RESIZE_AREA;
  if (convert_is_raw(format)) return area ? kRouteRawArea : kRouteRawLinear;
  return area ? kRouteArea : kRouteLinear;
}

// What the route adds to the device record's format word.  A mapped record carries the other two bits as well: they are what
// keeps the four kernels of sl2_convert.hip off it.
constexpr int convert_route_bits(ConvRoute r) {
  return r == kRouteArea ? kConvAreaBit : r == kRouteRawLinear ? kConvRawBit : r == kRouteRawArea ? (kConvAreaBit | kConvRawBit)
       : r == kRouteRemap ? (kConvRemapBit | kConvAreaBit | kConvRawBit) : 0;
}

// ---- the plan
struct ConvPlan {
  int count[kConvRoutes] = {};      // sequences per route
  int start[kConvRoutes] = {};      // where a listed route begins in `list` (kRouteLinear has none: 0)
  std::vector<int32_t> list;        // the listed routes' sequences, route after route (they share no sequence): at most nseq
  int bands = 0;                    // workgroups per sequence: bands of kConvBandRows output rows
  // dynamic LDS bytes of a route's launch.  k_convert_area: a word per source column of the widest listed source.  k_raw_linear:
  // the raw stage, kRawSlots rows of the widest listed Bayer source up to kRawLdsBytes, 0 with none.  k_raw_area: both, colsum first
  int lds[kConvRoutes] = {};
  int raw_area_colsum = 0;          // k_raw_area's colsum part (the kernel takes it and the rest, its raw stage, as arguments)
};

inline ConvPlan convert_plan(int nseq, const uint8_t* have, const sl2_frame_source* src, const int32_t* filter, const int32_t* remap,
                             int out_h) {
  ConvPlan p;
  p.bands = (out_h + kConvBandRows - 1) / kConvBandRows;
  std::vector<int32_t> of[kConvRoutes];
  int widest[kConvRoutes] = {}, stage[kConvRoutes] = {};
  for (int s = 0; s < nseq; ++s) {
    const ConvRoute r = convert_route(have[s] != 0, filter[s], src[s].format, remap[s]);
    if (r == kRouteNone) continue;
    ++p.count[r];
    if (r != kRouteLinear) of[r].push_back(s);
    if (src[s].width > widest[r]) widest[r] = src[s].width;
    if (convert_is_bayer(src[s].format)) {
      const int want = kRawSlots * conv_row_pad(src[s].width);
      const int capped = want < kRawLdsBytes ? want : kRawLdsBytes;
      if (capped > stage[r]) stage[r] = capped;
    }
  }
  for (int r = kRouteArea; r < kConvRoutes; ++r) {
    p.start[r] = (int)p.list.size();
    p.list.insert(p.list.end(), of[r].begin(), of[r].end());
  }
  const auto colsum = [](int w) { return 4 * ((w + 3) / 4 * 4); };
  p.raw_area_colsum = colsum(widest[kRouteRawArea]);
  p.lds[kRouteArea] = colsum(widest[kRouteArea]);
  p.lds[kRouteRawLinear] = stage[kRouteRawLinear];
  p.lds[kRouteRawArea] = p.raw_area_colsum + stage[kRouteRawArea];
  return p;
}

}  // namespace sl2
