// Raw camera frames -> the engine's 8-bit grey image: colour-to-grey and bilinear resize in the 8-bit
// integer forms of the reference's framegrabber (usbcamgrabber.cpp:75-113: cv::cvtColor with 14-bit coefficients, then
// cv::resize INTER_LINEAR with 11-bit coefficients).  SL2_HD: the same source is the body of k_convert_frames
// (sl2_convert.hip) and of sl2_convert_frame_host, and a stand-alone host program can include it (tests/frame_convert_host.cpp).
//
// Floating point enters only through convert_taps, which the HOST evaluates (sl2_converter_set_sources uploads its tables):
// the kernel and the host form then run the same integer arithmetic on the same tables, so their bytes agree by construction.
#pragma once
#include "../../include/scenelib2_amd.h"
#include "sl2_math.hpp"

namespace sl2 {

constexpr int kConvertMaxWidth = 4096;     // source pixels per row: what the kernel's LDS staging holds (sl2_convert.hip)
constexpr int kConvertMaxHeight = 16384;   // source rows: what a packed tap's index field holds
constexpr int kConvertMaxOut = 4096;       // output pixels per axis
constexpr int kConvertFormats = 5;

// bytes per source pixel
SL2_HD int convert_bpp(int format) { return format == SL2_PIX_GRAY8 ? 1 : (format == SL2_PIX_RGB24 || format == SL2_PIX_BGR24) ? 3 : 2; }
SL2_HD bool convert_is_422(int format) { return format == SL2_PIX_UYVY || format == SL2_PIX_YUYV; }

// cvtColor's RGB -> grey, 14-bit coefficients (they sum to 16384)
SL2_HD int convert_rgb_grey(int r, int g, int b) { return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14; }

// Grey value of pixel x of a source row
SL2_HD int convert_grey(int format, const uint8_t* row, int x) {
  switch (format) {
    case SL2_PIX_RGB24: return convert_rgb_grey(row[3 * x], row[3 * x + 1], row[3 * x + 2]);
    case SL2_PIX_BGR24: return convert_rgb_grey(row[3 * x + 2], row[3 * x + 1], row[3 * x]);
    case SL2_PIX_UYVY: return row[2 * x + 1];
    case SL2_PIX_YUYV: return row[2 * x];
    default: return row[x];
  }
}

// The two taps of output position d along an axis of S source and D output pixels: source indices i and min(i + 1, S - 1)
// with the 11-bit weights w0 and w1.  (w0 + w1 is 2048 except where the float 1 - f had to round: then it is off by one.)
SL2_HD void convert_taps(int S, int D, int d, int* i0, int* w0, int* w1) {
  const double scale = (double)S / (double)D;
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int i = (int)floorf(f);
  f = f - (float)i;
  if (i < 0) { i = 0; f = 0.0f; }
  if (i >= S - 1) { i = S - 1; f = 0.0f; }
  *i0 = i;
  *w1 = (int)rintf(f * 2048.0f);
  *w0 = (int)rintf((1.0f - f) * 2048.0f);
}

// A tap in one word: bits 0-13 the index, 14-25 w1 (0 .. 2048), 26-27 w0 - (2048 - w1) + 1 (0 .. 2).
SL2_HD bool convert_pack_tap(int i0, int w0, int w1, uint32_t* out) {
  const int delta = w0 - (2048 - w1) + 1;
  if (i0 < 0 || i0 >= kConvertMaxHeight || w1 < 0 || w1 > 2048 || delta < 0 || delta > 2) return false;
  *out = (uint32_t)i0 | ((uint32_t)w1 << 14) | ((uint32_t)delta << 26);
  return true;
}
SL2_HD void convert_unpack_tap(uint32_t t, int* i0, int* w0, int* w1) {
  *i0 = (int)(t & 16383u);
  *w1 = (int)((t >> 14) & 4095u);
  *w0 = 2048 - *w1 + (int)((t >> 26) & 3u) - 1;
}

// resize's 8-bit INTER_LINEAR: the horizontal pass of one source row, then the vertical combination of two of them
SL2_HD int convert_hpass(int g0, int g1, int a0, int a1) { return g0 * a0 + g1 * a1; }
SL2_HD uint8_t convert_vpass(int h0, int h1, int b0, int b1) {
  return (uint8_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
}

// bytes of one source row, and the bytes of the raw buffer a source reaches (its last row is not padded to the pitch)
SL2_HD uint64_t convert_row_bytes(const sl2_frame_source& s) { return (uint64_t)s.width * (uint64_t)convert_bpp(s.format); }
SL2_HD uint64_t convert_source_end(const sl2_frame_source& s) {
  return s.offset + (uint64_t)(s.height - 1) * (uint64_t)s.pitch + convert_row_bytes(s);
}

// Why a source cannot be converted (nullptr: it can).  check_reach: also that it ends inside the raw_bytes of the raw buffer.
inline const char* convert_source_fault(const sl2_frame_source& s, uint64_t raw_bytes, bool check_reach) {
  if (s.format < 0 || s.format >= kConvertFormats) return "unknown pixel format";
  if (s.width < 1 || s.height < 1) return "width or height below 1";
  if (s.width > kConvertMaxWidth) return "width over 4096";
  if (s.height > kConvertMaxHeight) return "height over 16384";
  if (convert_is_422(s.format) && (s.width & 1)) return "odd width with a 4:2:2 format";
  if (s.pitch < 0 || (uint64_t)s.pitch < convert_row_bytes(s)) return "pitch below the bytes of a row";
  if (check_reach && (s.offset > raw_bytes || convert_source_end(s) - s.offset > raw_bytes - s.offset)) return "source reaches past the raw buffer";
  return nullptr;
}

// One output pixel from the packed taps of its column and row.
SL2_HD uint8_t convert_pixel(int format, const uint8_t* base, int pitch, int width, int height, uint32_t ctap, uint32_t rtap) {
  int x0, a0, a1, y0, b0, b1;
  convert_unpack_tap(ctap, &x0, &a0, &a1);
  convert_unpack_tap(rtap, &y0, &b0, &b1);
  const int x1 = x0 + 1 < width ? x0 + 1 : width - 1;
  const int y1 = y0 + 1 < height ? y0 + 1 : height - 1;
  const uint8_t* r0 = base + (size_t)y0 * (size_t)pitch;
  const uint8_t* r1 = base + (size_t)y1 * (size_t)pitch;
  const int h0 = convert_hpass(convert_grey(format, r0, x0), convert_grey(format, r0, x1), a0, a1);
  const int h1 = convert_hpass(convert_grey(format, r1, x0), convert_grey(format, r1, x1), a0, a1);
  return convert_vpass(h0, h1, b0, b1);
}

// The packed tap tables of one source: out_width column taps, then out_height row taps.  False: a tap does not pack (never
// seen; the caller refuses the source).
inline bool convert_tap_table(int src_w, int src_h, int out_w, int out_h, uint32_t* col, uint32_t* row) {
  int i, w0, w1;
  for (int x = 0; x < out_w; ++x) { convert_taps(src_w, out_w, x, &i, &w0, &w1); if (!convert_pack_tap(i, w0, w1, &col[x])) return false; }
  for (int y = 0; y < out_h; ++y) { convert_taps(src_h, out_h, y, &i, &w0, &w1); if (!convert_pack_tap(i, w0, w1, &row[y])) return false; }
  return true;
}

// The host form's body: one source into out[out_h][out_w].  col / row: scratch of out_w and out_h words.
inline bool convert_frame_host_body(const sl2_frame_source& s, const uint8_t* raw, int out_w, int out_h, uint32_t* col, uint32_t* row,
                                    uint8_t* out) {
  if (!convert_tap_table(s.width, s.height, out_w, out_h, col, row)) return false;
  const uint8_t* base = raw + s.offset;
  for (int y = 0; y < out_h; ++y)
    for (int x = 0; x < out_w; ++x)
      out[(size_t)y * out_w + x] = convert_pixel(s.format, base, s.pitch, s.width, s.height, col[x], row[y]);
  return true;
}

}  // namespace sl2
