// Raw camera frames -> the engine's 8-bit grey image: colour-to-grey and bilinear resize in the 8-bit
// integer forms of the reference's framegrabber (usbcamgrabber.cpp:75-113: cv::cvtColor with 14-bit coefficients, then
// cv::resize INTER_LINEAR with 11-bit coefficients).  SL2_HD: the same source is the body of k_convert_frames
// (sl2_convert.hip) and of sl2_convert_frame_host, and a stand-alone host program can include it (tests/frame_convert_host.cpp).
//
// SL2_RESIZE_AREA, the exact box average for large reductions, is at the end of the file: integers only, no tables.
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
constexpr int kConvertFormats = 5;          // the contiguous 8-bit formats of the reference's webcam: ids 0 .. 4

// Machine-vision sources (scenelib2_amd.h, "raw camera frames"; parity with OpenCV unpinned: this text is the definition).
// Deep grey, N = 10, 12, 16: 16-bit little-endian words, g = (v & (2^N - 1)) >> (N - 8); offset and pitch even.
// Bayer: one byte a pixel, the name is the 2 x 2 tile at the source's pixel (0,0); see convert_bayer_grey.
SL2_HD bool convert_is_deep(int format) { return format >= SL2_PIX_GRAY10 && format <= SL2_PIX_GRAY16; }
SL2_HD bool convert_is_bayer(int format) { return format >= SL2_PIX_BAYER_RGGB8 && format <= SL2_PIX_BAYER_BGGR8; }
SL2_HD bool convert_is_raw(int format) { return convert_is_deep(format) || convert_is_bayer(format); }
SL2_HD bool convert_format_known(int format) { return (format >= 0 && format < kConvertFormats) || convert_is_raw(format); }
SL2_HD int convert_deep_bits(int format) { return format == SL2_PIX_GRAY10 ? 10 : format == SL2_PIX_GRAY12 ? 12 : 16; }

// bytes per source pixel
SL2_HD int convert_bpp(int format) {
  return format == SL2_PIX_GRAY8 || convert_is_bayer(format) ? 1 : (format == SL2_PIX_RGB24 || format == SL2_PIX_BGR24) ? 3 : 2;
}
SL2_HD bool convert_is_422(int format) { return format == SL2_PIX_UYVY || format == SL2_PIX_YUYV; }

// cvtColor's RGB -> grey, 14-bit coefficients (they sum to 16384)
SL2_HD int convert_rgb_grey(int r, int g, int b) { return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14; }

// Deep grey: the top eight of the low `bits` bits of a 16-bit word
SL2_HD int convert_deep_grey(int bits, uint32_t v) { return (int)((v & ((1u << bits) - 1u)) >> (bits - 8)); }

// Grey value of pixel x of a source row (every format whose grey needs one row: all but Bayer)
SL2_HD int convert_grey(int format, const uint8_t* row, int x) {
  switch (format) {
    case SL2_PIX_RGB24: return convert_rgb_grey(row[3 * x], row[3 * x + 1], row[3 * x + 2]);
    case SL2_PIX_BGR24: return convert_rgb_grey(row[3 * x + 2], row[3 * x + 1], row[3 * x]);
    case SL2_PIX_UYVY: return row[2 * x + 1];
    case SL2_PIX_YUYV: return row[2 * x];
    case SL2_PIX_GRAY10: case SL2_PIX_GRAY12: case SL2_PIX_GRAY16:
      return convert_deep_grey(convert_deep_bits(format), (uint32_t)row[2 * x] | ((uint32_t)row[2 * x + 1] << 8));
    default: return row[x];
  }
}

// Bayer: index i of an axis of S >= 2 pixels, reflected about the edge pixel (-1 -> 1, S -> S - 2): the colour phase survives
SL2_HD int convert_reflect(int i, int S) { return i < 0 ? -i : i >= S ? 2 * (S - 1) - i : i; }

// Bayer grey of site (x, y) from its value c, h2 = left + right, v2 = up + down and d4 = the four diagonals: bilinear demosaic in
// exact quarters (R4, G4, B4), then the weights of convert_rgb_grey with ONE rounding; at most 16384 * 1020 + 32768.  The colour
// of a site is letter (y & 1) * 2 + (x & 1) of the format's name: red sits at parity (format & 1, format >> 1 & 1).
// A constant mosaic maps to itself, and a mosaic of a flat colour (R, G, B) to convert_rgb_grey(R, G, B):
// (4 X + 32768) >> 16 == (X + 8192) >> 14.
SL2_HD int convert_bayer_grey(int format, int c, int h2, int v2, int d4, int x, int y) {
  const int px = (x ^ format) & 1, py = (y ^ (format >> 1)) & 1;      // 0: red's column / row
  int r4, g4, b4;
  if (px == py) { g4 = h2 + v2; r4 = px ? d4 : 4 * c; b4 = px ? 4 * c : d4; }      // a red or a blue site
  else { g4 = 4 * c; r4 = py ? 2 * v2 : 2 * h2; b4 = py ? 2 * h2 : 2 * v2; }      // green: red to its left and right in red's rows
  return (4899 * r4 + 9617 * g4 + 1868 * b4 + 32768) >> 16;
}

// Grey value of pixel (x, y) of a W x H source whose pixel (0,0) is at base: any format
SL2_HD int convert_grey_at(int format, const uint8_t* base, int pitch, int W, int H, int x, int y) {
  if (!convert_is_bayer(format)) return convert_grey(format, base + (size_t)y * (size_t)pitch, x);
  const int xl = convert_reflect(x - 1, W), xr = convert_reflect(x + 1, W);
  const uint8_t* ru = base + (size_t)convert_reflect(y - 1, H) * (size_t)pitch;
  const uint8_t* rc = base + (size_t)y * (size_t)pitch;
  const uint8_t* rd = base + (size_t)convert_reflect(y + 1, H) * (size_t)pitch;
  return convert_bayer_grey(format, rc[x], rc[xl] + rc[xr], ru[x] + rd[x], ru[xl] + ru[xr] + rd[xl] + rd[xr], x, y);
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
  if (!convert_format_known(s.format)) return "unknown pixel format";
  if (s.width < 1 || s.height < 1) return "width or height below 1";
  if (s.width > kConvertMaxWidth) return "width over 4096";
  if (s.height > kConvertMaxHeight) return "height over 16384";
  if (convert_is_422(s.format) && (s.width & 1)) return "odd width with a 4:2:2 format";
  if (convert_is_bayer(s.format) && (s.width < 2 || s.height < 2)) return "a Bayer source under 2 pixels on an axis";
  if (convert_is_deep(s.format) && ((s.offset | (uint64_t)(uint32_t)s.pitch) & 1)) return "odd offset or pitch with a 16-bit format";
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
  const int h0 = convert_hpass(convert_grey_at(format, base, pitch, width, height, x0, y0), convert_grey_at(format, base, pitch, width, height, x1, y0), a0, a1);
  const int h1 = convert_hpass(convert_grey_at(format, base, pitch, width, height, x0, y1), convert_grey_at(format, base, pitch, width, height, x1, y1), a0, a1);
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

// ---- SL2_RESIZE_AREA: the exact box average (scenelib2_amd.h, "raw camera frames"), integers only, no tables.
// Along an axis of S source and D output pixels, S >= D, in units of 1/D of a source pixel: output d covers [d S, (d + 1) S),
// source i covers [i D, (i + 1) D).  All products stay below 16384 * 4096 = 2^26.
SL2_HD int convert_area_first(int S, int D, int d) { return (int)(((uint32_t)d * (uint32_t)S) / (uint32_t)D); }
SL2_HD int convert_area_last(int S, int D, int d) { return (int)((((uint32_t)d + 1u) * (uint32_t)S - 1u) / (uint32_t)D); }
SL2_HD int convert_area_weight(int S, int D, int d, int i) {
  const int hi = (i + 1) * D < (d + 1) * S ? (i + 1) * D : (d + 1) * S;
  const int lo = i * D > d * S ? i * D : d * S;
  return hi - lo;
}

// The taps of one output column, as the horizontal pass wants them: first and last source column, their two weights; every
// column between them weighs D.  (One tap: x1 == x0 and w0 is its weight.)
struct AreaCol { int x0, x1, w0, w1; };
SL2_HD AreaCol convert_area_col(int S, int D, int d) {
  AreaCol c;
  c.x0 = convert_area_first(S, D, d); c.x1 = convert_area_last(S, D, d);
  c.w0 = convert_area_weight(S, D, d, c.x0); c.w1 = convert_area_weight(S, D, d, c.x1);
  return c;
}

// sum_x wx(d, x) g[x] over one row of values (g[0] is source column `origin`).  Of grey bytes it is at most 255 S < 2^20; of
// column sums (sum_y wy g <= 255 Sy) it is the pixel's acc, and ACC is as wide as that needs.
template <typename ACC, typename T>
SL2_HD ACC convert_area_hsum(const T* g, int origin, const AreaCol& c, int D) {
  ACC h = (ACC)c.w0 * (ACC)g[c.x0 - origin];
  if (c.x1 > c.x0) {
    ACC mid = 0;
    for (int x = c.x0 + 1; x < c.x1; ++x) mid += (ACC)g[x - origin];
    h += (ACC)D * mid + (ACC)c.w1 * (ACC)g[c.x1 - origin];
  }
  return h;
}

// Whether acc <= 255 n (n = Sx Sy source pixels) needs 64 bits: the rounding forms 2 acc + n
SL2_HD bool convert_area_wide(int src_w, int src_h) { return 511ull * (uint64_t)src_w * (uint64_t)src_h > 0xffffffffull; }

// floor((2 acc + n) / (2 n)): the exact mean, halves rounded up
SL2_HD uint8_t convert_area_round(uint64_t acc, uint32_t n) { return (uint8_t)((2ull * acc + n) / (2ull * n)); }
SL2_HD uint8_t convert_area_round(uint32_t acc, uint32_t n) { return (uint8_t)((2u * acc + n) / (2u * n)); }

// Why a source cannot be reduced to out_w x out_h with the area filter (nullptr: it can)
inline const char* convert_area_fault(const sl2_frame_source& s, int out_w, int out_h) {
  if (s.width < out_w || s.height < out_h) return "the area filter only reduces: its source is smaller than the output";
  return nullptr;
}

// The host form's body under SL2_RESIZE_AREA.  grey: scratch of s.width bytes; cols: out_w entries; acc: out_w entries.
inline void convert_frame_host_area_body(const sl2_frame_source& s, const uint8_t* raw, int out_w, int out_h, uint8_t* grey, AreaCol* cols,
                                         uint64_t* acc, uint8_t* out) {
  const uint8_t* base = raw + s.offset;
  const uint32_t n = (uint32_t)s.width * (uint32_t)s.height;
  for (int x = 0; x < out_w; ++x) cols[x] = convert_area_col(s.width, out_w, x);
  for (int dy = 0; dy < out_h; ++dy) {
    for (int x = 0; x < out_w; ++x) acc[x] = 0;
    const int y0 = convert_area_first(s.height, out_h, dy), y1 = convert_area_last(s.height, out_h, dy);
    for (int y = y0; y <= y1; ++y) {
      for (int x = 0; x < s.width; ++x) grey[x] = (uint8_t)convert_grey_at(s.format, base, s.pitch, s.width, s.height, x, y);
      const uint32_t wy = (uint32_t)convert_area_weight(s.height, out_h, dy, y);
      for (int x = 0; x < out_w; ++x) acc[x] += (uint64_t)(wy * convert_area_hsum<uint32_t>(grey, 0, cols[x], out_w));      // wy h < 2^32
    }
    for (int x = 0; x < out_w; ++x) out[(size_t)dy * out_w + x] = convert_area_round(acc[x], n);
  }
}

// ---- The lens remap (scenelib2_amd.h, "the lens remap"): a sequence follows a per-pixel map into its source's grey plane, the
// equivalent of cv::remap over cv::initUndistortRectifyMap's map.  A map belongs to a source size W x H and to the output size:
// int32 xy[out_h][out_w][2], (X, Y) the position in the source grey plane in 1/32 of a source pixel, pixel centres on integers
// (X = 32 x is column x: rectify_source's convention), X == SL2_REMAP_BORDER meaning no source.  Per output pixel, in 32-bit
// integers: a border entry gives 0; else fx = X & 31, ix = (X - fx) / 32 (two's complement: the floor), fy and iy likewise; a
// tap is g[iy][ix] where 0 <= ix < W and 0 <= iy < H, else 0, g being convert_grey_at's grey of the source's format (for Bayer
// the demosaic, the neighbours of an in-image tap reflected as everywhere); a neighbour whose weight is 0 is not read;
//   out = ((32 - fx)(32 - fy) p00 + fx (32 - fy) p10 + (32 - fx) fy p01 + fx fy p11 + 512) >> 10.
// rectify_pixel's arithmetic (sl2_rectify_dev.hpp) over convert_grey_at: the identity for the identity map, a constant source
// stays constant wherever all four taps lie inside.  NO anti-aliasing: two taps an axis whatever the map's local scale, so a map
// that reduces by much more than two aliases like SL2_RESIZE_LINEAR.
//
// remap_pixel is that rule without a branch, because on the device a branch around a load is a round trip to memory that the
// next load waits for: a tap that does not count - outside the image, a neighbour of weight 0, any tap of a border entry (ix =
// -2^26: none is inside) - gets the weight 0, and the byte fetched for it comes from the clamped, in-image coordinate and is
// discarded.  So "is not read" holds in the sense that matters: nothing outside the W x H source is ever addressed, whatever the
// entry.  Bayer: the 3 x 3 neighbourhoods of the four taps overlap in a 4 x 4 block, columns reflect(ix - 1 + j) and rows
// reflect(iy - 1 + i) (clamped where the tap they serve is itself outside): sixteen bytes instead of thirty-six, and for an
// in-image tap exactly the bytes convert_grey_at names.
SL2_HD int remap_clamp(int i, int S) { return i < 0 ? 0 : i >= S ? S - 1 : i; }

SL2_HD uint8_t remap_pixel(int format, const uint8_t* base, int pitch, int W, int H, int32_t X, int32_t Y) {
  const int fx = X & 31, fy = Y & 31;
  const int ix = (X - fx) / 32, iy = (Y - fy) / 32;      // X - fx is a multiple of 32 and no smaller than INT32_MIN
  const bool cx0 = ix >= 0 && ix < W, cx1 = fx != 0 && ix + 1 >= 0 && ix + 1 < W;
  const bool cy0 = iy >= 0 && iy < H, cy1 = fy != 0 && iy + 1 >= 0 && iy + 1 < H;
  const int w00 = cx0 && cy0 ? (32 - fx) * (32 - fy) : 0, w10 = cx1 && cy0 ? fx * (32 - fy) : 0;
  const int w01 = cx0 && cy1 ? (32 - fx) * fy : 0, w11 = cx1 && cy1 ? fx * fy : 0;
  int p00, p10, p01, p11;
  if (!convert_is_bayer(format)) {
    const int x0 = remap_clamp(ix, W), x1 = remap_clamp(ix + 1, W);
    const uint8_t* r0 = base + (size_t)remap_clamp(iy, H) * (size_t)pitch;
    const uint8_t* r1 = base + (size_t)remap_clamp(iy + 1, H) * (size_t)pitch;
    p00 = convert_grey(format, r0, x0); p10 = convert_grey(format, r0, x1);
    p01 = convert_grey(format, r1, x0); p11 = convert_grey(format, r1, x1);
  } else {
    int p[4][4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) {
      const uint8_t* row = base + (size_t)remap_clamp(convert_reflect(iy - 1 + i, H), H) * (size_t)pitch;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int j = 0; j < 4; ++j) p[i][j] = row[remap_clamp(convert_reflect(ix - 1 + j, W), W)];
    }
    // the tap at column ix + a, row iy + b has its centre at p[b + 1][a + 1]
#define SL2_REMAP_BAYER(a, b)                                                                                        \
  convert_bayer_grey(format, p[b + 1][a + 1], p[b + 1][a] + p[b + 1][a + 2], p[b][a + 1] + p[b + 2][a + 1],          \
                     p[b][a] + p[b][a + 2] + p[b + 2][a] + p[b + 2][a + 2], ix + a, iy + b)
    p00 = SL2_REMAP_BAYER(0, 0); p10 = SL2_REMAP_BAYER(1, 0); p01 = SL2_REMAP_BAYER(0, 1); p11 = SL2_REMAP_BAYER(1, 1);
#undef SL2_REMAP_BAYER
  }
  return (uint8_t)((w00 * p00 + w10 * p10 + w01 * p01 + w11 * p11 + 512) >> 10);
}

// Whether an entry can reach a source pixel with a weight above 0: columns ix (always weighed) and ix + 1 (where fx != 0), rows likewise
SL2_HD bool remap_reaches(int W, int H, int32_t X, int32_t Y) {
  if (X == SL2_REMAP_BORDER) return false;
  const int fx = X & 31, fy = Y & 31;
  const int ix = (X - fx) / 32, iy = (Y - fy) / 32;
  const bool col = (ix >= 0 && ix < W) || (fx && ix == -1), row = (iy >= 0 && iy < H) || (fy && iy == -1);
  return col && row;
}

// The device form of a map ("the lens remap").  sl2_converter_set_map turns every entry that reaches no
// source pixel into the border, so a live entry has X + 32 in 1 .. 32 (W + 1) - 1 and Y + 32 in 1 .. 32 (H + 1) - 1.  Where the
// bits of those two ranges sum to 32 or less - every source up to 2046 x 2046, 4096 x 511 ... - an entry is ONE word, X + 32 in
// the low xbits bits and Y + 32 above them, the border all ones (never a live entry's word: checked when the form is chosen).  Else it is two words,
// X and Y as they are: 38 bits at the caps.
constexpr uint32_t kRemapBorderWord = 0xffffffffu;
SL2_HD int remap_bits(int S) { int b = 0; while (((32u * ((uint32_t)S + 1u) - 1u) >> b) != 0u) ++b; return b; }
// xbits of the one-word form, 0: the source needs the two-word form
SL2_HD int remap_packed_xbits(int W, int H) {
  const int bx = remap_bits(W), by = remap_bits(H);
  if (bx + by > 32) return 0;
  const uint32_t top = ((32u * ((uint32_t)H + 1u) - 1u) << bx) | (32u * ((uint32_t)W + 1u) - 1u);      // the largest live word
  return top == kRemapBorderWord ? 0 : bx;
}
SL2_HD uint32_t remap_pack(int xbits, int32_t X, int32_t Y) { return (uint32_t)(X + 32) | ((uint32_t)(Y + 32) << xbits); }
SL2_HD void remap_unpack(int xbits, uint32_t w, int32_t* X, int32_t* Y) {
  if (w == kRemapBorderWord) { *X = SL2_REMAP_BORDER; *Y = 0; return; }
  *X = (int32_t)(w & ((1u << xbits) - 1u)) - 32;
  *Y = (int32_t)(w >> xbits) - 32;
}

// The host form's body: one source through the map xy[out_h][out_w][2] into out[out_h][out_w]
inline void remap_frame_host_body(const sl2_frame_source& s, const int32_t* xy, const uint8_t* raw, int out_w, int out_h, uint8_t* out) {
  const uint8_t* base = raw + s.offset;
  for (size_t i = 0; i < (size_t)out_w * (size_t)out_h; ++i)
    out[i] = remap_pixel(s.format, base, s.pitch, s.width, s.height, xy[2 * i], xy[2 * i + 1]);
}

// ---- Maps from calibrations (scenelib2_amd.h, "maps from calibrations"): host only, FP64, -ffp-contract=off.  Every line is
// the header's, in its order of operations.
constexpr double kLensSourceMax = 1048576.0;      // a source position beyond +-2^20 is the border (so that 32 us fits an int)

// Image-plane coordinates (a, b) of target pixel (x, y): x to the right, y down (OpenCV's x', y').  False: the border.
inline bool lens_target_ray(const sl2_camera& t, int x, int y, double* a, double* b) {
  const double cx = (double)x - t.u0, cy = (double)y - t.v0;
  const double f = 1.0 - (2.0 * t.kd1) * (cx * cx + cy * cy);
  if (!(f > 0.0)) return false;
  const double s = sqrt(f);
  *a = (cx / s) / t.fku;
  *b = (cy / s) / t.fkv;
  return true;
}

// Where the lens images (a, b): the source position in pixels.  False: the border.
inline bool lens_project(const sl2_lens& l, double a, double b, double* us, double* vs) {
  const double* k = l.k;
  if (l.model == SL2_LENS_RADIAL1) {
    const double px = l.fx * a, py = l.fy * b;
    const double q = 1.0 + (2.0 * k[0]) * (px * px + py * py);
    if (!(q > 0.0)) return false;
    const double s = sqrt(q);
    *us = px / s + l.cx; *vs = py / s + l.cy;
    return true;
  }
  if (l.model == SL2_LENS_BROWN) {
    const double r2 = a * a + b * b, r4 = r2 * r2, r6 = r4 * r2;
    const double num = ((1.0 + k[0] * r2) + k[1] * r4) + k[4] * r6;
    const double den = ((1.0 + k[5] * r2) + k[6] * r4) + k[7] * r6;
    if (den == 0.0) return false;
    const double rad = num / den, ab = a * b;
    const double xd = (a * rad + (2.0 * k[2]) * ab) + k[3] * (r2 + 2.0 * (a * a));
    const double yd = (b * rad + k[2] * (r2 + 2.0 * (b * b))) + (2.0 * k[3]) * ab;
    *us = l.fx * xd + l.cx; *vs = l.fy * yd + l.cy;
    return true;
  }
  // SL2_LENS_FISHEYE
  const double r = sqrt(a * a + b * b);
  if (r == 0.0) { *us = l.cx; *vs = l.cy; return true; }
  const double th = atan(r);
  const double t2 = th * th, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
  const double thd = th * ((((1.0 + k[0] * t2) + k[1] * t4) + k[2] * t6) + k[3] * t8);
  const double sc = thd / r;
  *us = l.fx * (a * sc) + l.cx; *vs = l.fy * (b * sc) + l.cy;
  return true;
}

inline void lens_map_entry(const sl2_lens& l, const sl2_camera& t, int x, int y, int32_t* X, int32_t* Y) {
  double a, b, us, vs;
  *X = SL2_REMAP_BORDER; *Y = 0;
  if (!lens_target_ray(t, x, y, &a, &b) || !lens_project(l, a, b, &us, &vs)) return;
  // (a NaN or an infinity fails one of the four comparisons)
  if (!(us >= -kLensSourceMax && us <= kLensSourceMax && vs >= -kLensSourceMax && vs <= kLensSourceMax)) return;
  *X = (int32_t)floor(us * 32.0 + 0.5);
  *Y = (int32_t)floor(vs * 32.0 + 0.5);
}

}  // namespace sl2
