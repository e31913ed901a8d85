// Stand-alone bounds program of the lens remap (tests/test_frame_remap_host.py compiles it with -fsanitize=address,undefined and
// runs it): remap_frame_host_body of scenelib2_amd/csrc/sl2_convert_dev.hpp for every format, every source in a heap block of
// EXACTLY offset + (height - 1) * pitch + row bytes, the map and the output in blocks of exactly their sizes, under maps that
// point at and around every edge of the source: every position of a ring three pixels wide around the image in steps that cover
// every fraction class (0, 1, 16, 31), the extreme int32 positions, the border entry.  A tap read outside the image, a weighted
// neighbour taken past the last row, or an overflow in the index arithmetic stops the program here.  It also checks what the
// definition promises (the identity; a constant inside), that what sl2_converter_set_map calls unreachable gives 0, and that
// the device form of an entry unpacks to the entry for sizes on both sides of the one-word limit.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../scenelib2_amd/csrc/sl2_convert_dev.hpp"

using namespace sl2;

static uint32_t rng_state = 24680u;
static uint8_t next_byte() { rng_state = rng_state * 1664525u + 1013904223u; return (uint8_t)(rng_state >> 24); }

// The positions along an axis of S pixels that matter: around both edges in every fraction class, the middle, the extremes
static std::vector<int32_t> edge_positions(int S) {
  std::vector<int32_t> p;
  const int fr[4] = {0, 1, 16, 31};
  for (int i = -3; i <= 2; ++i)
    for (int f : fr) { p.push_back(32 * i + f); p.push_back(32 * (S - 1 + i) + f); }
  p.push_back(32 * (S / 2) + 7);
  const int32_t far[8] = {INT32_MIN, INT32_MIN + 1, INT32_MIN + 31, INT32_MIN + 32, INT32_MAX, INT32_MAX - 31, -(1 << 25), 1 << 25};
  for (int32_t v : far) p.push_back(v);
  return p;
}

static bool run(int sw, int sh, int fmt, int pad, uint64_t offset, int fill) {
  sl2_frame_source s;
  s.width = sw; s.height = sh; s.format = fmt; s.pitch = sw * convert_bpp(fmt) + pad; s.offset = offset;
  const uint64_t need = convert_source_end(s);
  if (convert_source_fault(s, need, true)) { printf("a good source was refused\n"); return false; }
  uint8_t* raw = (uint8_t*)malloc(need);
  for (uint64_t i = 0; i < need; ++i) raw[i] = fill < 0 ? next_byte() : (uint8_t)fill;
  const std::vector<int32_t> xs = edge_positions(sw), ys = edge_positions(sh);
  const int ow = (int)xs.size(), oh = (int)ys.size();
  int32_t* xy = (int32_t*)malloc(sizeof(int32_t) * 2 * ow * oh);
  uint8_t* out = (uint8_t*)malloc((size_t)ow * oh);
  for (int y = 0; y < oh; ++y)
    for (int x = 0; x < ow; ++x) { xy[2 * (y * ow + x)] = xs[x]; xy[2 * (y * ow + x) + 1] = ys[y]; }
  remap_frame_host_body(s, xy, raw, ow, oh, out);
  const int fill_grey = fill < 0 ? 0 : convert_is_deep(fmt) ? convert_deep_grey(convert_deep_bits(fmt), (uint32_t)fill * 257u)
                      : (fmt == SL2_PIX_RGB24 || fmt == SL2_PIX_BGR24) ? convert_rgb_grey(fill, fill, fill) : fill;
  const int xbits = remap_packed_xbits(sw, sh);
  bool ok = true;
  for (int y = 0; y < oh && ok; ++y)
    for (int x = 0; x < ow && ok; ++x) {
      const int32_t X = xs[x], Y = ys[y];
      const uint8_t got = out[y * ow + x];
      const bool reach = remap_reaches(sw, sh, X, Y);
      if (!reach && got != 0) { printf("an entry that reaches nothing gave %d\n", got); ok = false; }
      if (X == SL2_REMAP_BORDER && got != 0) { printf("a border entry gave %d\n", got); ok = false; }
      const bool inside = X != SL2_REMAP_BORDER && X >= 0 && X <= 32 * (sw - 1) && Y >= 0 && Y <= 32 * (sh - 1);
      if (fill >= 0 && inside && got != fill_grey) { printf("format %d: constant %d came out as %d inside\n", fmt, fill, got); ok = false; }
      if (inside && !(X & 31) && !(Y & 31) && got != convert_grey_at(fmt, raw + s.offset, s.pitch, sw, sh, X / 32, Y / 32)) { printf("identity broken\n"); ok = false; }
      if (reach) {      // the device form gives the entry back
        int32_t X2, Y2;
        if (xbits) {
          const uint32_t w = remap_pack(xbits, X, Y);
          if (w == kRemapBorderWord) { printf("a live entry packs to the border word\n"); ok = false; }
          remap_unpack(xbits, w, &X2, &Y2);
          if (X2 != X || Y2 != Y) { printf("%d x %d: (%d, %d) unpacks to (%d, %d)\n", sw, sh, X, Y, X2, Y2); ok = false; }
        }
      }
    }
  free(out); free(xy); free(raw);
  return ok;
}

// Every live entry of a W x H source survives the one-word form where remap_packed_xbits allows it: the four corners of the
// live range suffice (the fields are independent), and the border word is none of them
static bool packs(int W, int H, bool want_packed) {
  const int xbits = remap_packed_xbits(W, H);
  if ((xbits != 0) != want_packed) { printf("%d x %d: one-word form %s\n", W, H, xbits ? "chosen" : "not chosen"); return false; }
  if (!xbits) return true;
  const int32_t xs[2] = {-31, 32 * W - 1}, ys[2] = {-31, 32 * H - 1};
  for (int32_t X : xs)
    for (int32_t Y : ys) {
      int32_t X2, Y2;
      const uint32_t w = remap_pack(xbits, X, Y);
      remap_unpack(xbits, w, &X2, &Y2);
      if (w == kRemapBorderWord || X2 != X || Y2 != Y || !remap_reaches(W, H, X, Y)) { printf("%d x %d: (%d, %d) does not survive\n", W, H, X, Y); return false; }
    }
  int32_t X2, Y2;
  remap_unpack(xbits, kRemapBorderWord, &X2, &Y2);
  return X2 == SL2_REMAP_BORDER;
}

int main() {
  const int shapes[6][2] = {{2, 2}, {3, 3}, {2, 5}, {47, 17}, {16, 9}, {4096, 6}};
  const int formats[12] = {SL2_PIX_GRAY8, SL2_PIX_RGB24, SL2_PIX_BGR24, SL2_PIX_UYVY, SL2_PIX_YUYV, SL2_PIX_GRAY10, SL2_PIX_GRAY12, SL2_PIX_GRAY16,
                           SL2_PIX_BAYER_RGGB8, SL2_PIX_BAYER_GRBG8, SL2_PIX_BAYER_GBRG8, SL2_PIX_BAYER_BGGR8};
  const int pads8[3] = {0, 1, 13}, pads16[3] = {0, 2, 14};
  const uint64_t offsets8[4] = {0, 1, 7, 15}, offsets16[3] = {0, 2, 14};
  long cases = 0;
  for (const auto& sh : shapes)
    for (int fmt : formats) {
      const int sw = convert_is_422(fmt) && (sh[0] & 1) ? sh[0] + 1 : sh[0];
      const bool deep = convert_is_deep(fmt);
      for (int pi = 0; pi < 3; ++pi) {
        if (!run(sw, sh[1], fmt, deep ? pads16[pi] : pads8[pi], deep ? offsets16[(pi + cases) % 3] : offsets8[(pi + cases) % 4], -1)) return 1;
        ++cases;
      }
      const int fills[3] = {0, 127, 255};
      for (int fill : fills) {
        if (!run(sw, sh[1], fmt, 0, 0, fill)) return 1;
        ++cases;
      }
    }
  // the one-word form: up to 32 bits for the two fields, and never where the largest live word is the border word
  if (!packs(1, 1, true) || !packs(640, 480, true) || !packs(1280, 960, true) || !packs(1920, 1080, true) || !packs(2046, 2047, true) ||
      !packs(2047, 2047, false) || !packs(2048, 2047, false) || !packs(4096, 511, true) || !packs(4096, 512, false) || !packs(1022, 4095, true) || !packs(1023, 4095, false) ||
      !packs(4096, 16384, false) || !packs(1, 16384, true))
    return 1;
  printf("ok %ld cases\n", cases);
  return 0;
}
