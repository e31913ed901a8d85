// Stand-alone bounds program of the machine-vision formats (tests/test_frame_convert_raw_host.py compiles it with
// -fsanitize=address,undefined and runs it): both host bodies of scenelib2_amd/csrc/sl2_convert_dev.hpp for the deep grey and the
// Bayer formats over the edge shapes, every source in a heap block of EXACTLY offset + (height - 1) * pitch + row bytes, every
// output and every scratch array in a block of exactly its size - a Bayer neighbour taken from outside the image instead of
// reflected, or the high byte of a row's last word read past it, stops the program here.  It also checks what the definition
// promises: the identity, a constant image mapping to itself, a flat colour mapping to convert_rgb_grey.
#include <cstdio>
#include <cstdlib>

#include "../scenelib2_amd/csrc/sl2_convert_dev.hpp"

using namespace sl2;

static uint32_t rng_state = 97531u;
static uint8_t next_byte() { rng_state = rng_state * 1664525u + 1013904223u; return (uint8_t)(rng_state >> 24); }

// fill: -1 random bytes, else that byte everywhere.  Returns false after printing what went wrong.
static bool run(int sw, int sh, int ow, int oh, int fmt, int filter, int pad, uint64_t offset, int fill) {
  sl2_frame_source s;
  s.width = sw; s.height = sh; s.format = fmt; s.pitch = sw * convert_bpp(fmt) + pad; s.offset = offset;
  const uint64_t need = convert_source_end(s);
  if (convert_source_fault(s, need, true) || (filter == SL2_RESIZE_AREA && convert_area_fault(s, ow, oh))) { printf("a good source was refused\n"); return false; }
  if (!convert_source_fault(s, need - 1, true)) { printf("a source one byte past its buffer was accepted\n"); return false; }
  uint8_t* raw = (uint8_t*)malloc(need);
  uint8_t* out = (uint8_t*)malloc((size_t)ow * oh);
  for (uint64_t i = 0; i < need; ++i) raw[i] = fill < 0 ? next_byte() : (uint8_t)fill;
  if (filter == SL2_RESIZE_AREA) {
    uint8_t* grey = (uint8_t*)malloc((size_t)sw);
    AreaCol* cols = (AreaCol*)malloc(sizeof(AreaCol) * ow);
    uint64_t* acc = (uint64_t*)malloc(sizeof(uint64_t) * ow);
    convert_frame_host_area_body(s, raw, ow, oh, grey, cols, acc, out);
    free(acc); free(cols); free(grey);
  } else {
    uint32_t* col = (uint32_t*)malloc(sizeof(uint32_t) * ow);
    uint32_t* row = (uint32_t*)malloc(sizeof(uint32_t) * oh);
    const bool packed = convert_frame_host_body(s, raw, ow, oh, col, row, out);
    free(row); free(col);
    if (!packed) { printf("a tap did not pack\n"); free(out); free(raw); return false; }
  }
  // a constant source: Bayer keeps the byte, deep grey the top eight of its N bits
  const int fill_grey = fill < 0 ? 0 : convert_is_bayer(fmt) ? fill : convert_deep_grey(convert_deep_bits(fmt), (uint32_t)fill * 257u);
  bool ok = true;
  for (int y = 0; y < oh && ok; ++y)
    for (int x = 0; x < ow && ok; ++x) {
      const uint8_t got = out[(size_t)y * ow + x];
      if (ow == sw && oh == sh && got != convert_grey_at(fmt, raw + s.offset, s.pitch, sw, sh, x, y)) { printf("identity broken\n"); ok = false; }
      if (fill >= 0 && got != fill_grey) { printf("format %d, %d x %d -> %d x %d: constant %d came out as %d\n", fmt, sw, sh, ow, oh, fill, got); ok = false; }
    }
  free(out); free(raw);
  return ok;
}

// A mosaic sampled from a flat colour gives convert_rgb_grey at every site, the corners and edges included
static bool flat(int fmt, int sw, int sh, int r, int g, int b) {
  sl2_frame_source s;
  s.width = sw; s.height = sh; s.format = fmt; s.pitch = sw; s.offset = 0;
  uint8_t* raw = (uint8_t*)malloc(convert_source_end(s));
  const char* name = fmt == SL2_PIX_BAYER_RGGB8 ? "RGGB" : fmt == SL2_PIX_BAYER_GRBG8 ? "GRBG" : fmt == SL2_PIX_BAYER_GBRG8 ? "GBRG" : "BGGR";
  for (int y = 0; y < sh; ++y)
    for (int x = 0; x < sw; ++x) {
      const char c = name[(y & 1) * 2 + (x & 1)];
      raw[(size_t)y * sw + x] = (uint8_t)(c == 'R' ? r : c == 'G' ? g : b);
    }
  bool ok = true;
  for (int y = 0; y < sh && ok; ++y)
    for (int x = 0; x < sw && ok; ++x)
      if (convert_grey_at(fmt, raw, s.pitch, sw, sh, x, y) != convert_rgb_grey(r, g, b)) { printf("format %d: flat colour broken at (%d, %d)\n", fmt, x, y); ok = false; }
  free(raw);
  return ok;
}

int main() {
  // source and output size; AREA where the source is no smaller
  const int shapes[14][4] = {{2, 2, 1, 1}, {3, 3, 1, 1}, {2, 3, 7, 5}, {3, 2, 33, 17}, {15, 9, 7, 5}, {16, 17, 7, 5}, {17, 9, 16, 8}, {31, 17, 11, 9},
                             {33, 17, 33, 17}, {47, 17, 33, 17}, {11, 9, 11, 9}, {1001, 40, 11, 9}, {4096, 6, 7, 5}, {4096, 6, 33, 17}};
  const int formats[7] = {SL2_PIX_GRAY10, SL2_PIX_GRAY12, SL2_PIX_GRAY16, SL2_PIX_BAYER_RGGB8, SL2_PIX_BAYER_GRBG8, SL2_PIX_BAYER_GBRG8,
                          SL2_PIX_BAYER_BGGR8};
  const int pads8[3] = {0, 1, 13}, pads16[3] = {0, 2, 14};
  const uint64_t offsets8[4] = {0, 1, 7, 15}, offsets16[3] = {0, 2, 14};
  long cases = 0;
  for (const auto& sh : shapes)
    for (int fmt : formats)
      for (int filter = SL2_RESIZE_LINEAR; filter <= SL2_RESIZE_AREA; ++filter) {
        if (filter == SL2_RESIZE_AREA && (sh[0] < sh[2] || sh[1] < sh[3])) continue;
        for (int pi = 0; pi < 3; ++pi) {
          const bool deep = convert_is_deep(fmt);
          const int pad = deep ? pads16[pi] : pads8[pi];
          const uint64_t offset = deep ? offsets16[(pi + cases) % 3] : offsets8[(pi + cases) % 4];
          if (!run(sh[0], sh[1], sh[2], sh[3], fmt, filter, pad, offset, -1)) return 1;
          ++cases;
        }
        const int fills[5] = {0, 1, 127, 254, 255};
        for (int fill : fills) {
          if (!run(sh[0], sh[1], sh[2], sh[3], fmt, filter, 0, 0, fill)) return 1;
          ++cases;
        }
      }
  for (int fmt = SL2_PIX_BAYER_RGGB8; fmt <= SL2_PIX_BAYER_BGGR8; ++fmt) {
    if (!flat(fmt, 2, 2, 255, 0, 0) || !flat(fmt, 3, 2, 0, 255, 0) || !flat(fmt, 2, 3, 0, 0, 255) || !flat(fmt, 17, 9, 201, 37, 118) ||
        !flat(fmt, 16, 8, 255, 255, 255))
      return 1;
    cases += 5;
  }
  // what is refused: Bayer under 2 pixels on an axis, an odd offset or pitch with 16-bit words, the unassigned ids
  sl2_frame_source s;
  s.width = 1; s.height = 8; s.format = SL2_PIX_BAYER_RGGB8; s.pitch = 8; s.offset = 0;
  if (!convert_source_fault(s, 1 << 20, true)) { printf("a 1 x N Bayer source was accepted\n"); return 1; }
  s.width = 8; s.height = 1;
  if (!convert_source_fault(s, 1 << 20, true)) { printf("an N x 1 Bayer source was accepted\n"); return 1; }
  s.height = 8; s.format = SL2_PIX_GRAY12; s.pitch = 17;
  if (!convert_source_fault(s, 1 << 20, true)) { printf("an odd pitch was accepted\n"); return 1; }
  s.pitch = 16; s.offset = 3;
  if (!convert_source_fault(s, 1 << 20, true)) { printf("an odd offset was accepted\n"); return 1; }
  s.offset = 2;
  if (convert_source_fault(s, 1 << 20, true)) { printf("a good source was refused\n"); return 1; }
  for (int id = -1; id < 40; ++id) {
    const bool known = (id >= 0 && id < kConvertFormats) || (id >= 16 && id <= 18) || (id >= 24 && id <= 27);
    if (convert_format_known(id) != known) { printf("format id %d misjudged\n", id); return 1; }
  }
  printf("ok %ld cases\n", cases);
  return 0;
}
