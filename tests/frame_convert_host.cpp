// Stand-alone bounds program of the frame conversion (tests/test_frame_convert_host.py compiles it with
// -fsanitize=address,undefined and runs it): the host body of scenelib2_amd/csrc/sl2_convert_dev.hpp over the edge shapes, every
// source in a heap block of EXACTLY offset + (height - 1) * pitch + row bytes and every output in a block of exactly
// out_width * out_height - a tap that reads one byte past a row, or a store past the image, is a heap-buffer-overflow here.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../scenelib2_amd/csrc/sl2_convert_dev.hpp"

using namespace sl2;

static uint32_t rng_state = 12345u;
static uint8_t next_byte() { rng_state = rng_state * 1664525u + 1013904223u; return (uint8_t)(rng_state >> 24); }

int main() {
  const int outs[4][2] = {{320, 240}, {33, 17}, {7, 5}, {1, 1}};
  const int srcs[11][2] = {{1, 1}, {2, 2}, {5, 3}, {31, 17}, {320, 240}, {321, 241}, {322, 242}, {160, 120}, {640, 480}, {961, 3}, {4096, 2}};
  const int pads[3] = {0, 1, 13};
  const uint64_t offsets[3] = {0, 1, 7};
  long cases = 0, pixels = 0;
  for (const auto& o : outs)
    for (const auto& sz : srcs)
      for (int fmt = 0; fmt < kConvertFormats; ++fmt) {
        if (convert_is_422(fmt) && (sz[0] & 1)) continue;
        for (int pi = 0; pi < 3; ++pi) {
          sl2_frame_source s;
          s.width = sz[0]; s.height = sz[1]; s.format = fmt;
          s.pitch = sz[0] * convert_bpp(fmt) + pads[pi];
          s.offset = offsets[(pi + fmt + cases) % 3];
          const uint64_t need = convert_source_end(s);
          if (convert_source_fault(s, need, true)) { printf("exact size refused\n"); return 1; }
          if (!convert_source_fault(s, need - 1, true)) { printf("one byte short accepted\n"); return 1; }
          uint8_t* raw = (uint8_t*)malloc(need);
          uint8_t* out = (uint8_t*)malloc((size_t)o[0] * o[1]);
          uint32_t* col = (uint32_t*)malloc(sizeof(uint32_t) * o[0]);
          uint32_t* row = (uint32_t*)malloc(sizeof(uint32_t) * o[1]);
          for (uint64_t i = 0; i < need; ++i) raw[i] = next_byte();
          if (!convert_frame_host_body(s, raw, o[0], o[1], col, row, out)) { printf("a tap did not pack\n"); return 1; }
          if (o[0] == s.width && o[1] == s.height)      // the identity size reproduces the grey plane
            for (int y = 0; y < o[1]; ++y)
              for (int x = 0; x < o[0]; ++x)
                if (out[(size_t)y * o[0] + x] != convert_grey(fmt, raw + s.offset + (size_t)y * s.pitch, x)) { printf("identity broken\n"); return 1; }
          ++cases; pixels += (long)o[0] * o[1];
          free(row); free(col); free(out); free(raw);
        }
      }
  // every tap of every extent up to the caps' neighbourhood packs and unpacks to itself
  const int extents[] = {1, 2, 3, 5, 17, 240, 241, 320, 321, 480, 961, 1080, 2160, 4096, 16384};
  for (int S : extents)
    for (int D : extents) {
      if (D > kConvertMaxOut) continue;
      for (int d = 0; d < D; ++d) {
        int i, w0, w1, j, v0, v1;
        uint32_t t;
        convert_taps(S, D, d, &i, &w0, &w1);
        if (i < 0 || i > S - 1 || !convert_pack_tap(i, w0, w1, &t)) { printf("tap %d of %d -> %d does not pack\n", d, S, D); return 1; }
        convert_unpack_tap(t, &j, &v0, &v1);
        if (j != i || v0 != w0 || v1 != w1) { printf("tap %d of %d -> %d does not survive packing\n", d, S, D); return 1; }
      }
    }
  printf("ok %ld cases %ld pixels\n", cases, pixels);
  return 0;
}
