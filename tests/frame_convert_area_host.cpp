// Stand-alone bounds program of the area filter (tests/test_frame_convert_area_host.py compiles it with
// -fsanitize=address,undefined and runs it): the SL2_RESIZE_AREA host body of scenelib2_amd/csrc/sl2_convert_dev.hpp over the small
// shapes and the wide-accumulator case, every source in a heap block of EXACTLY offset + (height - 1) * pitch + row bytes, every
// output and every scratch array in a block of exactly its size - a tap one column past a row, a weight that overflows its
// integer or a store past the image stops the program here.  It also checks what the definition promises: weights in 1 .. D
// that sum to S, the identity, and a constant image mapping to itself.
#include <cstdio>
#include <cstdlib>

#include "../scenelib2_amd/csrc/sl2_convert_dev.hpp"

using namespace sl2;

static uint32_t rng_state = 2468u;
static uint8_t next_byte() { rng_state = rng_state * 1664525u + 1013904223u; return (uint8_t)(rng_state >> 24); }

// fill: -1 random bytes, else that byte everywhere.  Returns false after printing what went wrong.
static bool run(int sw, int sh, int ow, int oh, int fmt, int pad, uint64_t offset, int fill) {
  sl2_frame_source s;
  s.width = sw; s.height = sh; s.format = fmt; s.pitch = sw * convert_bpp(fmt) + pad; s.offset = offset;
  const uint64_t need = convert_source_end(s);
  if (convert_source_fault(s, need, true) || convert_area_fault(s, ow, oh)) { printf("a good source was refused\n"); return false; }
  uint8_t* raw = (uint8_t*)malloc(need);
  uint8_t* out = (uint8_t*)malloc((size_t)ow * oh);
  uint8_t* grey = (uint8_t*)malloc((size_t)sw);
  AreaCol* cols = (AreaCol*)malloc(sizeof(AreaCol) * ow);
  uint64_t* acc = (uint64_t*)malloc(sizeof(uint64_t) * ow);
  for (uint64_t i = 0; i < need; ++i) raw[i] = fill < 0 ? next_byte() : (uint8_t)fill;
  convert_frame_host_area_body(s, raw, ow, oh, grey, cols, acc, out);
  bool ok = true;
  for (int y = 0; y < oh && ok; ++y)
    for (int x = 0; x < ow && ok; ++x) {
      const uint8_t got = out[(size_t)y * ow + x];
      if (ow == sw && oh == sh && got != convert_grey(fmt, raw + s.offset + (size_t)y * s.pitch, x)) { printf("identity broken\n"); ok = false; }
      if (fill >= 0 && fmt == SL2_PIX_GRAY8 && got != fill) { printf("%d x %d -> %d x %d: constant %d came out as %d\n", sw, sh, ow, oh, fill, got); ok = false; }
    }
  free(acc); free(cols); free(grey); free(out); free(raw);
  return ok;
}

int main() {
  const int shapes[8][4] = {{1, 1, 1, 1}, {2, 2, 1, 1}, {5, 3, 1, 1}, {31, 17, 7, 5}, {33, 17, 33, 17}, {322, 242, 320, 240}, {4096, 18, 33, 17},
                            {4096, 2, 7, 1}};
  const int pads[3] = {0, 1, 13};
  const uint64_t offsets[3] = {0, 1, 7};
  long cases = 0;
  for (const auto& sh : shapes)
    for (int fmt = 0; fmt < kConvertFormats; ++fmt) {
      if (convert_is_422(fmt) && (sh[0] & 1)) continue;
      for (int pi = 0; pi < 3; ++pi) {
        if (!run(sh[0], sh[1], sh[2], sh[3], fmt, pads[pi], offsets[(pi + fmt + cases) % 3], -1)) return 1;
        ++cases;
      }
    }
  // 255 Sx Sy needs more than 32 bits
  if (!convert_area_wide(4096, 4200) || convert_area_wide(1920, 1080)) { printf("accumulator width misjudged\n"); return 1; }
  if (!run(4096, 4200, 7, 5, SL2_PIX_GRAY8, 0, 0, 255) || !run(4096, 4200, 320, 240, SL2_PIX_GRAY8, 0, 0, 255) ||
      !run(4096, 4200, 7, 5, SL2_PIX_GRAY8, 0, 0, -1))
    return 1;
  cases += 3;
  // the weights of every extent up to the caps: 1 .. D each, summing to S, the taps joined end to end
  const int extents[] = {1, 2, 3, 5, 7, 17, 240, 241, 320, 321, 480, 961, 1080, 2160, 4096, 16384};
  for (int S : extents)
    for (int D : extents) {
      if (D > kConvertMaxOut || D > S) continue;
      int prev_last = -1;
      for (int d = 0; d < D; ++d) {
        const int i0 = convert_area_first(S, D, d), i1 = convert_area_last(S, D, d);
        if (i0 < 0 || i1 >= S || i1 < i0 || (i0 != prev_last && i0 != prev_last + 1)) { printf("taps of %d of %d -> %d\n", d, S, D); return 1; }
        long sum = 0;
        for (int i = i0; i <= i1; ++i) {
          const int w = convert_area_weight(S, D, d, i);
          if (w < 1 || w > D) { printf("weight %d of %d -> %d\n", w, S, D); return 1; }
          sum += w;
        }
        if (sum != S) { printf("weights of %d of %d -> %d sum to %ld\n", d, S, D, sum); return 1; }
        prev_last = i1;
      }
      if (prev_last != S - 1) { printf("%d -> %d does not end at the last pixel\n", S, D); return 1; }
    }
  printf("ok %ld cases\n", cases);
  return 0;
}
