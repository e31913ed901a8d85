// Stand-alone bounds program of the frame monitor (tests/test_frame_monitor_host.py compiles it with -fsanitize=address,undefined
// and runs it): frame_stats_host_body of scenelib2_amd/csrc/sl2_frame_monitor_dev.hpp over a heap block of EXACTLY width * height
// bytes for every shape given on the command line (the case table's) and every content, so a neighbour read outside the frame, a
// chunk read past its last byte or an overflow in the index arithmetic stops the program here.  It also checks every record
// against a plain per-pixel loop written from the header's text, the band arithmetic, the gate validator and the verdict rules.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../scenelib2_amd/csrc/sl2_frame_monitor_dev.hpp"

using namespace sl2;

static uint32_t rng_state = 13579u;
static uint8_t next_byte() { rng_state = rng_state * 1664525u + 1013904223u; return (uint8_t)(rng_state >> 24); }

// The definition, pixel by pixel
static void plain(const uint8_t* f, int W, int H, sl2_frame_stats* s) {
  memset(s, 0, sizeof(*s));
  const int64_t n = (int64_t)W * H;
  s->min = 255; s->max = 0;
  for (int64_t i = 0; i < n; ++i) {
    s->sum += f[i]; s->sum_sq += (uint64_t)f[i] * f[i];
    if (f[i] < s->min) s->min = f[i];
    if (f[i] > s->max) s->max = f[i];
    ++s->hist[f[i] >> 4];
  }
  for (int y = 1; y + 1 < H; ++y)
    for (int x = 1; x + 1 < W; ++x) {
      const int dx = (int)f[(int64_t)y * W + x + 1] - (int)f[(int64_t)y * W + x - 1];
      const int dy = (int)f[(int64_t)(y + 1) * W + x] - (int)f[(int64_t)(y - 1) * W + x];
      s->gradient_energy += (uint64_t)(dx * dx + dy * dy);
    }
  for (int64_t k = 0; 8 * k < n; ++k) {
    uint64_t word = 0;
    for (int j = 0; j < 8 && 8 * k + j < n; ++j) word |= (uint64_t)f[8 * k + j] << (8 * j);
    uint64_t z = word ^ ((uint64_t)(k + 1) * 0x9E3779B97F4A7C15ull);
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    s->digest += z;
  }
}

static bool run(int W, int H, int content) {
  const size_t n = (size_t)W * H;
  uint8_t* f = (uint8_t*)malloc(n);          // exactly the frame
  for (size_t i = 0; i < n; ++i) {
    const int x = (int)(i % W), y = (int)(i / W);
    f[i] = content == 0 ? next_byte() : content == 1 ? 0 : content == 2 ? 255 : content == 3 ? (uint8_t)(((x + y) & 1) * 255)
         : (uint8_t)(((x == 0 || x == W - 1) && (y == 0 || y == H - 1)) || y % kFrameBandRows == 0 || y % kFrameBandRows == kFrameBandRows - 1 ? 250 : 16);
  }
  sl2_frame_stats got, want;
  memset(&got, 0xA5, sizeof(got));
  frame_stats_host_body(f, W, H, &got);
  plain(f, W, H, &want);
  free(f);
  if (memcmp(&got, &want, sizeof(got)) != 0) { printf("record differs: %d x %d content %d\n", W, H, content); return false; }
  return true;
}

int main(int argc, char** argv) {
  static_assert(sizeof(sl2_frame_stats) == 104 && sizeof(sl2_frame_gate) == 32, "layouts");
  int runs = 0;
  for (int a = 1; a + 1 < argc; a += 2) {
    const int W = atoi(argv[a]), H = atoi(argv[a + 1]);
    if (!frame_size_ok(W, H)) { printf("bad shape\n"); return 1; }
    for (int content = 0; content < 5; ++content, ++runs)
      if (!run(W, H, content)) return 1;
  }
  if (runs == 0) { printf("no shapes given\n"); return 1; }
  // bands: a multiple of 16 rows, never more than kFrameMaxBands of them, every row covered
  const int heights[] = {1, kFrameBandRows - 1, kFrameBandRows, kFrameBandRows + 1, 240, kFrameBandRows * kFrameMaxBands, kFrameBandRows * kFrameMaxBands + 1,
                         1 << 24, 2147483647};
  for (int h : heights) {
    const int r = frame_band_rows(h), b = frame_bands(h);
    if (r % kFrameChunk != 0 || r < kFrameBandRows || b < 1 || b > kFrameMaxBands || (int64_t)r * b < h || (int64_t)r * (b - 1) >= h) {
      printf("bands of height %d: %d rows x %d\n", h, r, b);
      return 1;
    }
  }
  if (frame_size_ok(0, 1) || frame_size_ok(1, 0) || frame_size_ok(65536, 32768) || !frame_size_ok(65536, 32767) || !frame_size_ok(1, 2147483647)) { printf("sizes\n"); return 1; }
  // the validator and the rules
  sl2_frame_gate g;
  memset(&g, 0, sizeof(g));
  if (frame_gate_fault(g)) { printf("the zero gate was refused\n"); return 1; }
  g.dark_bins = 16; g.bright_bins = 16;
  if (frame_gate_fault(g)) { printf("16 bins were refused\n"); return 1; }
  g.dark_bins = 17;
  if (!frame_gate_fault(g)) { printf("17 dark bins passed\n"); return 1; }
  g.dark_bins = 0; g.bright_bins = 17;
  if (!frame_gate_fault(g)) { printf("17 bright bins passed\n"); return 1; }
  sl2_frame_stats s;
  memset(&s, 0, sizeof(s));
  s.min = 10; s.max = 20; s.hist[0] = 5; s.hist[15] = 7; s.gradient_energy = 100; s.digest = 42;
  memset(&g, 0, sizeof(g));
  if (frame_verdict(s, g, true, 42) != 0) { printf("the zero gate fired\n"); return 1; }
  g.min_range = 11; g.dark_bins = 1; g.max_dark_pixels = 4; g.bright_bins = 1; g.max_bright_pixels = 6; g.reject_repeated = 1; g.min_gradient_energy = 101;
  if (frame_verdict(s, g, true, 42) != 31u || frame_verdict(s, g, false, 42) != 15u || frame_verdict(s, g, true, 43) != 15u) { printf("rules\n"); return 1; }
  g.min_range = 10; g.max_dark_pixels = 5; g.max_bright_pixels = 7; g.min_gradient_energy = 100;
  if (frame_verdict(s, g, false, 0) != 0) { printf("thresholds\n"); return 1; }
  printf("ok %d runs\n", runs);
  return 0;
}
