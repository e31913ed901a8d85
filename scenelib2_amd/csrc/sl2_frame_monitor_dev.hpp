// The frame monitor (include/scenelib2_amd.h, "the frame monitor"): exact integer statistics of an
// engine-size grey frame and the gate that turns them into a verdict.  SL2_HD: the same source is the per-chunk and per-word
// arithmetic of k_frame_stats and k_frame_gate (sl2_frame_monitor.hip), the body of sl2_frame_stats_host and
// sl2_frame_verdict_host, and what a stand-alone host program includes (tests/frame_monitor_host.cpp).
//
// A frame is n = W * H bytes with pitch W, so it is ONE run of bytes and every quantity but the gradient is a sum over that run.
// The unit of work is a CHUNK: 16 consecutive bytes at a frame-relative offset that is a multiple of 16 - two digest words, one
// 16-byte load where the frame's address allows it.  The gradient of a pixel reads its four neighbours at i - 1, i + 1, i - W and
// i + W; inside the image (1 <= x <= W - 2, 1 <= y <= H - 2) all four lie in the frame.
#pragma once
#include "../../include/scenelib2_amd.h"
#include "sl2_math.hpp"

namespace sl2 {

constexpr int kFrameChunk = 16;            // bytes per chunk: two digest words
constexpr int kFrameThreads = 256;         // k_frame_stats: threads per workgroup, one chunk each per pass
constexpr int kFrameBandRows = 32;         // rows per workgroup of k_frame_stats (scenelib2_amd_testing.h repeats it for the tests)
constexpr int kFrameMaxBands = 4096;       // bands per sequence at most: a taller frame gets taller bands (frame_band_rows)
static_assert(kFrameBandRows % kFrameChunk == 0, "a band starts on a chunk boundary whatever the width");

// Rows per band for a frame of `height` rows: kFrameBandRows, or for frames of more than kFrameBandRows * kFrameMaxBands rows the
// multiple of 16 that keeps the band count within kFrameMaxBands.  A multiple of 16 rows times any width is a multiple of 16
// bytes: no chunk straddles two bands.
SL2_HD int frame_band_rows(int height) {
  if (height <= kFrameBandRows * kFrameMaxBands) return kFrameBandRows;
  const int rows = (int)(((int64_t)height + kFrameMaxBands - 1) / kFrameMaxBands);
  return (rows + kFrameChunk - 1) / kFrameChunk * kFrameChunk;
}
SL2_HD int frame_bands(int height) { const int r = frame_band_rows(height); return (int)(((int64_t)height + r - 1) / r); }

// A size the monitor and the host form take: n = width * height in 1 .. 2^31 - 1
SL2_HD bool frame_size_ok(int width, int height) {
  return width >= 1 && height >= 1 && (int64_t)width * height < ((int64_t)1 << 31);
}

// Why a gate is refused, or nullptr
SL2_HD const char* frame_gate_fault(const sl2_frame_gate& g) {
  if (g.dark_bins > 16u) return "dark_bins over 16";
  if (g.bright_bins > 16u) return "bright_bins over 16";
  return nullptr;
}

SL2_HD uint64_t frame_mix64(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
// The digest's term of word k (bytes past the frame's end are zero in `word`)
SL2_HD uint64_t frame_word_term(uint64_t word, uint64_t k) { return frame_mix64(word ^ ((k + 1) * 0x9E3779B97F4A7C15ull)); }

// The gradient energy of one pixel from its left, right, upper and lower neighbours: at most 2 * 255^2
SL2_HD uint32_t frame_grad_term(int l, int r, int u, int d) { return (uint32_t)((r - l) * (r - l) + (d - u) * (d - u)); }

// What one lane (or the host loop) accumulates.  hist is 16 named counters so that a kernel keeps them in registers.
struct FrameAcc {
  uint64_t sum = 0, sum_sq = 0, grad = 0, digest = 0;
  uint32_t mn = 0xFFFFFFFFu, mx = 0;
  uint32_t hist[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

// Sixteen bytes as four little-endian words
struct FrameChunk { uint32_t w[4]; };
SL2_HD int frame_chunk_byte(const FrameChunk& c, int j) { return (int)((c.w[j >> 2] >> (8 * (j & 3))) & 255u); }

// Bytes [off, off + 16) of a frame of n bytes, one byte at a time; what lies outside [0, n) reads as 0 and is not touched
SL2_HD FrameChunk frame_load_bytes(const uint8_t* f, int64_t off, int64_t n) {
  FrameChunk c;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int q = 0; q < 4; ++q) {
    uint32_t w = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 4; ++j) {
      const int64_t i = off + 4 * q + j;
      if (i >= 0 && i < n) w |= (uint32_t)f[i] << (8 * j);
    }
    c.w[q] = w;
  }
  return c;
}

// One chunk into the accumulator.  c: the chunk's index (its bytes are [16 c, 16 c + 16) of the frame), cnt: how many of them lie
// in the frame (1 .. 16; the bytes of `self` past cnt are zero), left / right: the bytes at 16 c - 1 and 16 c + 16 (anything
// where the frame has none), up / down: the bytes at 16 c - W .. and 16 c + W .. (anything outside the frame: a pixel inside the
// image has all four neighbours in the frame, and the others are masked out).
SL2_HD void frame_chunk_accumulate(FrameAcc& a, const FrameChunk& self, int left, int right, const FrameChunk& up,
                                   const FrameChunk& down, int64_t c, int cnt, int W, int H) {
  // the digest: two words
  const uint64_t w0 = (uint64_t)self.w[0] | ((uint64_t)self.w[1] << 32), w1 = (uint64_t)self.w[2] | ((uint64_t)self.w[3] << 32);
  a.digest += frame_word_term(w0, (uint64_t)(2 * c));
  if (cnt > 8) a.digest += frame_word_term(w1, (uint64_t)(2 * c + 1));
  // position of the chunk's first pixel
  const int64_t i0 = c * kFrameChunk;
  int y = (int)(i0 / W), x = (int)(i0 - (int64_t)y * W);
  uint32_t sum = 0, sq = 0, grad = 0, mn = a.mn, mx = a.mx;
  // the histogram of the chunk in two words of 4-bit fields (8 pixels each, so a field holds its count)
  uint64_t h0 = 0, h1 = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int j = 0; j < kFrameChunk; ++j) {
    if (j < cnt) {
      const uint32_t v = (uint32_t)frame_chunk_byte(self, j);
      sum += v; sq += v * v;
      mn = v < mn ? v : mn; mx = v > mx ? v : mx;
      const uint64_t one = (uint64_t)1 << ((v >> 2) & 0x3Cu);      // field v >> 4
      if (j < 8) h0 += one; else h1 += one;
      if (x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2) {
        const int l = j == 0 ? left : frame_chunk_byte(self, j == 0 ? 0 : j - 1);
        const int r = j == kFrameChunk - 1 ? right : frame_chunk_byte(self, j == kFrameChunk - 1 ? j : j + 1);
        grad += frame_grad_term(l, r, frame_chunk_byte(up, j), frame_chunk_byte(down, j));
      }
    }
    if (++x == W) { x = 0; ++y; }
  }
  a.sum += sum; a.sum_sq += sq; a.grad += grad; a.mn = mn; a.mx = mx;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int b = 0; b < 16; ++b) a.hist[b] += (uint32_t)((h0 >> (4 * b)) & 15u) + (uint32_t)((h1 >> (4 * b)) & 15u);
}

// The chunk count of a frame of n bytes
SL2_HD int64_t frame_chunks(int64_t n) { return (n + kFrameChunk - 1) / kFrameChunk; }

SL2_HD void frame_acc_to_stats(const FrameAcc& a, sl2_frame_stats* s) {
  s->sum = a.sum; s->sum_sq = a.sum_sq; s->gradient_energy = a.grad; s->digest = a.digest;
  s->min = a.mn; s->max = a.mx;
  for (int b = 0; b < 16; ++b) s->hist[b] = a.hist[b];
}

// sl2_frame_stats_host: every chunk in turn through the byte loader
inline void frame_stats_host_body(const uint8_t* f, int W, int H, sl2_frame_stats* out) {
  const int64_t n = (int64_t)W * H;
  FrameAcc a;
  for (int64_t c = 0; c < frame_chunks(n); ++c) {
    const int64_t off = c * kFrameChunk;
    const int cnt = n - off < kFrameChunk ? (int)(n - off) : kFrameChunk;
    const FrameChunk self = frame_load_bytes(f, off, n), up = frame_load_bytes(f, off - W, n), down = frame_load_bytes(f, off + W, n);
    const int left = off >= 1 ? f[off - 1] : 0, right = off + kFrameChunk < n ? f[off + kFrameChunk] : 0;
    frame_chunk_accumulate(a, self, left, right, up, down, c, cnt, W, H);
  }
  frame_acc_to_stats(a, out);
}

// The gate: the OR of the rules that fire.  Integers only.
SL2_HD uint32_t frame_verdict(const sl2_frame_stats& s, const sl2_frame_gate& g, bool have_previous, uint64_t previous_digest) {
  uint32_t v = 0;
  if (g.min_range != 0 && s.max - s.min < g.min_range) v |= SL2_FRAME_FLAT;
  if (g.dark_bins != 0) {
    uint64_t dark = 0;
    for (uint32_t b = 0; b < 16u; ++b) if (b < g.dark_bins) dark += s.hist[b];
    if (dark > g.max_dark_pixels) v |= SL2_FRAME_DARK;
  }
  if (g.bright_bins != 0) {
    uint64_t bright = 0;
    for (uint32_t b = 0; b < 16u; ++b) if (b + g.bright_bins >= 16u) bright += s.hist[b];
    if (bright > g.max_bright_pixels) v |= SL2_FRAME_BRIGHT;
  }
  if (g.min_gradient_energy != 0 && s.gradient_energy < g.min_gradient_energy) v |= SL2_FRAME_BLURRED;
  if (g.reject_repeated != 0 && have_previous && s.digest == previous_digest) v |= SL2_FRAME_REPEATED;
  return v;
}

}  // namespace sl2
