// Stand-alone bounds program of the world view's arithmetic and of the pick rule (tests/test_world_view_host.py compiles it with
// -fsanitize=address,undefined and runs it): the SL2_HD functions of scenelib2_amd/csrc/sl2_world_view_dev.hpp over the cases of
// tests/world_view_cases.py, which the test writes to a file together with what the NumPy restatement expects.  Every input and
// every list sits in a heap block of EXACTLY its size: a read beyond a list is a heap-buffer-overflow here, an int that leaves
// its range a runtime error.
//
// File: int32 nmath, then per case sl2_view view; double xv[7], y[3], Pyy[9]; expected: double m[3], Sigma[9]; int32 has_marker,
// mk[2], has_ring, rc[2]; double q[4] (zeros where absent); int32 glyph[16][5] (drawn, four coordinates; zeros where not
// drawn); double ext[6] (the extents of xv and y); int32 axes[3][5].  Doubles are compared as bytes: the header fixes the
// order of every operation.
// Then int32 npick, then per case int32 width, height, count, npatches, nclicks; sl2_overlay_item items[count]; int32
// clicks[nclicks][2]; expected int32 picked[nclicks][2].
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../scenelib2_amd/csrc/sl2_world_view_dev.hpp"

using namespace sl2;

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  static_assert(sizeof(sl2_overlay_item) == 64 && sizeof(sl2_view) == 88, "record sizes");
  if (argc < 2) { printf("usage: world_view_host CASEFILE\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
  int32_t nmath = 0;
  if (!get(f, &nmath, 4)) { printf("short file\n"); return 2; }
  int rings = 0, edges = 0;
  for (int c = 0; c < nmath; ++c) {
    sl2_view* view = (sl2_view*)malloc(sizeof(sl2_view));
    double* xv = (double*)malloc(sizeof(double) * 7);
    double* y = (double*)malloc(sizeof(double) * 3);
    double* Pyy = (double*)malloc(sizeof(double) * 9);
    double want_d[12], want_q[4], want_ext[6];
    int32_t want_i[6], want_glyph[16 * 5], want_axes[3 * 5];
    if (!get(f, view, sizeof(sl2_view)) || !get(f, xv, 56) || !get(f, y, 24) || !get(f, Pyy, 72) || !get(f, want_d, sizeof(want_d)) ||
        !get(f, want_i, sizeof(want_i)) || !get(f, want_q, sizeof(want_q)) || !get(f, want_glyph, sizeof(want_glyph)) ||
        !get(f, want_ext, sizeof(want_ext)) || !get(f, want_axes, sizeof(want_axes))) {
      printf("short file in case %d\n", c);
      return 2;
    }
    double xp[7], got_d[12], Jy[9], q[4] = {0.0, 0.0, 0.0, 0.0};
    world_view_pose(*view, xp);
    world_zeroed(xp, y, got_d, Jy);
    world_sigma(Jy, Pyy, got_d + 3);
    bool has_marker = false, has_ring = false;
    int mk[2] = {0, 0}, rc[2] = {0, 0};
    world_feature(*view, xp, y, Pyy, true, true, &has_marker, mk, &has_ring, rc, q);
    if (!has_ring) q[0] = q[1] = q[2] = q[3] = 0.0;
    const int32_t got_i[6] = {has_marker ? 1 : 0, has_marker ? mk[0] : 0, has_marker ? mk[1] : 0, has_ring ? 1 : 0, has_ring ? rc[0] : 0, has_ring ? rc[1] : 0};
    if (memcmp(got_d, want_d, sizeof(got_d)) != 0 || memcmp(got_i, want_i, sizeof(got_i)) != 0 || memcmp(q, want_q, sizeof(q)) != 0) {
      int at = 0;
      while (at < 12 && memcmp(got_d + at, want_d + at, 8) == 0) ++at;
      printf("case %d: feature differs: double %d is %.17g, expected %.17g; marker %d (%d, %d) expected %d (%d, %d); ring %d (%d, %d) expected %d (%d, %d)\n", c,
             at, at < 12 ? got_d[at] : 0.0, at < 12 ? want_d[at] : 0.0, got_i[0], got_i[1], got_i[2], want_i[0], want_i[1], want_i[2], got_i[3],
             got_i[4], got_i[5], want_i[3], want_i[4], want_i[5]);
      return 1;
    }
    rings += has_ring ? 1 : 0;
    for (int e = 0; e < kWorldGlyphEdges; ++e) {
      int out[4] = {0, 0, 0, 0};
      const bool drawn = world_glyph_segment(*view, xp, xv, e, out);
      const int32_t got[5] = {drawn ? 1 : 0, drawn ? out[0] : 0, drawn ? out[1] : 0, drawn ? out[2] : 0, drawn ? out[3] : 0};
      if (memcmp(got, want_glyph + 5 * e, sizeof(got)) != 0) {
        printf("case %d: glyph edge %d is (%d: %d %d %d %d), expected (%d: %d %d %d %d)\n", c, e, got[0], got[1], got[2], got[3], got[4],
               want_glyph[5 * e], want_glyph[5 * e + 1], want_glyph[5 * e + 2], want_glyph[5 * e + 3], want_glyph[5 * e + 4]);
        return 1;
      }
      edges += drawn ? 1 : 0;
    }
    double ext[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < 3; ++k) { world_extend(&ext[2 * k], &ext[2 * k + 1], xv[k]); world_extend(&ext[2 * k], &ext[2 * k + 1], y[k]); }
    if (memcmp(ext, want_ext, sizeof(ext)) != 0) { printf("case %d: the extents differ\n", c); return 1; }
    for (int k = 0; k < kWorldAxes; ++k) {
      int out[4] = {0, 0, 0, 0};
      const bool drawn = world_axis_segment(*view, xp, ext[2 * k], ext[2 * k + 1], k, out);
      const int32_t got[5] = {drawn ? 1 : 0, drawn ? out[0] : 0, drawn ? out[1] : 0, drawn ? out[2] : 0, drawn ? out[3] : 0};
      if (memcmp(got, want_axes + 5 * k, sizeof(got)) != 0) {
        printf("case %d: axis %d is (%d: %d %d %d %d), expected (%d: %d %d %d %d)\n", c, k, got[0], got[1], got[2], got[3], got[4], want_axes[5 * k],
               want_axes[5 * k + 1], want_axes[5 * k + 2], want_axes[5 * k + 3], want_axes[5 * k + 4]);
        return 1;
      }
    }
    free(Pyy); free(y); free(xv); free(view);
  }
  int32_t npick = 0;
  if (!get(f, &npick, 4)) { printf("short file\n"); return 2; }
  long clicks_done = 0;
  for (int c = 0; c < npick; ++c) {
    int32_t hd[5];
    if (!get(f, hd, sizeof(hd))) { printf("short file\n"); return 2; }
    const int w = hd[0], h = hd[1], count = hd[2], npatches = hd[3], nclicks = hd[4];
    // (an empty list is a null pointer: nothing of it may be read)
    sl2_overlay_item* items = count > 0 ? (sl2_overlay_item*)malloc(sizeof(sl2_overlay_item) * (size_t)count) : nullptr;
    int32_t* clicks = (int32_t*)malloc(8 * (size_t)nclicks);
    int32_t* want = (int32_t*)malloc(8 * (size_t)nclicks);
    if (!get(f, items, sizeof(sl2_overlay_item) * (size_t)count) || !get(f, clicks, 8 * (size_t)nclicks) || !get(f, want, 8 * (size_t)nclicks)) {
      printf("short file in pick case %d\n", c);
      return 2;
    }
    for (int k = 0; k < nclicks; ++k) {
      int32_t got[2] = {7, 7};
      pick_host_body(w, h, items, count, npatches, clicks[2 * k], clicks[2 * k + 1], got);
      if (got[0] != want[2 * k] || got[1] != want[2 * k + 1]) {
        printf("pick case %d, click (%d, %d): (%d, %d), expected (%d, %d)\n", c, clicks[2 * k], clicks[2 * k + 1], got[0], got[1], want[2 * k], want[2 * k + 1]);
        return 1;
      }
      ++clicks_done;
    }
    free(want); free(clicks); free(items);
  }
  fclose(f);
  printf("ok %d math cases %d rings %d glyph edges %d pick cases %ld clicks\n", (int)nmath, rings, edges, (int)npick, clicks_done);
  return 0;
}
