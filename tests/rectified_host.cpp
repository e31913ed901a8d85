// Stand-alone bounds program of the rectified view's two pixel rules (tests/test_rectified_host.py compiles it with
// -fsanitize=address,undefined and runs it): the host bodies of scenelib2_amd/csrc/sl2_overlay_dev.hpp (with SL2_ITEM_SEGMENT)
// and sl2_rectify_dev.hpp over the case lists of tests/rectified_cases.py, which the test writes to a file together with what
// the NumPy restatement expects.  Every frame, list, patch array and output sits in a heap block of EXACTLY its size: a tap
// beyond the source or a store past the image is a heap-buffer-overflow here, an int that leaves its range a runtime error.
//
// File: int32 nsegcases, then per case int32 width, height, count, npatches, patch_stride; uint8 frame[width * height];
// sl2_overlay_item items[count]; uint8 patches[(npatches - 1) * patch_stride + 121] (npatches > 0); uint8 expected[3 * width * height].
// Then int32 nremapcases, then per case int32 width, height; double u0, v0, kd1; uint8 frame[width * height];
// uint8 expected[width * height].
// Then int32 nscene, then per case double cam[4] (fku, fkv, u0, v0), xp[7], y[3], Pxx[49], Pxy[21], Pyy[9]; expected: double m[3],
// Sigma[9]; int32 drawn; double centre[2], q[4] (zeros where not drawn).  Then int32 nsegments, then per case double cam[4], a[3],
// b[3]; expected int32 drawn, out[4] (zeros where not drawn).  Doubles are compared as bytes: the header fixes the order of
// every operation.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../scenelib2_amd/csrc/sl2_overlay_dev.hpp"
#include "../scenelib2_amd/csrc/sl2_rectify_dev.hpp"

using namespace sl2;

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  static_assert(sizeof(sl2_overlay_item) == 64, "sl2_overlay_item");
  if (argc < 2) { printf("usage: rectified_host CASEFILE\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
  int32_t ncases = 0;
  if (!get(f, &ncases, 4)) { printf("short file\n"); return 2; }
  long pixels = 0;
  for (int c = 0; c < ncases; ++c) {
    int32_t hd[5];
    if (!get(f, hd, sizeof(hd))) { printf("short file\n"); return 2; }
    const int w = hd[0], h = hd[1], count = hd[2], npatches = hd[3], stride = hd[4];
    const size_t px = (size_t)w * h, pbytes = npatches > 0 ? (size_t)(npatches - 1) * stride + SL2_PATCH_BYTES : 0;
    uint8_t* frame = (uint8_t*)malloc(px);
    sl2_overlay_item* items = (sl2_overlay_item*)malloc(sizeof(sl2_overlay_item) * (size_t)(count > 0 ? count : 1));
    uint8_t* patches = pbytes ? (uint8_t*)malloc(pbytes) : nullptr;
    uint8_t* want = (uint8_t*)malloc(3 * px);
    uint8_t* out = (uint8_t*)malloc(3 * px);
    OverlayPrep* prep = (OverlayPrep*)malloc(sizeof(OverlayPrep) * (size_t)(count + 1));
    if (!get(f, frame, px) || !get(f, items, sizeof(sl2_overlay_item) * (size_t)count) || !get(f, patches, pbytes) || !get(f, want, 3 * px)) {
      printf("short file in segment case %d\n", c);
      return 2;
    }
    memset(out, 0xA5, 3 * px);
    overlay_draw_host_body(frame, w, h, items, count, patches, (size_t)stride, npatches, prep, out);
    if (memcmp(out, want, 3 * px) != 0) {
      size_t at = 0;
      while (out[at] == want[at]) ++at;
      printf("segment case %d (%d x %d, %d items): byte %zu is %d, expected %d\n", c, w, h, count, at, out[at], want[at]);
      return 1;
    }
    pixels += (long)px;
    free(prep); free(out); free(want); free(patches); free(items); free(frame);
  }
  int32_t nremap = 0;
  if (!get(f, &nremap, 4)) { printf("short file\n"); return 2; }
  for (int c = 0; c < nremap; ++c) {
    int32_t hd[2];
    double cam[3];
    if (!get(f, hd, sizeof(hd)) || !get(f, cam, sizeof(cam))) { printf("short file\n"); return 2; }
    const int w = hd[0], h = hd[1];
    const size_t px = (size_t)w * h;
    uint8_t* frame = (uint8_t*)malloc(px);
    uint8_t* want = (uint8_t*)malloc(px);
    uint8_t* out = (uint8_t*)malloc(px);
    if (!get(f, frame, px) || !get(f, want, px)) { printf("short file in remap case %d\n", c); return 2; }
    memset(out, 0xA5, px);
    rectify_host_body(frame, w, h, cam[0], cam[1], cam[2], out);
    if (memcmp(out, want, px) != 0) {
      size_t at = 0;
      while (out[at] == want[at]) ++at;
      printf("remap case %d (%d x %d): byte %zu is %d, expected %d\n", c, w, h, at, out[at], want[at]);
      return 1;
    }
    pixels += (long)px;
    free(out); free(want); free(frame);
  }
  int32_t nscene = 0;
  if (!get(f, &nscene, 4)) { printf("short file\n"); return 2; }
  for (int c = 0; c < nscene; ++c) {
    double* in = (double*)malloc(sizeof(double) * 93);
    double want_d[18], got_d[18];
    int32_t want_drawn = 0;
    if (!get(f, in, sizeof(double) * 93) || !get(f, want_d, sizeof(double) * 12) || !get(f, &want_drawn, 4) || !get(f, want_d + 12, sizeof(double) * 6)) {
      printf("short file in scene case %d\n", c);
      return 2;
    }
    double Jx[21], Jy[9];
    memset(got_d, 0, sizeof(got_d));
    scene_zeroed_jac(in + 4, in + 11, got_d, Jx, Jy);
    scene_sigma(Jx, Jy, in + 14, in + 63, in + 84, got_d + 3);
    const int32_t drawn = scene_conic(in[0], in[1], in[2], in[3], got_d, got_d + 3, got_d + 12, got_d + 14) ? 1 : 0;
    if (!drawn) memset(got_d + 12, 0, sizeof(double) * 6);
    if (drawn != want_drawn || memcmp(got_d, want_d, sizeof(got_d)) != 0) {
      int at = 0;
      while (at < 18 && memcmp(got_d + at, want_d + at, 8) == 0) ++at;
      printf("scene case %d: drawn %d, expected %d; double %d is %.17g, expected %.17g\n", c, drawn, want_drawn, at, at < 18 ? got_d[at] : 0.0,
             at < 18 ? want_d[at] : 0.0);
      return 1;
    }
    free(in);
  }
  int32_t nseg3 = 0;
  if (!get(f, &nseg3, 4)) { printf("short file\n"); return 2; }
  for (int c = 0; c < nseg3; ++c) {
    double* in = (double*)malloc(sizeof(double) * 10);
    int32_t want[5], got[5] = {0, 0, 0, 0, 0};
    if (!get(f, in, sizeof(double) * 10) || !get(f, want, sizeof(want))) { printf("short file in 3-D segment case %d\n", c); return 2; }
    int out[4] = {0, 0, 0, 0};
    got[0] = scene_segment(in[0], in[1], in[2], in[3], in + 4, in + 7, out) ? 1 : 0;
    if (got[0]) for (int k = 0; k < 4; ++k) got[1 + k] = out[k];
    if (memcmp(got, want, sizeof(got)) != 0) {
      printf("3-D segment case %d: (%d: %d %d %d %d), expected (%d: %d %d %d %d)\n", c, got[0], got[1], got[2], got[3], got[4], want[0], want[1],
             want[2], want[3], want[4]);
      return 1;
    }
    free(in);
  }
  fclose(f);
  printf("ok %d segment cases %d remap cases %d scene cases %d 3-D segments %ld pixels\n", (int)ncases, (int)nremap, (int)nscene, (int)nseg3, pixels);
  return 0;
}
