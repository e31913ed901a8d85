// Stand-alone bounds program of the overlay rasteriser (tests/test_overlay_host.py compiles it with -fsanitize=address,undefined
// and runs it): the host body of scenelib2_amd/csrc/sl2_overlay_dev.hpp over the case list of tests/overlay_cases.py, which the
// test writes to a file together with what the NumPy restatement expects.  Every frame, list, patch array and output sits in a
// heap block of EXACTLY its size (the patch array ends 121 bytes into its last entry): a read past a template or a store past the
// image is a heap-buffer-overflow here, an int that leaves its range in a box is a runtime error.
//
// File: int32 ncases, then per case int32 width, height, count, npatches, patch_stride; uint8 frame[width * height];
// sl2_overlay_item items[count]; uint8 patches[(npatches - 1) * patch_stride + 121] (npatches > 0); uint8 expected[3 * width * height].
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../scenelib2_amd/csrc/sl2_overlay_dev.hpp"

using namespace sl2;

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  static_assert(sizeof(sl2_overlay_item) == 64, "sl2_overlay_item");
  if (argc < 2) { printf("usage: overlay_host CASEFILE\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
  int32_t ncases = 0;
  if (!get(f, &ncases, 4)) { printf("short file\n"); return 2; }
  long pixels = 0, items_seen = 0;
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
      printf("short file in case %d\n", c);
      return 2;
    }
    memset(out, 0xA5, 3 * px);
    overlay_draw_host_body(frame, w, h, items, count, patches, (size_t)stride, npatches, prep, out);
    if (memcmp(out, want, 3 * px) != 0) {
      size_t at = 0;
      while (out[at] == want[at]) ++at;
      printf("case %d (%d x %d, %d items): byte %zu is %d, expected %d\n", c, w, h, count, at, out[at], want[at]);
      return 1;
    }
    pixels += (long)px; items_seen += count;
    free(prep); free(out); free(want); free(patches); free(items); free(frame);
  }
  fclose(f);
  // the particle counter against the reference's loop (graphictool.cpp:716-733), and its bound
  for (int n = 0; n <= 1024; ++n) {
    const int step = overlay_particle_step(n);
    int counter = 1, drawn = 0;
    for (int k = 0; k < n; ++k) {
      bool ref;
      if (counter != step) { ++counter; ref = false; } else { counter = 1; ref = true; }
      if (ref != ((k + 1) % step == 0)) { printf("counter differs at n = %d, particle %d\n", n, k); return 1; }
      drawn += ref ? 1 : 0;
    }
    if (drawn > 19) { printf("%d particles drawn of %d\n", drawn, n); return 1; }
  }
  printf("ok %d cases %ld items %ld pixels\n", (int)ncases, items_seen, pixels);
  return 0;
}
