// What the tracker is doing, as pictures (C ABI): four cameras replay the recording of scene.cfg with mapping on - three of them
// drop a frame now and then - and for two of the four sequences every frame is written out annotated, the way the reference's
// GraphicTool::DrawRawAR shows it on screen:
//
//   sl2_draw_overlays          the draw list of each sequence and its rasterisation on the device, one call, one copy of the
//                              RGB images: search ellipses (red matched, blue failed, green marked), every feature's template
//                              where it was matched or is predicted (yellow frame: not selected), the string of particle ellipses
//                              of a partially initialised feature, the initialisation boxes
//   sl2_overlay_items          the same lists as records, for a client that draws vectors itself: counted per kind and colour here
//
// Camera 2's lens is covered for every sixth frame, so that failed matches (blue) show as well as matched ones (red).
// The frames land in --out as seq<S>_frame<K>.ppm.  The first feature of each map is the marked one.
//
//   overlay_monoslam --cfg scene.cfg --frames dir --out dir [--no-mapping]
#include "scene_cfg.hpp"

#define CHECK(call)                                                                        \
  do {                                                                                     \
    const int rc_ = (call);                                                                \
    if (rc_ != SL2_OK) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, sl2_last_error()); return 1; } \
  } while (0)

static int list_dir(const std::string& dir, std::vector<std::string>& paths) {
  int count = 0;
  if (sl2_list_frames(dir.c_str(), nullptr, 0, &count) != SL2_OK) return 1;
  std::vector<char> buf((size_t)count * 4096 + 1);
  if (sl2_list_frames(dir.c_str(), buf.data(), buf.size(), &count) != SL2_OK) return 1;
  const char* p = buf.data();
  for (int i = 0; i < count; ++i) {
    const char* e = strchr(p, '\n');
    paths.push_back(e ? std::string(p, e) : std::string(p));
    if (!e) break;
    p = e + 1;
  }
  return 0;
}

static int write_ppm(const std::string& path, const uint8_t* rgb, int w, int h) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
  fprintf(f, "P6\n%d %d\n255\n", w, h);
  const bool ok = fwrite(rgb, 1, (size_t)3 * w * h, f) == (size_t)3 * w * h;
  fclose(f);
  return ok ? 0 : 1;
}

int main(int argc, char** argv) {
  std::string cfg, frames_dir, out_dir;
  bool mapping = true;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--cfg" && i + 1 < argc) cfg = argv[++i];
    else if (a == "--frames" && i + 1 < argc) frames_dir = argv[++i];
    else if (a == "--out" && i + 1 < argc) out_dir = argv[++i];
    else if (a == "--no-mapping") mapping = false;
    else { fprintf(stderr, "usage: %s --cfg scene.cfg --frames dir --out dir [--no-mapping]\n", argv[0]); return 2; }
  }
  if (cfg.empty() || frames_dir.empty() || out_dir.empty()) { fprintf(stderr, "need --cfg, --frames and --out\n"); return 2; }
  Scene sc;
  if (int rc = load_scene(cfg, sc)) return rc;
  std::vector<std::string> paths;
  if (list_dir(frames_dir, paths) || paths.empty()) { fprintf(stderr, "cannot list %s: %s\n", frames_dir.c_str(), sl2_last_error()); return 1; }
  if (sl2_device_count() < 1) { fprintf(stderr, "no HIP device: this engine has no CPU path\n"); return 3; }
  const int B = 4, max_features = 32, first_shown = 1, shown = 2;      // sequences 1 and 2 are drawn
  const int W = sc.cam.width, H = sc.cam.height;
  const size_t fb = (size_t)W * H;
  sl2_engine* eng = nullptr;
  CHECK(sl2_create(&sc.cam, &sc.prm, B, max_features, 0, nullptr, &eng));
  for (int s = 0; s < B; ++s) {
    CHECK(sl2_set_vehicle_state(eng, s, 1, sc.xv, sc.Pxx));
    for (int k = 0; k < sc.n_known; ++k) CHECK(sl2_add_known_features(eng, s, 1, 1, &sc.y[3 * k], &sc.xp[7 * k], &sc.patches[121 * k]));
  }
  const int kpart = sc.prm.max_features_to_init_at_once < 1 ? 1 : (sc.prm.max_features_to_init_at_once > 4 ? 4 : sc.prm.max_features_to_init_at_once);
  const int stride = (int)sl2_overlay_item_bound(max_features, kpart);
  std::vector<sl2_overlay_item> items((size_t)stride * shown);
  std::vector<int32_t> counts(shown), marked(shown, 0);      // label 0, the first known feature, is the marked one
  std::vector<uint8_t> frames(B * fb), rgb((size_t)shown * 3 * fb), active(B);
  printf("%d sequences, %d known features each, %d frames, mapping %s; sequences %d and %d are drawn, at most %d items each\n", B, sc.n_known,
         (int)paths.size(), mapping ? "on" : "off", first_shown, first_shown + 1, stride);
  for (int k = 0; k < (int)paths.size(); ++k) {
    int w = 0, h = 0;
    if (sl2_read_image(paths[(size_t)k].c_str(), frames.data(), fb, &w, &h) != SL2_OK || w != W || h != H) {
      fprintf(stderr, "%s: %s\n", paths[(size_t)k].c_str(), sl2_last_error());
      return 1;
    }
    for (int s = 1; s < B; ++s) memcpy(&frames[s * fb], frames.data(), fb);
    // camera 2's lens is covered for every sixth frame: nothing matches in a frame without texture, so its selected features
    // fail their searches and the display shows them blue (frames 6, 12, 18 ...; where that is a frame it drops, nothing happens)
    const bool covered = k > 0 && k % 6 == 0;
    if (covered) memset(&frames[2 * fb], 128, fb);
    for (int s = 0; s < B; ++s) active[s] = (s == 0 || (k + 1) % (s + 3) != 0) ? 1 : 0;      // camera s > 0 drops every (s + 3)rd frame
    CHECK(sl2_set_active_sequences(eng, 0, B, active.data(), /*mask_on_device=*/0));
    CHECK(sl2_go_one_step(eng, frames.data(), fb, /*frames_on_device=*/0, /*save_trajectory=*/1, /*enable_mapping=*/mapping ? 1 : 0));
    // list and draw in one call: the frames of the two sequences shown, the RGB images back in one copy
    CHECK(sl2_draw_overlays(eng, first_shown, shown, &frames[first_shown * fb], fb, /*frames_on_device=*/0, SL2_OVERLAY_ALL, marked.data(), rgb.data(),
                            3 * fb, /*out_on_device=*/0));
    // the lists themselves, as a vector client would take them
    CHECK(sl2_overlay_items(eng, first_shown, shown, SL2_OVERLAY_ALL, marked.data(), items.data(), stride, counts.data(), /*on_device=*/0));
    for (int i = 0; i < shown; ++i) {
      int rings = 0, patches = 0, rects = 0, red = 0, blue = 0, yellow = 0, green = 0;
      for (int q = 0; q < counts[i]; ++q) {
        const sl2_overlay_item& it = items[(size_t)i * stride + q];
        rings += it.kind == SL2_ITEM_RING; patches += it.kind == SL2_ITEM_PATCH; rects += it.kind == SL2_ITEM_RECT;
        red += it.rgb[0] == 255 && it.rgb[1] == 0; blue += it.rgb[2] == 255; yellow += it.rgb[0] == 255 && it.rgb[1] == 255;
        green += it.rgb[0] == 0 && it.rgb[1] == 255;
      }
      char name[64];
      snprintf(name, sizeof(name), "/seq%d_frame%03d.ppm", first_shown + i, k);
      if (write_ppm(out_dir + name, &rgb[(size_t)i * 3 * fb], W, H)) return 1;
      printf("frame %3d seq %d  items %3d  rings %2d  patches %2d  boxes %d  red %2d  blue %2d  yellow %2d  green %2d\n", k, first_shown + i, counts[i],
             rings, patches, rects, red, blue, yellow, green);
    }
  }
  sl2_destroy(eng);
  return 0;
}
