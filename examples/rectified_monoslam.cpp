// What the tracker knows, as pictures (C ABI): three cameras with three lens distortions replay the recording of scene.cfg with
// mapping on, and for every sequence every frame is written out the way the reference's GraphicTool::DrawRectifiedAR shows the
// MAP on screen - the frame with its camera's distortion removed and the 3-D scene over it:
//
//   sl2_draw_rectified         undistort, list and draw on the device, one call, one copy of the RGB images: the trajectory
//                              (yellow), a 3 x 3 marker on every feature's 3-D position (red matched, blue failed, yellow
//                              unselected, green marked), the outline of its 3-sigma ellipsoid relative to the camera, the ray of a
//                              partially initialised feature
//   sl2_scene_items            the same lists as records, for a client that draws vectors itself: counted per kind here
//   sl2_rectify_frames         the undistorted grey frames alone, for a vision consumer behind the tracker
//
// The frames land in --out as seq<S>_frame<K>.ppm.  The first feature of each map is the marked one.
//
//   rectified_monoslam --cfg scene.cfg --frames dir --out dir [--no-mapping]
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
  const int B = 3, max_features = 32;
  const int W = sc.cam.width, H = sc.cam.height;
  const size_t fb = (size_t)W * H;
  sl2_engine* eng = nullptr;
  CHECK(sl2_create(&sc.cam, &sc.prm, B, max_features, 0, nullptr, &eng));
  for (int s = 0; s < B; ++s) {
    CHECK(sl2_set_vehicle_state(eng, s, 1, sc.xv, sc.Pxx));
    for (int k = 0; k < sc.n_known; ++k) CHECK(sl2_add_known_features(eng, s, 1, 1, &sc.y[3 * k], &sc.xp[7 * k], &sc.patches[121 * k]));
  }
  // sequence 0 keeps the recording's lens; 1 and 2 are DISPLAYED as if the lens bent more (the tracker still runs on the
  // recording's calibration: the display calibration is set before each drawing call and taken back after it)
  sl2_camera shown[3] = {sc.cam, sc.cam, sc.cam};
  shown[1].kd1 = sc.cam.kd1 * 4.0;
  shown[2].kd1 = -sc.cam.kd1 * 2.0;
  sl2_camera tracked[3] = {sc.cam, sc.cam, sc.cam};
  const int kpart = sc.prm.max_features_to_init_at_once < 1 ? 1 : (sc.prm.max_features_to_init_at_once > 4 ? 4 : sc.prm.max_features_to_init_at_once);
  const int stride = (int)sl2_scene_item_bound(max_features, kpart);
  std::vector<sl2_overlay_item> items((size_t)stride * B);
  std::vector<int32_t> counts(B), marked(B, 0);      // label 0, the first known feature, is the marked one
  std::vector<uint8_t> frames(B * fb), grey(B * fb), rgb((size_t)B * 3 * fb);
  printf("%d sequences, %d known features each, %d frames, mapping %s; at most %d items each\n", B, sc.n_known, (int)paths.size(), mapping ? "on" : "off",
         stride);
  for (int k = 0; k < (int)paths.size(); ++k) {
    int w = 0, h = 0;
    if (sl2_read_image(paths[(size_t)k].c_str(), frames.data(), fb, &w, &h) != SL2_OK || w != W || h != H) {
      fprintf(stderr, "%s: %s\n", paths[(size_t)k].c_str(), sl2_last_error());
      return 1;
    }
    for (int s = 1; s < B; ++s) memcpy(&frames[s * fb], frames.data(), fb);
    CHECK(sl2_go_one_step(eng, frames.data(), fb, /*frames_on_device=*/0, /*save_trajectory=*/1, /*enable_mapping=*/mapping ? 1 : 0));
    CHECK(sl2_set_cameras(eng, 0, B, shown));
    // undistort, list and draw in one call: the RGB images back in one copy
    CHECK(sl2_draw_rectified(eng, 0, B, frames.data(), fb, /*frames_on_device=*/0, SL2_SCENE_ALL, marked.data(), rgb.data(), 3 * fb, /*out_on_device=*/0));
    // the lists themselves, as a vector client would take them, and the undistorted grey frames alone
    CHECK(sl2_scene_items(eng, 0, B, SL2_SCENE_ALL, marked.data(), items.data(), stride, counts.data(), /*on_device=*/0));
    CHECK(sl2_rectify_frames(eng, 0, B, frames.data(), fb, /*frames_on_device=*/0, grey.data(), fb, /*out_on_device=*/0));
    CHECK(sl2_set_cameras(eng, 0, B, tracked));
    for (int s = 0; s < B; ++s) {
      int segments = 0, rays = 0, markers = 0, rings = 0, green = 0;
      for (int q = 0; q < counts[s]; ++q) {
        const sl2_overlay_item& it = items[(size_t)s * stride + q];
        segments += it.kind == SL2_ITEM_SEGMENT && it.label < 0; rays += it.kind == SL2_ITEM_SEGMENT && it.label >= 0;
        markers += it.kind == SL2_ITEM_RECT && it.a[0] == it.a[2]; rings += it.kind == SL2_ITEM_RING;
        green += it.rgb[0] == 0 && it.rgb[1] == 255;
      }
      size_t moved = 0;
      for (size_t p = 0; p < fb; ++p) moved += grey[s * fb + p] != frames[s * fb + p];
      char name[64];
      snprintf(name, sizeof(name), "/seq%d_frame%03d.ppm", s, k);
      if (write_ppm(out_dir + name, &rgb[(size_t)s * 3 * fb], W, H)) return 1;
      printf("frame %3d seq %d  items %3d  trajectory %3d  rays %d  markers %2d  ellipsoids %2d  green %d  pixels moved %6zu\n", k, s, counts[s], segments,
             rays, markers, rings, green, moved);
    }
  }
  sl2_destroy(eng);
  return 0;
}
