// The map from outside, and a click into it (C ABI): two cameras replay the recording of scene.cfg, and after every frame each
// sequence's map is written out the way the reference's main pane, GraphicTool::Draw3dScene, shows it - the camera as a wire
// glyph, its trajectory, a marker and the 3-sigma ellipsoid of every feature, the rays of features being initialised and the
// axes - seen through a virtual camera that is FITTED to the map:
//
//   sl2_world_items     the lists as records, with the extents of each map (what the axes span)
//   sl2_view_look_at    a view from above and behind the extents' centre, far enough to hold them
//   sl2_draw_world      fill, list and draw on the device, one call, one copy of the RGB images (any size: 480 x 360 here)
//   sl2_pick_items_batch  after the last frame: a click on the marker of one feature per sequence answers its label
//                       (GraphicTool::Picker), which is then marked and deleted (sl2_delete_features)
//
// The frames land in --out as seq<S>_frame<K>.ppm.
//
//   world_view_monoslam --cfg scene.cfg --frames dir --out dir [--no-mapping]
#include <cmath>

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
  const int B = 2, max_features = 32;
  const int W = sc.cam.width, H = sc.cam.height, VW = 480, VH = 360;
  const size_t fb = (size_t)W * H, vb = (size_t)3 * VW * VH;
  sl2_engine* eng = nullptr;
  CHECK(sl2_create(&sc.cam, &sc.prm, B, max_features, 0, nullptr, &eng));
  for (int s = 0; s < B; ++s) {
    CHECK(sl2_set_vehicle_state(eng, s, 1, sc.xv, sc.Pxx));
    for (int k = 0; k < sc.n_known; ++k) CHECK(sl2_add_known_features(eng, s, 1, 1, &sc.y[3 * k], &sc.xp[7 * k], &sc.patches[121 * k]));
  }
  const int kpart = sc.prm.max_features_to_init_at_once < 1 ? 1 : (sc.prm.max_features_to_init_at_once > 4 ? 4 : sc.prm.max_features_to_init_at_once);
  const int stride = (int)sl2_world_item_bound(max_features, kpart);
  std::vector<sl2_overlay_item> items((size_t)stride * B);
  std::vector<int32_t> counts(B), marked(B, -1);
  std::vector<double> extents(6 * (size_t)B);
  std::vector<sl2_view> views(B);
  std::vector<uint8_t> frames(B * fb), rgb((size_t)B * vb);
  // the reference example's view, with a focal length for the 480 x 360 pane: the first look, before the extents are known
  const double ref_eye[3] = {0.0, 0.18, -1.4}, ref_target[3] = {0.0, 0.13, 0.0}, up[3] = {0.0, 1.0, 0.0};
  const double focal = 1.5 * sc.cam.fku;
  for (int s = 0; s < B; ++s) CHECK(sl2_view_look_at(ref_eye, ref_target, up, focal, focal, VW / 2.0, VH / 2.0, &views[s]));
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
    // the extents of each map (any view serves for them), then a view fitted to them: sequence 0 from behind and above, sequence
    // 1 from the side
    CHECK(sl2_world_items(eng, 0, B, views.data(), B, SL2_WORLD_ALL, marked.data(), items.data(), stride, counts.data(), extents.data(), /*on_device=*/0));
    for (int s = 0; s < B; ++s) {
      const double* ex = &extents[6 * (size_t)s];
      const double centre[3] = {0.5 * (ex[0] + ex[1]), 0.5 * (ex[2] + ex[3]), 0.5 * (ex[4] + ex[5])};
      const double size = std::max(0.2, std::max(ex[1] - ex[0], std::max(ex[3] - ex[2], ex[5] - ex[4])));
      const double eye[3] = {centre[0] + (s == 0 ? 0.15 : 1.6) * size, centre[1] + 0.5 * size, centre[2] - (s == 0 ? 1.8 : 0.6) * size};
      CHECK(sl2_view_look_at(eye, centre, up, focal, focal, VW / 2.0, VH / 2.0, &views[s]));
    }
    CHECK(sl2_draw_world(eng, 0, B, views.data(), B, VW, VH, /*background=*/0, SL2_WORLD_ALL, marked.data(), rgb.data(), vb, /*out_on_device=*/0));
    CHECK(sl2_world_items(eng, 0, B, views.data(), B, SL2_WORLD_ALL, marked.data(), items.data(), stride, counts.data(), extents.data(), /*on_device=*/0));
    for (int s = 0; s < B; ++s) {
      int glyph = 0, axes = 0, segments = 0, rays = 0, markers = 0, rings = 0;
      for (int q = 0; q < counts[s]; ++q) {
        const sl2_overlay_item& it = items[(size_t)s * stride + q];
        const bool seg = it.kind == SL2_ITEM_SEGMENT;
        glyph += seg && it.rgb[0] == 150; axes += seg && it.rgb[2] == 255; segments += seg && it.label < 0 && it.rgb[2] == 0;
        rays += seg && it.label >= 0; markers += it.kind == SL2_ITEM_RECT && it.a[0] == it.a[2]; rings += it.kind == SL2_ITEM_RING;
      }
      char name[64];
      snprintf(name, sizeof(name), "/seq%d_frame%03d.ppm", s, k);
      if (write_ppm(out_dir + name, &rgb[(size_t)s * vb], VW, VH)) return 1;
      const double* ex = &extents[6 * (size_t)s];
      printf("frame %3d seq %d  items %3d  glyph %2d  trajectory %3d  rays %d  markers %2d  ellipsoids %2d  axes %d  extents %.3f %.3f %.3f %.3f %.3f %.3f\n", k, s,
             counts[s], glyph, segments, rays, markers, rings, axes, ex[0], ex[1], ex[2], ex[3], ex[4], ex[5]);
    }
  }
  // the click: in sequence s, on the marker of the (s + 1)-th feature that has one.  The list is rebuilt with the features box
  // alone, as the reference's picker redraws with the boxes of the last frame: no ellipsoid outline is in the way
  CHECK(sl2_world_items(eng, 0, B, views.data(), B, SL2_WORLD_FEATURES, marked.data(), items.data(), stride, counts.data(), nullptr, /*on_device=*/0));
  std::vector<int32_t> clicks(2 * (size_t)B, -1), picked(2 * (size_t)B, -1), want(B, -1);
  for (int s = 0; s < B; ++s) {
    int seen = 0;
    for (int q = 0; q < counts[s]; ++q) {
      const sl2_overlay_item& it = items[(size_t)s * stride + q];
      if (it.kind == SL2_ITEM_RECT && it.a[0] == it.a[2] && it.a[0] >= 0 && it.a[0] < VW && it.a[1] >= 0 && it.a[1] < VH && seen++ == s) {
        clicks[2 * s] = it.a[0]; clicks[2 * s + 1] = it.a[1]; want[s] = it.label;
        break;
      }
    }
  }
  CHECK(sl2_pick_items_batch(0, nullptr, B, VW, VH, items.data(), stride, counts.data(), 0, clicks.data(), picked.data(), /*on_device=*/0));
  std::vector<int32_t> labels(B), deleted(B, 0);
  for (int s = 0; s < B; ++s) labels[s] = picked[2 * s];      // (-1: nothing under the click - that sequence is left alone)
  CHECK(sl2_delete_features(eng, 0, B, labels.data(), deleted.data()));
  std::vector<sl2_feature_info> feats(max_features);
  for (int s = 0; s < B; ++s) {
    int n = 0, still = 0;
    CHECK(sl2_get_features(eng, s, feats.data(), max_features, 0, &n));
    for (int q = 0; q < n; ++q) still += feats[(size_t)q].label == labels[s];
    printf("pick seq %d  click %d %d  marker of label %d  picked label %d item %d  deleted %d  still listed %d  features left %d\n", s, clicks[2 * s],
           clicks[2 * s + 1], want[s], picked[2 * s], picked[2 * s + 1], deleted[s], still, n);
  }
  sl2_destroy(eng);
  return 0;
}
